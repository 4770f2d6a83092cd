"""`core` -- MI355X-native drop-in for the reference's `core` package on the SAC/TQC/TD3/MADDPG/BCQ/TD3BC/CQL/IQL/PPO/A2C/TRPO/DQN/QRDQN/ARS + two-series
CSTR path (reference: core/__init__.py:1-40). Algorithms are imported lazily so that host-only
utilities (and the CPU test-suite) do not need a GPU."""
import os

with open(os.path.join(os.path.dirname(__file__), "version.txt")) as _fh:  # the reference forgot to ship this file
    __version__ = _fh.read().strip()

__all__ = ["SAC", "TQC", "TD3", "MADDPG", "IDDPG", "DDPG", "BCQ", "TD3BC", "CQL", "IQL", "PPO", "A2C", "DQN", "QRDQN", "ARS", "TRPO", "HerReplayBuffer", "__version__"]


def __getattr__(name):
    if name == "SAC":
        from core.sac import SAC
        return SAC
    if name == "TQC":
        from core.tqc import TQC
        return TQC
    if name in ("TD3", "DDPG"):
        import core.td3 as m
        return getattr(m, name)
    if name == "IDDPG":
        from core.iddpg import IDDPG
        return IDDPG
    if name == "MADDPG":
        from core.maddpg import MADDPG
        return MADDPG
    if name == "BCQ":
        from core.bcq import BCQ
        return BCQ
    if name == "TD3BC":
        from core.td3bc import TD3BC
        return TD3BC
    if name == "CQL":
        from core.cql import CQL
        return CQL
    if name == "IQL":
        from core.iql import IQL
        return IQL
    if name == "PPO":
        from core.ppo import PPO
        return PPO
    if name == "A2C":
        from core.a2c import A2C
        return A2C
    if name == "DQN":
        from core.dqn import DQN
        return DQN
    if name == "QRDQN":
        from core.qrdqn import QRDQN
        return QRDQN
    if name == "ARS":
        from core.ars import ARS
        return ARS
    if name == "TRPO":
        from core.trpo import TRPO
        return TRPO
    if name == "HerReplayBuffer":
        from core.her import HerReplayBuffer
        return HerReplayBuffer
    raise AttributeError(f"module 'core' has no attribute {name!r}")
