"""CPU-side checks of the n-step sampler: exports, host argument checks (never-dereferenced fake pointers), constructor refusals."""
import ctypes as C
import inspect
import os

import pytest

from conftest import ROOT
from core import _native as nv

NAMES = ("cstr_replay_sample_nstep_mt19937_f32", "cstr_replay_sample_nstep_packed_mt19937_f32", "cstr_replay_gather_nstep_packed_f32")
NULL, FAKE, ODD = C.c_void_p(None), C.c_void_p(0x1000), C.c_void_p(0x1004)


def ring(obs_dim=4, act_dim=2):
    return nv.Ring(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 8, 3, obs_dim, act_dim)


def call(name, n_steps=3, batch=8, first=FAKE, ring_=None, ctl=FAKE, src=FAKE):
    """`first`: out_obs / x_data; `src`: mt_state of the sampling forms, sample_idx of the gather"""
    lib, r, g = nv.lib(), ring_ or ring(), nv.NStepGpow.of(0.9)
    tail = (C.c_int64(batch), n_steps, g, first, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL, NULL)
    if name == NAMES[2]:
        return lib.cstr_replay_gather_nstep_packed_f32(C.byref(r), ctl, 0, NULL, C.c_uint64(0), src, *tail)
    return getattr(lib, name)(C.byref(r), ctl, src, *tail)


@pytest.mark.parametrize("name", NAMES)
def test_exported_declared_and_checked_on_the_host(name):
    assert name in nv.SYMBOLS and hasattr(nv.lib(), name)
    assert name + "(" in open(os.path.join(ROOT, "include", "cstr_rl_hip.h")).read()
    assert call(name, first=NULL) == -1 and call(name, first=ODD) == -1 and call(name, ctl=NULL) == -1 and call(name, src=NULL) == -1
    assert call(name, n_steps=0) == -2 and call(name, n_steps=17) == -2
    assert call(name, ring_=ring(4, 4)) == -2 and call(name, ring_=ring(5, 2)) == -2
    assert call(name, batch=nv.MAX_SAMPLE_BATCH + 1) == -2 and call(name, batch=0) == -1
    assert nv.lib().cstr_abi_version() == 5


def test_public_names_and_refusals():
    import core
    from core.common.buffers import NStepReplayBuffer, PrioritizedReplayBuffer, ReplayBuffer
    from core.common.off_policy_algorithm import OffPolicyAlgorithm
    from core.common.type_aliases import NStepReplayBufferSamples, ReplayBufferSamples
    from core.her import HerReplayBuffer
    from core.maddpg import MADDPG

    assert "NStepReplayBuffer" in core.__all__ and core.NStepReplayBuffer is NStepReplayBuffer and issubclass(NStepReplayBuffer, ReplayBuffer)
    assert NStepReplayBufferSamples._fields == ReplayBufferSamples._fields + ("discounts", "fold")
    for bad in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="n_steps"):
            NStepReplayBuffer._check_n_steps(bad)
        with pytest.raises(ValueError, match="n_steps"):
            core.SAC("MlpPolicy", None, n_steps=bad)
    for cls, what in ((PrioritizedReplayBuffer, "Prioritized"), (HerReplayBuffer, "Her")):
        with pytest.raises(NotImplementedError, match=what):
            core.DQN("MlpPolicy", None, n_steps=3, replay_buffer_class=cls)
    with pytest.raises(NotImplementedError, match="multi-agent"):
        MADDPG._check_n_step_buffer(3, None, None)
    for name in ("BCQ", "TD3BC", "CQL", "IQL"):
        with pytest.raises(NotImplementedError, match="offline"):
            getattr(core, name)._check_n_step_buffer(1, NStepReplayBuffer, None)
    with pytest.raises(ValueError, match="disagree"):
        OffPolicyAlgorithm._check_n_step_buffer(3, NStepReplayBuffer, dict(n_steps=5))
    for cls in (core.SAC, core.TQC, core.TD3, core.DDPG, core.DQN, core.QRDQN):
        p = inspect.signature(cls).parameters["n_steps"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1
