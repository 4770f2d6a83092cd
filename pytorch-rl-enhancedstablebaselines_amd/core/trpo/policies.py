"""TRPO's policy alias: PPO's `MlpPolicy` (core.common.policies.ActorCriticPolicy; separate `pi` / `vf` trunks by default, so actor and
critic share no trainable parameter). The goal face ("MultiInputPolicy") and the CNN policies are not built."""
from core.ppo.policies import MlpPolicy

__all__ = ["MlpPolicy"]
