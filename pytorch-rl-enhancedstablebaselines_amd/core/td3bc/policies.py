"""TD3+BC's policy: TD3's `TD3Policy` (same modules, same construction order, same state_dict) that normalises the observations it
is asked to act on with the dataset's statistics. `MlpPolicy` only."""
from typing import Optional, Tuple

import torch as th

from core.td3.policies import TD3Policy


class TD3BCPolicy(TD3Policy):
    # TD3BC sets both: `normalize_states` says the networks were trained on normalised observations, `obs_norm` = (mean, std) float32
    # device rows. Plain attributes, not buffers: the state_dict stays TD3Policy's (the statistics travel in the archive's data).
    normalize_states: bool = False
    obs_norm: Optional[Tuple[th.Tensor, th.Tensor]] = None

    def normalize_obs(self, observation: th.Tensor) -> th.Tensor:
        if not self.normalize_states:
            return observation
        if self.obs_norm is None:
            raise RuntimeError("TD3BCPolicy: normalize_states is set but the dataset statistics are missing")
        mean, std = self.obs_norm
        return (observation - mean.to(observation.device)) / std.to(observation.device)

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        return self.actor(self.normalize_obs(observation))


MlpPolicy = TD3BCPolicy
