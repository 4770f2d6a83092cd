"""Named tuples of the reference API (core/common/type_aliases.py:49-101); field order is API."""
from enum import Enum
from typing import NamedTuple

import torch as th


class ReplayBufferSamples(NamedTuple):
    observations: th.Tensor
    actions: th.Tensor
    next_observations: th.Tensor
    dones: th.Tensor
    rewards: th.Tensor


class PrioritizedReplayBufferSamples(NamedTuple):
    """What PrioritizedReplayBuffer samples: the five fields, the importance weights [B, 1] and the sum-tree leaf of every row [B]
    (leaf = ring row * n_envs + env), which `update_priorities` takes back."""
    observations: th.Tensor
    actions: th.Tensor
    next_observations: th.Tensor
    dones: th.Tensor
    rewards: th.Tensor
    weights: th.Tensor
    leaf_indices: th.Tensor


class NStepReplayBufferSamples(NamedTuple):
    """What NStepReplayBuffer samples: the five fields (rewards = the discounted n-step return, next_observations / dones of the step
    the window ends at), then `discounts` [B, 1] = gamma^m for a window of m steps and `fold` [B, 1] = 1 - (1 - dones) gamma^(m-1):
    the value a TD-target launch with a scalar gamma takes in place of `dones`, (1 - fold) gamma == (1 - dones) discounts."""
    observations: th.Tensor
    actions: th.Tensor
    next_observations: th.Tensor
    dones: th.Tensor
    rewards: th.Tensor
    discounts: th.Tensor
    fold: th.Tensor


def td_done(samples) -> th.Tensor:
    """The termination operand of the TD-target launches: `fold` of an n-step sample, `dones` of every other one."""
    return getattr(samples, "fold", samples.dones)


def td_discount(samples, gamma: float):
    """The discount of the torch-statement targets, rewards + (1 - dones) * discount * next_q: `discounts` of an n-step sample, else gamma."""
    return getattr(samples, "discounts", gamma)


class DictReplayBufferSamples(NamedTuple):
    """reference: core/common/type_aliases.py (DictReplayBufferSamples); observations / next_observations: {key: tensor}"""
    observations: dict
    actions: th.Tensor
    next_observations: dict
    dones: th.Tensor
    rewards: th.Tensor


class RolloutBufferSamples(NamedTuple):
    observations: th.Tensor
    actions: th.Tensor
    old_values: th.Tensor
    old_log_prob: th.Tensor
    advantages: th.Tensor
    returns: th.Tensor


class DictRolloutBufferSamples(NamedTuple):
    """reference: core/common/type_aliases.py (DictRolloutBufferSamples); observations: {key: tensor}"""
    observations: dict
    actions: th.Tensor
    old_values: th.Tensor
    old_log_prob: th.Tensor
    advantages: th.Tensor
    returns: th.Tensor


class GoalRolloutBufferSamples(DictRolloutBufferSamples):
    """What DictRolloutBuffer.get() yields: the reference's six fields, and beside them `rows` [batch, 6], the flat rows the dict's
    tensors are column views of (what the kernels read)."""
    rows: th.Tensor = None


class RolloutReturn(NamedTuple):
    episode_timesteps: int
    n_episodes: int
    continue_training: bool


class TrainFrequencyUnit(Enum):
    STEP = "step"
    EPISODE = "episode"


class TrainFreq(NamedTuple):
    frequency: int
    unit: TrainFrequencyUnit
