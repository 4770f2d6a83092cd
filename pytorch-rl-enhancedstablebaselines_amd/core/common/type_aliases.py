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
