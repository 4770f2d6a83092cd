"""`collect_offline_dataset` (reference: experiments/basic_test/HalfCheetah_TD3_offline_collect.py:17-139): roll a trained controller
out, with a share of uniformly random actions, into a `ReplayBuffer` that `BCQ(dataset=...)` trains on.

The reference's script loads a model from a path, builds a one-env `DummyVecEnv` and loops `predict` / `step` / `add` on the host. Here
the model object and a `CSTRVecEnv` are passed in and the whole collection is ONE launch (cstr_collect_episodes_f32): the policy
network, the exploration draw, the env step, the ring row and the episode accounting of every vec-step happen inside the kernel, for
all envs. There is no host-loop fallback: a (model, env) pair the launch does not cover raises ValueError.

Deviations from the script, both deliberate:
  * next_observations holds the TERMINAL observation at an episode's end -- what `OffPolicyAlgorithm._store_transition` and every collect
    kernel of this package store -- where the script stores `vec_env.step`'s return value, i.e. the observation after the auto-reset;
  * the random share comes from a counter-based Philox stream keyed by `seed` (one block per (env, step)), not from NumPy's global stream.
"""
import json
import os
from typing import Optional, Tuple

import numpy as np
import torch as th

from core.common import evaluation
from core.common.buffers import ReplayBuffer
from core.common.save_util import save_to_pkl


def episode_stats(num_episodes: int, total_transitions: int, returns: np.ndarray) -> dict:
    """The script's `stats` dict (:116-123) over the returns of the episodes that ended."""
    r = np.asarray(returns, np.float64)
    return dict(num_episodes=int(num_episodes), total_transitions=int(total_transitions), mean_reward=float(np.mean(r)), std_reward=float(np.std(r)),
                min_reward=float(np.min(r)), max_reward=float(np.max(r)))


def ended_returns(ep_return: np.ndarray, ep_done: np.ndarray, rewards, dones) -> np.ndarray:
    """Returns of the episodes that ended, from the launch's [N, ep_stride] slots; where an env ended more episodes than it has slots
    (only an env on the NaN path does: every step ends one), recomputed in float64 from the recorded `rewards` / `dones` [T, N]
    (callables returning them, so that the ring is only read back when needed)."""
    ep_done = np.asarray(ep_done)
    if (ep_done > ep_return.shape[1]).any():
        return evaluation.segment_episodes(rewards(), dones())[1]
    return np.concatenate([ep_return[i, :ep_done[i]] for i in range(ep_done.shape[0])]) if ep_done.sum() else np.zeros(0)


def collect_offline_dataset(model, env, num_episodes: int = 100, random_action_prob: float = 0.1, use_mixed_policy: bool = True,
                            dataset_path: Optional[str] = None, dataset_name: str = "offline_dataset", seed: int = 0) -> Tuple[ReplayBuffer, dict]:
    """Roll `model`'s deterministic policy out on `env` (a bare Box-face `CSTRVecEnv`), replacing the action of a step by a uniform draw
    over the action space with probability `random_action_prob` (never, with `use_mixed_policy=False`), and return (replay_buffer, stats).

    The env is reset; every env then runs T = ceil(num_episodes / n_envs) * max_steps vec-steps in one launch into a fresh
    `ReplayBuffer(T * n_envs, n_envs=n_envs)` whose every row is valid (`pos == 0`, `full`). `stats` has the script's keys: `num_episodes`
    = episodes that ENDED (at least the request; more only when NaN actions end episodes early), `total_transitions` = T * n_envs,
    `mean_reward` / `std_reward` / `min_reward` / `max_reward` over the ended episodes' returns (float64 sums of the float32 rewards).
    With `dataset_path` the buffer is written to `<dataset_path>/<dataset_name>_buffer.pkl` (`save_to_pkl`) and the stats to
    `<dataset_name>_stats.json`. Supported: SAC without gSDE, TD3 / DDPG, PPO / A2C with a two-layer `policy_net`; anything else raises
    ValueError naming the reason."""
    why = evaluation._why_not_collected(model, env)
    if why is not None:
        raise ValueError(f"collect_offline_dataset does not cover {why}")
    if int(num_episodes) <= 0:
        raise ValueError(f"num_episodes must be positive, got {num_episodes}")
    prob = float(random_action_prob) if use_mixed_policy else 0.0
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"random_action_prob = {random_action_prob} is not a probability")
    n, limit = env.num_envs, int(env.coef.max_steps)
    n_steps = -(-int(num_episodes) // n) * limit
    rb = ReplayBuffer(n_steps * n, env.observation_space, env.action_space, device=env.device, n_envs=n)
    env.reset_device()
    ep_return, _, ep_done = evaluation._collect_launch(model, env, rb.ring, n_steps, explore_prob=prob, seed=seed, ep_stride=n_steps // limit + 1)
    rb._adds = rb.buffer_size  # every row is valid: pos = 0, full (what from_arrays sets)
    rb.ring.ctl.copy_(th.tensor([0, 1, 0, rb._adds], dtype=th.int64))
    returns = ended_returns(ep_return, ep_done, lambda: rb.rewards.cpu().numpy(), lambda: rb.dones.cpu().numpy())
    stats = episode_stats(returns.shape[0], n_steps * n, returns)
    if dataset_path is not None:
        os.makedirs(dataset_path, exist_ok=True)
        save_to_pkl(os.path.join(dataset_path, f"{dataset_name}_buffer.pkl"), rb)
        with open(os.path.join(dataset_path, f"{dataset_name}_stats.json"), "w") as f:
            json.dump(stats, f, indent=4)
    return rb, stats
