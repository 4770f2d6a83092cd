"""`HerReplayBuffer` (reference: core/her/her_replay_buffer.py:15-409) for the goal face of `CSTRVecEnv`, stored in HBM and served by
the kernels of csrc/cstr_her.hip:

  * the (4, 2) replay ring holds `observation` / `next_observation`, actions, rewards, dones, timeouts; beside it live
    `desired_goal`, `ep_start`, `ep_length` [rows, n_envs] and `_current_ep_start` [n_envs]. Achieved goals are not stored: the goal
    has one dimension and is column 2 of the stored observation rows;
  * `add` / `add_device` is one launch at the device-resident ring position, episode bookkeeping included;
  * `sample` is one launch on the device image of NumPy's legacy MT19937 stream: the index draw of `np.random.choice`, the goal draw
    of the strategy, the relabelled goals and their rewards, bit for bit what the reference computes from the same buffer and stream.

`copy_info_dict=True` is refused (infos are not kept in HBM; the reward of this env needs none).
"""
import warnings
from typing import Any, Optional, Union

import numpy as np
import torch as th

from core.common import hip_ops
from core.common.buffers import ReplayBuffer
from core.common.spaces import Dict, get_action_dim
from core.common.type_aliases import DictReplayBufferSamples, ReplayBufferSamples
from core.common.utils import get_device
from core.common.vec_env.cstr_vec_env import GOAL_KEYS, goal_dict_to_rows
from core.her.goal_selection_strategy import KEY_TO_GOAL_STRATEGY, GoalSelectionStrategy

NO_EPISODE_MSG = ("Unable to sample before the end of the first episode. We recommend choosing a value "
                  "for learning_starts that is greater than the maximum number of timesteps in the environment.")  # :198-201
NO_ENV_MSG = "You must initialize HerReplayBuffer with a VecEnv so it can compute rewards for virtual transitions"  # :316-318


def _check_goal_env(env) -> None:
    if not getattr(getattr(env, "unwrapped", env), "goal_conditioned", False) or not hasattr(env, "coef"):
        raise ValueError("HerReplayBuffer needs the goal face of the env: CSTRVecEnv(num_envs, goal_conditioned=True)")


class HerReplayBuffer(ReplayBuffer):
    """reference: core/her/her_replay_buffer.py:15-99 (constructor signature, defaults and attributes)."""

    def __init__(self, buffer_size: int, observation_space, action_space, env, device: Union[th.device, str] = "auto", n_envs: int = 1,
                 optimize_memory_usage: bool = False, handle_timeout_termination: bool = True, n_sampled_goal: int = 4,
                 goal_selection_strategy: Union[GoalSelectionStrategy, str] = "future", copy_info_dict: bool = False,
                 sampler_stream: Optional[th.Tensor] = None):
        if not isinstance(observation_space, Dict) or tuple(observation_space.keys()) != GOAL_KEYS:
            raise ValueError(f"HerReplayBuffer needs the goal face's Dict observation space with keys {GOAL_KEYS}, got {observation_space!r}")
        if optimize_memory_usage:
            raise ValueError("DictReplayBuffer does not support optimize_memory_usage")  # the reference's DictReplayBuffer assertion
        if copy_info_dict:
            raise ValueError("copy_info_dict=True is not built: infos are not kept in HBM (the reward of the goal face needs none)")
        if env is not None:
            _check_goal_env(env)
        self.observation_space, self.action_space = observation_space, action_space
        self.obs_shape = {k: tuple(s.shape) for k, s in observation_space.items()}
        if (self.obs_shape["achieved_goal"], self.obs_shape["desired_goal"], self.obs_shape["observation"]) != ((1,), (1,), (4,)):
            raise ValueError(f"HerReplayBuffer supports the CSTR goal face (goal (1,), observation (4,)), got {self.obs_shape}")
        self.action_dim = get_action_dim(action_space)
        self.n_envs = n_envs
        self._adds = 0
        self.buffer_size = max(buffer_size // n_envs, 1)
        self.optimize_memory_usage, self.handle_timeout_termination = optimize_memory_usage, handle_timeout_termination
        self.env = env
        self.copy_info_dict = copy_info_dict
        if isinstance(goal_selection_strategy, str):  # :77-85
            key = goal_selection_strategy.lower()
            assert key in KEY_TO_GOAL_STRATEGY, f"Invalid goal selection strategy, please use one of {list(GoalSelectionStrategy)}"
            self.goal_selection_strategy = KEY_TO_GOAL_STRATEGY[key]
        else:
            self.goal_selection_strategy = goal_selection_strategy
        assert isinstance(self.goal_selection_strategy, GoalSelectionStrategy), \
            f"Invalid goal selection strategy, please use one of {list(GoalSelectionStrategy)}"
        self.n_sampled_goal = n_sampled_goal
        self.her_ratio = 1 - (1.0 / (self.n_sampled_goal + 1))  # :90
        self.device = get_device(device)
        self._stream = sampler_stream
        self.normalizer = None
        self._predrawn = None
        self._alloc()

    def _alloc(self) -> None:
        with th.cuda.device(self.device):
            self.ring = hip_ops.DeviceRing(self.buffer_size, self.n_envs, 4, self.action_dim, self.device)
            self.her = hip_ops.DeviceHer(self.ring, self.device)
        r = self.ring
        self.observations = {"observation": r.observations, "desired_goal": self.her.desired_goal}
        self.next_observations = {"observation": r.next_observations, "desired_goal": self.her.desired_goal}
        self.actions, self.rewards, self.dones, self.timeouts = r.actions, r.rewards, r.dones, r.timeouts

    # ---- the reference's bookkeeping attributes, readable as arrays (:97-99) ----------------------------------------------------
    @property
    def ep_start(self) -> np.ndarray:
        return self.her.ep_start.cpu().numpy().astype(np.int64)

    @property
    def ep_length(self) -> np.ndarray:
        return self.her.ep_length.cpu().numpy().astype(np.int64)

    @property
    def _current_ep_start(self) -> np.ndarray:
        return self.her.cur_ep_start.cpu().numpy().astype(np.int64)

    def nb_virtual(self, batch_size: int) -> int:
        return int(self.her_ratio * batch_size)  # :218

    @property
    def strategy_key(self) -> str:
        return self.goal_selection_strategy.name.lower()

    def set_env(self, env) -> None:
        """:124-133"""
        if self.env is not None:
            raise ValueError("Trying to set env of already initialized environment.")
        _check_goal_env(env)
        self.env = env

    # ---- pickling (:101-122): without the env; arrays as host NumPy with the reference's shapes -----------------------------------
    _HER_FIELDS = ("desired_goal", "ep_start", "ep_length", "cur_ep_start")

    def __getstate__(self) -> dict:
        st = {k: getattr(self, k) for k in ("buffer_size", "observation_space", "action_space", "obs_shape", "action_dim", "n_envs",
                                            "optimize_memory_usage", "handle_timeout_termination", "copy_info_dict", "goal_selection_strategy",
                                            "n_sampled_goal", "her_ratio")}
        r = self.ring
        st.update(observation=r.observations.cpu().numpy(), next_observation=r.next_observations.cpu().numpy(), actions=r.actions.cpu().numpy(),
                  rewards=r.rewards.cpu().numpy(), dones=r.dones.cpu().numpy(), timeouts=r.timeouts.cpu().numpy())
        st.update({k: getattr(self.her, k).cpu().numpy() for k in self._HER_FIELDS})
        st.update(pos=self.pos, full=self.full, adds=self._adds, device=str(self.device),
                  sampler_stream=None if self._stream is None else self._stream.cpu().numpy())
        return st

    def __setstate__(self, st: dict) -> None:
        assert "env" not in st
        for k in ("buffer_size", "observation_space", "action_space", "obs_shape", "action_dim", "n_envs", "optimize_memory_usage",
                  "handle_timeout_termination", "copy_info_dict", "goal_selection_strategy", "n_sampled_goal", "her_ratio"):
            setattr(self, k, st[k])
        self.device = get_device(st.get("device", "auto"))
        self.env = None
        self._alloc()
        r = self.ring
        for t, k in ((r.observations, "observation"), (r.next_observations, "next_observation"), (r.actions, "actions"), (r.rewards, "rewards"),
                     (r.dones, "dones"), (r.timeouts, "timeouts")):
            t.copy_(th.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(t.shape))
        self.her.desired_goal.copy_(th.from_numpy(np.ascontiguousarray(st["desired_goal"], dtype=np.float32)))
        for k in ("ep_start", "ep_length", "cur_ep_start"):
            getattr(self.her, k).copy_(th.from_numpy(np.ascontiguousarray(st[k], dtype=np.int32)))
        self.her.rebuild_summaries()
        self._adds = int(st["adds"])
        r.ctl.copy_(th.tensor([int(st["pos"]), int(bool(st["full"])), 0, self._adds], dtype=th.int64))
        ss = st.get("sampler_stream")
        self._stream = None if ss is None else th.from_numpy(np.ascontiguousarray(ss)).to(self.device)
        self.normalizer, self._predrawn = None, None

    def to(self, device) -> "HerReplayBuffer":
        device = get_device(device)
        if device != self.device:
            env, st = self.env, self.__getstate__()
            st["device"] = str(device)
            self.__setstate__(st)
            self.env = env
        return self

    def reset(self) -> None:
        super().reset()
        for t in (self.her.ep_start, self.her.ep_length, self.her.cur_ep_start, self.her.row_valid, self.her.valid_bits):
            t.zero_()

    # ---- add ----------------------------------------------------------------------------------------------------------------------
    def add_device(self, obs_rows: th.Tensor, next_rows: th.Tensor, action: th.Tensor, reward: th.Tensor, done: th.Tensor,
                   timeout: th.Tensor) -> None:
        """`add` on flat device rows [n_envs, 6] (what `CSTRVecEnv.step_device` returns on the goal face): one launch, no host sync."""
        with th.cuda.device(self.device):
            hip_ops.her_add(self.ring, self.her, obs_rows, next_rows, action, reward, done, timeout)
        self._adds += 1

    def add(self, obs: dict, next_obs: dict, action, reward, done, infos: Optional[list]) -> None:
        """:135-167 with dict observations, as the reference takes them. next_obs["desired_goal"] equals obs["desired_goal"] within an
        episode (the terminal observation keeps the old goal), so one goal array serves both."""
        n = self.n_envs
        if infos is None or not self.handle_timeout_termination:
            timeout = np.zeros(n, np.float32)
        elif isinstance(infos, (th.Tensor, np.ndarray)):
            timeout = infos
        else:
            timeout = np.array([info.get("TimeLimit.truncated", False) for info in infos])
        rows, nrows = goal_dict_to_rows(obs).reshape(n, hip_ops.GOAL_ROW), goal_dict_to_rows(next_obs).reshape(n, hip_ops.GOAL_ROW)
        self.add_device(self._dev(rows, (n, hip_ops.GOAL_ROW)), self._dev(nrows, (n, hip_ops.GOAL_ROW)), self._dev(action, (n, self.action_dim)),
                        self._dev(reward, (n,)), self._dev(done, (n,)), self._dev(timeout, (n,)))

    def note_fused_add(self) -> None:
        """The goal face's fused collect launch (hip_ops.goal_collect_step) wrote a row with its episode bookkeeping and advanced the
        device position: keep the host mirror (`pos` / `full` follow `_adds`) in step, as `add_device` does."""
        self._adds += 1

    # ---- sample -------------------------------------------------------------------------------------------------------------------
    def alloc_batch(self, batch_size: int) -> ReplayBufferSamples:
        """The contiguous batch the learner uses: observations / next_observations are flat rows [B, 6]."""
        e = lambda *s: th.empty(*s, dtype=th.float32, device=self.device)  # noqa: E731
        w = hip_ops.GOAL_ROW
        return ReplayBufferSamples(e(batch_size, w), e(batch_size, self.action_dim), e(batch_size, w), e(batch_size, 1), e(batch_size, 1))

    def sample_into(self, out: ReplayBufferSamples, row_idx=None, env_idx=None, env=None, goal_row=None, forced=None,
                    check: bool = False) -> ReplayBufferSamples:
        """`sample` into caller-owned tensors. row_idx / env_idx / goal_row: optional int64 [B] outputs (output order: real transitions
        first). forced = (rows, envs) or (rows, envs, goal_rows), int64 [B] device tensors in draw order: teacher-forced sampling.
        check=True reads one device word back and raises the reference's RuntimeError when no episode has ended yet; the training path
        checks once when training starts."""
        if env is not None or self.normalizer is not None:
            raise ValueError("HerReplayBuffer does not go through VecNormalize")
        assert self.env is not None, NO_ENV_MSG
        batch = out.observations.shape[0]
        f_row, f_env, f_goal = (tuple(forced) + (None,))[:3] if forced is not None else (None, None, None)
        with th.cuda.device(self.device):
            hip_ops.her_sample(self.env.coef, self.ring, self.her, self.sampler_stream, batch, self.nb_virtual(batch), self.strategy_key,
                               out.observations, out.actions, out.next_observations, out.dones, out.rewards, row_idx, env_idx, goal_row,
                               f_row, f_env, f_goal)
        if check and forced is None:
            self.check_can_sample()
        return out

    def check_can_sample(self) -> None:
        """Raises the reference's error (:197-201) if the last launch found no valid transition. One device word is read back."""
        if int(self.her.status.item()) != 0:
            raise RuntimeError(NO_EPISODE_MSG)

    def has_valid_transition(self) -> bool:
        """np.any(ep_length > 0) from the sampler's own summary (a host read)."""
        return bool(int(self.her.row_valid.sum().item()) > 0)

    @staticmethod
    def as_dict_samples(flat: ReplayBufferSamples) -> DictReplayBufferSamples:
        """Dict entries are column views of the flat rows."""
        cut = lambda x: {"achieved_goal": x[:, 0:1], "desired_goal": x[:, 1:2], "observation": x[:, 2:6]}  # noqa: E731
        return DictReplayBufferSamples(cut(flat.observations), flat.actions, cut(flat.next_observations), flat.dones, flat.rewards)

    def sample(self, batch_size: int, env: Any = None) -> DictReplayBufferSamples:
        """:186-246"""
        return self.as_dict_samples(self.sample_into(self.alloc_batch(batch_size), env=env, check=True))

    def sample_with_indices(self, batch_size: int, forced=None):
        i64 = lambda: th.empty(batch_size, dtype=th.int64, device=self.device)  # noqa: E731
        bi, ei, gi = i64(), i64(), i64()
        return self.sample_into(self.alloc_batch(batch_size), bi, ei, goal_row=gi, forced=forced, check=True), bi, ei, gi

    def alloc_packed_batch(self, batch_size: int, with_pi: bool = True):
        raise ValueError("HerReplayBuffer has no packed batches; use alloc_batch / sample_into")

    def sample_packed_into(self, pb, row_idx=None, env_idx=None):
        raise ValueError("HerReplayBuffer has no packed batches; use alloc_batch / sample_into")

    # ---- truncate_last_trajectory (:386-408), on the host: it runs once after load_replay_buffer ---------------------------------
    def truncate_last_trajectory(self) -> None:
        cur, pos, rows = self._current_ep_start, self.pos, self.buffer_size
        if (cur != pos).any():
            warnings.warn(
                "The last trajectory in the replay buffer will be truncated.\n"
                "If you are in the same episode as when the replay buffer was saved,\n"
                "you should use `truncate_last_trajectory=False` to avoid that issue."
            )
            ep_length = self.ep_length
            for env_idx in np.where(cur != pos)[0]:
                self.dones[pos - 1, env_idx] = 1.0  # :402 (a negative index wraps like NumPy's)
                start, end = int(cur[env_idx]), pos  # _compute_episode_length (:169-184)
                if end < start:
                    end += rows
                ep_length[np.arange(start, end) % rows, env_idx] = end - start
                cur[env_idx] = pos
                if self.handle_timeout_termination:
                    self.timeouts[pos - 1, env_idx] = 1.0  # :407-408
            self.her.ep_length.copy_(th.from_numpy(ep_length.astype(np.int32)))
            self.her.cur_ep_start.copy_(th.from_numpy(cur.astype(np.int32)))
            self.her.rebuild_summaries()
