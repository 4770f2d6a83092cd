"""`OfflineAlgorithm`: learning from a fixed replay dataset, no rollouts
(reference: core/common/offline_policy_algorithm.py:52-371).

Dataset forms (reference: a path to a pickled ReplayBuffer, :196-242): a pickle written by this package's `save_replay_buffer` /
`save_to_pkl`; a `ReplayBuffer` of this package (the reference reads `self.verbose` before its base constructor ran and dies on an
object, :134-137: accepting it is the fix); an `.npz` with the reference's array names and shapes (`read_npz_dataset`). A pickle
written by the reference holds gymnasium objects and is not loadable here. The loaded buffer REPLACES `self.replay_buffer`
(:237-238), so the dataset's own `n_envs` and size apply."""
import os
import pathlib
import sys
import time
import warnings
from typing import Optional, Union

import numpy as np

from core.common.buffers import ReplayBuffer
from core.common.callbacks import BaseCallback, MaybeCallback
from core.common.off_policy_algorithm import OffPolicyAlgorithm

NPZ_FIELDS = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")


def check_dataset_arg(dataset) -> None:
    """reference :187-194 (type) and :209-210 (existence), on the host before anything is built"""
    if isinstance(dataset, (str, pathlib.Path)):
        if not os.path.exists(dataset):
            raise FileNotFoundError(f"Dataset file not found: {dataset}")
    elif not isinstance(dataset, ReplayBuffer):
        raise ValueError(f"Dataset must be a path string or a ReplayBuffer instance, got {type(dataset)}")


def read_npz_dataset(path) -> dict:
    """The portable dataset form: `observations`, `next_observations` [R, N, D], `actions` [R, N, A], `rewards`, `dones`, `timeouts`
    [R, N] (the reference's ReplayBuffer attributes, core/common/buffers.py:212-234), optional `pos` and `full` (absent: every row
    is valid). Returns host float32 arrays + pos / full; raises ValueError on a missing name or a shape that does not fit."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in NPZ_FIELDS if k not in z.files]
        if missing:
            raise ValueError(f"dataset {path}: missing arrays {missing} (needs {list(NPZ_FIELDS)})")
        out = {k: np.ascontiguousarray(z[k], dtype=np.float32) for k in NPZ_FIELDS}
        pos = int(z["pos"]) if "pos" in z.files else 0
        full = bool(z["full"]) if "full" in z.files else "pos" not in z.files
    obs = out["observations"]
    if obs.ndim != 3:
        raise ValueError(f"dataset {path}: observations must be [rows, n_envs, obs_dim], got shape {obs.shape}")
    r, n, _ = obs.shape
    if out["next_observations"].shape != obs.shape:
        raise ValueError(f"dataset {path}: next_observations {out['next_observations'].shape} != observations {obs.shape}")
    if out["actions"].ndim != 3 or out["actions"].shape[:2] != (r, n):
        raise ValueError(f"dataset {path}: actions must be [{r}, {n}, act_dim], got shape {out['actions'].shape}")
    for k in ("rewards", "dones", "timeouts"):
        if out[k].shape != (r, n):
            raise ValueError(f"dataset {path}: {k} must be [{r}, {n}], got shape {out[k].shape}")
    if r == 0 or n == 0:
        raise ValueError(f"dataset {path}: no rows (observations has shape {obs.shape})")
    if not 0 <= pos < r:
        raise ValueError(f"dataset {path}: pos {pos} outside [0, {r})")
    out.update(pos=pos, full=full)
    return out


def buffer_from_arrays(arrays: dict, observation_space, action_space, device) -> ReplayBuffer:
    """An HBM ReplayBuffer holding `read_npz_dataset`'s arrays (rows, n_envs and widths from the arrays themselves)."""
    obs, act = arrays["observations"], arrays["actions"]
    r, n, d = obs.shape
    a = act.shape[2]
    if tuple(observation_space.shape) != (d,) or int(np.prod(action_space.shape)) != a:
        raise ValueError(f"dataset has obs_dim {d} / act_dim {a}, the env has {tuple(observation_space.shape)} / {tuple(action_space.shape)}")
    return ReplayBuffer.from_arrays(observation_space, action_space, device, pos=int(arrays["pos"]), full=bool(arrays["full"]),
                                    **{k: arrays[k] for k in NPZ_FIELDS})


class OfflineAlgorithm(OffPolicyAlgorithm):
    """reference :52-371. `behavior_cloning_warmup`, `conservative_weight` and `n_eval_episodes` are stored; what the reference does
    with them is the subclass's."""

    def __init__(self, policy, env, learning_rate, dataset: Union[str, ReplayBuffer, None] = None, buffer_size: int = 1_000_000,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, gradient_steps: int = 1, dataset_buffer_class=None,
                 dataset_buffer_kwargs: Optional[dict] = None, n_eval_episodes: int = 10, behavior_cloning_warmup: int = 0,
                 conservative_weight: float = 0.0, policy_kwargs: Optional[dict] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, verbose: int = 0, device="auto", support_multi_env: bool = False,
                 monitor_wrapper: bool = True, seed: Optional[int] = None, use_sde: bool = False, sde_sample_freq: int = -1,
                 sde_support: bool = False, supported_action_spaces: Optional[tuple] = None):
        check_dataset_arg(dataset)
        if env is None:  # the reference dies in set_random_seed without one (its DummyEnv branch needs the object it crashes on)
            raise ValueError("an offline algorithm needs `env` (ONE environment): its spaces define the networks")
        if isinstance(dataset, ReplayBuffer):
            buffer_size = max(buffer_size, int(dataset.size() * 1.1))  # :134-135
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, buffer_size=buffer_size, learning_starts=0,
                         batch_size=batch_size, tau=tau, gamma=gamma, train_freq=(1, "step"), gradient_steps=gradient_steps,
                         action_noise=None, replay_buffer_class=dataset_buffer_class, replay_buffer_kwargs=dataset_buffer_kwargs,
                         policy_kwargs=policy_kwargs, stats_window_size=stats_window_size, tensorboard_log=tensorboard_log,
                         verbose=verbose, device=device, support_multi_env=support_multi_env, monitor_wrapper=monitor_wrapper,
                         seed=seed, use_sde=use_sde, sde_sample_freq=sde_sample_freq, use_sde_at_warmup=False, sde_support=sde_support,
                         supported_action_spaces=supported_action_spaces)
        self.dataset = dataset
        self.n_eval_episodes = n_eval_episodes
        self.behavior_cloning_warmup = behavior_cloning_warmup
        self.conservative_weight = conservative_weight
        self.bc_loss = None
        self._n_updates = 0

    # ---- dataset ---------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        """reference :180-194. The dataset is resolved FIRST: it replaces the replay buffer anyway (:237-238), so the
        `buffer_size`-row ring the reference allocates and drops is never built in HBM."""
        if isinstance(self.dataset, ReplayBuffer):
            self._copy_dataset_to_buffer(self.dataset)
        else:
            self.load_dataset(self.dataset)
        super()._setup_model()

    def load_dataset(self, path) -> None:
        """reference :196-221"""
        if self.verbose > 0:
            print(f"Loading dataset from {path}")
        check_dataset_arg(path)
        try:
            if str(path).endswith(".npz"):
                source = buffer_from_arrays(read_npz_dataset(path), self.observation_space, self.action_space, self.device)
            else:
                from core.common.save_util import load_from_pkl

                source = load_from_pkl(path, self.verbose)
            self._copy_dataset_to_buffer(source)
        except FileNotFoundError:
            raise
        except Exception as e:  # noqa: BLE001  (:217-221)
            raise ValueError(f"Dataset loading failed. Error type: {type(e).__name__}, Message: {e}") from e

    def _copy_dataset_to_buffer(self, source_buffer) -> None:
        """reference :223-242"""
        if source_buffer is None or not isinstance(source_buffer, ReplayBuffer):
            raise ValueError("Incompatible buffer types")
        if source_buffer.size() == 0:
            raise ValueError("Loaded dataset is empty")
        self.replay_buffer = source_buffer.to(self.device)
        self._graph = None  # captured graphs hold the old ring's pointers
        if self.verbose > 0:
            print(f"Finished copying dataset. Replay buffer contains {self.replay_buffer.size()} transitions")

    # ---- learn -----------------------------------------------------------------------------------------------------
    def learn(self, total_timesteps: int, callback: MaybeCallback = None, log_interval: int = 4, tb_log_name: str = "run",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        """reference :244-301: per iteration train(gradient_steps), num_timesteps += n_envs, the callback, the log cadence."""
        total_timesteps, callback = self._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)
        callback.on_training_start(locals(), globals())
        if self.behavior_cloning_warmup > 0:
            self._behavior_cloning_warmup(callback)
        while self.num_timesteps < total_timesteps:
            if not self._learn_iteration(callback, log_interval):
                break
        callback.on_training_end()
        return self

    def _eager_iteration(self, callback: BaseCallback, log_interval: Optional[int]) -> bool:
        self.train(gradient_steps=self.gradient_steps, batch_size=self.batch_size)
        self.num_timesteps += self.n_envs
        self._update_current_progress_remaining(self.num_timesteps, self._total_timesteps)
        self._on_step()
        if not getattr(callback, "is_noop", False):
            callback.update_locals(locals())
        if not callback.on_step():
            return False
        if log_interval is not None and self.num_timesteps % log_interval == 0:
            self._dump_logs()
        return True

    # ---- hipGraph hooks (core/common/graph_replay.py): one replay = one iteration's gradient steps, no rollout ------------
    def _graph_eligible(self, callback: BaseCallback) -> bool:
        return (type(self.replay_buffer) is ReplayBuffer and self._callback_allows_replay(callback) and self.gradient_steps >= 1
                and getattr(self, "fused_learner", False) and not getattr(self, "debug_capture", False))

    def _graph_cache_key(self, unroll: int) -> tuple:
        return (id(self.replay_buffer.ring), self.batch_size, self.gradient_steps, self._graph_phase(), unroll)

    def _graph_body(self) -> None:
        self.policy.set_training_mode(True)
        self._train_device_only(self.gradient_steps, self.batch_size)

    def _graph_host_bookkeeping(self, log_interval: Optional[int]) -> None:
        self.num_timesteps += self.n_envs
        self._update_current_progress_remaining(self.num_timesteps, self._total_timesteps)
        self._train_host_only(self.gradient_steps)
        if log_interval is not None and self.num_timesteps % log_interval == 0:
            self._dump_logs()

    def _behavior_cloning_warmup(self, callback: BaseCallback) -> None:
        raise NotImplementedError("Subclasses must implement _behavior_cloning_warmup method")  # :303-310

    def _behavior_cloning_update(self, observations: np.ndarray, actions: np.ndarray) -> float:
        raise NotImplementedError("Subclasses must implement _behavior_cloning_update method")  # :312-321

    def collect_rollouts(self, env, callback, train_freq, replay_buffer, action_noise=None, learning_starts: int = 0,
                         log_interval: Optional[int] = None) -> None:
        """reference :333-349"""
        warnings.warn("Offline RL algorithms do not collect rollouts during training. "
                      "Use learn() directly or evaluate() to assess the trained policy.")

    def _dump_logs(self) -> None:
        """reference :351-370"""
        time_elapsed = max((time.time_ns() - self.start_time) / 1e9, sys.float_info.epsilon)
        fps = int((self.num_timesteps - self._num_timesteps_at_start) / time_elapsed)
        self.logger.record("time/fps", fps)
        self.logger.record("time/time_elapsed", int(time_elapsed), exclude="tensorboard")
        self.logger.record("time/total_timesteps", self.num_timesteps, exclude="tensorboard")
        self.logger.record("dataset/size", self.replay_buffer.size())
        self.logger.record("training/bc_warmup_steps", self.behavior_cloning_warmup)
        if hasattr(self, "conservative_weight"):
            self.logger.record("training/conservative_weight", self.conservative_weight)
        self.logger.dump(step=self.num_timesteps)
