"""`BaseAlgorithm`: constructor contract, env wrapping, seeding, lr schedule, learn-time bookkeeping
(reference: core/common/base_class.py:69-889; only what the off-policy CSTR path touches), and save/load in the
reference's zip layout (core/common/save_util.py)."""
import time
from collections import deque
from typing import Any, Optional, Union

import numpy as np
import torch as th

from core.common import distributed as dist_util
from core.common.callbacks import BaseCallback, MaybeCallback, to_callback
from core.common.logger import Logger, configure_logger
from core.common.spaces import Box, Discrete, MultiDiscrete, as_box, as_discrete, as_multi_discrete
from core.common.utils import get_device, get_schedule_fn, set_random_seed, update_learning_rate
from core.common.vec_env import CSTRVecEnv, VecEnv, unwrap_vec_normalize


class BaseAlgorithm:
    policy_aliases: dict = {}
    goal_face_support = False  # SAC, TD3, DDPG (HER), PPO, A2C: the goal face of CSTRVecEnv (a Dict observation space)
    goal_space = None          # that Dict space; `observation_space` is then the Box of its flat row, which is what the learner sees

    def _accept_goal_face(self, policy, env) -> None:
        """The env has a Dict observation space (reference: base_class.py:206-210 and what this stack builds of HER)."""
        from core.common.policies import MultiInputMixin

        name = type(self).__name__
        if not self.goal_face_support:
            raise ValueError(f"{name} does not support a Dict observation space (the goal face of the env): HER is built for SAC, TD3 and DDPG, "
                             "and PPO and A2C take the face with `MultiInputPolicy`")
        if not (isinstance(self.policy_class, type) and issubclass(self.policy_class, MultiInputMixin)):
            raise ValueError(self._goal_face_policy_message(policy))
        inner = getattr(env, "unwrapped", env)
        if unwrap_vec_normalize(env) is not None or not (isinstance(inner, CSTRVecEnv) and inner is env and inner.goal_conditioned):
            raise ValueError(f"{name} on a Dict observation space needs a bare CSTRVecEnv(goal_conditioned=True): VecNormalize and other "
                             "wrappers are not built for the goal face")
        if self.world_size > 1:
            raise ValueError(f"{name} on the goal face does not run data-parallel (world_size = {self.world_size})")
        if self.use_sde:
            raise ValueError(f"{name} on the goal face does not support gSDE (use_sde=True)")
        self.goal_space = env.observation_space
        one = np.ones(self.goal_space.flat_dim(), np.float32)
        self.observation_space = Box(-one, one, dtype=np.float32)

    def _goal_face_policy_message(self, policy) -> str:
        """what a policy without the CombinedExtractor is told on a Dict observation space (reference: base_class.py:210)"""
        return f"You must use `MultiInputPolicy` when working with dict observation space, not {policy}"

    def __init__(self, policy, env, learning_rate, policy_kwargs: Optional[dict] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, verbose: int = 0, device: Union[th.device, str] = "auto",
                 support_multi_env: bool = False, monitor_wrapper: bool = True, seed: Optional[int] = None,
                 use_sde: bool = False, sde_sample_freq: int = -1, supported_action_spaces: Optional[tuple] = None):
        if isinstance(policy, str):
            self.policy_class = self._get_policy_from_name(policy)
        else:
            self.policy_class = policy
        self.device = get_device(device)
        self.verbose = verbose
        self.policy_kwargs = {} if policy_kwargs is None else policy_kwargs
        self.num_timesteps = 0
        self._total_timesteps = 0
        self._num_timesteps_at_start = 0
        self.seed = seed
        self.action_noise = None
        self.start_time = 0
        self.learning_rate = learning_rate
        self.tensorboard_log = tensorboard_log
        self._last_obs = None
        self._last_episode_starts = None
        self._last_original_obs = None
        self._episode_num = 0
        self.use_sde, self.sde_sample_freq = use_sde, sde_sample_freq
        self._current_progress_remaining = 1.0
        self._stats_window_size = stats_window_size
        self.ep_info_buffer: Optional[deque] = None
        self.ep_success_buffer: Optional[deque] = None
        self._n_updates = 0
        self._custom_logger = False
        self._logger: Optional[Logger] = None
        self._vec_normalize_env = None
        self.rank, self.world_size = dist_util.rank_world()
        self.env: Optional[VecEnv] = None
        self.policy = None
        if env is not None:
            env = self._wrap_env(env, self.verbose)
            if isinstance(getattr(env.observation_space, "spaces", None), dict):
                self._accept_goal_face(policy, env)
            else:
                self.observation_space = as_box(env.observation_space)
            self.action_space = self._as_action_space(env.action_space)
            self.n_envs = env.num_envs
            self.env = env
            self._vec_normalize_env = unwrap_vec_normalize(env)  # reference base_class.py:195
            # reference base_class.py:202-208: a class that names Discrete alone (DQN) takes a Discrete space and nothing else, one that
            # names "Box" and Discrete (PPO, A2C) takes either; every other class takes a Box
            wants_discrete = supported_action_spaces is not None and Discrete in supported_action_spaces
            wants_box = not wants_discrete or "Box" in supported_action_spaces
            if isinstance(self.action_space, MultiDiscrete):  # PPO and A2C name it; nobody else takes the factored face
                admitted = supported_action_spaces is not None and MultiDiscrete in supported_action_spaces
                supported_action_spaces = supported_action_spaces or ("Box",)
            else:
                admitted = wants_discrete if isinstance(self.action_space, Discrete) else wants_box
            if not admitted:
                raise AssertionError(f"The algorithm only supports {supported_action_spaces} as action spaces "
                                     f"but {self.action_space} was provided")
            if not support_multi_env and self.n_envs > 1:
                raise ValueError("Error: the model does not support multiple envs; it requires a single vectorized environment.")
            if isinstance(self.action_space, Box):  # reference base_class.py:215-218
                assert np.all(np.isfinite(np.array([self.action_space.low, self.action_space.high]))), \
                    "Continuous action space must have a finite lower and upper bound"

    # ---- env / policy plumbing --------------------------------------------------------------------------------
    @staticmethod
    def _as_action_space(space):
        d = as_discrete(space)
        if d is None:
            d = as_multi_discrete(space)
        return d if d is not None else as_box(space)

    @staticmethod
    def _wrap_env(env, verbose: int = 0) -> VecEnv:
        """reference: base_class.py:220-253. A VecEnv passes through untouched; a bare TwoSeriesCSTREnv becomes a
        1-env device CSTRVecEnv (the reference would wrap it in Monitor + DummyVecEnv)."""
        if isinstance(env, VecEnv):
            return env
        from twoseriescstr import TwoSeriesCSTREnv

        if isinstance(env, TwoSeriesCSTREnv):
            return CSTRVecEnv(1, **env.vec_kwargs())
        if all(hasattr(env, a) for a in ("num_envs", "observation_space", "action_space", "reset", "step")):
            return env  # duck-typed VecEnv (compatibility path)
        raise ValueError(f"Unsupported environment {type(env).__name__}: pass a CSTRVecEnv, a DummyVecEnv of "
                         "TwoSeriesCSTREnv or a TwoSeriesCSTREnv")

    def _get_policy_from_name(self, policy_name: str):
        """reference: base_class.py:345-360"""
        if policy_name in self.policy_aliases:
            return self.policy_aliases[policy_name]
        raise ValueError(f"Policy {policy_name} unknown")

    def _setup_lr_schedule(self) -> None:
        self.lr_schedule = get_schedule_fn(self.learning_rate)

    def _update_current_progress_remaining(self, num_timesteps: int, total_timesteps: int) -> None:
        self._current_progress_remaining = 1.0 - float(num_timesteps) / float(total_timesteps)

    def _update_learning_rate(self, optimizers) -> None:
        """reference: base_class.py:303-317"""
        self.logger.record("train/learning_rate", self.lr_schedule(self._current_progress_remaining))
        if not isinstance(optimizers, list):
            optimizers = [optimizers]
        for optimizer in optimizers:
            update_learning_rate(optimizer, self.lr_schedule(self._current_progress_remaining))
            if hasattr(optimizer, "sync_lr"):
                optimizer.sync_lr()

    def set_random_seed(self, seed: Optional[int] = None) -> None:
        """reference: base_class.py:582-595"""
        if seed is None:
            return
        set_random_seed(seed, using_cuda=True, device=self.device)
        self.action_space.seed(seed)
        if self.env is not None:
            self.env.seed(seed)
        self._reseed_device_rng(seed)

    def _reseed_device_rng(self, seed: int) -> None:
        """Device-resident counter RNG streams of the fused kernels follow `set_random_seed` like torch's generator does."""
        fa = getattr(self, "_fast_actor", None)
        if fa is not None and hasattr(fa, "seed_rng"):
            fa.seed_rng(seed + 1000003 * self.rank)
        dist = getattr(getattr(getattr(self, "policy", None), "actor", None), "action_dist", None)  # gSDE exploration-matrix stream
        if hasattr(dist, "seed_rng"):
            dist.seed_rng(seed + 1000003 * self.rank)
        ctl = getattr(self, "_rng_ctl", None)  # target-smoothing noise stream (TD3 / MADDPG)
        if ctl is not None:
            from core.common import hip_ops

            ctl.copy_(hip_ops.new_rng_ctl(seed + 1000003 * self.rank, ctl.device))

    def _device_rng(self):
        """In-kernel Philox stream for this algorithm's own noise kernels, seeded from torch's seed at first use."""
        if getattr(self, "_rng_ctl", None) is None:
            from core.common import hip_ops

            self._rng_ctl = hip_ops.new_rng_ctl(th.initial_seed(), self.device)
        return self._rng_ctl

    def get_env(self):
        return self.env

    def set_env(self, env, force_reset: bool = True) -> None:
        env = self._wrap_env(env, self.verbose)
        if env.num_envs != self.n_envs:
            raise AssertionError("The number of environments to be set is different from the number of environments in the model")
        is_dict = isinstance(getattr(env.observation_space, "spaces", None), dict)
        if is_dict != (self.goal_space is not None):
            raise ValueError("Observation spaces do not match: a model of the goal face needs CSTRVecEnv(goal_conditioned=True), and only such a model takes it")
        same_obs = env.observation_space == self.goal_space if is_dict else as_box(env.observation_space) == self.observation_space
        if not same_obs or self._as_action_space(env.action_space) != self.action_space:
            raise ValueError("Observation/action spaces do not match")
        if force_reset:
            self._last_obs = None
        self.env = env
        self._vec_normalize_env = unwrap_vec_normalize(env)  # reference base_class.py:525

    def get_vec_normalize_env(self):
        """reference: base_class.py:491-498"""
        return self._vec_normalize_env

    @property
    def _denv(self) -> Optional[CSTRVecEnv]:
        """the device-resident env underneath `self.env` (itself, or the one a VecNormalize wraps); None otherwise"""
        inner = getattr(self.env, "unwrapped", None)
        return inner if isinstance(inner, CSTRVecEnv) else None

    @property
    def logger(self) -> Logger:
        if self._logger is None:
            self._logger = configure_logger(self.verbose)
        return self._logger

    def set_logger(self, logger: Logger) -> None:
        self._logger = logger
        self._custom_logger = True

    def _init_callback(self, callback: MaybeCallback) -> BaseCallback:
        callback = to_callback(callback)
        callback.init_callback(self)
        return callback

    # ---- learn-time bookkeeping ---------------------------------------------------------------------------------
    def _setup_learn(self, total_timesteps: int, callback: MaybeCallback = None, reset_num_timesteps: bool = True,
                     tb_log_name: str = "run", progress_bar: bool = False):
        """reference: base_class.py:406-460"""
        self.start_time = time.time_ns()
        if self.ep_info_buffer is None or reset_num_timesteps:
            self.ep_info_buffer = deque(maxlen=self._stats_window_size)
            self.ep_success_buffer = deque(maxlen=self._stats_window_size)
        if self.action_noise is not None:
            self.action_noise.reset()
        if reset_num_timesteps:
            self.num_timesteps = 0
            self._episode_num = 0
        else:
            total_timesteps += self.num_timesteps
        self._total_timesteps = total_timesteps
        self._num_timesteps_at_start = self.num_timesteps
        if reset_num_timesteps or self._last_obs is None:
            assert self.env is not None
            self._last_obs = self.env.reset_device() if self._denv is not None else self.env.reset()
            self._last_episode_starts = np.ones((self.env.num_envs,), dtype=bool)
            # a seeded TwoSeriesCSTREnv.reset re-seeds the GLOBAL numpy stream (twoseriescstr.py:164): the replay
            # sampler's stream ends up seeded with seed + n_envs - 1 (SURVEY a-6)
            reseed = getattr(self._denv or self.env, "numpy_reseed", None)
            if reseed is not None:
                from core.common import legacy_rng

                np.random.seed(reseed)
                legacy_rng.seed(reseed, self.device)
                (self._denv or self.env).numpy_reseed = None
                self._numpy_reseeded(reseed)
        if not self._custom_logger:
            self._logger = configure_logger(self.verbose, self.tensorboard_log, tb_log_name, reset_num_timesteps)
        callback = self._init_callback(callback)
        return total_timesteps, callback

    def _numpy_reseeded(self, seed: int) -> None:
        """This model's own envs have just reseeded NumPy's global stream with `seed` (a seeded reset); for subclasses that keep a
        host image of that stream."""

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """reference: base_class.py:560-580"""
        return self.policy.predict(observation, state, episode_start, deterministic)

    def learn(self, total_timesteps: int, callback: MaybeCallback = None, log_interval: int = 100, tb_log_name: str = "run",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        raise NotImplementedError

    def train(self, *args: Any, **kwargs: Any) -> None:
        raise NotImplementedError

    # ---- checkpoints (reference: base_class.py:666-888, save_util.py:294-466) --------------------------------------
    _SAVE_HYPERS = ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "gradient_steps", "seed",
                    "policy_kwargs", "num_timesteps", "_n_updates", "_episode_num", "n_envs", "_total_timesteps",
                    "_num_timesteps_at_start", "_current_progress_remaining", "verbose")

    def _get_torch_save_params(self) -> tuple:
        """(state-dict attribute names, plain tensor attribute names) -- overridden per algorithm like the reference."""
        return ["policy"], []

    def _extra_save_data(self) -> dict:
        return {}

    def _recursive_getattr(self, name: str):
        obj = self
        for part in name.split("."):
            obj = getattr(obj, part)
        return obj

    def get_parameters(self) -> dict:
        """reference: base_class.py:827-840 -- {name: state_dict} for the policy and every optimiser"""
        names, _ = self._get_torch_save_params()
        return {name: self._recursive_getattr(name).state_dict() for name in names}

    def set_parameters(self, load_path_or_dict, exact_match: bool = True, device="auto") -> None:
        """reference: base_class.py:597-664. Values are copied INTO the arena views (module identity is preserved)."""
        if isinstance(load_path_or_dict, dict):
            params = load_path_or_dict
        else:
            from core.common.save_util import load_from_zip_file

            _, params, _ = load_from_zip_file(load_path_or_dict, device="cpu")
        names, _ = self._get_torch_save_params()
        updated = set()
        for name in params:
            if name not in names:
                raise ValueError(f"Key {name} is an invalid object name.")
            target = self._recursive_getattr(name)
            if name == "policy" or isinstance(target, th.nn.Module):
                own = target.state_dict()
                if exact_match and set(own) != set(params[name]):
                    raise ValueError(f"Names of parameters do not match agents' parameters: expected {sorted(own)}, got {sorted(params[name])}")
                with th.no_grad():
                    for k, v in params[name].items():
                        if k in own:
                            own[k].copy_(th.as_tensor(v).to(own[k].device))
            else:
                target.load_state_dict(params[name])
            updated.add(name)
        if exact_match and updated != set(names):
            raise ValueError(f"Names of parameters do not match agents' parameters: expected {names}, got {sorted(updated)}")

    def save(self, path, exclude=None, include=None) -> None:
        """reference: base_class.py:842-888. Writes the same archive members; `data` holds the JSON-able constructor
        arguments and counters (nothing is pickled)."""
        from core import __version__
        from core.common.save_util import save_to_zip_file

        data = {k: getattr(self, k) for k in self._SAVE_HYPERS if hasattr(self, k)}
        tf = getattr(self, "train_freq", None)
        if tf is not None and hasattr(tf, "unit"):
            data["train_freq"] = [tf.frequency, tf.unit.value]
        data["algo"] = type(self).__name__
        for nm, sp in (("observation_space", self.observation_space), ("action_space", self.action_space)):
            if isinstance(sp, Discrete):
                data[nm] = {"n": sp.n, "start": sp.start, "shape": [], "dtype": str(sp.dtype)}
                continue
            if isinstance(sp, MultiDiscrete):
                data[nm] = {"nvec": sp.nvec.tolist(), "shape": list(sp.shape), "dtype": str(sp.dtype)}
                continue
            data[nm] = {"low": np.asarray(sp.low).tolist(), "high": np.asarray(sp.high).tolist(), "shape": list(sp.shape), "dtype": str(sp.dtype)}
        if self.goal_space is not None:  # the Dict space of the goal face, key by key; HER's own arguments (plain JSON, nothing pickled)
            data["observation_space"] = {"spaces": {k: {"low": np.asarray(s.low).tolist(), "high": np.asarray(s.high).tolist(),
                                                        "shape": list(s.shape), "dtype": str(s.dtype)} for k, s in self.goal_space.items()}}
            rb = getattr(self, "replay_buffer", None)
            if rb is not None and hasattr(rb, "n_sampled_goal"):
                data["her_kwargs"] = {"n_sampled_goal": int(rb.n_sampled_goal), "goal_selection_strategy": rb.strategy_key}
        data.update(self._extra_save_data())
        for k in (exclude or []):
            data.pop(k, None)
        _, var_names = self._get_torch_save_params()
        variables = {n: self._recursive_getattr(n).detach().clone() for n in var_names} if var_names else None
        save_to_zip_file(path, data=data, params=self.get_parameters(), pytorch_variables=variables, version=__version__)

    @classmethod
    def load(cls, path, env=None, device="auto", custom_objects=None, print_system_info: bool = False, force_reset: bool = True, **kwargs):
        """reference: base_class.py:666-825. Works for archives written by this stack and for archives written by the
        reference (only `weights_only` tensors and plain JSON are read; `env` must then be passed)."""
        from core.common.save_util import load_from_zip_file

        data, params, variables = load_from_zip_file(path, device="cpu")
        if env is None:
            raise ValueError("load(): pass `env` (environments are not stored in the archive)")
        cls._check_archive(data, env)
        ctor = {k: data[k] for k in cls._ctor_keys() if k in data}
        goal_archive = isinstance(data.get("observation_space"), dict) and "spaces" in data["observation_space"]
        goal_env = isinstance(getattr(getattr(env, "observation_space", None), "spaces", None), dict)
        if goal_archive != goal_env:
            raise ValueError("load(): the archive holds a model of the goal face (a Dict observation space) and the env has none"
                             if goal_archive else "load(): the env has the goal face (a Dict observation space) and the archive's model has none")
        if goal_archive and "replay_buffer_class" not in kwargs and "buffer_size" in cls._ctor_keys():  # the off-policy classes: HER
            from core.her import HerReplayBuffer

            ctor["replay_buffer_class"], ctor["replay_buffer_kwargs"] = HerReplayBuffer, dict(data.get("her_kwargs", {}))
        if "train_freq" in data and isinstance(data["train_freq"], list):
            ctor["train_freq"] = (int(data["train_freq"][0]), str(data["train_freq"][1]))
        ctor.update(kwargs)
        cls._check_load_arguments(data, ctor)
        model = cls._construct_for_load(env, device, ctor)
        model.set_parameters(params, exact_match=True)
        for name, value in (variables or {}).items():
            tgt = model._recursive_getattr(name)
            with th.no_grad():
                tgt.copy_(th.as_tensor(value).to(tgt.device).reshape(tgt.shape))
        for k in ("num_timesteps", "_n_updates", "_episode_num", "_total_timesteps", "_num_timesteps_at_start"):
            if k in data:
                setattr(model, k, data[k])
        model._restore_extra(data)
        if model.use_sde:
            model.policy.reset_noise()  # :823-824
        return model

    @classmethod
    def _check_archive(cls, data: dict, env) -> None:
        """Hook of load(): refuse an archive that does not fit `env` before anything is built."""

    @classmethod
    def _check_load_arguments(cls, data: dict, ctor: dict) -> None:
        """Hook of load(): refuse constructor arguments (the archive's, overridden by load()'s own keywords) that do not fit what the
        archive's parameters were written for, before anything is built."""

    def _restore_extra(self, data: dict) -> None:
        """Hook of load(): the class's own counters out of the archive's `data`."""

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "gradient_steps", "seed", "policy_kwargs")

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        goal_env = isinstance(getattr(getattr(env, "observation_space", None), "spaces", None), dict)
        return cls("MultiInputPolicy" if goal_env else "MlpPolicy", env, device=device, **ctor)
