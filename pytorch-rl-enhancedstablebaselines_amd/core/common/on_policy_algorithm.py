"""`OnPolicyAlgorithm`: rollout collection into a device `RolloutBuffer` and the collect / train loop
(reference: core/common/on_policy_algorithm.py:21-346). Nothing here belongs to one algorithm: the subclass supplies `train()`.

The device rollout step (a `CSTRVecEnv` underneath, the policy on the kernel path) keeps everything in HBM and never synchronises
with the host: policy and value forward, the Gaussian head launch, the env step, the value net on the terminal observations (used
only where an episode was truncated), the buffer's add launch (timeout bootstrap, next step's episode starts and the episode
statistics included). Any other VecEnv takes the reference's NumPy loop.

On the goal face (`CSTRVecEnv(goal_conditioned=True)`, "MultiInputPolicy", a `DictRolloutBuffer`) the same step runs on the env's flat
rows [achieved_goal | desired_goal | observation]: a copy of `env.flat`, the policy at K = 6, the goal face's one-launch env step, the
value net on the terminal rows, the add launch of the 6-float row. The NumPy loop handles dict observations through
`policy.obs_to_tensor`, a dict `terminal_observation` included.

Minibatch order: the reference draws `np.random.permutation(T * N)` per epoch from the process-global legacy stream, which the
last seeded env reset left seeded with seed + n_envs - 1. With a device env the same sequence comes from a `RandomState` of the
algorithm's own: it is (re)created when this model's own envs perform a seeded reset (`_numpy_reseeded`) and runs on across later
`learn()` calls, whose resets are unseeded, as the reference's stream does. Any other VecEnv seeds NumPy's global stream itself;
there the buffer draws from that stream."""
import sys
import time
from typing import Optional

import numpy as np
import torch as th

from core.common import blas, fused
from core.common.base_class import BaseAlgorithm
from core.common.buffers import DictRolloutBuffer, RolloutBuffer
from core.common.callbacks import BaseCallback, MaybeCallback
from core.common.spaces import Discrete, MultiDiscrete, as_discrete, as_multi_discrete
from core.common.vec_env import VecEnv
from core.common.vec_env.cstr_vec_env import goal_rows_to_dict


class OnPolicyAlgorithm(BaseAlgorithm):
    goal_face_support = True  # with "MultiInputPolicy": a MultiInputActorCriticPolicy and a DictRolloutBuffer
    flat_rmsprop = False  # True (A2C): torch.optim.RMSprop in the policy's kwargs becomes the flat kernel form (arena.FlatRMSprop)

    def __init__(self, policy, env, learning_rate, n_steps: int, gamma: float, gae_lambda: float, ent_coef: float, vf_coef: float,
                 max_grad_norm: float, use_sde: bool, sde_sample_freq: int, rollout_buffer_class=None,
                 rollout_buffer_kwargs: Optional[dict] = None, stats_window_size: int = 100, tensorboard_log: Optional[str] = None,
                 monitor_wrapper: bool = True, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device="auto", _init_setup_model: bool = True, supported_action_spaces: Optional[tuple] = None):
        if use_sde:
            raise ValueError(f"{type(self).__name__} does not support gSDE (use_sde=True): on-policy gSDE is not built")
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, policy_kwargs=policy_kwargs, verbose=verbose, device=device,
                         use_sde=use_sde, sde_sample_freq=sde_sample_freq, support_multi_env=True, monitor_wrapper=monitor_wrapper,
                         seed=seed, stats_window_size=stats_window_size, tensorboard_log=tensorboard_log,
                         supported_action_spaces=supported_action_spaces)
        if self.world_size > 1:
            raise NotImplementedError(f"data-parallel {type(self).__name__} is not built")
        if self._vec_normalize_env is not None:
            raise NotImplementedError(f"{type(self).__name__} on a VecNormalize-wrapped env is not built")
        self.n_steps = n_steps
        self.gamma = gamma
        self.gae_lambda = gae_lambda
        self.ent_coef = ent_coef
        self.vf_coef = vf_coef
        self.max_grad_norm = max_grad_norm
        self.rollout_buffer_class = rollout_buffer_class
        self.rollout_buffer_kwargs = rollout_buffer_kwargs or {}
        self.rollout_buffer: Optional[RolloutBuffer] = None
        self._starts_on = None  # where the current episode starts live: "device", "host", None = both (just reset)
        self._ep_window = (0.0, 0.0, 0.0)
        self._ep_totals_at_dump = (0.0, 0.0, 0.0)
        if _init_setup_model:
            self._setup_model()

    def _goal_face_policy_message(self, policy) -> str:
        return (f"{type(self).__name__} with {policy} does not support a Dict observation space (the goal face of the env): "
                "use `MultiInputPolicy`")

    def enable_graph_capture(self, enabled: bool = True) -> None:
        if enabled:
            raise NotImplementedError(f"{type(self).__name__} has no hipGraph replay: learn() launches eagerly")

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        """reference :115-140"""
        self._setup_lr_schedule()
        blas.configure()
        self.set_random_seed(self.seed)
        space = self.goal_space if self.goal_space is not None else self.observation_space  # the goal face: the Dict space
        if self.rollout_buffer_class is None:  # :121-125
            self.rollout_buffer_class = DictRolloutBuffer if self.goal_space is not None else RolloutBuffer
        self.rollout_buffer = self.rollout_buffer_class(self.n_steps, space, self.action_space, device=self.device,
                                                        gamma=self.gamma, gae_lambda=self.gae_lambda, n_envs=self.n_envs,
                                                        **self.rollout_buffer_kwargs)
        # built on the CPU generator in the reference's construction order, then moved into ONE flat arena by the policy itself
        self.policy = self.policy_class(space, self.action_space, self.lr_schedule, use_sde=self.use_sde, **self.policy_kwargs)
        self.policy.to_device_arenas(self.device, flat_rmsprop=self.flat_rmsprop)
        n, dev = self.n_envs, self.device
        self._fast = None
        if self.policy.flat_optimizers() and fused.FastActorCritic.supported(self.policy):
            self._fast = fused.FastActorCritic(self.policy, self._device_rng())
        self._fused_learner = self._fast is not None
        self.policy.fast = self._fast
        self._ep_return = th.zeros(n, dtype=th.float32, device=dev)
        self._ep_len = th.zeros(n, dtype=th.int32, device=dev)
        self._ep_stats = th.zeros(4, dtype=th.float64, device=dev)
        self._episode_starts_dev = th.ones(n, dtype=th.float32, device=dev)
        self._obs_prev = th.zeros(n, *self.observation_space.shape, dtype=th.float32, device=dev)

    @property
    def fused_learner(self) -> bool:
        """True: the kernel path (per-layer Linear kernels, or rocBLAS GEMMs with CSTR_FUSED_LINEAR=0, and csrc/cstr_ppo.hip / cstr_a2c.hip);
        False: the reference's own torch statements on the arena parameters (another optimiser class, widths the kernels decline)."""
        return self._fused_learner

    @fused_learner.setter
    def fused_learner(self, value: bool) -> None:
        if value and self._fast is None:
            raise ValueError(f"this {type(self).__name__} model has no kernel path (unsupported widths or a non-default optimiser)")
        self._fused_learner = bool(value)
        self.policy.fast = self._fast if value else None

    def _setup_learn(self, total_timesteps, callback=None, reset_num_timesteps=True, tb_log_name="run", progress_bar=False):
        resetting = reset_num_timesteps or self._last_obs is None
        out = super()._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)
        if resetting:  # the envs were reset: every env starts an episode, nothing is accumulated yet
            self._episode_starts_dev.fill_(1.0)
            self._starts_on = None
            self._ep_return.zero_()
            self._ep_len.zero_()
        if self._denv is not None and self.rollout_buffer.permutation_rng is None:
            self.rollout_buffer.permutation_rng = np.random.RandomState()  # no seeded reset so far: OS entropy, as an unseeded np.random
        return out

    def _numpy_reseeded(self, seed: int) -> None:
        """A seeded reset of this model's envs (seed + n_envs - 1, the last env wins): the minibatch permutations restart there."""
        self.rollout_buffer.permutation_rng = np.random.RandomState(seed)

    # ---- rollouts -------------------------------------------------------------------------------------------------
    def _device_rollout(self) -> bool:
        rb = self.rollout_buffer
        if self._denv is not None and self._denv.goal_conditioned:  # the flat rows of the goal face into a DictRolloutBuffer
            return self._fused_learner and type(rb) is DictRolloutBuffer and rb.n_envs == self._denv.num_envs and rb.action_dim == self._denv.act_dim
        return (self._denv is not None and self._fused_learner and type(rb) is RolloutBuffer and rb.n_envs == self._denv.num_envs
                and rb.obs_shape[0] == self._denv.obs_dim
                and rb.action_dim == (1 if self._denv.discrete_actions is not None else self._denv.act_dim))  # Discrete: the index; MultiDiscrete: the level pair, act_dim floats

    def collect_rollouts(self, env: VecEnv, callback: BaseCallback, rollout_buffer: RolloutBuffer, n_rollout_steps: int) -> bool:
        """reference :162-268"""
        assert self._last_obs is not None, "No previous observation was provided"
        self.policy.set_training_mode(False)
        n_steps = 0
        rollout_buffer.reset()
        callback.on_rollout_start()
        noop_cb = getattr(callback, "is_noop", False)
        fast = self._device_rollout()
        denv = self._denv
        while n_steps < n_rollout_steps:
            if fast:
                with th.cuda.device(self.device):
                    new_obs, rewards, dones, step = self._device_rollout_step(denv)
            else:
                new_obs, rewards, dones, actions, values, log_probs = self._host_rollout_step(env)
            self.num_timesteps += env.num_envs
            if not noop_cb:
                callback.update_locals(locals())
            if not callback.on_step():
                return False
            n_steps += 1
            if fast:  # the add follows on_step, as in the reference (:247-256): a callback that stops the rollout leaves no row behind
                with th.cuda.device(self.device):
                    rollout_buffer.add_device(*step)
                self._last_obs = new_obs
            else:
                rollout_buffer.add(self._last_obs, actions, rewards, self._last_episode_starts, values, log_probs)
                self._last_obs, self._last_episode_starts = new_obs, dones
        with th.no_grad(), th.cuda.device(self.device):
            last_obs = new_obs if isinstance(new_obs, th.Tensor) else self.policy.obs_to_tensor(new_obs)[0]
            values = self.policy.predict_values(last_obs)  # :258-260
            rollout_buffer.compute_returns_and_advantage(last_values=values.reshape(-1), dones=dones)
        if not noop_cb:
            callback.update_locals(locals())
        callback.on_rollout_end()
        return True

    def _device_rollout_step(self, env):
        """One vec-step entirely in HBM (:199-245), no host synchronisation. Returns the new observations, rewards, dones and the
        operands of the buffer's add launch (static tensors; the write position is a device control word)."""
        fast = self._fast
        if self._starts_on == "host":  # the NumPy loop ran last (fused_learner was switched): its episode starts come over
            self._episode_starts_dev.copy_(th.as_tensor(np.asarray(self._last_episode_starts, np.float32)))
        self._starts_on = "device"
        self._obs_prev.copy_(env.flat if env.goal_conditioned else env.obs)
        actions, values, log_probs, env_actions = fast.act(self._obs_prev)
        new_obs, rewards, dones, timeouts, terminal_obs = env.step_device(env_actions)
        with th.no_grad():
            terminal_values = fast.values(terminal_obs)  # read only where the episode was truncated (:236-245)
        step = (self._obs_prev, actions, rewards, self._episode_starts_dev, values.reshape(-1), log_probs, timeouts,
                terminal_values.reshape(-1), dones, self._ep_return, self._ep_len, self._ep_stats)
        return new_obs, rewards, dones, step

    def _host_rollout_step(self, env):
        """The reference's NumPy statements (:199-245) for a VecEnv that is not device-resident."""
        if isinstance(self._last_obs, th.Tensor):  # the device env's own observation tensor: the step below overwrites it
            self._last_obs = self._last_obs.cpu().numpy()
            if self.goal_space is not None:  # the goal face's flat rows: the host loop keeps the dict, as env.step returns it
                self._last_obs = goal_rows_to_dict(self._last_obs)
        if self._starts_on == "device":  # the device rollout ran last: its episode starts come over
            self._last_episode_starts = self._episode_starts_dev.cpu().numpy() > 0
        self._starts_on = "host"
        with th.no_grad():
            obs_tensor = self.policy.obs_to_tensor(self._last_obs)[0]
            actions, values, log_probs = self.policy(obs_tensor)
            actions, values, log_probs = actions.clone(), values.clone(), log_probs.clone()
        actions_np = actions.cpu().numpy()
        if isinstance(self.action_space, Discrete):  # :228-232: indices step the env as they are and are stored as [n, 1]
            clipped = actions_np
            actions_np = actions_np.reshape(-1, 1)
        elif isinstance(self.action_space, MultiDiscrete):  # the integer level pairs [n, 2] step the env unclipped and are stored as they are
            clipped = actions_np
        else:
            clipped = np.clip(actions_np, self.action_space.low, self.action_space.high)
        new_obs, rewards, dones, infos = env.step(clipped)
        rewards = np.array(rewards, dtype=np.float32)
        ret = self._ep_return.cpu().numpy() + rewards
        length = self._ep_len.cpu().numpy() + 1
        for idx, done in enumerate(dones):
            if done:
                self.ep_info_buffer.append({"r": float(ret[idx]), "l": int(length[idx])})
                ret[idx], length[idx] = 0.0, 0
                if infos[idx].get("terminal_observation") is not None and infos[idx].get("TimeLimit.truncated", False):
                    terminal_obs = self.policy.obs_to_tensor(infos[idx]["terminal_observation"])[0]
                    with th.no_grad():
                        terminal_value = self.policy.predict_values(terminal_obs)[0]
                    rewards[idx] += np.float32(self.gamma) * terminal_value.cpu().numpy().astype(np.float32).reshape(-1)[0]
        self._ep_return.copy_(th.as_tensor(ret.astype(np.float32)))
        self._ep_len.copy_(th.as_tensor(length.astype(np.int32)))
        return new_obs, rewards, dones, actions_np, values, log_probs

    def train(self) -> None:
        raise NotImplementedError

    # ---- logging --------------------------------------------------------------------------------------------------
    def _dump_logs(self, iteration: int) -> None:
        """reference :277-297. The device rollout keeps the episode counters in HBM: one read of four doubles per dump; the means
        cover the episodes that finished since the last dump that saw any."""
        time_elapsed = max((time.time_ns() - self.start_time) / 1e9, sys.float_info.epsilon)
        fps = int((self.num_timesteps - self._num_timesteps_at_start) / time_elapsed)
        self.logger.record("time/iterations", iteration, exclude="tensorboard")
        if len(self.ep_info_buffer) > 0:  # the NumPy loop's Monitor-style records
            self.logger.record("rollout/ep_rew_mean", float(np.mean([e["r"] for e in self.ep_info_buffer])))
            self.logger.record("rollout/ep_len_mean", float(np.mean([e["l"] for e in self.ep_info_buffer])))
        else:
            n_ep, ret_sum, len_sum, _ = self._ep_stats.cpu().tolist()
            self._episode_num = int(n_ep)
            w0, w1, w2 = self._ep_totals_at_dump
            if n_ep > w0:
                self._ep_window = (n_ep - w0, ret_sum - w1, len_sum - w2)
                self._ep_totals_at_dump = (n_ep, ret_sum, len_sum)
            if self._ep_window[0] > 0:
                self.logger.record("rollout/ep_rew_mean", self._ep_window[1] / self._ep_window[0])
                self.logger.record("rollout/ep_len_mean", self._ep_window[2] / self._ep_window[0])
        self.logger.record("time/fps", fps)
        self.logger.record("time/time_elapsed", int(time_elapsed), exclude="tensorboard")
        self.logger.record("time/total_timesteps", self.num_timesteps, exclude="tensorboard")
        self.logger.dump(step=self.num_timesteps)

    def learn(self, total_timesteps: int, callback: MaybeCallback = None, log_interval: int = 1, tb_log_name: str = "OnPolicyAlgorithm",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        """reference :299-340"""
        iteration = 0
        total_timesteps, callback = self._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)
        callback.on_training_start(locals(), globals())
        assert self.env is not None
        while self.num_timesteps < total_timesteps:
            continue_training = self.collect_rollouts(self.env, callback, self.rollout_buffer, n_rollout_steps=self.n_steps)
            if not continue_training:
                break
            iteration += 1
            self._update_current_progress_remaining(self.num_timesteps, total_timesteps)
            if log_interval is not None and iteration % log_interval == 0:
                assert self.ep_info_buffer is not None
                self._dump_logs(iteration)
            self.train()
        callback.on_training_end()
        return self

    @classmethod
    def _check_archive(cls, data: dict, env) -> None:
        """An archive written on a Discrete face fits an env with the same number of indices only (and a Box archive a Box env, a MultiDiscrete
        archive an env with the same `nvec`): the policy's head is built from the env's action space."""
        saved = data.get("action_space")
        if not isinstance(saved, dict) or not ({"n", "low", "nvec"} & set(saved)):
            return  # an archive of the reference: its spaces are not stored as plain data
        saved_n = saved.get("n")
        saved_nvec = None if saved.get("nvec") is None else [int(k) for k in saved["nvec"]]
        face = as_discrete(getattr(env, "action_space", None))
        multi = None if face is not None else as_multi_discrete(getattr(env, "action_space", None))
        if saved_n != (None if face is None else int(face.n)) or saved_nvec != (None if multi is None else [int(k) for k in multi.nvec]):
            was = f"MultiDiscrete({saved_nvec})" if saved_nvec is not None else ("a Box action space" if saved_n is None else f"Discrete({saved_n})")
            raise ValueError(f"the archive was written for {was}, the env has {getattr(env, 'action_space', None)} "
                             f"(discrete_actions={getattr(getattr(env, 'unwrapped', env), 'discrete_actions', None)})")

    def _get_torch_save_params(self) -> tuple:
        """reference :342-345"""
        return ["policy", "policy.optimizer"], []
