"""`OffPolicyAlgorithm`: the collect -> store -> sample -> train runtime
(reference: core/common/off_policy_algorithm.py:27-605), rebuilt around a device-resident loop.

Reference iteration (per vec-step): python loop over N envs, deepcopy of N info dicts, 5 H2D copies per
sample, 4 `.item()` syncs per gradient step. Here, when the env is a `CSTRVecEnv` and the buffer is the HBM
`ReplayBuffer`, one iteration is: actor forward (one whole-network HIP launch above 1024 envs) -> ONE fused HIP launch
(action scaling chain + env step + auto-reset + ring row write + episode statistics) -> `train()`. Nothing
returns to the host except, every `stats_sync_interval` vec-steps, four doubles of episode statistics.
Any other VecEnv goes through the NumPy compatibility path with the reference's exact semantics.
"""
import os
import sys
import time
from typing import Any, Optional, Union

import numpy as np
import torch as th

from core.common import blas, chain, fused, hip_ops
from core.common.base_class import BaseAlgorithm
from core.common.buffers import ReplayBuffer
from core.common.callbacks import BaseCallback, MaybeCallback
from core.common.graph_replay import GraphReplay
from core.common.logger import DeviceMean
from core.common.type_aliases import RolloutReturn, TrainFreq, TrainFrequencyUnit
from core.common.utils import should_collect_more_steps
from core.common.vec_env import CSTRVecEnv, VecEnv

# the captured iteration's rollout as ONE launch (policy + collect step + replay index draw; hip_ops.rollout_step). "0": the
# separate policy / collect / sampler launches (A/B knob; both forms are bit-identical, tests/test_rollout_step.py)
FUSED_ROLLOUT = os.environ.get("CSTR_FUSED_ROLLOUT", "1") != "0"
# the goal face's vec-step as ONE launch (hip_ops.goal_collect_step). "0": the element-wise action chain, the row copy, the env step,
# the HER add and the statistics ops as separate launches, never replayed from a graph (A/B knob; both forms are bit-identical,
# tests/test_goal_collect.py)
HER_FUSED_COLLECT = os.environ.get("CSTR_HER_FUSED_COLLECT", "1") != "0"


class OffPolicyAlgorithm(GraphReplay, BaseAlgorithm):
    train_batch_size: Optional[int] = None  # `batch_size` of a train() call that names none (the reference's per-class default)
    packed_batch_with_pi = True             # the packed batch carries x_pi = (obs | pi(obs)) rows for the actor step
    chain_type: Optional[type] = None       # the row-chain form of this class's gradient step (core/common/chain.py)
    _single_step = False                    # this train() call is ONE gradient step whose loss kernels store the logged values

    def __init__(self, policy, env, learning_rate, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq: Union[int, tuple] = (1, "step"),
                 gradient_steps: int = 1, action_noise=None, replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None,
                 optimize_memory_usage: bool = False, policy_kwargs: Optional[dict] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, verbose: int = 0, device="auto", support_multi_env: bool = False,
                 monitor_wrapper: bool = True, seed: Optional[int] = None, use_sde: bool = False, sde_sample_freq: int = -1,
                 use_sde_at_warmup: bool = False, sde_support: bool = True, supported_action_spaces: Optional[tuple] = None):
        if use_sde and not sde_support:  # TD3 / DDPG / MADDPG / IDDPG (sde_support=False in the reference too)
            raise ValueError(f"{type(self).__name__} does not support gSDE (use_sde=True)")
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, policy_kwargs=policy_kwargs,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, verbose=verbose, device=device,
                         support_multi_env=support_multi_env, monitor_wrapper=monitor_wrapper, seed=seed, use_sde=use_sde,
                         sde_sample_freq=sde_sample_freq, supported_action_spaces=supported_action_spaces)
        if sde_support and (use_sde or "use_sde" in self.policy_kwargs):
            self.policy_kwargs["use_sde"] = self.use_sde  # reference :137-138
        self.buffer_size = buffer_size
        self.batch_size = batch_size
        self.learning_starts = learning_starts
        self.tau = tau
        self.gamma = gamma
        self.gradient_steps = gradient_steps
        self.action_noise = action_noise
        self.optimize_memory_usage = optimize_memory_usage
        self.replay_buffer: Optional[ReplayBuffer] = None
        self.replay_buffer_class = replay_buffer_class
        self.replay_buffer_kwargs = replay_buffer_kwargs or {}
        self.train_freq = train_freq
        self.use_sde_at_warmup = use_sde_at_warmup
        self._init_graph_state()
        self._rng_advance = None  # (rng_ctl, rows) the next fused collect launch owes the rollout policy launch (SAC)
        self.stats_sync_interval = 100   # vec-steps between host reads of the device episode counters
        self._steps_since_sync = 0
        self._episodes_at_last_dump = 0
        self._ep_window = (0.0, 0.0, 0.0)

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _convert_train_freq(self) -> None:
        """reference: off_policy_algorithm.py:148-170"""
        if not isinstance(self.train_freq, TrainFreq):
            train_freq = self.train_freq
            if not isinstance(train_freq, tuple):
                train_freq = (train_freq, "step")
            try:
                train_freq = (train_freq[0], TrainFrequencyUnit(train_freq[1]))
            except ValueError as e:
                raise ValueError(f"The unit of the `train_freq` must be either 'step' or 'episode' not '{train_freq[1]}'!") from e
            if not isinstance(train_freq[0], int):
                raise ValueError(f"The frequency of `train_freq` must be an integer and not {train_freq[0]}")
            self.train_freq = TrainFreq(*train_freq)

    def _setup_model(self) -> None:
        """reference: off_policy_algorithm.py:172-212"""
        self._chain_cache = {}  # row-chain step objects hold raw pointers of the policy's tensors: rebuilt with the policy
        self._setup_lr_schedule()
        blas.configure()
        if self.world_size > 1 and self._denv is not None:
            self._denv.seed_offset = self.rank * self.n_envs  # seed_r = seed + rank * n_envs
        self.set_random_seed(self.seed)
        if self.replay_buffer_class is None:
            self.replay_buffer_class = ReplayBuffer
        from core.her import HerReplayBuffer

        is_her = isinstance(self.replay_buffer_class, type) and issubclass(self.replay_buffer_class, HerReplayBuffer)
        if is_her != (self.goal_space is not None):
            raise ValueError("HerReplayBuffer needs the goal face of the env (CSTRVecEnv(goal_conditioned=True)) and a MultiInputPolicy" if is_her
                             else "the goal face of the env needs replay_buffer_class=HerReplayBuffer (a plain DictReplayBuffer is not built)")
        if self.replay_buffer is None:
            kw = dict(self.replay_buffer_kwargs)
            if is_her:  # reference :184-196: the buffer computes the rewards of relabelled transitions with the env
                kw["env"] = self.env
            self.replay_buffer = self.replay_buffer_class(self.buffer_size, self.goal_space if is_her else self.observation_space,
                                                          self.action_space, device=self.device, n_envs=self.n_envs,
                                                          optimize_memory_usage=self.optimize_memory_usage, **kw)
        self._her_checked = False
        # built on the CPU generator in the reference's construction order (same seed -> same initial weights),
        # then moved into the HBM arenas by the policy itself
        self.policy = self._make_policy()
        self.policy.to_device_arenas(self.device)
        if self.world_size > 1:
            self.policy.broadcast_from_rank0()
            for opt in self.policy.flat_optimizers():
                opt.grad_scale = 1.0 / self.world_size
            if self.seed is not None:  # same init everywhere, different exploration noise per shard
                th.manual_seed(self.seed + 1000003 * self.rank)
        self._convert_train_freq()
        n = self.n_envs
        self._ep_return = th.zeros(n, dtype=th.float32, device=self.device)
        self._ep_stats = th.zeros(4, dtype=th.float64, device=self.device)

    def _make_policy(self):
        space = self.goal_space if self.goal_space is not None else self.observation_space  # a MultiInputPolicy takes the Dict space
        return self.policy_class(space, self.action_space, self.lr_schedule, **self.policy_kwargs)

    def save_replay_buffer(self, path) -> None:
        """reference: off_policy_algorithm.py:214-222"""
        from core.common.save_util import save_to_pkl

        assert self.replay_buffer is not None, "The replay buffer is not defined"
        save_to_pkl(path, self.replay_buffer, self.verbose)

    def load_replay_buffer(self, path, truncate_last_traj: bool = True) -> None:
        """reference: off_policy_algorithm.py:224-254"""
        from core.common.save_util import load_from_pkl
        from core.her import HerReplayBuffer

        self.replay_buffer = load_from_pkl(path, self.verbose)
        assert isinstance(self.replay_buffer, ReplayBuffer), "The replay buffer must inherit from ReplayBuffer class"
        if isinstance(self.replay_buffer, HerReplayBuffer) != (self.goal_space is not None):
            raise ValueError("load_replay_buffer: a HerReplayBuffer belongs to a model of the goal face, and only to such a model")
        self.replay_buffer.to(self.device)  # :252-253
        if isinstance(self.replay_buffer, HerReplayBuffer):  # :243-250
            assert self.env is not None, "You must pass an environment at load time when using `HerReplayBuffer`"
            self.replay_buffer.set_env(self.env)
            if truncate_last_traj:
                self.replay_buffer.truncate_last_trajectory()
        self.replay_buffer.normalizer = self._vec_normalize_env
        self._her_checked = False
        self._graph = None  # captured graphs hold the old ring's pointers

    def _her_path(self) -> bool:
        """The device rollout on the goal face: policy forward on the flat rows, then cstr_goal_collect_step_f32 (env step + HER add)."""
        from core.her import HerReplayBuffer

        env, rb = self._denv, self.replay_buffer
        return env is not None and env.goal_conditioned and isinstance(rb, HerReplayBuffer) and rb.n_envs == env.num_envs

    def _device_rollout(self) -> bool:
        return self._fast_path() or self._her_path()

    def _fast_path(self) -> bool:
        rb = self.replay_buffer
        env = self._denv
        return (env is not None and type(rb) is ReplayBuffer and rb.n_envs == env.num_envs
                and rb.obs_shape[0] == env.obs_dim and rb.action_dim == env.act_dim)

    # ---- learn ----------------------------------------------------------------------------------------------------
    def _setup_learn(self, total_timesteps, callback=None, reset_num_timesteps=True, tb_log_name="run", progress_bar=False):
        from core.common.noise import (DeviceNormalActionNoise, LegacyStreamNormalActionNoise, LegacyStreamOUActionNoise,
                                       NormalActionNoise, OrnsteinUhlenbeckActionNoise, VectorizedActionNoise)

        self.replay_buffer.normalizer = self._vec_normalize_env  # sample(..., env=self._vec_normalize_env), sac.py:215
        opt = getattr(getattr(self.policy, "actor", None), "optimizer", None)
        if hasattr(opt, "refresh_shadow"):  # weights may have been loaded / set since the last learn(): graphs replay, Python does not
            opt.refresh_shadow()
        base = self.action_noise
        if isinstance(base, VectorizedActionNoise) and base.n_envs == self.env.num_envs:
            base = base.base_noise
        if isinstance(base, NormalActionNoise) and self._device_rollout() and np.size(base._mu) <= 8:
            # the reference's n_envs sequential np.random.normal draws per vec-step (noise.py:44-45, :141-142) as one
            # kernel on the HBM image of the same legacy stream the replay sampler uses: bit-faithful interleaving
            self.action_noise = LegacyStreamNormalActionNoise(base._mu, base._sigma, self.env.num_envs, self.device,
                                                              lambda: self.replay_buffer.sampler_stream)
        elif isinstance(base, OrnsteinUhlenbeckActionNoise) and self._device_rollout() and np.size(base._mu) <= 8:
            # noise.py:84-89 per env on the same stream, float64 state in HBM
            self.action_noise = LegacyStreamOUActionNoise(base._mu, base._sigma, base._theta, base._dt, base.initial_noise,
                                                          self.env.num_envs, self.device, lambda: self.replay_buffer.sampler_stream)
        elif self.action_noise is not None and self.env.num_envs > 1 and not hasattr(self.action_noise, "noises") \
                and not isinstance(self.action_noise, (DeviceNormalActionNoise, LegacyStreamNormalActionNoise, LegacyStreamOUActionNoise)):
            self.action_noise = VectorizedActionNoise(self.action_noise, self.env.num_envs)
        return super()._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)

    def learn(self, total_timesteps: int, callback: MaybeCallback = None, log_interval: int = 4, tb_log_name: str = "run",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        """reference: off_policy_algorithm.py:309-355"""
        total_timesteps, callback = self._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)
        callback.on_training_start(locals(), globals())
        assert self.env is not None, "You must set the environment before calling learn()"
        assert isinstance(self.train_freq, TrainFreq)
        while self.num_timesteps < total_timesteps:
            if not self._learn_iteration(callback, log_interval):
                break
        if self._device_rollout():
            self._sync_episode_stats(log_interval, force=True)
        callback.on_training_end()
        return self

    def _eager_iteration(self, callback: BaseCallback, log_interval: Optional[int]) -> bool:
        """Body of the reference's `while` loop (off_policy_algorithm.py:331-351): one rollout, then train."""
        rollout = self.collect_rollouts(self.env, train_freq=self.train_freq, action_noise=self.action_noise,
                                        callback=callback, learning_starts=self.learning_starts,
                                        replay_buffer=self.replay_buffer, log_interval=log_interval)
        if not rollout.continue_training:
            return False
        if self.num_timesteps > 0 and self.num_timesteps > self.learning_starts:
            gradient_steps = self.gradient_steps if self.gradient_steps >= 0 else rollout.episode_timesteps
            if gradient_steps > 0 and not self._her_checked and self._her_path():
                # HerReplayBuffer.sample's check (her_replay_buffer.py:197-201), once, when training starts: one host read
                self._her_checked = True
                if not self.replay_buffer.has_valid_transition():
                    from core.her.her_replay_buffer import NO_EPISODE_MSG

                    raise RuntimeError(NO_EPISODE_MSG)
            if gradient_steps > 0:
                self.train(batch_size=self.batch_size, gradient_steps=gradient_steps)
        return True

    # ---- hipGraph replay of the steady-state iteration: the hooks of core/common/graph_replay.py ------------------------
    def _graph_eligible(self, callback: BaseCallback) -> bool:
        from core.common.noise import DeviceNormalActionNoise, LegacyStreamNormalActionNoise, LegacyStreamOUActionNoise

        # the goal face replays its fused collect launch only, and only behind the eager iteration that made HerReplayBuffer.sample's
        # one-time "has an episode ended" check (`_eager_iteration`): an unchecked model stays eager until it has
        her = HER_FUSED_COLLECT and self._her_checked and self._her_path()
        return ((her or self._fast_path()) and self._callback_allows_replay(callback)
                and (self.action_noise is None
                     or isinstance(self.action_noise, (DeviceNormalActionNoise, LegacyStreamNormalActionNoise, LegacyStreamOUActionNoise)))
                and self.train_freq == TrainFreq(1, TrainFrequencyUnit.STEP)
                and self.gradient_steps >= 1 and self.num_timesteps >= self.learning_starts
                and self.num_timesteps + self.n_envs > self.learning_starts and not getattr(self, "debug_capture", False))

    def _graph_cache_key(self, unroll: int) -> tuple:
        vn = self._vec_normalize_env
        return (id(self._denv.coef), self.batch_size, self.gradient_steps, self._graph_phase(), None if vn is None else (id(vn), vn.cfg_key),
                unroll)

    def _graph_body(self) -> None:
        env, rb = self._denv, self.replay_buffer
        self.policy.set_training_mode(False)
        self._sde_rollout_resets(0)
        noise = None if self.action_noise is None else self.action_noise().contiguous()
        net = self._rollout_net() if (FUSED_ROLLOUT and self._vec_normalize_env is None and self._use_packed_batch()) else None
        if net is None:
            self._device_collect_step(self._policy_out_device(self._rollout_obs()), self._action_mode(False), noise, self.action_noise)
        else:
            # policy network + sampling + collect step + the first gradient step's replay index draw in ONE launch; the gather
            # launch of that gradient step advances the ring position and the policy's Philox offset (hip_ops.rollout_step)
            idx = rb.predraw_indices(self.batch_size)
            hip_ops.rollout_step(env.obs, *net["weights"], net["act"], net["head"], net["out_act"], net["w2_swz"], net["rng_ctl"], env.coef,
                                 env.integrator, rb.ring, env.obs, env.step_count, self._action_mode(False), self.action_space.low,
                                 self.action_space.high, noise=noise, pcg_state=env.pcg_state, static_init=env.static_init,
                                 reward_out=env._rew, done_out=env._done, ep_return=self._ep_return, ep_stats=self._ep_stats,
                                 mt_state=rb.sampler_stream, sample_idx=idx)
            rb.note_predrawn(idx, None if net["rng_ctl"] is None else (net["rng_ctl"], env.num_envs))
            self._after_device_step(self.action_noise)
        self.policy.set_training_mode(True)
        self._train_device_only(self.gradient_steps, self.batch_size)
        if net is not None:
            rb._no_predrawn("the iteration's first gradient step")

    def _rollout_net(self) -> Optional[dict]:
        """The rollout policy as operands of hip_ops.rollout_step (weights = (w1, b1, w2, b2, w3, b3), act, head, out_act, w2_swz,
        rng_ctl), or None when the one-launch rollout does not cover this algorithm / network (the separate launches run then)."""
        return None

    def _graph_host_bookkeeping(self, log_interval: Optional[int]) -> None:
        self.replay_buffer.note_fused_add()
        self._last_obs = self._rollout_obs()
        self.num_timesteps += self.n_envs
        self._update_current_progress_remaining(self.num_timesteps, self._total_timesteps)
        self._train_host_only(self.gradient_steps)
        self._sync_episode_stats(log_interval)

    def _graph_shift_phase(self, iterations: int) -> None:
        self._n_updates += iterations * self.gradient_steps  # what `_train_host_only` adds per iteration (TD3 / MADDPG / BCQ phases)

    def _drop_recording_debts(self) -> None:
        rb = getattr(self, "replay_buffer", None)
        if rb is not None and hasattr(rb, "_predrawn"):
            rb._predrawn = None
        self._rng_advance = None

    def _sde_rollout_resets(self, num_collected_steps: int) -> None:
        """gSDE: the exploration matrices are redrawn (one per env) when a rollout starts (:550-551) and every `sde_sample_freq`
        collected steps (:556-558); a graph-captured iteration is a one-step rollout and records both draws."""
        if not self.use_sde:
            return
        if num_collected_steps == 0:
            self.policy.reset_noise(self.env.num_envs)
        if self.sde_sample_freq > 0 and num_collected_steps % self.sde_sample_freq == 0:
            self.policy.reset_noise(self.env.num_envs)

    def _warmup(self, learning_starts: int) -> bool:
        """:386: uniform warm-up actions, unless gSDE acts from the start (use_sde_at_warmup)"""
        return self.num_timesteps < learning_starts and not (self.use_sde and self.use_sde_at_warmup)

    # ---- action selection -----------------------------------------------------------------------------------------
    def _action_mode(self, warmup: bool) -> int:
        """`squashed` bit field of cstr_collect_step_f32: bit 0 = the input is the actor's tanh output (predict()
        unscales it first); bit 1 = multi-agent behaviour (no scale/unscale round trip, no noise)."""
        return 0 if warmup else 1

    def _take_rng_advance(self):
        adv, self._rng_advance = self._rng_advance, None
        return adv

    def _policy_out_device(self, obs: th.Tensor) -> th.Tensor:
        """Actor output for the fused collect kernel: squashed ([-1,1]) action, device tensor [N, A], no grad."""
        with th.no_grad():
            return self.policy._predict(obs, deterministic=False).contiguous()

    def _sample_action(self, learning_starts: int, action_noise=None, n_envs: int = 1):
        """reference: off_policy_algorithm.py:364-411 (NumPy compatibility path)"""
        if self._warmup(learning_starts):
            unscaled_action = self.action_space.sample_batch(n_envs)
        else:
            assert self._last_obs is not None, "self._last_obs was not set"
            unscaled_action, _ = self.predict(self._last_obs, deterministic=False)
        scaled_action = self.policy.scale_action(unscaled_action)
        if action_noise is not None:
            scaled_action = np.clip(scaled_action + action_noise(), -1, 1)
        buffer_action = scaled_action
        action = self.policy.unscale_action(scaled_action)
        return action, buffer_action

    # ---- train(): the plumbing every learner shares -----------------------------------------------------------------
    def train(self, gradient_steps: int, batch_size: Optional[int] = None) -> None:
        """reference: sac.py:199-296, td3.py:154-211, maddpg.py:117-191, bcq.py:129-213 = host prologue (lr schedule) + device work +
        host epilogue (logger)."""
        if batch_size is None:
            batch_size = self.train_batch_size
            if batch_size is None:
                raise TypeError(f"{type(self).__name__}.train() missing 1 required positional argument: 'batch_size'")
        self.policy.set_training_mode(True)
        self._train_host_pre()
        self._train_device_only(gradient_steps, batch_size)
        self._train_host_only(gradient_steps)

    def _use_packed_batch(self) -> bool:
        return False

    def _stock_buffer(self) -> bool:
        """The HBM `ReplayBuffer` itself, without a VecNormalize normaliser: its rows can be sampled straight into critic-input rows."""
        return type(self.replay_buffer) is ReplayBuffer and self.replay_buffer.normalizer is None

    def _batch(self, batch_size: int):
        """The contiguous sample tensors (and this class's step tensors) for `batch_size`; they replace a packed batch."""
        if self._static_batch is None or self._static_batch.observations.shape[0] != batch_size or self._packed is not None:
            self._static_batch, self._packed = self.replay_buffer.alloc_batch(batch_size), None
            self._alloc_step_tensors(batch_size)
        return self._static_batch

    def _packed_batch(self, batch_size: int):
        """The critic-input rows (obs | act) the sampler writes directly; `_static_batch` becomes views of them."""
        if self._packed is None or self._packed.x_data.shape[0] != batch_size:
            self._packed = self.replay_buffer.alloc_packed_batch(batch_size, with_pi=self.packed_batch_with_pi)
            self._static_batch = self._packed.samples
            self._alloc_packed_step_tensors(batch_size)
        return self._packed

    def _sample(self, batch_size: int, gather_ok=False) -> tuple:
        """The sampling prologue of a gradient step -> (packed batch | None, gather | None, sample views). With `_use_packed_batch()`
        the rows land in the critic-input buffers; otherwise in the contiguous batch (through the normaliser, if any).
        gather_ok (True, or a predicate on the packed batch): the step's first layer can fetch the rows itself, so indices the
        rollout launch has drawn are handed on (`gather` = ReplayBuffer.take_predrawn(pb)) instead of gathered here."""
        if not self._use_packed_batch():
            return None, None, self.replay_buffer.sample_into(self._batch(batch_size))
        pb, gather = self._packed_batch(batch_size), None
        if gather_ok and fused.USE_GATHER_IN_FIRST_LAYER and (gather_ok is True or gather_ok(pb)):
            gather = self.replay_buffer.take_predrawn(pb)
        if gather is None:
            self.replay_buffer.sample_packed_into(pb)  # the sample + the critics' cat([obs, act])
        return pb, gather, pb.samples

    def _alloc_step_tensors(self, batch_size: int) -> None:
        """Hook of `_batch`: the per-step tensors whose shape follows the batch size."""
        self._target_q = th.empty(batch_size, 1, dtype=th.float32, device=self.device)

    def _alloc_packed_step_tensors(self, batch_size: int) -> None:
        """Hook of `_packed_batch` (`self._packed` is the new batch)."""
        self._alloc_step_tensors(batch_size)

    def _n_delayed_updates(self, gradient_steps: int, delay: int) -> int:
        """How many of the next `gradient_steps` updates are a `delay`-th one (the delayed policy update of TD3 / MADDPG / BCQ)."""
        return (self._n_updates + gradient_steps) // delay - self._n_updates // delay

    def _loss_slot(self, key: str) -> tuple:
        """(store_target, accumulate_target) of the loss kernel that logs `key`: the only gradient step of a train() call stores the
        value straight into the logged sum (no zero-fill launch); otherwise it goes to the `_loss_now` scratch and is added to the sum."""
        return (self._loss_sums[key], None) if self._single_step else (self._loss_now.get(key), self._loss_sums[key])

    def _chain_for(self, batch_size: int):
        """The row-chain form of the gradient step for this batch size (`chain_type`), or None: per-layer fused path. What is cached
        depends on shapes, architecture and the module flags alone; whether batches are packed follows the replay buffer's normaliser,
        which every learn() sets again, and is asked on every call."""
        if not self._use_packed_batch():
            return None
        cache, key = self._chain_cache, (batch_size, chain.USE_CHAIN, fused.USE_FUSED_LINEAR)
        if key not in cache:
            cache[key] = self.chain_type(self, batch_size) if self.chain_type.supported(self, batch_size) else None
        return cache[key]

    # ---- logging ---------------------------------------------------------------------------------------------------
    def _dump_logs(self) -> None:
        """reference: off_policy_algorithm.py:413-438"""
        time_elapsed = max((time.time_ns() - self.start_time) / 1e9, sys.float_info.epsilon)
        fps = int((self.num_timesteps - self._num_timesteps_at_start) / time_elapsed)
        if self.world_size > 1:
            fps *= self.world_size  # whole-job env-steps/s: every rank advances n_envs per vec-step
        self.logger.record("time/episodes", self._episode_num, exclude="tensorboard")
        n_ep, ret_sum, len_sum = self._ep_window
        if n_ep > 0:
            self.logger.record("rollout/ep_rew_mean", ret_sum / n_ep)
            self.logger.record("rollout/ep_len_mean", len_sum / n_ep)
        self.logger.record("time/fps", fps)
        self.logger.record("time/time_elapsed", int(time_elapsed), exclude="tensorboard")
        self.logger.record("time/total_timesteps", self.num_timesteps, exclude="tensorboard")
        if self.use_sde:  # :429-430, resolved when the logger writes
            with th.no_grad():
                self.logger.record("train/std", DeviceMean(self.actor.get_std().mean(), 1))
        self.logger.dump(step=self.num_timesteps)

    def _sync_episode_stats(self, log_interval: Optional[int], force: bool = False) -> None:
        """One blocking read of four doubles (episodes, sum of returns, sum of lengths). The reference learns about
        finished episodes from the host-side `dones` every vec-step (:590-602); here the counters live in HBM."""
        self._steps_since_sync += 1
        if not force and self._steps_since_sync < self.stats_sync_interval:
            return
        self._steps_since_sync = 0
        n_ep, ret_sum, len_sum, _ = self._ep_stats.cpu().tolist()
        self._episode_num = int(n_ep)
        done_since = self._episode_num - self._episodes_at_last_dump
        if log_interval is not None and done_since >= log_interval:
            w0, w1, w2 = getattr(self, "_ep_totals_at_dump", (0.0, 0.0, 0.0))
            self._ep_window = (n_ep - w0, ret_sum - w1, len_sum - w2)
            self._ep_totals_at_dump = (n_ep, ret_sum, len_sum)
            self._episodes_at_last_dump = self._episode_num
            self._dump_logs()

    def _on_step(self) -> None:
        pass

    # ---- storage (compatibility path) ------------------------------------------------------------------------------
    def _store_transition(self, replay_buffer, buffer_action, new_obs, reward, dones, infos) -> None:
        """reference: off_policy_algorithm.py:445-508"""
        next_obs = np.array(new_obs, copy=True)
        for i, done in enumerate(dones):
            if done and infos[i].get("terminal_observation") is not None:
                next_obs[i] = infos[i]["terminal_observation"]
        replay_buffer.add(self._last_obs, next_obs, buffer_action, reward, dones, infos)
        self._last_obs = new_obs

    # ---- rollouts --------------------------------------------------------------------------------------------------
    def collect_rollouts(self, env: VecEnv, callback: BaseCallback, train_freq: TrainFreq, replay_buffer: ReplayBuffer,
                         action_noise=None, learning_starts: int = 0, log_interval: Optional[int] = None) -> RolloutReturn:
        """reference: off_policy_algorithm.py:510-605"""
        self.policy.set_training_mode(False)
        num_collected_steps, num_collected_episodes = 0, 0
        assert train_freq.frequency > 0, "Should at least collect one step or episode."
        if env.num_envs > 1:
            assert train_freq.unit == TrainFrequencyUnit.STEP, "You must use only one env when doing episodic training."
        her = self._her_path()
        if self.goal_space is not None and not (her and train_freq.unit == TrainFrequencyUnit.STEP):
            raise ValueError("the goal face is collected on the device only: CSTRVecEnv(goal_conditioned=True), a HerReplayBuffer with the "
                             "env's n_envs, and a train_freq in steps")
        fast = (her or self._fast_path()) and train_freq.unit == TrainFrequencyUnit.STEP
        noop_cb = getattr(callback, "is_noop", False)
        callback.on_rollout_start()
        continue_training = True
        while should_collect_more_steps(train_freq, num_collected_steps, num_collected_episodes):
            self._sde_rollout_resets(num_collected_steps)
            if her:
                self._collect_one_her(env.unwrapped, replay_buffer, action_noise, learning_starts)
                new_obs, rewards, dones = self._last_obs, env._rew, env._done  # device tensors (for callbacks)
                infos = None
            elif fast:
                self._collect_one_fused(env.unwrapped, replay_buffer, action_noise, learning_starts)
                new_obs, rewards, dones = self._last_obs, env._rew, env._done  # device tensors (for callbacks)
                infos: Any = None
            else:
                if isinstance(self._last_obs, th.Tensor):
                    self._last_obs = self._last_obs.cpu().numpy()
                actions, buffer_actions = self._sample_action(learning_starts, action_noise, env.num_envs)
                new_obs, rewards, dones, infos = env.step(actions)
            self.num_timesteps += env.num_envs
            num_collected_steps += 1
            if not noop_cb:
                callback.update_locals(locals())
            if not callback.on_step():
                return RolloutReturn(num_collected_steps * env.num_envs, num_collected_episodes, continue_training=False)
            if not fast:
                self._store_transition(replay_buffer, buffer_actions, new_obs, rewards, dones, infos)
            self._update_current_progress_remaining(self.num_timesteps, self._total_timesteps)
            self._on_step()
            if fast:
                self._sync_episode_stats(log_interval)
            else:
                for idx, done in enumerate(dones):
                    if done:
                        num_collected_episodes += 1
                        self._episode_num += 1
                        if action_noise is not None:
                            kwargs = dict(indices=[idx]) if env.num_envs > 1 else {}
                            action_noise.reset(**kwargs)
                        if log_interval is not None and self._episode_num % log_interval == 0:
                            self._dump_logs()
        callback.on_rollout_end()
        return RolloutReturn(num_collected_steps * env.num_envs, num_collected_episodes, continue_training)

    def _collect_one_fused(self, env: CSTRVecEnv, rb: ReplayBuffer, action_noise, learning_starts: int) -> None:
        """One vec-step entirely in HBM: reference statements :561 (_sample_action), :564 (env.step), :580
        (_store_transition -> ReplayBuffer.add) in one HIP launch after the actor forward."""
        n = env.num_envs
        if self._warmup(learning_starts):
            # warm-up: uniform actions from the action space's own generator (:386-388); drawn on the host
            pol = th.as_tensor(self.action_space.sample_batch(n)).to(self.device)
            squashed = self._action_mode(warmup=True)
        else:
            pol = self._policy_out_device(self._rollout_obs())
            squashed = self._action_mode(warmup=False)
        noise = None
        if action_noise is not None:
            z = action_noise()
            noise = z if isinstance(z, th.Tensor) else th.as_tensor(np.asarray(z, np.float32))
            noise = noise.to(self.device, th.float32).reshape(n, -1).contiguous()
        with th.cuda.device(self.device):
            self._device_collect_step(pol, squashed, noise, action_noise)
        rb.note_fused_add()
        self._last_obs = self._rollout_obs()

    def _collect_one_her(self, env: CSTRVecEnv, rb, action_noise, learning_starts: int) -> None:
        """One vec-step on the goal face, entirely in HBM and without a host synchronisation: reference statements :561 (_sample_action),
        :564 (env.step) and :580 (_store_transition -> HerReplayBuffer.add) with Monitor's episode statistics in one HIP launch after the
        actor forward (cstr_goal_collect_step_f32): `_collect_one_fused`, whose observation (`_rollout_obs`) and launch
        (`_device_collect_step`) are the goal face's here."""
        if not HER_FUSED_COLLECT:
            return self._collect_one_her_elementwise(env, rb, action_noise, learning_starts)
        self._collect_one_fused(env, rb, action_noise, learning_starts)

    def _collect_one_her_elementwise(self, env: CSTRVecEnv, rb, action_noise, learning_starts: int) -> None:
        """`_collect_one_her` as the launches the fused one replaces (CSTR_HER_FUSED_COLLECT=0, the A/B form): :561 (_sample_action,
        :364-411: the same float32 expressions as the fused collect step, here as element-wise device ops), :564 (env.step =
        cstr_goal_vec_step_f32) and :580 (_store_transition -> HerReplayBuffer.add = cstr_her_add_f32), then Monitor's episode statistics."""
        n, dev = env.num_envs, self.device
        if not hasattr(self, "_act_lo"):
            self._act_lo = th.as_tensor(np.asarray(self.action_space.low, np.float32), device=dev)
            self._act_hi = th.as_tensor(np.asarray(self.action_space.high, np.float32), device=dev)
        lo, hi = self._act_lo, self._act_hi
        if self._warmup(learning_starts):
            v = th.as_tensor(self.action_space.sample_batch(n)).to(dev)  # :386-388, drawn on the host like the Box face's warm-up
        else:
            pol = self._policy_out_device(env.flat)
            adv = self._take_rng_advance()  # SAC's rollout head leaves its Philox offset to the launch behind it
            if adv is not None:
                adv[0][1] += adv[1]
            v = lo + (0.5 * (pol + 1.0) * (hi - lo))  # predict(): unscale_action (policies.py:375, :413)
        sc = 2.0 * ((v - lo) / (hi - lo)) - 1.0  # scale_action (policies.py:402)
        if action_noise is not None:
            z = action_noise()
            z = z if isinstance(z, th.Tensor) else th.as_tensor(np.asarray(z, np.float32))
            sc = th.clamp(sc + z.to(dev, th.float32).reshape(n, -1), -1.0, 1.0)  # :401-402
        sc = sc.contiguous()                                 # buffer_action (:405)
        ea = (lo + (0.5 * (sc + 1.0) * (hi - lo))).contiguous()  # unscale_action (:406)
        if getattr(self, "_her_rows", None) is None or self._her_rows.shape != env.flat.shape:
            self._her_rows = th.empty_like(env.flat)
            self._ep_len = th.zeros(n, dtype=th.float32, device=dev)
        self._her_rows.copy_(env.flat)  # _last_obs: the step overwrites the env's rows
        _, rew, done, tout, nxt = env.step_device(ea)
        rb.add_device(self._her_rows, nxt, sc, rew, done, tout)
        # Monitor semantics: return / length of the episodes that end here (core/common/monitor.py:96-109), accumulated in HBM
        ret, length = self._ep_return + rew, self._ep_len + 1.0
        self._ep_stats[0] += done.sum().double()
        self._ep_stats[1] += (ret * done).sum().double()
        self._ep_stats[2] += (length * done).sum().double()
        self._ep_return.copy_(ret * (1.0 - done))
        self._ep_len.copy_(length * (1.0 - done))
        self._after_device_step(action_noise)
        self._last_obs = env.flat

    def _rollout_obs(self) -> th.Tensor:
        """What the rollout policy sees: the env's observation, through VecNormalize when the env is wrapped in one."""
        vn = self._vec_normalize_env
        if self.goal_space is not None:
            return self._denv.flat
        return self._denv.obs if vn is None else vn.norm_obs_dev

    def _device_collect_step(self, pol: th.Tensor, squashed: int, noise: Optional[th.Tensor], action_noise) -> None:
        """The device rollout step behind the policy output `pol`, for the eager and the captured iteration alike: the fused collect
        launch (action scaling chain + env step + auto-reset + ring row write + episode statistics), then `_after_device_step`."""
        env, rb = self._denv, self.replay_buffer
        if env.goal_conditioned:  # the goal face: the env hands the launch its own arrays, the HER bookkeeping rides along
            env.collect_step_device(rb.ring, rb.her, pol, squashed, self.action_space.low, self.action_space.high, noise=noise,
                                    ep_return=self._ep_return, ep_stats=self._ep_stats, rng_advance=self._take_rng_advance())
        else:
            hip_ops.collect_step(env.coef, env.integrator, rb.ring, env.obs, env.step_count, pol, squashed,
                                 self.action_space.low, self.action_space.high, noise=noise, pcg_state=env.pcg_state, static_init=env.static_init,
                                 reward_out=env._rew, done_out=env._done, ep_return=self._ep_return, ep_stats=self._ep_stats,
                                 rng_advance=self._take_rng_advance())
        self._after_device_step(action_noise)

    def _after_device_step(self, action_noise) -> None:
        if hasattr(action_noise, "reset_done"):
            action_noise.reset_done(self._denv._done)  # action_noise.reset(indices of finished envs), :596-599
        if self._vec_normalize_env is not None:
            self._vec_normalize_env.after_device_step()  # VecNormalize.step_wait on the raw outputs (vec_normalize.py:174-204)
