"""DQN with the reference's constructor, defaults, `_on_step`, `train()` arithmetic and logger keys (reference: core/dqn/dqn.py:19-283)
on the HIP path, over the discretised valve face of the CSTR env (`CSTRVecEnv(num_envs, discrete_actions=K)`).

A vec-step on the kernel path: the Q network through the per-layer Linear kernels, one `RandomState.random_sample()` on the device
image of NumPy's legacy stream compared with the exploration rate (hip_ops.mt19937_rand_flag, dqn.py:245), the action selection
(hip_ops.dqn_act) and the fused collect launch. The replay ring keeps the VALVE PAIR of the chosen index, not the index: every env /
ring / sampler kernel is the continuous algorithms', `replay_buffer.sample()` returns valve pairs (the reference: int64 [B, 1]), and
a saved buffer is directly a BCQ dataset. A gradient step: the sample launch, `q_net_target(next_obs)` and `q_net(obs)`, ONE launch for
dqn.py:195-212 (hip_ops.dqn_loss: greedy target, gather, Huber loss, d loss / d q), the backward with one deferred weight-gradient
launch, the gradient clip over the flat arena and the FlatAdam step. Nothing synchronises with the host. Another optimiser class, or
`fused_learner = False`, runs the reference's own torch statements on the arena parameters; they are also the tests' reference.

`faithful_quirks=True` (default) keeps the reference's exploration: ONE `rand()` per vec-step, so all envs explore together or none
does. `False` explores per env (u < epsilon for each row, Philox). The exploration rate starts at 0.0 and is set in `_on_step`, so a
step uses the rate the previous step set (the reference's order); warm-up steps draw `action_space.sample()` and consume no `rand()`.

hipGraph replay (`enable_graph_capture`): one body = `train_freq` vec-steps, then `gradient_steps` gradient steps. The exploration
rate changes every vec-step, so it lives in HBM: before a replay the host evaluates the schedule for every vec-step of it and copies
the values into a slot array; each recorded launch reads its own slot. Target updates are part of the body; the cache key carries the
in-body positions at which `_n_calls` hits the update period.

Not built (each raises where reachable): CnnPolicy / MultiInputPolicy, a VecNormalize-wrapped env, data-parallel training
(world_size > 1), optimize_memory_usage, HER (core/her and the env's goal face serve SAC, TD3 and DDPG)."""
import warnings
from typing import List, Optional, Union

import numpy as np
import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.buffers import ReplayBuffer
from core.common.logger import DeviceMean
from core.common.off_policy_algorithm import OffPolicyAlgorithm
from core.common.spaces import Discrete
from core.common.type_aliases import TrainFrequencyUnit
from core.common.utils import get_linear_fn
from core.common.vec_env.cstr_vec_env import decode_valve_index
from core.dqn.policies import MlpPolicy

EPS_SLOTS = 1024  # exploration-rate slots in HBM: vec-steps one replayed graph may hold (train_freq * unroll)


class DQN(OffPolicyAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    train_batch_size = 100

    def __init__(self, policy, env, learning_rate=1e-4, buffer_size: int = 1_000_000, learning_starts: int = 100, batch_size: int = 32,
                 tau: float = 1.0, gamma: float = 0.99, train_freq: Union[int, tuple] = 4, gradient_steps: int = 1,
                 replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None, optimize_memory_usage: bool = False,
                 target_update_interval: int = 10000, exploration_fraction: float = 0.1, exploration_initial_eps: float = 1.0,
                 exploration_final_eps: float = 0.05, max_grad_norm: float = 10, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device: Union[th.device, str] = "auto", _init_setup_model: bool = True, faithful_quirks: bool = True):
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps,
                         action_noise=None, replay_buffer_class=replay_buffer_class, replay_buffer_kwargs=replay_buffer_kwargs,
                         policy_kwargs=policy_kwargs, stats_window_size=stats_window_size, tensorboard_log=tensorboard_log,
                         verbose=verbose, device=device, seed=seed, sde_support=False, optimize_memory_usage=optimize_memory_usage,
                         supported_action_spaces=(Discrete,), support_multi_env=True)
        if self.env is None:
            raise ValueError("DQN needs its environment at construction: CSTRVecEnv(num_envs, discrete_actions=K)")
        if self._vec_normalize_env is not None:
            raise NotImplementedError("DQN on a VecNormalize-wrapped env is not built")
        if self._denv is None or self._denv.discrete_actions is None:
            raise ValueError("DQN needs the discrete valve face of the device env: CSTRVecEnv(num_envs, discrete_actions=K)")
        if self.world_size > 1:
            raise NotImplementedError("DQN: data-parallel training (world_size > 1) is not built")
        self.exploration_initial_eps = exploration_initial_eps
        self.exploration_final_eps = exploration_final_eps
        self.exploration_fraction = exploration_fraction
        self.target_update_interval = target_update_interval
        self._n_calls = 0  # vec-steps so far: the target update counts these (:134-135)
        self.max_grad_norm = max_grad_norm
        self.exploration_rate = 0.0
        self.faithful_quirks = faithful_quirks
        self.debug_capture = False  # True: every gradient step keeps its Q values, targets, loss, gradient norm and sampled indices
        self.train_capture: List[dict] = []
        # teacher-forcing hooks (tests): batches (obs, index, next_obs, reward, done) the next gradient steps use instead of a sample,
        # and uniforms [n_envs, 2] the next vec-steps' action selection reads instead of drawing
        self.batch_queue: List[tuple] = []
        self.uniform_queue: List[th.Tensor] = []
        if _init_setup_model:
            self._setup_model()

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        env = self._denv
        self.levels = env.discrete_actions
        if self.replay_buffer is None:  # the ring holds the valve pair: the buffer is built over the env's valve space
            if self.replay_buffer_class is None:
                self.replay_buffer_class = ReplayBuffer
            self.replay_buffer = self.replay_buffer_class(self.buffer_size, self.observation_space, env.valve_space, device=self.device,
                                                          n_envs=self.n_envs, optimize_memory_usage=self.optimize_memory_usage,
                                                          **self.replay_buffer_kwargs)
        super()._setup_model()
        self.exploration_schedule = get_linear_fn(self.exploration_initial_eps, self.exploration_final_eps, self.exploration_fraction)
        if self.n_envs > 1 and self.n_envs > self.target_update_interval:
            warnings.warn("The number of environments used is greater than the target network "
                          f"update interval ({self.n_envs} > {self.target_update_interval}), "
                          "therefore the target network will be updated after each call to env.step() "
                          f"which corresponds to {self.n_envs} steps.")
        dev, n = self.device, self.n_envs
        from core.common.arena import FlatAdam

        self._setup_networks()
        self.fused_learner = isinstance(self.policy.optimizer, FlatAdam)
        self.policy.greedy_index = self._greedy_index
        z = lambda: th.zeros(1, dtype=th.float32, device=dev)  # noqa: E731
        self._loss_sums, self._loss_now = dict(loss=z()), dict(loss=z())
        self._static_batch, self._packed = None, None
        self._ws = hip_ops.new_ppo_workspace(dev)
        self._grad_norm = z()
        self._flag = th.zeros(1, dtype=th.int32, device=dev)
        self._valve = th.zeros(n, 2, dtype=th.float32, device=dev)
        self._eps_slots = th.zeros(EPS_SLOTS, dtype=th.float64, device=dev)
        self._eps_written: list = [0.0] * EPS_SLOTS
        self._slot_base = 0
        self._predict_eps = th.zeros(1, dtype=th.float64, device=dev)
        lo, hi = env.valve_space.low, env.valve_space.high
        self._valve_low, self._valve_high = [float(v) for v in lo], [float(v) for v in hi]

    def _setup_networks(self) -> None:
        """the policy's two networks under the reference's names (_create_aliases, :164-166) and as per-layer kernel passes"""
        self.q_net, self.q_net_target = self.policy.q_net, self.policy.q_net_target
        if not (fused.FastMLP.supported(self.q_net.q_net) and hip_ops.dqn_supported(int(self.action_space.n), self.levels)):
            raise NotImplementedError("DQN: the Q network must be Linear (+ ReLU / Tanh) layers over a valve face of 2..16 levels")
        self._fast_q = fused.FastMLP(self.q_net.q_net)
        self._fast_q_target = fused.FastMLP(self.q_net_target.q_net)

    def _reseed_device_rng(self, seed: int) -> None:
        super()._reseed_device_rng(seed)
        if getattr(self, "_rng_ctl", None) is None:  # the exploration stream follows the seed from the start
            self._rng_ctl = hip_ops.new_rng_ctl(seed, self.device)

    # ---- action selection -----------------------------------------------------------------------------------------
    def _q_values(self, obs: th.Tensor) -> th.Tensor:
        with th.no_grad():
            return self._fast_q(obs, train_params=False)

    def _greedy_index(self, obs: th.Tensor) -> th.Tensor:
        """argmax_a Q(obs, a) through the kernel path: int64 [n]"""
        with th.cuda.device(self.device):
            obs = obs.to(self.device, th.float32).contiguous()
            n = obs.shape[0]
            valve = th.empty(n, 2, dtype=th.float32, device=self.device)
            index = th.empty(n, dtype=th.int64, device=self.device)
            hip_ops.dqn_act(self._q_values(obs), self.levels, hip_ops.DQN_GREEDY, valve, index)
        return index

    def _write_eps(self, values: list, first: int = 0) -> None:
        """exploration rates into the HBM slots first .. first + len(values): one asynchronous fill per slot whose value changes
        (none once the schedule has reached its final value), the double travels as a kernel argument"""
        for i, v in enumerate(values, first):
            if self._eps_written[i] != v:
                self._eps_slots[i:i + 1].fill_(v)
                self._eps_written[i] = v

    def _device_vec_step(self, eps_slot: th.Tensor) -> None:
        """One vec-step, launches only: Q values, exploration draw, action selection, fused collect. `eps_slot`: the device double
        holding this step's exploration rate."""
        rb = self.replay_buffer
        q = self._q_values(self._rollout_obs())
        u = self.uniform_queue.pop(0).to(self.device, th.float32).contiguous() if self.uniform_queue else None
        rng = None if u is not None else self._device_rng()
        if self.faithful_quirks:  # :245: one rand() for the whole vec-step, on the stream the sampler shares
            hip_ops.mt19937_rand_flag(rb.sampler_stream, eps_slot, self._flag)
            hip_ops.dqn_act(q, self.levels, hip_ops.DQN_ALL_OR_NONE, self._valve, flag=self._flag, u=u, rng_ctl=rng)
        else:
            hip_ops.dqn_act(q, self.levels, hip_ops.DQN_PER_ROW, self._valve, eps=eps_slot, u=u, rng_ctl=rng)
        self._collect_valves()

    def _collect_valves(self) -> None:
        """the fused collect launch on `self._valve`: buffer action = env action = the valve pair (`squashed` bit 1)"""
        env, rb = self._denv, self.replay_buffer
        hip_ops.collect_step(env.coef, env.integrator, rb.ring, env.obs, env.step_count, self._valve, 2, self._valve_low, self._valve_high,
                             pcg_state=env.pcg_state, static_init=env.static_init, reward_out=env._rew, done_out=env._done,
                             ep_return=self._ep_return, ep_stats=self._ep_stats)

    def _collect_one_fused(self, env, rb, action_noise, learning_starts: int) -> None:
        with th.cuda.device(self.device):
            if self._warmup(learning_starts):
                # warm-up: uniform indices from the action space's own generator (off_policy_algorithm.py:386-388), drawn on the host
                idx = self.action_space.sample_batch(env.num_envs)
                self._valve.copy_(th.from_numpy(decode_valve_index(idx, self.levels)))
                self._collect_valves()
            else:
                self._write_eps([float(self.exploration_rate)])
                self._device_vec_step(self._eps_slots[0:1])
        rb.note_fused_add()
        self._last_obs = self._rollout_obs()

    def _sample_action(self, learning_starts: int, action_noise=None, n_envs: int = 1):
        raise NotImplementedError("DQN runs on the device path only: CSTRVecEnv(num_envs, discrete_actions=K) and the stock ReplayBuffer")

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """:228-256: epsilon-greedy around the policy's greedy index; the `rand()` comes from the device legacy stream"""
        if not deterministic:
            with th.cuda.device(self.device):
                self._predict_eps.fill_(float(self.exploration_rate))
                hip_ops.mt19937_rand_flag(self.replay_buffer.sampler_stream, self._predict_eps, self._flag)
            if bool(self._flag.item()):
                obs = np.asarray(observation.cpu() if isinstance(observation, th.Tensor) else observation)
                if obs.ndim == len(self.observation_space.shape) + 1:  # is_vectorized_observation
                    return self.action_space.sample_batch(obs.shape[0]), state
                return np.array(self.action_space.sample()), state
        return self.policy.predict(observation, state, episode_start, deterministic)

    # ---- _on_step (:168-182) ----------------------------------------------------------------------------------------
    def _target_period(self) -> int:
        return max(self.target_update_interval // self.n_envs, 1)

    def _target_update(self) -> None:
        """polyak_update(q_net, q_net_target, tau): one launch over the two flat arenas (there are no batch-norm statistics)"""
        self.policy.target_arena.polyak_from(self.policy.arena, self.tau)

    def _on_step_host(self) -> None:
        self.exploration_rate = self.exploration_schedule(self._current_progress_remaining)
        self.logger.record("rollout/exploration_rate", self.exploration_rate)

    def _on_step(self) -> None:
        self._n_calls += 1
        if self._n_calls % self._target_period() == 0:
            self._target_update()
        self._on_step_host()

    # ---- train (:184-226) -------------------------------------------------------------------------------------------
    def _alloc_step_tensors(self, batch_size: int) -> None:
        super()._alloc_step_tensors(batch_size)
        e = lambda *s: th.empty(*s, dtype=th.float32, device=self.device)  # noqa: E731
        self._g_q, self._cur_q = e(batch_size, int(self.action_space.n)), e(batch_size, 1)

    def _train_host_pre(self) -> None:
        self._update_learning_rate(self.policy.optimizer)

    def _graph_host_pre(self) -> None:
        """A replayed body trains AFTER its train_freq vec-steps: the learning-rate schedule sees the progress train() would see then,
        and every vec-step of the coming replay gets its exploration rate into its HBM slot."""
        tf, n = self.train_freq.frequency, self.n_envs
        keep = self._current_progress_remaining
        self._update_current_progress_remaining(self.num_timesteps + tf * n, self._total_timesteps)
        self._train_host_pre()
        self._current_progress_remaining = keep
        rates = [float(self.exploration_rate)]
        for k in range(1, tf * self._graph_unroll_now()):
            rates.append(float(self.exploration_schedule(1.0 - float(self.num_timesteps + k * n) / float(self._total_timesteps))))
        self._write_eps(rates)

    def _train_host_only(self, gradient_steps: int) -> None:
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/loss", DeviceMean(self._loss_sums["loss"], gradient_steps))

    def _next_batch(self, batch_size: int):
        """(samples, batch_inds, env_indices): the next teacher-forced batch, else a sample of the ring"""
        rd = self._batch(batch_size)
        if self.batch_queue:
            obs, index, next_obs, reward, done = self.batch_queue.pop(0)
            valve = decode_valve_index(np.asarray(index).reshape(-1), self.levels)
            for dst, src in zip((rd.observations, rd.actions, rd.next_observations, rd.dones, rd.rewards), (obs, valve, next_obs, done, reward)):
                dst.copy_(th.as_tensor(np.ascontiguousarray(src, dtype=np.float32)).reshape(dst.shape))
            return rd, None, None
        if self.debug_capture:
            bi, ei = (th.empty(batch_size, dtype=th.int64, device=self.device) for _ in range(2))
            return self.replay_buffer.sample_into(rd, bi, ei), bi, ei
        return self.replay_buffer.sample_into(rd), None, None

    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        self._single_step = gradient_steps == 1 and self.fused_learner
        if not self._single_step:
            self._loss_sums["loss"].zero_()
        with th.cuda.device(self.device):
            for _ in range(gradient_steps):
                rd, bi, ei = self._next_batch(batch_size)
                step = self._gradient_step_fused if self.fused_learner else self._gradient_step_torch
                cur, target, loss = step(rd)
                if self.debug_capture:
                    self.train_capture.append(dict(current_q=cur.detach().reshape(-1).clone(), target_q=target.reshape(-1).clone(),
                                                   loss=loss.detach().reshape(1).clone(), grad_norm=self._grad_norm.clone(),
                                                   batch_inds=None if bi is None else bi.clone(), env_indices=None if ei is None else ei.clone(),
                                                   **self._capture_extra()))

    def _capture_extra(self) -> dict:
        """what a subclass's gradient step adds to a `train_capture` entry"""
        return {}

    def _gradient_step_fused(self, rd):
        """:195-220 on the kernel path"""
        with th.no_grad():
            next_q = self._fast_q_target(rd.next_observations, train_params=False)
        q = self._fast_q(rd.observations, train_params=True)
        l_out, l_sum = self._loss_slot("loss")
        cap = self.debug_capture
        hip_ops.dqn_loss(q.detach(), next_q, rd.actions, rd.rewards, rd.dones, self.gamma, self.levels, self._g_q, l_out, self._ws,
                         loss_sum=l_sum, cur_q_out=self._cur_q if cap else None, target_out=self._target_q if cap else None)
        with fused.deferred_weight_grads():
            th.autograd.backward([q], [self._g_q])
        hip_ops.grad_clip(self.policy.arena.grad, self.max_grad_norm, self._ws, self._grad_norm)
        self.policy.optimizer.step()
        return self._cur_q, self._target_q, l_out

    def _gradient_step_torch(self, rd):
        """:195-220 as the reference's own torch statements on the arena parameters"""
        k = self.levels
        with th.no_grad():
            level = th.round(((rd.actions + 1.0) * float(k - 1)) / 2.0).clamp_(0, k - 1).long()
            index = (level[:, 0] * k + level[:, 1]).reshape(-1, 1)  # what the reference's buffer holds: int64 [B, 1]
            next_q_values = self.q_net_target(rd.next_observations)
            next_q_values, _ = next_q_values.max(dim=1)
            next_q_values = next_q_values.reshape(-1, 1)
            target_q_values = rd.rewards + (1 - rd.dones) * self.gamma * next_q_values
        current_q_values = self.q_net(rd.observations)
        current_q_values = th.gather(current_q_values, dim=1, index=index)
        loss = F.smooth_l1_loss(current_q_values, target_q_values)
        self._loss_sums["loss"] += loss.detach()
        self.policy.optimizer.zero_grad()
        loss.backward()
        norm = th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
        self._grad_norm.copy_(norm.detach().reshape(1))
        self.policy.optimizer.step()
        return current_q_values, target_q_values, loss

    # ---- hipGraph replay: the hooks of core/common/graph_replay.py for a body of train_freq vec-steps ---------------------
    def _graph_steps_per_iteration(self) -> int:
        return self.train_freq.frequency * self.n_envs

    def _update_positions(self, n_calls: int, count: int) -> tuple:
        """the k in 0 .. count - 1 at which vec-step n_calls + k + 1 is a target update"""
        period = self._target_period()
        return tuple(k for k in range(count) if (n_calls + k + 1) % period == 0)

    def _graph_eligible(self, callback) -> bool:
        tf = self.train_freq
        return (self._fast_path() and self._callback_allows_replay(callback) and tf.unit == TrainFrequencyUnit.STEP
                and self.gradient_steps >= 1 and self.num_timesteps >= self.learning_starts and not self.debug_capture
                and not self.batch_queue and not self.uniform_queue and tf.frequency * max(self.graph_unroll, 1) <= EPS_SLOTS)

    def _graph_phase(self) -> int:
        return sum(1 << k for k in self._update_positions(self._n_calls, self.train_freq.frequency))

    def _graph_cache_key(self, unroll: int) -> tuple:
        tf = self.train_freq.frequency
        return (id(self._denv.coef), self.batch_size, self.gradient_steps, tf, self.faithful_quirks, self.fused_learner,
                self._update_positions(self._n_calls, tf * unroll), unroll)

    def _graph_body(self) -> None:
        tf = self.train_freq.frequency
        self.policy.set_training_mode(False)
        updates = self._update_positions(self._n_calls, tf)
        for k in range(tf):
            s = self._slot_base + k
            self._device_vec_step(self._eps_slots[s:s + 1])
            if k in updates:
                self._target_update()
        self.policy.set_training_mode(True)
        self._train_device_only(self.gradient_steps, self.batch_size)

    def _graph_shift_phase(self, iterations: int) -> None:
        super()._graph_shift_phase(iterations)
        self._n_calls += iterations * self.train_freq.frequency
        self._slot_base += iterations * self.train_freq.frequency

    def _graph_host_bookkeeping(self, log_interval) -> None:
        for _ in range(self.train_freq.frequency):
            self.replay_buffer.note_fused_add()
            self.num_timesteps += self.n_envs
            self._update_current_progress_remaining(self.num_timesteps, self._total_timesteps)
            self._n_calls += 1  # the host half of _on_step: the target update is a launch of the body
            self._on_step_host()
        self._last_obs = self._rollout_obs()
        self._train_host_only(self.gradient_steps)
        self._sync_episode_stats(log_interval)

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "DQN", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def _get_torch_save_params(self) -> tuple:
        """reference: dqn.py:279-283"""
        return ["policy", "policy.optimizer"], []

    def _extra_save_data(self) -> dict:
        return dict(target_update_interval=self.target_update_interval, exploration_fraction=self.exploration_fraction,
                    exploration_initial_eps=self.exploration_initial_eps, exploration_final_eps=self.exploration_final_eps,
                    max_grad_norm=self.max_grad_norm, faithful_quirks=self.faithful_quirks, exploration_rate=self.exploration_rate,
                    _n_calls=self._n_calls, discrete_actions=self.levels)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return super()._ctor_keys() + ("target_update_interval", "exploration_fraction", "exploration_initial_eps",
                                       "exploration_final_eps", "max_grad_norm", "faithful_quirks")

    @classmethod
    def _check_archive(cls, data: dict, env) -> None:
        levels = getattr(getattr(env, "unwrapped", env), "discrete_actions", None)
        if "discrete_actions" in data and levels != data["discrete_actions"]:
            raise ValueError(f"the archive was written for discrete_actions={data['discrete_actions']}, the env has {levels}")

    def _restore_extra(self, data: dict) -> None:
        self.exploration_rate = float(data.get("exploration_rate", 0.0))
        self._n_calls = int(data.get("_n_calls", 0))
