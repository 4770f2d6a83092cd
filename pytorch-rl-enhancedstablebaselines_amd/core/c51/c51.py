"""C51, categorical DQN (Bellemare, Dabney & Munos 2017, "A Distributional Perspective on Reinforcement Learning") on DQN: the
exploration draw, the vec-step, the replay ring of valve pairs, the samplers (`n_steps` included), the hard target update, `predict`'s
epsilon-greedy, the hipGraph body and the checkpoint plumbing are DQN's (core/dqn/dqn.py), unchanged. The network outputs the logits
of a softmax over N = n_atoms atoms per action (core/c51/policies.py, [B, M, N], M = K * K valve pairs) on the fixed support
z_i = v_min + i * dz, dz = (v_max - v_min) / (N - 1), and three things change:

    greedy action:  argmax_a sum_i z_i softmax_i(logits(s)[a])
    with no gradient:  p' = softmax(categorical_net_target(s'));  a* = argmax_a sum_i z_i p'[a, i]
        Tz_j = clamp(r + (1 - d) * gamma * z_j, v_min, v_max);  b_j = (Tz_j - v_min) / dz
        m_i = sum_j p'[a*, j] * max(0, 1 - |b_j - i|)                        (the paper's projection, eq. 7, as a gather)
    loss = mean over b of -sum_i m_i log_softmax(categorical_net(s)[a])_i     (cross-entropy against the projected target)
    -> clip_grad_norm_ when max_grad_norm is not None -> Adam step, eps = 0.01 / batch_size by default

ACTION SELECTION RUNS ON THE FUSED ATOM HEAD. The expected value is not linear in the last layer, so QR-DQN's folded head does not
apply; hip_ops.c51_head_q runs the last layer's GEMM, the softmax over the atoms and the expectation in one launch on the hidden
activations, and the [n_envs, M * N] logits of a vec-step are never written. It reads the last layer's weight and bias in place in
front of every pass: nothing can go stale. A hidden width the kernel declines (not a multiple of 4, or above 512) takes the last
Linear launch plus torch's softmax and expectation. DQN's cstr_dqn_act_f32 takes the [n_envs, M] values either way.

A gradient step on the kernel path (FlatAdam, hip_ops.c51_supported: N <= 256): the sample launch, the target network on s' and the
online network on s through the per-layer kernels (full logit rows, [B, M * N]), ONE hip_ops.c51_loss call for everything between
them and loss.backward(), the backward with one deferred weight-gradient launch, the gradient clip only when asked for, the FlatAdam
step. `done` enters the loss only as (1 - done) * gamma, so an n-step batch hands over its fold and `n_steps > 1` needs nothing else.
Another optimiser class, N > 256 or `fused_learner = False` runs the same statements in torch on the arena parameters
(`_gradient_step_torch`, `c51_loss_torch`).

Not built (each raises where reachable): DQN's list (CnnPolicy / MultiInputPolicy, VecNormalize, data-parallel training,
optimize_memory_usage, HER), the MultiDiscrete face, prioritized replay (the loss launch takes no importance weights)."""
from typing import Optional, Union

import torch as th

from core.common import fused, hip_ops
from core.common.type_aliases import td_discount, td_done
from core.c51.policies import MlpPolicy
from core.dqn.dqn import DQN


def c51_loss_torch(logits: th.Tensor, next_logits: th.Tensor, index: th.Tensor, rewards: th.Tensor, coef: th.Tensor, v_min: float,
                   v_max: float) -> dict:
    """The statements of cstr_c51_loss_f32 in plain torch, in the dtype and on the device of its inputs: logits / next_logits [B, M, N]
    (online at s, target at s'), index int64 [B] the taken action, rewards and coef = (1 - done) * gamma [B, 1]. -> m, logp [B, N],
    row_loss [B], loss, next_index [B]; `loss` carries the graph to `logits`."""
    n = logits.shape[2]
    dz = (v_max - v_min) / (n - 1)
    support = th.linspace(v_min, v_max, n, dtype=logits.dtype, device=logits.device)
    rows = th.arange(logits.shape[0], device=logits.device)
    with th.no_grad():
        next_probs = th.softmax(next_logits, dim=2)
        next_index = (next_probs * support).sum(dim=2).argmax(dim=1)
        p = next_probs[rows, next_index]  # [B, N]
        tz = (rewards + coef * support).clamp(v_min, v_max)
        b = ((tz - v_min) / dz).clamp(0, n - 1)
        atoms = th.arange(n, dtype=logits.dtype, device=logits.device).view(1, n, 1)
        m = ((1 - (b.unsqueeze(1) - atoms).abs()).clamp(min=0) * p.unsqueeze(1)).sum(dim=2)  # m[b, i] = sum_j hat(b_j - i) p_j
    logp = th.log_softmax(logits[rows, index], dim=1)
    row_loss = -(m * logp).sum(dim=1)
    return dict(m=m, logp=logp, row_loss=row_loss, loss=row_loss.mean(), next_index=next_index)


class C51(DQN):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    supports_prioritized_replay = False  # the projection loss launch takes no importance weights

    def __init__(self, policy, env, learning_rate=1e-4, buffer_size: int = 1_000_000, learning_starts: int = 100, batch_size: int = 32,
                 tau: float = 1.0, gamma: float = 0.99, train_freq: Union[int, tuple] = 4, gradient_steps: int = 1,
                 replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None, optimize_memory_usage: bool = False,
                 target_update_interval: int = 10000, exploration_fraction: float = 0.1, exploration_initial_eps: float = 1.0,
                 exploration_final_eps: float = 0.05, max_grad_norm: Optional[float] = 10, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device: Union[th.device, str] = "auto", _init_setup_model: bool = True, faithful_quirks: bool = True, *, n_steps: int = 1,
                 v_min: float = -10.0, v_max: float = 10.0):
        self.v_min, self.v_max = float(v_min), float(v_max)
        if not (self.v_max > self.v_min and abs(self.v_min) < float("inf") and abs(self.v_max) < float("inf")):
            raise ValueError(f"C51: the support needs finite v_min < v_max, got v_min={v_min}, v_max={v_max}")
        policy_kwargs = self.default_policy_kwargs(policy_kwargs, batch_size)
        policy_kwargs.update(v_min=self.v_min, v_max=self.v_max)
        self.n_atoms = int(policy_kwargs.get("n_atoms", 51))
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps,
                         replay_buffer_class=replay_buffer_class, replay_buffer_kwargs=replay_buffer_kwargs,
                         optimize_memory_usage=optimize_memory_usage, target_update_interval=target_update_interval,
                         exploration_fraction=exploration_fraction, exploration_initial_eps=exploration_initial_eps,
                         exploration_final_eps=exploration_final_eps, max_grad_norm=max_grad_norm, stats_window_size=stats_window_size,
                         tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device,
                         _init_setup_model=_init_setup_model, faithful_quirks=faithful_quirks, n_steps=n_steps)

    @staticmethod
    def default_policy_kwargs(policy_kwargs: Optional[dict], batch_size: int) -> dict:
        """A copy of the caller's policy_kwargs with the published default filled in: when no optimiser class is named, Adam (the
        policy's default class) with the paper's eps = 0.01 / batch_size."""
        policy_kwargs = dict(policy_kwargs or {})
        n_atoms = int(policy_kwargs.get("n_atoms", 51))
        if n_atoms < 2:
            raise ValueError(f"C51: n_atoms must be at least 2, got {n_atoms}")
        if "optimizer_class" not in policy_kwargs:
            policy_kwargs["optimizer_kwargs"] = dict(eps=0.01 / batch_size)
        return policy_kwargs

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        super()._setup_model()
        m, n = int(self.action_space.n), self.n_atoms
        # the kernel path: DQN's (FlatAdam), with an atom count the loss launch takes; otherwise the torch statements
        self.fused_learner = bool(self.fused_learner and hip_ops.c51_supported(m, self.levels, n))
        hidden = self._fast_q.layers[-1][0].in_features
        self._head_kernel = hip_ops.c51_supported(m, self.levels, n, hidden)  # else: the last Linear launch + torch's softmax
        self._support = th.linspace(self.v_min, self.v_max, n, dtype=th.float32, device=self.device)

    def _setup_networks(self) -> None:
        self.categorical_net, self.categorical_net_target = self.policy.categorical_net, self.policy.categorical_net_target
        seq, seq_t = self.categorical_net.categorical_net, self.categorical_net_target.categorical_net
        if not (fused.FastMLP.supported(seq) and hip_ops.dqn_supported(int(self.action_space.n), self.levels)):
            raise NotImplementedError("C51: the categorical network must be Linear (+ ReLU / Tanh) layers over a valve face of 2..16 levels")
        self._fast_q, self._fast_q_target = fused.FastMLP(seq), fused.FastMLP(seq_t)
        if self._fast_q.layers[-1][1] != fused.ACT_NONE:
            raise NotImplementedError("C51: the categorical network's last layer must have no activation (its outputs are logits)")

    # ---- action selection -----------------------------------------------------------------------------------------
    def _q_values(self, obs: th.Tensor) -> th.Tensor:
        """sum_i z_i softmax_i(logits(obs)[a]) as [n, M]: the trunk layers, then the fused atom head on the last layer in place"""
        layers = self._fast_q.layers
        head = layers[-1][0]
        m = int(self.action_space.n)
        with th.no_grad():
            x = obs
            for lin, act in layers[:-1]:
                x = fused.linear(x, lin.weight, lin.bias, act, False)
            if self._head_kernel:
                q = th.empty(x.shape[0], m, dtype=th.float32, device=x.device)
                hip_ops.c51_head_q(x, head.weight, head.bias, self.levels, self.v_min, self.v_max, q)
                return q
            logits = fused.linear(x, head.weight, head.bias, fused.ACT_NONE, False).view(-1, m, self.n_atoms)
            return (th.softmax(logits, dim=2) * self._support).sum(dim=2)

    # ---- train ------------------------------------------------------------------------------------------------------
    def _alloc_step_tensors(self, batch_size: int) -> None:
        super()._alloc_step_tensors(batch_size)  # DQN's scalar-Q tensors stay allocated: inherited code may name them
        b, n, dev = batch_size, self.n_atoms, self.device
        e = lambda *s: th.empty(*s, dtype=th.float32, device=dev)  # noqa: E731
        self._gz, self._m, self._logp = e(b, n * int(self.action_space.n)), e(b, n), e(b, n)
        self._next_index = th.zeros(b, dtype=th.int64, device=dev)
        self._row_ws = th.zeros(b, dtype=th.float64, device=dev)

    def _capture_extra(self) -> dict:
        return dict(m=self._m.clone(), logp=self._logp.clone(), next_index=self._next_index.clone())

    def _gradient_step_fused(self, rd):
        """the train() statements on the kernel path"""
        with th.no_grad():
            z_next = self._fast_q_target(rd.next_observations, train_params=False)
        z = self._fast_q(rd.observations, train_params=True)
        l_out, l_sum = self._loss_slot("loss")
        cap = self.debug_capture
        hip_ops.c51_loss(z.detach(), z_next, rd.actions, rd.rewards, td_done(rd), self.gamma, self.levels, self.n_atoms, self.v_min, self.v_max,
                         self._gz, self._row_ws, loss_out=l_out, loss_sum=l_sum, m_out=self._m if cap else None,
                         logp_out=self._logp if cap else None, next_index_out=self._next_index if cap else None)
        with fused.deferred_weight_grads():
            th.autograd.backward([z], [self._gz])
        if self.max_grad_norm is not None:
            hip_ops.grad_clip(self.policy.arena.grad, self.max_grad_norm, self._ws, self._grad_norm)
        self.policy.optimizer.step()
        return self._logp, self._m, l_out

    def _gradient_step_torch(self, rd):
        """the same statements in plain torch on the arena parameters (c51_loss_torch); the index is recovered from the valve pair"""
        k = self.levels
        with th.no_grad():
            level = th.round(((rd.actions + 1.0) * float(k - 1)) / 2.0).clamp_(0, k - 1).long()
            index = level[:, 0] * k + level[:, 1]
            next_logits = self.categorical_net_target(rd.next_observations)
            coef = (1 - rd.dones) * td_discount(rd, self.gamma)
        out = c51_loss_torch(self.categorical_net(rd.observations), next_logits, index, rd.rewards, coef, self.v_min, self.v_max)
        self._m.copy_(out["m"]), self._logp.copy_(out["logp"].detach()), self._next_index.copy_(out["next_index"])
        loss = out["loss"]
        self._loss_sums["loss"] += loss.detach()
        self.policy.optimizer.zero_grad()
        loss.backward()
        if self.max_grad_norm is not None:
            norm = th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
            self._grad_norm.copy_(norm.detach().reshape(1))
        self.policy.optimizer.step()
        return self._logp, self._m, loss

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "C51", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        return dict(super()._extra_save_data(), n_atoms=self.n_atoms, v_min=self.v_min, v_max=self.v_max)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return super()._ctor_keys() + ("v_min", "v_max")

    @classmethod
    def _check_archive(cls, data: dict, env) -> None:
        super()._check_archive(data, env)  # discrete_actions against the env
        kept = (data.get("policy_kwargs") or {}).get("n_atoms", 51)
        if "n_atoms" in data and "policy_kwargs" in data and int(kept) != int(data["n_atoms"]):
            raise ValueError(f"the archive was written for n_atoms={data['n_atoms']}, its policy_kwargs say {kept}")

    @classmethod
    def _check_load_arguments(cls, data: dict, ctor: dict) -> None:
        """the archive's atom count and support against what the model is about to be built with: load()'s own keywords are in `ctor`"""
        asked = int((ctor.get("policy_kwargs") or {}).get("n_atoms", 51))
        if "n_atoms" in data and int(data["n_atoms"]) != asked:
            raise ValueError(f"the archive was written for n_atoms={data['n_atoms']}, the model is being built with {asked}")
        for key in ("v_min", "v_max"):  # the weights' distributions mean nothing on another support
            if key in data and key in ctor and float(ctor[key]) != float(data[key]):
                raise ValueError(f"the archive was written for {key}={data[key]}, the model is being built with {ctor[key]}")
