"""QR-DQN (Dabney et al. 2018, "Distributional Reinforcement Learning with Quantile Regression"; sb3_contrib.QRDQN) on DQN: the
exploration draw, the vec-step, the replay ring of valve pairs, the sampler, the hard target update, `predict`'s epsilon-greedy, the
hipGraph body and the checkpoint plumbing are DQN's (core/dqn/dqn.py), unchanged. The network outputs Nq = n_quantiles atoms per
action (core/qrdqn/policies.py, [B, Nq, M], M = K * K valve pairs) and three things change. With tau_i = (i + 0.5) / Nq:

    greedy action:  argmax_a mean_i Z(s)[i, a]
    with no gradient:  Z' = quantile_net_target(s');  a* = argmax_a mean_i Z'[i, a];  y_j = r + (1 - d) * gamma * Z'[j, a*]
    z_i = quantile_net(s)[i, a];  delta = y_j - z_i;  H = 0.5 delta^2 if |delta| <= 1 else |delta| - 0.5
    loss = mean over (b, j) of sum over i of |tau_i - 1[delta < 0]| * H     (quantile_huber_loss(..., sum_over_quantiles=True))
    -> clip_grad_norm_ when max_grad_norm is not None (the default is None) -> Adam step, eps = 0.01 / batch_size by default

ACTION SELECTION RUNS ON THE FOLDED HEAD. The mean over the atoms is linear in the last layer, so the rollout and `predict` never form
the [n_envs, Nq * M] atoms: hip_ops.qrdqn_fold_head averages the last layer's weight rows and biases over the atoms ([M, H] and [M],
buffers outside the arena), the trunk runs through the per-layer Linear kernels, one more Linear applies the folded head, and DQN's
cstr_dqn_act_f32 takes the [n_envs, M] means as Q values. The fold launch runs in front of EVERY such pass: it reads the last layer
once, and there is no cached copy that `load`, `set_parameters` or a torch-path optimiser step could leave stale.

A gradient step on the kernel path (FlatAdam, hip_ops.qrdqn_supported: Nq <= 256): the sample launch, the target network on s' and
the online network on s through the per-layer kernels (full atom rows, [B, Nq * M]), ONE hip_ops.qrdqn_loss call for everything
between them and loss.backward(), the backward with one deferred weight-gradient launch, the gradient clip only when asked for,
the FlatAdam step. Another optimiser class, Nq > 256 or `fused_learner = False` runs the published torch statements on the arena
parameters (`_gradient_step_torch`); the rollout keeps the folded head either way.

Not built (each raises where reachable): DQN's list (CnnPolicy / MultiInputPolicy, VecNormalize, data-parallel training,
optimize_memory_usage, HER), the MultiDiscrete face, IQN, and a gathered last layer that would evaluate only the Nq rows of the taken /
greedy action (the dense layer is small at batch 32)."""
from typing import Optional, Union

import torch as th

from core.common import fused, hip_ops
from core.dqn.dqn import DQN
from core.qrdqn.policies import MlpPolicy


def quantile_huber_loss(current_quantiles: th.Tensor, target_quantiles: th.Tensor, sum_over_quantiles: bool = True) -> th.Tensor:
    """sb3_contrib.common.utils.quantile_huber_loss for current [B, Nq] and target [B, Nq'] atoms: pairwise delta = target_j -
    current_i, Huber with kappa 1, weight |tau_i - 1[delta < 0]|; summed over the current quantile and averaged over the rest, or
    averaged over everything"""
    n_quantiles = current_quantiles.shape[-1]
    cum_prob = (th.arange(n_quantiles, device=current_quantiles.device, dtype=current_quantiles.dtype) + 0.5) / n_quantiles
    cum_prob = cum_prob.view(1, -1, 1)
    pairwise_delta = target_quantiles.unsqueeze(-2) - current_quantiles.unsqueeze(-1)
    abs_pairwise_delta = th.abs(pairwise_delta)
    huber_loss = th.where(abs_pairwise_delta > 1, abs_pairwise_delta - 0.5, pairwise_delta ** 2 * 0.5)
    loss = th.abs(cum_prob - (pairwise_delta.detach() < 0).to(current_quantiles.dtype)) * huber_loss
    return loss.sum(dim=-2).mean() if sum_over_quantiles else loss.mean()


class QRDQN(DQN):
    policy_aliases = {"MlpPolicy": MlpPolicy}

    def __init__(self, policy, env, learning_rate=5e-5, buffer_size: int = 1_000_000, learning_starts: int = 100, batch_size: int = 32,
                 tau: float = 1.0, gamma: float = 0.99, train_freq: Union[int, tuple] = 4, gradient_steps: int = 1,
                 replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None, optimize_memory_usage: bool = False,
                 target_update_interval: int = 10000, exploration_fraction: float = 0.005, exploration_initial_eps: float = 1.0,
                 exploration_final_eps: float = 0.01, max_grad_norm: Optional[float] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device: Union[th.device, str] = "auto", _init_setup_model: bool = True, faithful_quirks: bool = True):
        policy_kwargs = self.default_policy_kwargs(policy_kwargs, batch_size)
        self.n_quantiles = int(policy_kwargs.get("n_quantiles", 200))
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps,
                         replay_buffer_class=replay_buffer_class, replay_buffer_kwargs=replay_buffer_kwargs,
                         optimize_memory_usage=optimize_memory_usage, target_update_interval=target_update_interval,
                         exploration_fraction=exploration_fraction, exploration_initial_eps=exploration_initial_eps,
                         exploration_final_eps=exploration_final_eps, max_grad_norm=max_grad_norm, stats_window_size=stats_window_size,
                         tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device,
                         _init_setup_model=_init_setup_model, faithful_quirks=faithful_quirks)

    @staticmethod
    def default_policy_kwargs(policy_kwargs: Optional[dict], batch_size: int) -> dict:
        """A copy of the caller's policy_kwargs with the published default filled in: when no optimiser class is named, Adam (the
        policy's default class) with the paper's eps = 0.01 / batch_size."""
        policy_kwargs = dict(policy_kwargs or {})
        n_quantiles = int(policy_kwargs.get("n_quantiles", 200))
        if n_quantiles < 1:
            raise ValueError(f"QRDQN: n_quantiles must be at least 1, got {n_quantiles}")
        if "optimizer_class" not in policy_kwargs:
            policy_kwargs["optimizer_kwargs"] = dict(eps=0.01 / batch_size)
        return policy_kwargs

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        super()._setup_model()
        m, nq = int(self.action_space.n), self.n_quantiles
        # the kernel path: DQN's (FlatAdam), with an atom count the loss launch takes; otherwise the torch statements
        self.fused_learner = bool(self.fused_learner and hip_ops.qrdqn_supported(m, self.levels, nq))
        head = self._fast_q.layers[-1][0]
        self._w_mean = th.zeros(m, head.in_features, dtype=th.float32, device=self.device)  # the folded head, outside the arena
        self._b_mean = th.zeros(m, dtype=th.float32, device=self.device)

    def _setup_networks(self) -> None:
        self.quantile_net, self.quantile_net_target = self.policy.quantile_net, self.policy.quantile_net_target  # _create_aliases
        seq, seq_t = self.quantile_net.quantile_net, self.quantile_net_target.quantile_net
        if not (fused.FastMLP.supported(seq) and hip_ops.dqn_supported(int(self.action_space.n), self.levels)):
            raise NotImplementedError("QRDQN: the quantile network must be Linear (+ ReLU / Tanh) layers over a valve face of 2..16 levels")
        self._fast_q, self._fast_q_target = fused.FastMLP(seq), fused.FastMLP(seq_t)
        if self._fast_q.layers[-1][1] != fused.ACT_NONE:
            raise NotImplementedError("QRDQN: the quantile network's last layer must have no activation (the folded head is linear)")

    # ---- action selection -----------------------------------------------------------------------------------------
    def _q_values(self, obs: th.Tensor) -> th.Tensor:
        """mean_i Z(obs)[i, a] as [n, M]: the fold launch, the trunk layers, one Linear on the folded head"""
        layers = self._fast_q.layers
        head = layers[-1][0]
        with th.no_grad():
            hip_ops.qrdqn_fold_head(head.weight, head.bias, int(self.action_space.n), self._w_mean, self._b_mean)
            x = obs
            for lin, act in layers[:-1]:
                x = fused.linear(x, lin.weight, lin.bias, act, False)
            return fused.linear(x, self._w_mean, self._b_mean, fused.ACT_NONE, False)

    # ---- train ------------------------------------------------------------------------------------------------------
    def _alloc_step_tensors(self, batch_size: int) -> None:
        super()._alloc_step_tensors(batch_size)  # DQN's scalar-Q tensors stay allocated: inherited code may name them
        b, nq, dev = batch_size, self.n_quantiles, self.device
        e = lambda *s: th.empty(*s, dtype=th.float32, device=dev)  # noqa: E731
        self._gz, self._cur_z, self._target_z = e(b, nq * int(self.action_space.n)), e(b, nq), e(b, nq)
        self._next_index = th.zeros(b, dtype=th.int64, device=dev)
        self._row_ws = th.zeros(b, dtype=th.float64, device=dev)

    def _capture_extra(self) -> dict:
        return dict(next_index=self._next_index.clone())

    def _gradient_step_fused(self, rd):
        """the published train() statements on the kernel path"""
        with th.no_grad():
            z_next = self._fast_q_target(rd.next_observations, train_params=False)
        z = self._fast_q(rd.observations, train_params=True)
        l_out, l_sum = self._loss_slot("loss")
        cap = self.debug_capture
        hip_ops.qrdqn_loss(z.detach(), z_next, rd.actions, rd.rewards, rd.dones, self.gamma, self.levels, self.n_quantiles, self._gz,
                           self._row_ws, loss_out=l_out, loss_sum=l_sum, cur_out=self._cur_z if cap else None,
                           target_out=self._target_z if cap else None, next_index_out=self._next_index if cap else None)
        with fused.deferred_weight_grads():
            th.autograd.backward([z], [self._gz])
        if self.max_grad_norm is not None:
            hip_ops.grad_clip(self.policy.arena.grad, self.max_grad_norm, self._ws, self._grad_norm)
        self.policy.optimizer.step()
        return self._cur_z, self._target_z, l_out

    def _gradient_step_torch(self, rd):
        """the published train() statements in plain torch on the arena parameters; the index is recovered from the valve pair"""
        k, nq = self.levels, self.n_quantiles
        batch_size = rd.observations.shape[0]
        with th.no_grad():
            level = th.round(((rd.actions + 1.0) * float(k - 1)) / 2.0).clamp_(0, k - 1).long()
            index = (level[:, 0] * k + level[:, 1]).reshape(-1, 1)  # what the published buffer holds: int64 [B, 1]
            next_quantiles = self.quantile_net_target(rd.next_observations)
            next_greedy_actions = next_quantiles.mean(dim=1, keepdim=True).argmax(dim=2, keepdim=True)
            self._next_index.copy_(next_greedy_actions.reshape(-1))
            next_greedy_actions = next_greedy_actions.expand(batch_size, nq, 1)
            next_quantiles = next_quantiles.gather(dim=2, index=next_greedy_actions).squeeze(dim=2)
            target_quantiles = rd.rewards + (1 - rd.dones) * self.gamma * next_quantiles
        current_quantiles = self.quantile_net(rd.observations)
        actions = index[..., None].expand(batch_size, nq, 1)
        current_quantiles = th.gather(current_quantiles, dim=2, index=actions).squeeze(dim=2)
        loss = quantile_huber_loss(current_quantiles, target_quantiles, sum_over_quantiles=True)
        self._loss_sums["loss"] += loss.detach()
        self.policy.optimizer.zero_grad()
        loss.backward()
        if self.max_grad_norm is not None:
            norm = th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
            self._grad_norm.copy_(norm.detach().reshape(1))
        self.policy.optimizer.step()
        return current_quantiles, target_quantiles, loss

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "QRDQN", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        return dict(super()._extra_save_data(), n_quantiles=self.n_quantiles)

    @classmethod
    def _check_archive(cls, data: dict, env) -> None:
        super()._check_archive(data, env)  # discrete_actions against the env
        kept = (data.get("policy_kwargs") or {}).get("n_quantiles", 200)
        if "n_quantiles" in data and "policy_kwargs" in data and int(kept) != int(data["n_quantiles"]):
            raise ValueError(f"the archive was written for n_quantiles={data['n_quantiles']}, its policy_kwargs say {kept}")

    @classmethod
    def _check_load_arguments(cls, data: dict, ctor: dict) -> None:
        """the archive's atom count against the one the model is about to be built with: load()'s own policy_kwargs are in `ctor`"""
        asked = int((ctor.get("policy_kwargs") or {}).get("n_quantiles", 200))
        if "n_quantiles" in data and int(data["n_quantiles"]) != asked:
            raise ValueError(f"the archive was written for n_quantiles={data['n_quantiles']}, the model is being built with {asked}")
