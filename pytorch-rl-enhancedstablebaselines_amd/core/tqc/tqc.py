"""TQC (Kuznetsov et al. 2020, "Controlling Overestimation Bias with Truncated Mixture of Continuous Distributional Quantile
Critics"; sb3_contrib.TQC) on SAC: the actor, the rollout, the replay ring, the sampler, the entropy coefficient and the soft update
are SAC's, unchanged. Each of the G = n_critics critics outputs Nq = n_quantiles atoms instead of one Q value (core/tqc/policies.py),
and the two losses change. With k = top_quantiles_to_drop_per_net, M = G * Nq, n_keep = M - k * G, tau_i = (i + 0.5) / Nq, one gradient
step is, in SAC's order (core/sac/sac.py):

    a_pi, logp = actor(s);  a', logp' = actor(s');  alpha = exp(log_ent_coef) before its update; SAC's entropy-coefficient loss and step
    with no gradient:  Z' = critic_target(s', a') [B, G, Nq]; a row's M atoms pooled, sorted ascending, the smallest n_keep kept;
                       y_j = r + (1 - d) * gamma * (z'_(j) - alpha * logp')                                       j = 0 .. n_keep - 1
    Z = critic(s, a) [B, G, Nq];  delta = y_j - z_{g,i};  H = 0.5 delta^2 if |delta| <= 1 else |delta| - 0.5
    critic_loss = mean over (b, g, i, j) of |tau_i - 1[delta < 0]| * H        (quantile_huber_loss(..., sum_over_quantiles=False))
                                                                                                         -> Adam step on the critic
    qf_pi = mean over (g, i) of critic(s, a_pi), critic parameters frozen;  actor_loss = mean(alpha * logp - qf_pi)
                                                                                                         -> Adam step on the actor
    soft update of the target critics every target_update_interval steps

On the kernel path (a packed batch, FlatAdam optimisers, hip_ops.tqc_supported(G, Nq, k)) a step is: the packed sample, SAC's 2B-row
actor pass, the target critics on x_next and the critics on x_data as stacked layers ([G, B, Nq], the layout the loss launch reads),
cstr_tqc_critic_loss_f32 (truncation, targets, pairwise quantile-Huber loss, its gradient, the logged means, and SAC's
entropy-coefficient loss riding along), the critic's backward, the critic Adam with the entropy step, the frozen critics on x_pi,
cstr_tqc_actor_loss_f32, the backward down to the actor, the actor Adam with the soft update. Otherwise the step is
`_gradient_step_aten`: the statements above in plain torch on the nn.Modules. The row-chain kernels (core/common/chain.py) have
SAC's scalar losses built in and decline this class.
Not built: gSDE, a VecNormalize-wrapped env, data-parallel runs, the goal face and HER, more than 256 atoms on the kernel path."""
from typing import Optional, Union

import torch as th

from core.common import fused, hip_ops
from core.common.logger import DeviceMean
from core.common.vec_env import unwrap_vec_normalize
from core.sac.sac import SAC
from core.tqc.policies import MlpPolicy


def quantile_huber_loss(z: th.Tensor, y: th.Tensor) -> th.Tensor:
    """mean over (b, g, i, j) of |tau_i - 1[y_j - z_gi < 0]| * Huber(y_j - z_gi): z [B, G, Nq] the current atoms, y [B, n_keep] the
    targets (sb3_contrib's quantile_huber_loss with sum_over_quantiles=False)"""
    nq = z.shape[2]
    tau = (th.arange(nq, device=z.device, dtype=z.dtype) + 0.5) / nq
    delta = y[:, None, None, :] - z[:, :, :, None]
    ad = delta.abs()
    huber = th.where(ad > 1, ad - 0.5, delta ** 2 * 0.5)
    return (th.abs(tau[None, None, :, None] - (delta.detach() < 0).to(z.dtype)) * huber).mean()


class TQC(SAC):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    goal_face_support = False
    train_batch_size = 256
    chain_type = None

    def __init__(self, policy, env, learning_rate=3e-4, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq: Union[int, tuple] = 1,
                 gradient_steps: int = 1, action_noise=None, replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None,
                 optimize_memory_usage: bool = False, ent_coef: Union[str, float] = "auto", target_update_interval: int = 1,
                 target_entropy: Union[str, float] = "auto", top_quantiles_to_drop_per_net: int = 2, use_sde: bool = False,
                 sde_sample_freq: int = -1, use_sde_at_warmup: bool = False, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device="auto", _init_setup_model: bool = True):
        from core.her import HerReplayBuffer

        if use_sde or (policy_kwargs and policy_kwargs.get("use_sde")):
            raise ValueError("TQC does not support gSDE (use_sde=True)")
        if env is not None and unwrap_vec_normalize(env) is not None:
            raise ValueError("TQC does not take a VecNormalize-wrapped env: observation and reward normalisation are not built")
        if isinstance(replay_buffer_class, type) and issubclass(replay_buffer_class, HerReplayBuffer):
            raise ValueError("TQC does not support HerReplayBuffer (the goal face of the env): HER is built for SAC, TD3 and DDPG")
        n_quantiles = int((policy_kwargs or {}).get("n_quantiles", 25))
        k = int(top_quantiles_to_drop_per_net)
        if n_quantiles < 1:
            raise ValueError(f"TQC: n_quantiles must be at least 1, got {n_quantiles}")
        if k < 0:
            raise ValueError(f"TQC: top_quantiles_to_drop_per_net must not be negative, got {k}")
        if k >= n_quantiles:
            raise ValueError(f"TQC: top_quantiles_to_drop_per_net = {k} drops every atom of a critic with n_quantiles = {n_quantiles}")
        self.top_quantiles_to_drop_per_net = k
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps,
                         action_noise, replay_buffer_class=replay_buffer_class, replay_buffer_kwargs=replay_buffer_kwargs,
                         optimize_memory_usage=optimize_memory_usage, ent_coef=ent_coef, target_update_interval=target_update_interval,
                         target_entropy=target_entropy, stats_window_size=stats_window_size, tensorboard_log=tensorboard_log,
                         policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device, _init_setup_model=False)
        if self.world_size > 1:
            raise NotImplementedError("data-parallel TQC is not built")
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        super()._setup_model()
        g, nq, k = len(self.critic.q_networks), self.critic.n_quantiles, self.top_quantiles_to_drop_per_net
        self.n_critics, self.n_quantiles, self.n_target_quantiles = g, nq, g * nq - k * g
        # the kernel path: SAC's, with an atom count the two loss launches take; otherwise the torch statements
        self.fused_learner = bool(self.fused_learner and hip_ops.tqc_supported(g, nq, k))
        # [actor | critic | ent_coef_loss | ent_coef | target_mean | atom_mean]: SAC's four logged sums and the critic launch's two means
        self._loss_sum_buf = th.zeros(6, dtype=th.float32, device=self.device)
        sb = self._loss_sum_buf
        self._loss_sums = dict(actor=sb[0:1], critic=sb[1:2], ent_coef_loss=sb[2:3], ent_coef=sb[3:4], target_mean=sb[4:5], atom_mean=sb[5:6],
                               means=sb[4:6])

    def _chain_for(self, batch_size: int):
        return None  # the row-chain steps have SAC's scalar losses built in

    def _kernel_path(self) -> bool:
        return self.fused_learner and self._use_packed_batch()

    def _alloc_step_tensors(self, batch_size: int) -> None:
        super()._alloc_step_tensors(batch_size)
        e = lambda *s: th.zeros(*s, dtype=th.float32, device=self.device)  # noqa: E731
        g, nq = self.n_critics, self.n_quantiles
        self._gz, self._gz_pi, self._g_logp = e(g, batch_size, nq), e(g, batch_size, nq), e(batch_size)
        self._target_y, self._z_pi_mean = e(batch_size, self.n_target_quantiles), e(batch_size)
        self._tqc_ws = th.zeros(3 * batch_size, dtype=th.float64, device=self.device)

    # ---- gradient steps ----------------------------------------------------------------------------------------------------------
    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        # one gradient step per train() call (the default): the loss launches STORE the logged values, no zero-fill launch
        self._single_step = gradient_steps == 1 and self._kernel_path() and self.ent_coef_optimizer is not None
        if not self._single_step:
            self._loss_sum_buf.zero_()
        for gradient_step in range(gradient_steps):
            self._gradient_step(batch_size, gradient_step)

    def _train_host_only(self, gradient_steps: int) -> None:
        super()._train_host_only(gradient_steps)  # SAC's four keys; train/critic_loss is the quantile loss
        s = self._loss_sums
        self.logger.record("train/target_mean", DeviceMean(s["target_mean"], gradient_steps))
        self.logger.record("train/atom_mean", DeviceMean(s["atom_mean"], gradient_steps))

    def _gradient_step(self, batch_size: int, gradient_step: int) -> None:
        if self._kernel_path():
            return self._gradient_step_fused(batch_size, gradient_step)
        return self._gradient_step_aten(batch_size, gradient_step)

    @staticmethod
    def _atoms(zs: "fused.QOut"):
        """([G, B, Nq] atoms, the tensor(s) the backward starts from): the stacked output, or the one network's"""
        if zs.stacked is not None:
            return zs.stacked, zs.stacked
        return zs[0].unsqueeze(0), zs[0]

    def _gradient_step_fused(self, batch_size: int, gradient_step: int) -> None:
        s, pol, fa = self._loss_sums, self.policy, self._fast_actor
        (c_out, c_sum), (a_out, a_sum) = self._loss_slot("critic"), self._loss_slot("actor")
        pb, gather, rd = self._sample(batch_size, fa.pair_supported)
        if fa.pair_supported(pb):  # pi(s) and pi(s') in ONE 2B-row actor pass
            x_pi, log_prob, x_next, next_log_prob = fa.action_log_prob_pair(pb, gather=gather)
        else:  # the actor head writes the action columns of the critic inputs itself
            x_pi, log_prob = fa.action_log_prob(rd.observations, xbuf=pb.x_pi.detach())
            with th.no_grad():
                x_next, next_log_prob = fa.action_log_prob(rd.next_observations, train_params=False, xbuf=pb.x_next)

        # the target critics on x_next without gradients, then the critics on x_data: both [G, B, Nq]
        with th.no_grad():
            z_next, _ = self._atoms(self._fast_critic_target.forward_input(x_next.detach(), train_params=False))
        z, z_root = self._atoms(self._fast_critic.forward_input(pb.x_data))
        ent_opt = self.ent_coef_optimizer
        if ent_opt is not None:
            (ent_coef, ent_coef_sum), (e_out, e_sum) = self._loss_slot("ent_coef"), self._loss_slot("ent_coef_loss")
            alpha = dict(log_alpha=self.log_ent_coef.detach(), logp_pi=log_prob.detach(), target_entropy=self.target_entropy,
                         grad_out=self._ent_arena.grad[0:1], ent_coef_out=ent_coef, loss_out=e_out, loss_sum=e_sum, ent_coef_sum=ent_coef_sum)
        else:
            ent_coef, alpha = self.ent_coef_tensor.reshape(1), None
            s["ent_coef"] += ent_coef
        single = self._single_step
        # truncation, targets, the pairwise quantile-Huber loss and its gradient; the entropy coefficient's loss rides along
        hip_ops.tqc_critic_loss(z.detach(), z_next, next_log_prob.detach(), rd.rewards, rd.dones, ent_coef, self.gamma,
                                self.top_quantiles_to_drop_per_net, self._gz, self._tqc_ws, loss_out=c_out, loss_sum=c_sum,
                                target_out=self._target_y, means_out=s["means"] if single else None, means_sum=None if single else s["means"],
                                alpha=alpha)
        with fused.deferred_weight_grads():
            th.autograd.backward([z_root], [self._gz if z_root.dim() == 3 else self._gz[0]])
        if ent_opt is not None and self._ent_rides_critic:
            self.critic.optimizer.step_with(ent_opt)  # the entropy coefficient's step and the critic's in one launch
        else:
            if ent_opt is not None:
                ent_opt.step()
            self.critic.optimizer.step()

        # the updated critics, frozen, on x_pi; the gradient goes to the action columns and on down to the actor
        z_pi, z_pi_root = self._atoms(self._fast_critic.forward_input(x_pi, train_params=False))
        hip_ops.tqc_actor_loss(z_pi.detach(), log_prob.detach(), ent_coef, self._gz_pi, self._g_logp, loss_out=a_out, loss_sum=a_sum,
                               z_pi_mean=self._z_pi_mean)
        with fused.deferred_weight_grads():
            th.autograd.backward([log_prob, z_pi_root], [self._g_logp, self._gz_pi if z_pi_root.dim() == 3 else self._gz_pi[0]])
        if gradient_step % self.target_update_interval == 0:  # the actor's step and the soft update (disjoint arenas) in one launch
            self.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, self.tau))
        else:
            self.actor.optimizer.step()

        if self.debug_capture:
            means = s["means"].clone()  # of this step when it is the call's only one, else the call's running sums
            self.last_train_tensors = dict(z=z.detach().permute(1, 0, 2).clone(), y=self._target_y.clone(), z_pi_mean=self._z_pi_mean.clone(),
                                           log_prob=log_prob.detach().clone(), ent_coef=ent_coef.detach().clone(), critic_loss=c_out.clone(),
                                           actor_loss=a_out.clone(), means=means)

    def _gradient_step_aten(self, batch_size: int, gradient_step: int) -> None:
        """The statements of the module docstring in plain torch on the nn.Modules (autograd losses): what configurations the kernel
        path does not cover run, and the A/B reference in tests."""
        s = self._loss_sums
        rd = self.replay_buffer.sample_into(self._batch(batch_size))
        actions_pi, log_prob = self.actor.action_log_prob(rd.observations)
        log_prob = log_prob.reshape(-1, 1)

        if self.ent_coef_optimizer is not None and self.log_ent_coef is not None:
            ent_coef = th.exp(self.log_ent_coef.detach())
            ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
            s["ent_coef_loss"] += ent_coef_loss.detach()
            self.ent_coef_optimizer.zero_grad()
            ent_coef_loss.backward()
            self.ent_coef_optimizer.step()
        else:
            ent_coef = self.ent_coef_tensor.reshape(1)
        s["ent_coef"] += ent_coef.reshape(1)

        with th.no_grad():
            next_actions, next_log_prob = self.actor.action_log_prob(rd.next_observations)
            z_next = self.critic_target(rd.next_observations, next_actions)  # [B, G, Nq]
            z_sorted, _ = th.sort(z_next.reshape(z_next.shape[0], -1), dim=1)
            z_kept = z_sorted[:, :self.n_target_quantiles]
            y = rd.rewards + (1 - rd.dones) * self.gamma * (z_kept - ent_coef * next_log_prob.reshape(-1, 1))  # [B, n_keep]

        z = self.critic(rd.observations, rd.actions)  # [B, G, Nq]
        critic_loss = quantile_huber_loss(z, y)
        s["critic"] += critic_loss.detach()
        self.critic.optimizer.zero_grad()
        critic_loss.backward()
        self.critic.optimizer.step()

        qf_pi = self.critic(rd.observations, actions_pi).mean(dim=2).mean(dim=1, keepdim=True)
        actor_loss = (ent_coef * log_prob - qf_pi).mean()
        s["actor"] += actor_loss.detach()
        self.actor.optimizer.zero_grad()
        actor_loss.backward()
        self.actor.optimizer.step()

        if gradient_step % self.target_update_interval == 0:
            self.policy.critic_target_arena.polyak_from(self.policy.critic_arena, self.tau)

        with th.no_grad():
            means = th.stack([y.mean(), z.mean()]).detach()
            s["means"] += means
        if self.debug_capture:
            self.last_train_tensors = dict(z=z.detach().clone(), y=y.clone(), z_pi_mean=qf_pi.detach().reshape(-1).clone(),
                                           log_prob=log_prob.detach().reshape(-1).clone(), ent_coef=ent_coef.detach().clone(),
                                           critic_loss=critic_loss.detach().reshape(1).clone(), actor_loss=actor_loss.detach().reshape(1).clone(),
                                           means=means.clone())

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        return dict(super()._extra_save_data(), top_quantiles_to_drop_per_net=self.top_quantiles_to_drop_per_net)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return super()._ctor_keys() + ("top_quantiles_to_drop_per_net",)

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "TQC",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)
