"""IQL (Kostrikov, Nair & Levine 2021, "Offline Reinforcement Learning with Implicit Q-Learning") on SAC's actor and twin critic, with
a state-value network V (core/iql/policies.py). It never evaluates a Q function at an action the dataset does not hold, samples no
action and draws no noise. Per gradient step, with tau_e = expectile, M = exp_adv_max, every forward on the parameters the step
started with (the ordering of CORL's published iql.py):

    with no gradient:  qt = min(Qt_1(s, a), Qt_2(s, a))   (target critics);   v' = V(s')
    v = V(s);  u = qt - v
    value_loss  = mean_b( |tau_e - 1[u < 0]| * u^2 )                                  -> Adam step on V
    y = r + (1 - d) * gamma * v'
    critic_loss = 0.5 * sum_i mean_b( (Q_i(s, a) - y)^2 )                             -> Adam step on the critic (SAC's scale)
    w = min(exp(beta * u), M)                                                          a constant of the actor step
    (mean, ls_raw) = actor trunk + head on s;  ls = clamp(ls_raw, -20, 2)              SAC's actor
    logp = log pi(a | s) of the squashed diagonal Gaussian at the DATASET action: g = atanh(clamp(a, -1 + eps32, 1 - eps32)),
           logp = sum_k[ -(g_k - mean_k)^2 / (2 exp(2 ls_k)) - ls_k - 0.5 log(2 pi) ] - sum_k log(1 - a_k^2 + 1e-6)   (unclamped a_k)
    actor_loss  = mean_b( -w * logp )                                                  -> Adam step on the actor
    soft update of the target critics every target_update_interval steps (SAC's)

u = 0 takes weight tau_e; an overflowing exp(beta u) is clipped to M; |a_k| > 1 gives torch's NaN and is not guarded.
Not built: the deterministic-policy variant, observation and reward normalisation, a built-in cosine schedule (a callable
`learning_rate` works), online fine-tuning.

It sits on `OfflineAlgorithm` (the dataset forms, learn(), the hipGraph hooks). On the fused path (two critics, FlatAdam, a packed
batch) a step is: the target critics' forward on the sampled (obs | act) rows, ONE forward of V on the 2B rows [s; s']
(fused.FastValuePair), the critics' forward, the actor's distribution parameters (FastSacActor.dist_params), ONE launch for
everything between the forwards and the backwards (cstr_iql_loss_f32: the three losses, their gradients, the logged scalars), the
three backwards (V's on the B rows of s only), the optimiser steps, the soft update. Otherwise the step is `_gradient_step_aten`: the
same statement in plain torch on the nn.Modules. The row-chain kernels (core/common/chain.py) have SAC's losses built in and decline
this class."""
import math
from typing import Optional, Union

import numpy as np
import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.arena import FlatAdam
from core.common.logger import DeviceMean
from core.common.offline_policy_algorithm import OfflineAlgorithm
from core.common.vec_env import unwrap_vec_normalize
from core.iql.policies import MlpPolicy
from core.sac.sac import SAC

LOSS_KEYS = ("value", "critic", "actor")  # cstr_iql_loss_f32's loss row
AUX_KEYS = ("adv_mean", "weight_mean", "weight_clip_frac", "logp_mean", "v_mean", "target_mean")  # ... and its aux row


def squashed_log_prob(mean: th.Tensor, log_std: th.Tensor, actions: th.Tensor) -> th.Tensor:
    """log pi(actions) [B] of the squashed diagonal Gaussian (mean, clamped log_std) at given actions: the module docstring's statement"""
    eps = th.finfo(actions.dtype).eps
    a = actions.clamp(-1.0 + eps, 1.0 - eps)
    g = 0.5 * (a.log1p() - (-a).log1p())
    std = log_std.exp()
    lp = -((g - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))
    return lp.sum(dim=1) - th.log(1 - actions ** 2 + 1e-6).sum(dim=1)


class IQL(SAC, OfflineAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    goal_face_support = False
    train_batch_size = 256
    chain_type = None

    def __init__(self, policy, env, learning_rate=3e-4, dataset=None, buffer_size: int = 1_000_000, batch_size: int = 256,
                 tau: float = 0.005, gamma: float = 0.99, gradient_steps: int = 1, target_update_interval: int = 1,
                 expectile: float = 0.7, beta: float = 3.0, exp_adv_max: float = 100.0, behavior_cloning_warmup: int = 0,
                 n_eval_episodes: int = 10, policy_kwargs: Optional[dict] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, verbose: int = 0, device: Union[th.device, str] = "auto",
                 seed: Optional[int] = None, _init_setup_model: bool = True):
        if policy_kwargs and policy_kwargs.get("use_sde"):
            raise ValueError("IQL does not support gSDE (use_sde=True)")
        if env is not None and unwrap_vec_normalize(env) is not None:
            raise ValueError("IQL does not take a VecNormalize-wrapped env: observation normalisation is not built")
        if not (0.0 < expectile < 1.0):
            raise ValueError(f"IQL: expectile must lie inside (0, 1), got {expectile}")
        if not (beta >= 0.0):
            raise ValueError(f"IQL: beta must be a non-negative number, got {beta}")
        if not (exp_adv_max > 0.0):
            raise ValueError(f"IQL: exp_adv_max must be a positive number, got {exp_adv_max}")
        OfflineAlgorithm.__init__(self, policy=policy, env=env, dataset=dataset, learning_rate=learning_rate, buffer_size=buffer_size,
                                  batch_size=batch_size, tau=tau, gamma=gamma, gradient_steps=gradient_steps, dataset_buffer_class=None,
                                  dataset_buffer_kwargs=None, n_eval_episodes=n_eval_episodes,
                                  behavior_cloning_warmup=behavior_cloning_warmup, conservative_weight=0.0, policy_kwargs=policy_kwargs,
                                  stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, verbose=verbose, device=device,
                                  seed=seed)
        if self.world_size > 1:
            raise NotImplementedError("data-parallel IQL is not built")
        # SAC.__init__ is not run (its base-class call has the online signature): what it sets behind that call is set here and must
        # follow it. There is no entropy coefficient: SAC's set-up sees the constant 0 and builds no optimiser for one.
        self.target_entropy = 0.0
        self.log_ent_coef = None
        self.ent_coef = 0.0
        self.target_update_interval = target_update_interval
        self.ent_coef_optimizer = None
        self.debug_capture = False
        self.last_train_tensors: dict = {}
        self.expectile, self.beta, self.exp_adv_max = float(expectile), float(beta), float(exp_adv_max)
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        super()._setup_model()
        self.value_net = self.policy.value_net
        act_dim = int(np.prod(self.action_space.shape))
        # the kernel path: SAC's, with two critics, a V network the pair pass takes and an action width the loss launch takes;
        # otherwise the torch statements
        self.fused_learner = bool(self.fused_learner and len(self.critic.q_networks) == 2 and isinstance(self.value_net.optimizer, FlatAdam)
                                  and fused.FastValuePair.supported(self.value_net) and hip_ops.iql_supported(1, act_dim))
        if self.fused_learner:
            self._fast_value = fused.FastValuePair(self.value_net)
        # [value | critic | actor | adv_mean | weight_mean | weight_clip_frac | logp_mean | v_mean | target_mean]: the loss launch's loss
        # and aux rows
        self._loss_sum_buf = th.zeros(9, dtype=th.float32, device=self.device)
        b = self._loss_sum_buf
        self._loss_sums = dict(**{k: b[i:i + 1] for i, k in enumerate(LOSS_KEYS)}, **{k: b[3 + i:4 + i] for i, k in enumerate(AUX_KEYS)})
        self._loss_now = th.zeros(3, dtype=th.float32, device=self.device)
        self._aux_now = th.zeros(6, dtype=th.float32, device=self.device)

    def _chain_for(self, batch_size: int):
        return None  # the row-chain steps have SAC's losses built in

    def _graph_eligible(self, callback) -> bool:
        return super()._graph_eligible(callback) and self._use_packed_batch()  # the step draws nothing: no queue to look at

    def _alloc_step_tensors(self, batch_size: int) -> None:
        super()._alloc_step_tensors(batch_size)
        e = lambda *s: th.zeros(*s, dtype=th.float32, device=self.device)  # noqa: E731
        a = int(np.prod(self.action_space.shape))
        self._g_v, self._gq, self._g_params = e(batch_size), e(2, batch_size, 1), e(batch_size, 2 * a)
        self._adv, self._logp = e(batch_size), e(batch_size)

    # ---- gradient steps ----------------------------------------------------------------------------------------------------------
    def _train_host_pre(self) -> None:
        self._update_learning_rate([self.actor.optimizer, self.critic.optimizer, self.value_net.optimizer])

    def _gradient_step(self, batch_size: int, gradient_step: int) -> None:
        if self.fused_learner and self._use_packed_batch():
            return self._gradient_step_fused(batch_size, gradient_step)
        return self._gradient_step_aten(batch_size, gradient_step)

    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        # one gradient step per train() call (the default): the loss launch STORES the logged values, no zero-fill launch
        self._single_step = gradient_steps == 1 and self.fused_learner and self._use_packed_batch()
        if not self._single_step:
            self._loss_sum_buf.zero_()
        for gradient_step in range(gradient_steps):
            self._gradient_step(batch_size, gradient_step)

    def _gradient_step_fused(self, batch_size: int, gradient_step: int) -> None:
        pol, fa, b = self.policy, self._fast_actor, batch_size
        pb, _, rd = self._sample(batch_size)
        # the four forwards, all on the parameters the step started with
        with th.no_grad():
            qs_t = self._fast_critic_target.forward_input(pb.x_data, train_params=False)
        v2 = self._fast_value.forward(pb.x_pn[:, :pb.obs_dim]).view(-1)  # the sampler wrote s into x_pi's rows and s' into x_next's
        qs = self._fast_critic.forward_input(pb.x_data)
        params = fa.dist_params(rd.observations)
        # everything between the forwards and the backwards
        single = self._single_step
        buf = self._loss_sum_buf
        hip_ops.iql_loss(qs_t[0], qs_t[1], v2[:b], v2[b:], qs[0].detach(), qs[1].detach(), params.detach(), rd.actions, rd.rewards, rd.dones,
                         self.gamma, self.expectile, self.beta, self.exp_adv_max, g_v=self._g_v, gq1=self._gq[0], gq2=self._gq[1],
                         g_params=self._g_params, loss_out=buf[0:3] if single else self._loss_now, loss_sum=None if single else buf[0:3],
                         aux=buf[3:9] if single else self._aux_now, target_out=self._target_q, adv_out=self._adv, logp_out=self._logp)
        # the three backwards
        self._fast_value.backward(self._g_v)
        fused.backward_q(qs, self._gq)
        with fused.deferred_weight_grads():
            th.autograd.backward([params], [self._g_params])
        if not single:
            buf[3:9] += self._aux_now
        self.value_net.optimizer.step()
        self.critic.optimizer.step()
        if gradient_step % self.target_update_interval == 0:
            self.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, self.tau))
        else:
            self.actor.optimizer.step()

        if self.debug_capture:
            u = self._adv.clone()
            self.last_train_tensors = dict(u=u, w=th.clamp(th.exp(self.beta * u), max=self.exp_adv_max), y=self._target_q.reshape(-1).clone(),
                                           logp=self._logp.clone(), q=[q.detach().reshape(-1).clone() for q in qs], v=v2[:b].clone(),
                                           losses=(buf[0:3] if single else self._loss_now).clone(),
                                           aux=(buf[3:9] if single else self._aux_now).clone())

    def _gradient_step_aten(self, batch_size: int, gradient_step: int) -> None:
        """The statement of the module docstring in plain torch on the nn.Modules (autograd losses): what configurations the kernel
        path does not cover run, and the A/B reference in tests."""
        rd = self.replay_buffer.sample_into(self._batch(batch_size))
        obs, act = rd.observations, rd.actions
        with th.no_grad():
            qt, _ = th.min(th.cat(self.critic_target(obs, act), dim=1), dim=1, keepdim=True)
            v_next = self.value_net(rd.next_observations)
        v = self.value_net(obs)
        u = qt - v
        value_loss = (th.abs(self.expectile - (u < 0).to(u.dtype)) * u ** 2).mean()
        y = rd.rewards + (1 - rd.dones) * self.gamma * v_next
        qs = self.critic(obs, act)
        critic_loss = 0.5 * sum(F.mse_loss(q, y) for q in qs)
        e = th.exp(self.beta * u.detach())
        w = th.clamp(e, max=self.exp_adv_max)
        mean, log_std, _ = self.actor.get_action_dist_params(obs)  # log_std clamped to [-20, 2] there (SAC's actor)
        logp = squashed_log_prob(mean, log_std, act).reshape(-1, 1)
        actor_loss = (-w * logp).mean()

        for opt, loss in ((self.value_net.optimizer, value_loss), (self.critic.optimizer, critic_loss), (self.actor.optimizer, actor_loss)):
            opt.zero_grad()
            loss.backward()
        for opt in (self.value_net.optimizer, self.critic.optimizer, self.actor.optimizer):
            opt.step()
        if gradient_step % self.target_update_interval == 0:
            self.policy.critic_target_arena.polyak_from(self.policy.critic_arena, self.tau)

        with th.no_grad():
            losses = th.stack([value_loss.detach(), critic_loss.detach(), actor_loss.detach()])
            aux = th.stack([u.mean(), w.mean(), (e > self.exp_adv_max).to(u.dtype).mean(), logp.mean(), v.mean(), y.mean()]).detach()
            self._loss_sum_buf[0:3] += losses
            self._loss_sum_buf[3:9] += aux
        if self.debug_capture:
            self.last_train_tensors = dict(u=u.detach().reshape(-1).clone(), w=w.reshape(-1).clone(), y=y.reshape(-1).clone(),
                                           logp=logp.detach().reshape(-1).clone(), q=[q.detach().reshape(-1).clone() for q in qs],
                                           v=v.detach().reshape(-1).clone(), losses=losses.clone(), aux=aux.clone())

    def _train_host_only(self, gradient_steps: int) -> None:
        self._n_updates += gradient_steps
        s = self._loss_sums  # device-side sums of this train() call; resolved lazily when the logger dumps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        for key in LOSS_KEYS:
            self.logger.record(f"train/{key}_loss", DeviceMean(s[key], gradient_steps))
        for key in AUX_KEYS[:4]:
            self.logger.record(f"train/{key}", DeviceMean(s[key], gradient_steps))

    # ---- reference odds and ends -----------------------------------------------------------------------------------------------
    def _behavior_cloning_update(self, observations, actions) -> float:
        pass  # accepted, without effect (as BCQ)

    def _behavior_cloning_warmup(self, callback) -> None:
        pass

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "IQL",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return OfflineAlgorithm.learn(self, total_timesteps=total_timesteps, callback=callback, log_interval=log_interval,
                                      tb_log_name=tb_log_name, reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def _get_torch_save_params(self) -> tuple:
        return ["policy", "actor.optimizer", "critic.optimizer", "value_net.optimizer"], []

    def _extra_save_data(self) -> dict:
        d = dict(target_update_interval=self.target_update_interval, expectile=self.expectile, beta=self.beta, exp_adv_max=self.exp_adv_max,
                 behavior_cloning_warmup=self.behavior_cloning_warmup, n_eval_episodes=self.n_eval_episodes)
        if isinstance(self.dataset, str):
            d["dataset"] = self.dataset  # load() without dataset= reads it again
        return d

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "buffer_size", "batch_size", "tau", "gamma", "gradient_steps", "seed", "policy_kwargs",
                "target_update_interval", "expectile", "beta", "exp_adv_max", "behavior_cloning_warmup", "n_eval_episodes", "dataset")

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        ctor.pop("train_freq", None)  # the base class's (1, "step") placeholder is not a constructor argument here
        return super()._construct_for_load(env, device, ctor)
