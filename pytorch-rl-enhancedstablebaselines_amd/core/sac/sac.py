"""Soft Actor-Critic with the reference's constructor and `train()` arithmetic (reference: core/sac/sac.py:21-340).

One gradient step = HIP sampler (bit-exact indices + gather) -> actor/critic MLP forward/backward on
PyTorch-ROCm -> HIP `td_target_min` -> three one-launch Adam steps on flat arenas (RCCL all-reduce of each
arena's gradient first when data-parallel) -> one-launch polyak. Losses stay on the device: the reference's
four `.item()` syncs per step (:232, :236, :263, :276) are replaced by device-side running sums that the
logger resolves only when it dumps.
"""
from typing import Optional, Union

import numpy as np
import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.arena import FlatAdam, ParamArena
from core.common.chain import SacChain
from core.common.logger import DeviceMean
from core.common.off_policy_algorithm import OffPolicyAlgorithm
from core.sac.policies import MlpPolicy, MultiInputPolicy


class SAC(OffPolicyAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy, "MultiInputPolicy": MultiInputPolicy}
    goal_face_support = True  # HER on the goal face of the env
    train_batch_size = 64
    chain_type = SacChain

    def __init__(self, policy, env, learning_rate=3e-4, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq: Union[int, tuple] = 1,
                 gradient_steps: int = 1, action_noise=None, replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None,
                 optimize_memory_usage: bool = False, ent_coef: Union[str, float] = "auto", target_update_interval: int = 1,
                 target_entropy: Union[str, float] = "auto", use_sde: bool = False, sde_sample_freq: int = -1,
                 use_sde_at_warmup: bool = False, stats_window_size: int = 100, tensorboard_log: Optional[str] = None,
                 policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None, device="auto",
                 _init_setup_model: bool = True):
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq,
                         gradient_steps, action_noise, replay_buffer_class=replay_buffer_class,
                         replay_buffer_kwargs=replay_buffer_kwargs, policy_kwargs=policy_kwargs,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, verbose=verbose, device=device,
                         seed=seed, use_sde=use_sde, sde_sample_freq=sde_sample_freq, use_sde_at_warmup=use_sde_at_warmup,
                         optimize_memory_usage=optimize_memory_usage, supported_action_spaces=(object,), support_multi_env=True)
        self.target_entropy = target_entropy
        self.log_ent_coef: Optional[th.Tensor] = None
        self.ent_coef = ent_coef
        self.target_update_interval = target_update_interval
        self.ent_coef_optimizer = None
        self.debug_capture = False   # tests: keep target_q / current_q of the last gradient step
        self.last_train_tensors: dict = {}
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        """reference: sac.py:159-192"""
        super()._setup_model()
        self._create_aliases()
        if self.target_entropy == "auto":
            self.target_entropy = float(-np.prod(self.env.action_space.shape).astype(np.float32))
        else:
            self.target_entropy = float(self.target_entropy)
        if isinstance(self.ent_coef, str) and self.ent_coef.startswith("auto"):
            init_value = 1.0
            if "_" in self.ent_coef:
                init_value = float(self.ent_coef.split("_")[1])
                assert init_value > 0.0, "The initial value of ent_coef must be greater than 0"
            p = th.nn.Parameter(th.log(th.ones(1) * init_value))
            # its gradient lives in the tail of the critic's gradient buffer: one all-reduce serves both (data-parallel)
            tail = getattr(self.policy.critic_arena, "grad_tail", None)
            self._ent_arena = ParamArena([p], self.device, grad_storage=tail)
            self._ent_rides_critic = tail is not None
            self.log_ent_coef = p
            self.ent_coef_optimizer = FlatAdam(self._ent_arena, lr=self.lr_schedule(1))
            if self.world_size > 1:
                self.ent_coef_optimizer.grad_scale = 1.0 / self.world_size
        else:
            self.ent_coef_tensor = th.tensor(float(self.ent_coef), device=self.device)
        z = lambda: th.zeros(1, dtype=th.float32, device=self.device)  # noqa: E731
        self._loss_sum_buf = th.zeros(4, dtype=th.float32, device=self.device)  # one fill per train() instead of four
        sb = self._loss_sum_buf
        self._loss_sums = dict(actor=sb[0:1], critic=sb[1:2], ent_coef_loss=sb[2:3], ent_coef=sb[3:4])
        self._loss_now = dict(actor=z(), critic=z(), ent_coef=z())  # no ent_coef_loss: a step that is not stored is only summed
        self._static_batch, self._packed = None, None
        # fused learner path (core/common/fused.py): GEMMs in rocBLAS, everything else hand-written HIP
        self.fused_learner = self._fused_supported()
        if self.fused_learner:
            self._fast_actor = fused.FastSacActor(self.actor, self.policy.actor_head)
            self._fast_critic = fused.FastTwinCritic(self.critic, self.policy.critic_stack)
            self._fast_critic_target = fused.FastTwinCritic(self.critic_target, self.policy.critic_target_stack)
            # critic ensembles (policy_kwargs n_critics != 2): the N-critic loss heads, per-layer critic passes
            self._critic_block = fused.PerLayerTwinCritic(self._fast_critic, self._fast_critic_target, ensemble=len(self.critic.q_networks) != 2)
        if self.use_sde:  # the ATen path differentiates the matrices as torch expressions; the fused head reads the draw buffers
            self.actor.action_dist.torch_matrices = not self.fused_learner

    def _fused_supported(self) -> bool:
        return (1 <= len(self.critic.q_networks) <= hip_ops.nv.MAX_ENS_CRITICS and isinstance(self.actor.optimizer, FlatAdam)
                and isinstance(self.critic.optimizer, FlatAdam) and fused.FastMLP.supported(self.actor.latent_pi)
                and all(fused.FastMLP.supported(q) for q in self.critic.q_networks))

    def _policy_out_device(self, obs: th.Tensor) -> th.Tensor:
        if not self.fused_learner:
            return super()._policy_out_device(obs)
        fa = self._fast_actor
        with th.no_grad():
            out = fa.action_log_prob(obs, train_params=False, want_logp=False, defer_rng=True)[0]
        self._rng_advance, fa.deferred_rng = fa.deferred_rng, None  # the fused collect launch advances the Philox offset
        return out

    def _rollout_net(self):
        return self._fast_actor.rollout_operands(self._denv.obs) if self.fused_learner else None

    def _create_aliases(self) -> None:
        self.actor = self.policy.actor
        self.critic = self.policy.critic
        self.critic_target = self.policy.critic_target

    def _use_packed_batch(self) -> bool:
        """Sample straight into the critics' input rows (no torch.cat launches): the fused path with the merged actor head and
        the stock ReplayBuffer without a VecNormalize normaliser."""
        return (self.fused_learner and self._fast_actor.head is not None and self._stock_buffer()
                and self._fast_actor.act_dim <= hip_ops.nv.MAX_HEAD_ACT)

    def _train_host_pre(self) -> None:
        optimizers = [self.actor.optimizer, self.critic.optimizer]
        if self.ent_coef_optimizer is not None:
            optimizers += [self.ent_coef_optimizer]
        self._update_learning_rate(optimizers)  # :208

    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        # one gradient step per train() call (the default): the loss kernels STORE the logged values, no zero-fill launch
        self._single_step = gradient_steps == 1 and self.fused_learner and self.ent_coef_optimizer is not None
        if not self._single_step:
            self._loss_sum_buf.zero_()
        for gradient_step in range(gradient_steps):
            self._gradient_step(batch_size, gradient_step)

    def _train_host_only(self, gradient_steps: int) -> None:
        self._n_updates += gradient_steps
        s = self._loss_sums  # device-side sums of this train() call; resolved lazily when the logger dumps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/ent_coef", DeviceMean(s["ent_coef"], gradient_steps))
        self.logger.record("train/actor_loss", DeviceMean(s["actor"], gradient_steps))
        self.logger.record("train/critic_loss", DeviceMean(s["critic"], gradient_steps))
        if self.ent_coef_optimizer is not None:
            self.logger.record("train/ent_coef_loss", DeviceMean(s["ent_coef_loss"], gradient_steps))

    def _gradient_step(self, batch_size: int, gradient_step: int) -> None:
        if self.use_sde:  # :218-219 -- log_std may have changed since the last draw
            self.actor.reset_noise()
        if self.fused_learner:
            return self._gradient_step_fused(batch_size, gradient_step)
        return self._gradient_step_aten(batch_size, gradient_step)

    def _gradient_step_fused(self, batch_size: int, gradient_step: int) -> None:
        """The same statements as `_gradient_step_aten` (sac.py:215-287), evaluated on the fused path: losses are
        backward roots whose kernels emit d(loss)/d(inputs) directly; parameter gradients land in the arenas."""
        s, pol = self._loss_sums, self.policy
        (c_out, c_sum), (a_out, a_sum) = self._loss_slot("critic"), self._loss_slot("actor")
        chain = self._chain_for(batch_size)
        # a gather in the first layer behind the sample: the chain's actor launch, or the 2B-row actor pass below
        pb, gather, rd = self._sample(batch_size, True if chain is not None else self._fast_actor.pair_supported)  # :215
        if chain is not None:  # the row-chain kernels (core/common/chain.py): 8 launches instead of 20 (10 under data-parallel)
            return chain.step(self, pb, gather, gradient_step)
        blk = self._critic_block

        pair = pb is not None and self._fast_actor.pair_supported(pb)
        assert gather is None or pair
        if pair:  # :222 and :247 in ONE 2B-row actor pass (three launches instead of six)
            x_pi, log_prob, x_next, next_log_prob = self._fast_actor.action_log_prob_pair(pb, gather=gather)
        elif pb is not None:  # x_pi = (obs | pi(obs)): the actor head writes the action columns of the critic input itself
            x_pi, log_prob = self._fast_actor.action_log_prob(rd.observations, xbuf=pb.x_pi.detach())  # :222
        else:
            actions_pi, log_prob = self._fast_actor.action_log_prob(rd.observations)  # :222

        # :230-261. ONE launch for the three batch reductions between the forward passes and the critic backward: the entropy
        # coefficient's loss (ent_coef = exp(log_ent_coef) BEFORE the update, :230; the updated value is first used by the
        # next gradient step, so its optimiser step may wait for the critic's all-reduce: one collective instead of two),
        # the TD target (:245-254) and the critic loss (:258-261)
        with th.no_grad():
            if pb is None:
                next_actions, next_log_prob = self._fast_actor.action_log_prob(rd.next_observations, train_params=False)
                x_next = th.cat([rd.next_observations, next_actions], dim=1)
            elif not pair:
                x_next, next_log_prob = self._fast_actor.action_log_prob(rd.next_observations, train_params=False, xbuf=pb.x_next)
        # :250 and :258: ONE four-network chain on a packed batch (three launches instead of six), else the target's pass, then the critic's
        qs, qs_t = blk.forward(pb.x_data if pb is not None else th.cat([rd.observations, rd.actions], dim=1), x_next, pair=pb is not None)
        ent_opt = self.ent_coef_optimizer
        if ent_opt is not None:
            (ent_coef, ent_coef_sum), (e_out, e_sum) = self._loss_slot("ent_coef"), self._loss_slot("ent_coef_loss")
            alpha = dict(log_alpha=self.log_ent_coef.detach(), logp_pi=log_prob.detach(), target_entropy=self.target_entropy,
                         grad_out=self._ent_arena.grad[0:1], ent_coef_out=ent_coef, loss_out=e_out, loss_sum=e_sum, ent_coef_sum=ent_coef_sum)
        else:
            ent_coef, alpha = self.ent_coef_tensor.reshape(1), None
            s["ent_coef"] += ent_coef
        # the entropy coefficient's own collective and step (:240-243), as soon as the launch that leaves its gradient has been issued
        blk.td_step(qs, qs_t, rd, self.gamma, 0.5, self._target_q, c_out, c_sum, next_logp=next_log_prob, ent_coef=ent_coef, alpha=alpha,
                    after_loss=self._ent_coef_step if ent_opt is not None and not self._ent_rides_critic else None)  # :266-268
        self._allreduce_grads(pol.critic_arena)
        if ent_opt is not None and self._ent_rides_critic:
            # :240-243 (gradient averaged by the critic's collective) and :266-268 in one launch
            self.critic.optimizer.step_with(ent_opt)
        else:
            self.critic.optimizer.step()

        # :273-275 (critic weights frozen) and :279-281
        blk.sac_actor_pass(x_pi if pb is not None else th.cat([rd.observations, actions_pi], dim=1), log_prob, ent_coef, a_out, a_sum)
        self._allreduce_grads(pol.actor_arena)
        if gradient_step % self.target_update_interval == 0:  # :281 and :284-287 (disjoint arenas) in one launch
            self.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, self.tau))
        else:
            self.actor.optimizer.step()

        if self.debug_capture:
            self.last_train_tensors = blk.captured(qs, self._target_q, c_out, a_out, ent_coef=ent_coef.detach().clone(),
                                                   log_prob=log_prob.detach().clone())

    def _ent_coef_step(self) -> None:
        self._allreduce_grads(self._ent_arena)
        self.ent_coef_optimizer.step()

    def _chain_for(self, batch_size: int):
        step = super()._chain_for(batch_size)
        if step is not None and len(self.actor.action_dist.eps_queue) not in (0, 2):
            return None  # the chain step takes queued (teacher-forced) draws as the pi(obs) / pi(next_obs) pair only
        return step

    def _gradient_step_aten(self, batch_size: int, gradient_step: int) -> None:
        """Stock-ATen evaluation of the step (nn.Module forwards, autograd losses): the fallback for configurations the
        fused path does not cover (custom activations / optimisers, more than 16 critics) and the A/B reference in tests."""
        s = self._loss_sums
        replay_data = self.replay_buffer.sample_into(self._batch(batch_size))  # :215

        actions_pi, log_prob = self.actor.action_log_prob(replay_data.observations)  # :222
        log_prob = log_prob.reshape(-1, 1)

        if self.ent_coef_optimizer is not None and self.log_ent_coef is not None:
            ent_coef = th.exp(self.log_ent_coef.detach())  # :230
            ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
            s["ent_coef_loss"] += ent_coef_loss.detach()
            self.ent_coef_optimizer.zero_grad()  # :240-243
            ent_coef_loss.backward()
            self._allreduce_grads(self._ent_arena)
            self.ent_coef_optimizer.step()
        else:
            ent_coef = self.ent_coef_tensor.reshape(1)
        s["ent_coef"] += ent_coef.reshape(1)

        with th.no_grad():  # :245-254
            next_actions, next_log_prob = self.actor.action_log_prob(replay_data.next_observations)
            qs_t = self.critic_target(replay_data.next_observations, next_actions)
            if len(qs_t) == 2:
                q1_t, q2_t = qs_t
                target_q_values = self._target_q
                hip_ops.td_target_min(q1_t.contiguous(), q2_t.contiguous(), next_log_prob.reshape(-1, 1).contiguous(),
                                      replay_data.rewards, replay_data.dones, ent_coef.contiguous(), self.gamma, target_q_values)
            else:  # critic ensembles: the reference's own statements (:248-253)
                next_q_values, _ = th.min(th.cat(qs_t, dim=1), dim=1, keepdim=True)
                next_q_values = next_q_values - ent_coef * next_log_prob.reshape(-1, 1)
                target_q_values = replay_data.rewards + (1 - replay_data.dones) * self.gamma * next_q_values

        current_q_values = self.critic(replay_data.observations, replay_data.actions)  # :258
        critic_loss = 0.5 * sum(F.mse_loss(current_q, target_q_values) for current_q in current_q_values)  # :261
        s["critic"] += critic_loss.detach()
        self.critic.optimizer.zero_grad()  # :266-268
        critic_loss.backward()
        self._allreduce_grads(self.policy.critic_arena)
        self.critic.optimizer.step()

        q_values_pi = th.cat(self.critic(replay_data.observations, actions_pi), dim=1)  # :273-275
        min_qf_pi, _ = th.min(q_values_pi, dim=1, keepdim=True)
        actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
        s["actor"] += actor_loss.detach()
        self.actor.optimizer.zero_grad()  # :279-281
        actor_loss.backward()
        self._allreduce_grads(self.policy.actor_arena)
        self.actor.optimizer.step()

        if gradient_step % self.target_update_interval == 0:  # :284-287 (no batch-norm stats in MLPs)
            self.policy.critic_target_arena.polyak_from(self.policy.critic_arena, self.tau)

        if self.debug_capture:
            self.last_train_tensors = dict(target_q=target_q_values.clone(), current_q=[q.detach().clone() for q in current_q_values],
                                           critic_loss=critic_loss.detach().clone(), actor_loss=actor_loss.detach().clone(),
                                           ent_coef=ent_coef.detach().clone(), log_prob=log_prob.detach().clone())

    def _get_torch_save_params(self) -> tuple:
        """reference: sac.py:319-326"""
        state_dicts = ["policy", "actor.optimizer", "critic.optimizer"]
        if self.ent_coef_optimizer is not None:
            return state_dicts + ["ent_coef_optimizer"], ["log_ent_coef"]
        return state_dicts, ["ent_coef_tensor"]

    def _extra_save_data(self) -> dict:
        data = dict(ent_coef=self.ent_coef, target_update_interval=self.target_update_interval, target_entropy=self.target_entropy)
        if self.use_sde:
            data.update(use_sde=True, sde_sample_freq=self.sde_sample_freq, use_sde_at_warmup=self.use_sde_at_warmup)
        return data

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return super()._ctor_keys() + ("ent_coef", "target_update_interval", "target_entropy", "use_sde", "sde_sample_freq", "use_sde_at_warmup")

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "SAC",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval,
                             tb_log_name=tb_log_name, reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)
