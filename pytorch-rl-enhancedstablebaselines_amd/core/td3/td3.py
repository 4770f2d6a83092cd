"""TD3 (and DDPG as its special case) with the reference's constructor and `train()` arithmetic
(reference: core/td3/td3.py:19-240, core/ddpg/ddpg.py:14-130)."""
from typing import List, Optional, Union

import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.chain import Td3Chain
from core.common.logger import DeviceMean
from core.common.off_policy_algorithm import OffPolicyAlgorithm
from core.td3.policies import MlpPolicy, MultiInputPolicy


class TD3(OffPolicyAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy, "MultiInputPolicy": MultiInputPolicy}
    goal_face_support = True  # HER on the goal face of the env (DDPG inherits it)
    train_batch_size = 100
    chain_type = Td3Chain

    def __init__(self, policy, env, learning_rate=1e-3, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq: Union[int, tuple] = 1,
                 gradient_steps: int = 1, action_noise=None, replay_buffer_class=None, replay_buffer_kwargs: Optional[dict] = None,
                 optimize_memory_usage: bool = False, policy_delay: int = 2, target_policy_noise: float = 0.2,
                 target_noise_clip: float = 0.5, stats_window_size: int = 100, tensorboard_log: Optional[str] = None,
                 policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None, device="auto",
                 _init_setup_model: bool = True):
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq,
                         gradient_steps, action_noise=action_noise, replay_buffer_class=replay_buffer_class,
                         replay_buffer_kwargs=replay_buffer_kwargs, policy_kwargs=policy_kwargs,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, verbose=verbose, device=device,
                         seed=seed, sde_support=False, optimize_memory_usage=optimize_memory_usage,
                         supported_action_spaces=(object,), support_multi_env=True)
        self.policy_delay = policy_delay
        self.target_noise_clip = target_noise_clip
        self.target_policy_noise = target_policy_noise
        self.debug_capture = False
        self.last_train_tensors: dict = {}
        self.noise_queue: List[th.Tensor] = []  # teacher-forcing hook for the target-smoothing noise (td3.py:169)
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        super()._setup_model()
        self.actor, self.actor_target = self.policy.actor, self.policy.actor_target
        self.critic, self.critic_target = self.policy.critic, self.policy.critic_target
        z = lambda: th.zeros(1, dtype=th.float32, device=self.device)  # noqa: E731
        self._loss_sum_buf = th.zeros(2, dtype=th.float32, device=self.device)  # one fill per train() instead of two
        self._loss_sums = dict(actor=self._loss_sum_buf[0:1], critic=self._loss_sum_buf[1:2])
        self._loss_now = dict(actor=z(), critic=z())
        self._static_batch, self._packed = None, None
        from core.common.arena import FlatAdam

        self.fused_learner = (isinstance(self.actor.optimizer, FlatAdam) and isinstance(self.critic.optimizer, FlatAdam)
                              and fused.FastMLP.supported(self.actor.mu) and all(fused.FastMLP.supported(q) for q in self.critic.q_networks))
        if self.fused_learner:
            self._fast_actor, self._fast_actor_target = fused.FastMLP(self.actor.mu, self.actor.optimizer), fused.FastMLP(self.actor_target.mu)
            self._fast_critic, self._fast_critic_target = fused.FastTwinCritic(self.critic, self.policy.critic_stack), fused.FastTwinCritic(self.critic_target, self.policy.critic_target_stack)
            # critic ensembles (policy_kwargs n_critics > 2): min over all N targets, the loss and backward through all N critics;
            # n_critics == 1 (DDPG) stays on the twin loss head
            self._critic_block = fused.PerLayerTwinCritic(self._fast_critic, self._fast_critic_target, ensemble=len(self.critic.q_networks) > 2)

    def _policy_out_device(self, obs: th.Tensor) -> th.Tensor:
        if not self.fused_learner:
            return super()._policy_out_device(obs)
        with th.no_grad():
            return self._fast_actor(obs, train_params=False)

    def _rollout_net(self):
        return self._fast_actor.rollout_operands(self._denv.obs) if self.fused_learner else None

    def _use_packed_batch(self) -> bool:
        """Sample straight into the critics' input rows (no torch.cat launches) on the fused path with the stock buffer."""
        return self.fused_learner and self._stock_buffer()

    def _alloc_packed_step_tensors(self, batch_size: int) -> None:
        super()._alloc_packed_step_tensors(batch_size)
        self._act_t = th.empty(batch_size, self._packed.act_dim, dtype=th.float32, device=self.device)

    def _train_host_pre(self) -> None:
        self._update_learning_rate([self.actor.optimizer, self.critic.optimizer])

    def _graph_eligible(self, callback) -> bool:
        return super()._graph_eligible(callback) and not self.noise_queue

    def _graph_phase(self) -> int:
        # the delayed policy update makes iterations differ: one captured graph per residue of the update counter
        return self._n_updates % self.policy_delay

    def _train_host_only(self, gradient_steps: int) -> None:
        n_actor = self._n_delayed_updates(gradient_steps, self.policy_delay)
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        if n_actor > 0:
            self.logger.record("train/actor_loss", DeviceMean(self._loss_sums["actor"], n_actor))
        self.logger.record("train/critic_loss", DeviceMean(self._loss_sums["critic"], gradient_steps))

    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        # the reference keeps the last np.mean(actor_losses) until the next actor update (td3.py:207-211): a call without a
        # policy update zeroes the critic slot only, so a log dump after it still resolves the lazily-read actor loss
        n_actor = self._n_delayed_updates(gradient_steps, self.policy_delay)
        # one gradient step per train() call (the default) on the fused path: the loss kernels STORE the logged values into the
        # sums (an actor-less call leaves the actor's slot alone), no zero-fill launch
        self._single_step = gradient_steps == 1 and self.fused_learner
        if not self._single_step:
            (self._loss_sum_buf if n_actor > 0 else self._loss_sum_buf[1:2]).zero_()
        n_updates = self._n_updates  # host counter advances in _train_host_only
        for _ in range(gradient_steps):
            n_updates += 1
            if self.fused_learner:
                self._gradient_step_fused(batch_size, n_updates)
                continue
            replay_data = self.replay_buffer.sample_into(self._batch(batch_size))
            with th.no_grad():
                if self.noise_queue:
                    noise = self.noise_queue.pop(0).to(self.device)
                else:
                    noise = replay_data.actions.clone().normal_(0, self.target_policy_noise)  # :169
                noise = noise.clamp(-self.target_noise_clip, self.target_noise_clip)
                next_actions = (self.actor_target(replay_data.next_observations) + noise).clamp(-1, 1)
                qs = self.critic_target(replay_data.next_observations, next_actions)
                if len(qs) <= 2:
                    q1_t, q2_t = qs[0], qs[-1]  # n_critics == 1 (DDPG): min over one network
                    hip_ops.td_target_min(q1_t.contiguous(), q2_t.contiguous(), None, replay_data.rewards, replay_data.dones,
                                          None, self.gamma, self._target_q)
                    target_q_values = self._target_q
                else:  # critic ensembles: the reference's own statements (:174-176)
                    next_q_values, _ = th.min(th.cat(qs, dim=1), dim=1, keepdim=True)
                    target_q_values = replay_data.rewards + (1 - replay_data.dones) * self.gamma * next_q_values
            current_q_values = self.critic(replay_data.observations, replay_data.actions)
            critic_loss = sum(F.mse_loss(current_q, target_q_values) for current_q in current_q_values)  # no 0.5 (:182)
            self._loss_sums["critic"] += critic_loss.detach()
            self.critic.optimizer.zero_grad()
            critic_loss.backward()
            self._allreduce_grads(self.policy.critic_arena)
            self.critic.optimizer.step()
            actor_loss = None
            if n_updates % self.policy_delay == 0:  # :192-206
                actor_loss = self._actor_loss_torch(replay_data)
                self._loss_sums["actor"] += actor_loss.detach()
                self.actor.optimizer.zero_grad()
                actor_loss.backward()
                self._allreduce_grads(self.policy.actor_arena)
                self.actor.optimizer.step()
                self.policy.critic_target_arena.polyak_from(self.policy.critic_arena, self.tau)
                self.policy.actor_target_arena.polyak_from(self.policy.actor_arena, self.tau)
            if self.debug_capture:
                self.last_train_tensors = dict(target_q=target_q_values.clone(), current_q=[q.detach().clone() for q in current_q_values],
                                               critic_loss=critic_loss.detach().clone(),
                                               actor_loss=None if actor_loss is None else actor_loss.detach().clone())

    def _gradient_step_fused(self, batch_size: int, n_updates: int) -> None:
        """td3.py:161-206 on the fused path (core/common/fused.py)."""
        pol = self.policy
        chain = self._chain_for(batch_size)
        # a gather in the first layer behind the sample (:161): the chain's target-actor launch, or the target actor's first layer below
        pb, gather, rd = self._sample(batch_size, True if chain is not None else self._target_actor_gathers)
        if chain is not None:  # the row-chain kernels (core/common/chain.py): 4 launches (9 with the policy step) instead of 13 (22)
            return chain.step(self, pb, gather, n_updates)
        blk = self._critic_block
        with th.no_grad():  # :167-176
            if pb is not None:
                # target smoothing in ONE launch (clone + normal_ + clamp + add + clamp), written into x_next's action columns
                queued = self.noise_queue.pop(0).to(self.device, th.float32).contiguous() if self.noise_queue else None
                rng = None if queued is not None else self._device_rng()
                if fused.USE_SMOOTH_IN_LAST_LAYER and self._fast_actor_target.smooth_supported(rd.next_observations):
                    # ... inside the target actor's last layer (one launch less)
                    self._fast_actor_target(rd.next_observations, train_params=False, gather=gather,
                                            smooth=dict(noise=queued, rng_ctl=rng, sigma=self.target_policy_noise, clip=self.target_noise_clip,
                                                        out=pb.x_next[:, pb.obs_dim:]))
                else:
                    a_t = self._fast_actor_target(rd.next_observations, train_params=False, gather=gather)
                    hip_ops.target_smooth(a_t, queued, rng, self.target_policy_noise, self.target_noise_clip, pb.x_next[:, pb.obs_dim:])
                x_next = pb.x_next
            else:
                noise = self.noise_queue.pop(0).to(self.device) if self.noise_queue else rd.actions.clone().normal_(0, self.target_policy_noise)
                noise = noise.clamp(-self.target_noise_clip, self.target_noise_clip)
                next_actions = (self._fast_actor_target(rd.next_observations, train_params=False) + noise).clamp(-1, 1)
                x_next = th.cat([rd.next_observations, next_actions], dim=1)
        # :173 and :179: ONE four-network chain on a packed batch (three launches instead of six), else the target's pass, then the critic's
        qs, qs_t = blk.forward(pb.x_data if pb is not None else th.cat([rd.observations, rd.actions], dim=1), x_next, pair=pb is not None)
        # TD target (:174-176) + critic loss (:182, no 0.5) + the critic's backward
        c_out, c_sum = self._loss_slot("critic")
        blk.td_step(qs, qs_t, rd, self.gamma, 1.0, self._target_q, c_out, c_sum)
        self._allreduce_grads(pol.critic_arena)
        self.critic.optimizer.step()
        actor_done = False
        if n_updates % self.policy_delay == 0:  # :192-206
            a_out = self._actor_pass_fused(pb, rd, blk)
            self._allreduce_grads(pol.actor_arena)
            # the actor's step, the critics' soft update (disjoint arenas) and the actor target's soft update (by the threads that
            # have just computed the new actor weights) in ONE launch (:199, :204, :205)
            if not pol.actor_target_arena.same_layout(pol.actor_arena):
                raise ValueError("Iterables have different lengths")  # zip_strict's error (utils.py:447)
            self.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, self.tau),
                                           own_target=(pol.actor_target_arena.flat, self.tau))
            actor_done = True
        if self.debug_capture:
            self.last_train_tensors = blk.captured(qs, self._target_q, c_out, a_out if actor_done else None)

    # ---- the actor pass: what a subclass with another actor loss replaces (core/td3bc/td3bc.py) --------------------------------
    def _actor_loss_torch(self, replay_data) -> th.Tensor:
        """:194 as the reference's torch statement"""
        return -self.critic.q1_forward(replay_data.observations, self.actor(replay_data.observations)).mean()

    def _actor_pass_fused(self, pb, rd, blk) -> th.Tensor:
        """:192-197 on the fused path: the actor's forward, the loss and the backward down to the actor's gradients; returns the
        tensor the loss value was stored in."""
        if pb is not None and fused.USE_FUSED_LINEAR and self._fast_actor.layers[-1][0].out_features > 1:
            # the actor's last layer writes into x_pi = (obs | .): no torch.cat, and its backward reads the action columns
            # of the critic's input gradient in place
            x_pi = self._fast_actor(rd.observations, xbuf=pb.x_pi.detach())
        else:
            x_pi = th.cat([rd.observations, self._fast_actor(rd.observations)], dim=1)
        a_out, a_sum = self._loss_slot("actor")
        blk.neg_mean_pass(x_pi, a_out, a_sum)  # -mean(Q1) (:194) through the (frozen) first Q network
        return a_out

    def _target_actor_gathers(self, pb) -> bool:
        return self._fast_actor_target.gather_supported(pb.samples.next_observations)

    def _get_torch_save_params(self) -> tuple:
        """reference: td3.py:234-240"""
        return ["policy", "actor.optimizer", "critic.optimizer"], []

    def _extra_save_data(self) -> dict:
        return dict(policy_delay=self.policy_delay, target_policy_noise=self.target_policy_noise, target_noise_clip=self.target_noise_clip)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return super()._ctor_keys() + ("policy_delay", "target_policy_noise", "target_noise_clip")

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "TD3",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval,
                             tb_log_name=tb_log_name, reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)


class DDPG(TD3):
    """reference: core/ddpg/ddpg.py:14-130 -- TD3 with policy_delay 1, one critic and a smoothing draw clamped to [-0, 0]
    (the reference passes target_policy_noise=0.1, target_noise_clip=0.0: the attribute values are kept, the noise is zero)."""

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return OffPolicyAlgorithm._ctor_keys()

    def __init__(self, policy, env, learning_rate=1e-3, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq: Union[int, tuple] = 1,
                 gradient_steps: int = 1, action_noise=None, replay_buffer_class=None, replay_buffer_kwargs=None,
                 optimize_memory_usage: bool = False, tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None,
                 verbose: int = 0, seed: Optional[int] = None, device="auto", _init_setup_model: bool = True):
        policy_kwargs = dict(policy_kwargs or {})
        policy_kwargs.setdefault("n_critics", 1)
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq,
                         gradient_steps, action_noise, replay_buffer_class, replay_buffer_kwargs, optimize_memory_usage,
                         policy_delay=1, target_policy_noise=0.1, target_noise_clip=0.0, tensorboard_log=tensorboard_log,
                         policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device,
                         _init_setup_model=_init_setup_model)
