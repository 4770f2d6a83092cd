"""BCQ (Batch-Constrained deep Q-learning) with the reference's constructor and `train()` arithmetic
(reference: core/bcq/bcq.py:21-245). Per gradient step (:137-213): the VAE step, the copy of the VAE into the target actor, the TD
target from ten perturbed candidates per next state, the critic step and -- every `actor_delay`-th step -- the perturbation net's step
and the soft target updates.

Where this differs from the reference: `faithful_quirks=True` (default) reproduces its target grouping -- row i of the
target takes the max over flat entries 10 i ... 10 i + 9 of the [sample][state] candidate list, which belong to ten DIFFERENT next
states (:171-172) --, `False` takes the max over a state's own ten candidates; noise comes from a device Philox stream unless it is
teacher-forced through `noise_queue`."""
from typing import List, Optional, Union

import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.logger import DeviceMean
from core.common.offline_policy_algorithm import OfflineAlgorithm
from core.bcq.policies import MlpPolicy

TRAIN_SAMPLES = 10  # candidates per next state in train() (:161)


class BCQ(OfflineAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    train_batch_size = 100
    packed_batch_with_pi = False  # the candidates have their own rows (fused.FastBcq)

    def __init__(self, policy, env, dataset=None, learning_rate=3e-4, buffer_size: int = 1_000_000, batch_size: int = 256,
                 tau: float = 0.005, gamma: float = 0.99, gradient_steps: int = 1, behavior_cloning_warmup: int = 0,
                 n_eval_episodes: int = 10, policy_kwargs: Optional[dict] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, verbose: int = 0, device: Union[th.device, str] = "auto",
                 seed: Optional[int] = None, actor_delay: int = 2, _init_setup_model: bool = True, faithful_quirks: bool = True):
        super().__init__(policy=policy, env=env, dataset=dataset, learning_rate=learning_rate, buffer_size=buffer_size,
                         batch_size=batch_size, tau=tau, gamma=gamma, gradient_steps=gradient_steps, dataset_buffer_class=None,
                         dataset_buffer_kwargs=None, n_eval_episodes=n_eval_episodes, behavior_cloning_warmup=behavior_cloning_warmup,
                         conservative_weight=0.0, policy_kwargs=policy_kwargs, stats_window_size=stats_window_size,
                         tensorboard_log=tensorboard_log, verbose=verbose, device=device, seed=seed)
        if self.world_size > 1:
            raise NotImplementedError("data-parallel BCQ is not built")
        self.actor_delay = actor_delay
        self.faithful_quirks = faithful_quirks
        self.debug_capture = False
        self.last_train_tensors: dict = {}
        # teacher-forcing hook: each gradient step pops the raw draws of policies.py:82 ([B, L]), :123 ([10 B, L], before the clamp)
        # and, on actor steps, :123 again ([B, L])
        self.noise_queue: List[th.Tensor] = []
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        from core.common.arena import FlatAdam

        super()._setup_model()
        pol = self.policy
        self.actor, self.actor_target = pol.actor, pol.actor_target
        self.critic, self.critic_target = pol.critic, pol.critic_target
        z = lambda: th.zeros(1, dtype=th.float32, device=self.device)  # noqa: E731
        self._loss_sum_buf = th.zeros(3, dtype=th.float32, device=self.device)
        self._loss_sums = dict(actor=self._loss_sum_buf[0:1], critic=self._loss_sum_buf[1:2], vae=self._loss_sum_buf[2:3])
        self._loss_now = dict(actor=z(), critic=z(), vae=z())
        self._static_batch, self._packed = None, None
        self._fused_learner = (all(isinstance(o, FlatAdam) for o in (self.actor.vae_optimizer, self.actor.perturbation_optimizer,
                                                                     self.critic.optimizer)) and fused.FastBcq.supported(pol))
        if self._fused_learner:
            pol.fast = self._fast = fused.FastBcq(pol)
            self._fast.rng_ctl = self._device_rng()  # one Philox stream for train() and predict(); set_random_seed reseeds it in place
            # the target is computed here (`bcq_target`), so the losses are launches of their own: no loss-root form
            self._critic_block = fused.PerLayerTwinCritic(self._fast.critic, self._fast.critic_t, loss_roots=False)

    @property
    def fused_learner(self) -> bool:
        """True: the kernel path (fused Linear kernels, or rocBLAS GEMMs with CSTR_FUSED_LINEAR=0); False: the reference's own torch
        statements on the arena parameters (also for n_critics != 2, a latent / action width the kernels decline, another optimiser)."""
        return self._fused_learner

    @fused_learner.setter
    def fused_learner(self, value: bool) -> None:
        if value and getattr(self, "_fast", None) is None:
            raise ValueError("this BCQ model has no kernel path (n_critics != 2, unsupported widths or a non-default optimiser)")
        self._fused_learner = bool(value)
        self.policy.fast = self._fast if value else None

    # ---- batches -----------------------------------------------------------------------------------------------------
    def _alloc_step_tensors(self, batch_size: int) -> None:
        pass  # `_step_bufs`: the kernel path's step tensors follow the batch it actually sampled

    def _use_packed_batch(self) -> bool:
        return self._fused_learner and self._stock_buffer()

    def _step_bufs(self, batch_size: int):
        b = getattr(self, "_bufs", None)
        if b is None or b["target_q"].shape[0] != batch_size:
            e = lambda *sh: th.empty(*sh, dtype=th.float32, device=self.device)  # noqa: E731
            lat, a = self._fast.latent, self._fast.act_dim
            b = self._bufs = dict(target_q=e(batch_size, 1), g_recon=e(batch_size, a), gkl=(e(batch_size, lat), e(batch_size, lat)))
        return b

    # ---- train -------------------------------------------------------------------------------------------------------
    def _train_host_pre(self) -> None:
        self._update_learning_rate([self.actor.perturbation_optimizer, self.actor.vae_optimizer, self.critic.optimizer])  # :134

    def _graph_eligible(self, callback) -> bool:
        return super()._graph_eligible(callback) and not self.noise_queue and self._use_packed_batch()

    def _graph_phase(self) -> int:
        return self._n_updates % self.actor_delay  # the delayed actor step: one captured graph per residue

    def _train_host_only(self, gradient_steps: int) -> None:
        n_actor = self._n_delayed_updates(gradient_steps, self.actor_delay)
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        if n_actor > 0:  # :210-211 (the last mean stays logged until the next actor step)
            self.logger.record("train/actor_loss", DeviceMean(self._loss_sums["actor"], n_actor))
        self.logger.record("train/critic_loss", DeviceMean(self._loss_sums["critic"], gradient_steps))
        self.logger.record("train/vae_loss", DeviceMean(self._loss_sums["vae"], gradient_steps))

    def _pop_noise(self) -> Optional[th.Tensor]:
        return self.noise_queue.pop(0).to(self.device, th.float32).contiguous() if self.noise_queue else None

    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        n_actor = self._n_delayed_updates(gradient_steps, self.actor_delay)
        # one gradient step per call on the kernel path: the loss kernels STORE the logged values (an actor-less call leaves the actor's
        # slot alone, so a log dump after it still resolves the last actor loss), no zero-fill launch
        self._single_step = gradient_steps == 1 and self._fused_learner
        if not self._single_step:
            (self._loss_sum_buf if n_actor > 0 else self._loss_sum_buf[1:3]).zero_()
        n_updates = self._n_updates  # the host counter advances in _train_host_only
        for _ in range(gradient_steps):
            n_updates += 1
            if self._fused_learner:
                self._gradient_step_fused(batch_size, n_updates)
            else:
                self._gradient_step_torch(batch_size, n_updates)

    def _gradient_step_torch(self, batch_size: int, n_updates: int) -> None:
        """bcq.py:137-207 as the reference's own torch statements on the arena parameters."""
        s, pol = self._loss_sums, self.policy
        rd = self.replay_buffer.sample_into(self._batch(batch_size))  # :140
        recon, mean, std = self.actor.vae(state=rd.observations, action=rd.actions, eps=self._pop_noise())  # :143
        recon_loss = F.mse_loss(recon, rd.actions)
        kl_loss = -0.5 * (1 + th.log(std.pow(2)) - mean.pow(2) - std.pow(2)).mean()
        vae_loss = recon_loss + 0.5 * kl_loss
        self.actor.vae_optimizer.zero_grad()
        vae_loss.backward()
        self.actor.vae_optimizer.step()
        s["vae"] += vae_loss.detach()
        with th.no_grad():
            pol.vae_target_arena.flat.copy_(pol.vae_arena.flat)  # :160
            cand = self.actor_target(rd.next_observations, num_samples=TRAIN_SAMPLES, noise=self._pop_noise())
            rep = rd.next_observations.repeat(TRAIN_SAMPLES, 1)
            next_q, _ = th.min(th.cat(self.critic_target(rep, cand), dim=1), dim=1, keepdim=True)  # min over ALL critics
            next_q_min = next_q
            if self.faithful_quirks:
                next_q = next_q.reshape(batch_size, TRAIN_SAMPLES).max(1)[0].unsqueeze(1)  # :171-172
            else:
                next_q = next_q.reshape(TRAIN_SAMPLES, batch_size).max(0)[0].unsqueeze(1)  # a state's own candidates
            target_q = rd.rewards + (1 - rd.dones) * self.gamma * next_q
        current_q = self.critic(rd.observations, rd.actions)
        critic_loss = sum(F.mse_loss(q, target_q) for q in current_q)
        s["critic"] += critic_loss.detach()
        self.critic.optimizer.zero_grad()
        critic_loss.backward()
        self.critic.optimizer.step()
        actor_loss = None
        if n_updates % self.actor_delay == 0:  # :189-207
            actor_loss = -self.critic.q1_forward(rd.observations, self.actor(rd.observations, num_samples=1, noise=self._pop_noise())).mean()
            s["actor"] += actor_loss.detach()
            self.actor.perturbation_optimizer.zero_grad()
            actor_loss.backward()
            self.actor.perturbation_optimizer.step()
            pol.critic_target_arena.polyak_from(pol.critic_arena, self.tau)
            pol.pert_target_arena.polyak_from(pol.pert_arena, self.tau)
            pol.vae_target_arena.flat.copy_(pol.vae_arena.flat)  # polyak of the VAE, then the copy over it (:201-203)
        if self.debug_capture:
            self.last_train_tensors = dict(target_q=target_q.clone(), current_q=[q.detach().clone() for q in current_q],
                                           critic_loss=critic_loss.detach().clone(), vae_loss=vae_loss.detach().clone(),
                                           recon=recon.detach().clone(), next_q_min=next_q_min.clone(),
                                           actor_loss=None if actor_loss is None else actor_loss.detach().clone())

    def _gradient_step_fused(self, batch_size: int, n_updates: int) -> None:
        """bcq.py:137-207 on the kernel path (core/common/fused.py FastBcq, csrc/cstr_bcq.hip)."""
        pol, fast, blk = self.policy, self._fast, self._critic_block
        pb, _, rd = self._sample(batch_size)  # :140 (+ cat([obs, act]) for the encoder and the critics)
        # (a VecNormalize'd buffer: the contiguous batch, one cat launch)
        x_data = pb.x_data if pb is not None else th.cat([rd.observations, rd.actions], dim=1)
        B = x_data.shape[0]
        bufs = self._step_bufs(B)
        # VAE step (:143-154): encoder, merged head + latent launch, decoder, loss launch, backward, Adam; the copy into the target
        # actor (:160) rides in the Adam launch (own_target with tau = 1: target = 1 * p + 0 * target)
        recon, params, std = fast.vae_forward(x_data, rd.observations, self._pop_noise(), bufs["gkl"])
        v_out, v_sum = self._loss_slot("vae")
        hip_ops.bcq_vae_loss(recon.detach(), rd.actions, params, std, bufs["g_recon"], bufs["gkl"][0], bufs["gkl"][1], v_out, v_sum)
        with fused.deferred_weight_grads():
            th.autograd.backward([recon], [bufs["g_recon"]])
        self.actor.vae_optimizer.step_with(own_target=(pol.vae_target_arena.flat, 1.0))
        # target (:161-173)
        with th.no_grad():
            x_next = fast.candidates(rd.next_observations, TRAIN_SAMPLES, self._pop_noise(), target=True)
            q_t = fast.critic_t.forward_input(x_next, train_params=False)
            hip_ops.bcq_target(q_t.stacked, B, TRAIN_SAMPLES, self.faithful_quirks, rd.rewards, rd.dones, self.gamma, bufs["target_q"])
        # critic step (:176-186)
        # both Q networks per layer in one pointer-table launch, as SAC / TD3 evaluate their critics (fused._TwinPairFn)
        qs = fused.twin_chain_forward(fast.critic, x_data) if fused.twin_chain_supported(fast.critic) else fast.critic.forward_input(x_data)
        c_out, c_sum = self._loss_slot("critic")
        blk.q_loss_step(qs, bufs["target_q"], 1.0, c_out, c_sum)
        self.critic.optimizer.step()
        actor_done = False
        if n_updates % self.actor_delay == 0:  # :189-207
            x_pi = fast.candidates(rd.observations, 1, self._pop_noise(), target=False, with_grad=True)
            a_out, a_sum = self._loss_slot("actor")
            blk.neg_mean_pass(x_pi, a_out, a_sum)
            # the perturbation net's step, its own soft target update and the critics' in ONE launch; the target VAE already equals
            # the VAE (the reference's polyak + copy of it, :201-203, is the identity on it)
            self.actor.perturbation_optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, self.tau),
                                                        own_target=(pol.pert_target_arena.flat, self.tau))
            actor_done = True
        if self.debug_capture:
            self.last_train_tensors = blk.captured(qs, bufs["target_q"], c_out, a_out if actor_done else None, vae_loss=v_out.clone(),
                                                   recon=recon.detach().clone(), next_q_min=th.min(q_t.stacked, dim=0)[0])

    # ---- reference odds and ends -------------------------------------------------------------------------------------
    def _behavior_cloning_update(self, observations, actions) -> float:
        pass  # reference :240-241

    def _behavior_cloning_warmup(self, callback) -> None:
        pass  # reference :243-244: accepted, without effect

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "BCQ",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def _get_torch_save_params(self) -> tuple:
        """reference: bcq.py:236-238"""
        return ["policy", "actor.vae_optimizer", "actor.perturbation_optimizer", "critic.optimizer"], []

    def _extra_save_data(self) -> dict:
        d = dict(actor_delay=self.actor_delay, faithful_quirks=self.faithful_quirks, behavior_cloning_warmup=self.behavior_cloning_warmup,
                 n_eval_episodes=self.n_eval_episodes)
        if isinstance(self.dataset, str):
            d["dataset"] = self.dataset  # load() without dataset= reads it again (what the reference's load -> _setup_model does)
        return d

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        ctor.pop("train_freq", None)  # the base class's (1, "step") placeholder is not a constructor argument here
        return super()._construct_for_load(env, device, ctor)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "buffer_size", "batch_size", "tau", "gamma", "gradient_steps", "seed", "policy_kwargs", "actor_delay",
                "faithful_quirks", "behavior_cloning_warmup", "n_eval_episodes", "dataset")
