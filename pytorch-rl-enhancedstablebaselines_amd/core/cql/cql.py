"""CQL (Kumar et al. 2020, "Conservative Q-Learning for Offline Reinforcement Learning"): SAC's gradient step (core/sac/sac.py) on
batches of a fixed dataset, with the importance-sampled CQL(H) term of the published SAC-based implementation added to the critic loss.
Per gradient step, with N = cql_n_actions, A = act_dim, T = cql_temp, w = conservative_weight:

    a_pi, logp      = actor(s)   (SAC's statement, with gradient: the actor loss uses it)
    ent_coef step                (SAC's, unchanged)
    with no gradient:
      params_s, params_s' = actor trunk + head on s and on s'          (mean | raw log_std, ONCE per state)
      for k < N:  a_rand[b,k] ~ U(-1,1)^A
                  a_cur[b,k]  ~ pi(.|s_b),  lp_cur[b,k] = log pi(a_cur[b,k] | s_b)     (squashed Gaussian, SAC's formula)
                  a_nxt[b,k]  ~ pi(.|s'_b), lp_nxt[b,k] = log pi(a_nxt[b,k] | s'_b)
      a', logp'     = SAC's next action / log-prob (the sample the TD target uses, as in SAC)
      y = r + (1-d) * gamma * (min_i Qt_i(s',a') - [backup_entropy] * ent_coef * logp')
    for each critic i:
      c_i[b, :] = [ Q_i(s_b, a_rand[b,k]) - A*log(0.5) ... | Q_i(s_b, a_cur[b,k]) - lp_cur[b,k] ... | Q_i(s_b, a_nxt[b,k]) - lp_nxt[b,k] ... ]
      lse_i[b]  = T * logsumexp_j( c_i[b,j] / T )
    critic_loss = 0.5 * sum_i [ mean_b (Q_i(s_b,a_b) - y_b)^2  +  w * ( mean_b lse_i[b] - mean_b Q_i(s_b,a_b) ) ]
    actor_loss  = SAC's: mean(ent_coef * logp - min_i Q_i(s, a_pi))     (critics frozen, after the critic's Adam step)
    soft update = SAC's

All 3N candidate actions are evaluated at the CURRENT state s_b, the pi(.|s') ones included, as in the published code. Candidates and
their log-probs are constants of the critic step: no gradient reaches the actor from it. The uniform density term is A*log(0.5) for the
action box (-1, 1), which is the buffer's action scaling. The whole critic loss is 0.5 x the published one: `w` keeps its published
meaning relative to the Bellman term while the Bellman term keeps SAC's 0.5 * sum mse scale. `cql_importance_sample=False` drops the
three corrections and appends Q_i(s_b, a_b) as a (3N+1)-th entry (the published variant).

Defaults: conservative_weight 5.0, cql_n_actions 10, cql_temp 1.0 and cql_importance_sample True are the published implementation's
(min_q_weight, num_random, temp; its MuJoCo runs use weights 5 and 10); backup_entropy False is its `deterministic_backup=True`.
Not built: the Lagrange form of w, max_q_backup, the behaviour-cloning warm start of the actor, observation normalisation.

It sits on `OfflineAlgorithm` (the dataset forms, learn(), the hipGraph hooks) and takes SAC's policy class, actor head and
entropy-coefficient step. On the fused path (two critics, 3N + 1 <= 64, FlatAdam, a packed batch) the candidate actions are ONE launch
(cstr_cql_candidates_f32) from the head outputs of SAC's 2B-row actor pass -- the trunk runs once per state, not on 2 N B repeated
rows; they land in rows B.. of one wide critic input whose first B rows are the sampled (obs | act) rows themselves; the twin critic
runs ONE forward and ONE backward on the (1 + 3N) B rows, with everything between them (TD target, Bellman term, log-sum-exp, its
softmax gradient, the logged scalars) in ONE launch (cstr_cql_q_loss_f32). Otherwise the step is `_gradient_step_aten`: the same
statement in plain torch on the nn.Modules, the candidates sampled from the distribution parameters once per state. The row-chain
kernels (core/common/chain.py) have SAC's critic loss built in and decline this class."""
import math
from typing import List, Optional, Tuple, Union

import numpy as np
import torch as th
from torch.nn import functional as F

from core.common import hip_ops
from core.common.logger import DeviceMean
from core.common.offline_policy_algorithm import OfflineAlgorithm
from core.common.vec_env import unwrap_vec_normalize
from core.cql.policies import MlpPolicy
from core.sac.sac import SAC

AUX_KEYS = ("bellman", "cql", "lse", "q_data")  # cstr_cql_q_loss_f32's aux row


class CQL(SAC, OfflineAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    goal_face_support = False
    train_batch_size = 256
    chain_type = None

    def __init__(self, policy, env, learning_rate=3e-4, dataset=None, buffer_size: int = 1_000_000, batch_size: int = 256,
                 tau: float = 0.005, gamma: float = 0.99, gradient_steps: int = 1, ent_coef: Union[str, float] = "auto",
                 target_update_interval: int = 1, target_entropy: Union[str, float] = "auto", conservative_weight: float = 5.0,
                 cql_n_actions: int = 10, cql_temp: float = 1.0, cql_importance_sample: bool = True, backup_entropy: bool = False,
                 behavior_cloning_warmup: int = 0, n_eval_episodes: int = 10, policy_kwargs: Optional[dict] = None,
                 stats_window_size: int = 100, tensorboard_log: Optional[str] = None, verbose: int = 0,
                 device: Union[th.device, str] = "auto", seed: Optional[int] = None, _init_setup_model: bool = True):
        if policy_kwargs and policy_kwargs.get("use_sde"):
            raise ValueError("CQL does not support gSDE (use_sde=True)")
        if env is not None and unwrap_vec_normalize(env) is not None:
            raise ValueError("CQL does not take a VecNormalize-wrapped env: observation normalisation is not built")
        if not (conservative_weight >= 0.0):
            raise ValueError(f"CQL: conservative_weight must be a non-negative number, got {conservative_weight}")
        if not (cql_temp > 0.0):
            raise ValueError(f"CQL: cql_temp must be a positive number, got {cql_temp}")
        if int(cql_n_actions) != cql_n_actions or cql_n_actions < 1:
            raise ValueError(f"CQL: cql_n_actions must be a positive integer, got {cql_n_actions}")
        OfflineAlgorithm.__init__(self, policy=policy, env=env, dataset=dataset, learning_rate=learning_rate, buffer_size=buffer_size,
                                  batch_size=batch_size, tau=tau, gamma=gamma, gradient_steps=gradient_steps, dataset_buffer_class=None,
                                  dataset_buffer_kwargs=None, n_eval_episodes=n_eval_episodes,
                                  behavior_cloning_warmup=behavior_cloning_warmup, conservative_weight=float(conservative_weight),
                                  policy_kwargs=policy_kwargs, stats_window_size=stats_window_size, tensorboard_log=tensorboard_log,
                                  verbose=verbose, device=device, seed=seed)
        if self.world_size > 1:
            raise NotImplementedError("data-parallel CQL is not built")
        # SAC.__init__ is not run (its base-class call has the online signature): what it sets behind that call is set here and must
        # follow it
        self.target_entropy = target_entropy
        self.log_ent_coef: Optional[th.Tensor] = None
        self.ent_coef = ent_coef
        self.target_update_interval = target_update_interval
        self.ent_coef_optimizer = None
        self.debug_capture = False
        self.last_train_tensors: dict = {}
        self.cql_n_actions = int(cql_n_actions)
        self.cql_temp = float(cql_temp)
        self.cql_importance_sample = bool(cql_importance_sample)
        self.backup_entropy = bool(backup_entropy)
        # teacher-forcing hook: (u [B, N, A] uniforms in [-1, 1), eps [B, 2N, A] standard normals: rows [0, N) for pi(.|s), [N, 2N) for pi(.|s'))
        self.cql_noise_queue: List[Tuple[th.Tensor, th.Tensor]] = []
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        super()._setup_model()
        act_dim = int(np.prod(self.action_space.shape))
        # the kernel path: SAC's, with two critics and a candidate count / action width the two launches take; otherwise the torch statements
        self.fused_learner = bool(self.fused_learner and len(self.critic.q_networks) == 2 and hip_ops.cql_supported(self.cql_n_actions, act_dim))
        # [actor | critic | ent_coef_loss | ent_coef | bellman | cql | lse | q_data]: the loss launch's aux row is the last four
        self._loss_sum_buf = th.zeros(8, dtype=th.float32, device=self.device)
        b = self._loss_sum_buf
        self._loss_sums = dict(actor=b[0:1], critic=b[1:2], ent_coef_loss=b[2:3], ent_coef=b[3:4],
                               **{k: b[4 + i:5 + i] for i, k in enumerate(AUX_KEYS)})
        self._aux_now = th.zeros(4, dtype=th.float32, device=self.device)

    def _chain_for(self, batch_size: int):
        return None  # the row-chain critic step has SAC's loss built in

    def _graph_eligible(self, callback) -> bool:
        return (super()._graph_eligible(callback) and self._use_packed_batch() and not self.cql_noise_queue
                and not self.actor.action_dist.eps_queue)

    # ---- the wide critic input: [B sampled (obs | act) rows | B * 3N candidate rows], the sampler writes the first B itself ----------
    def _alloc_packed_step_tensors(self, batch_size: int) -> None:
        super()._alloc_packed_step_tensors(batch_size)
        pb, n3 = self._packed, 3 * self.cql_n_actions
        d, a = pb.obs_dim, pb.act_dim
        e = lambda *s: th.zeros(*s, dtype=th.float32, device=self.device)  # noqa: E731
        self._x_wide = e((1 + n3) * batch_size, d + a)
        pb.x_data = self._x_wide[:batch_size]  # the packed batch's (obs | act) rows ARE the head of the wide input: no row copy
        pb.samples = pb.samples._replace(observations=pb.x_data[:, :d], actions=pb.x_data[:, d:])
        self._static_batch = pb.samples
        self._cql_corr = e(batch_size, n3)
        self._cql_params = e(2 * batch_size, 2 * a)  # the 2B-row actor pass's head outputs: s rows, then s' rows

    def _draw_cql_noise(self, batch: int, act_dim: int):
        """(u, eps) of the torch-statement path: the queued pair, or torch's generator"""
        n = self.cql_n_actions
        if self.cql_noise_queue:
            u, eps = self.cql_noise_queue.pop(0)
            return (u.to(self.device, th.float32).reshape(batch, n, act_dim).contiguous(),
                    eps.to(self.device, th.float32).reshape(batch, 2 * n, act_dim).contiguous())
        return (th.rand(batch, n, act_dim, device=self.device) * 2.0 - 1.0, th.randn(batch, 2 * n, act_dim, device=self.device))

    # ---- gradient steps ----------------------------------------------------------------------------------------------------------
    def _gradient_step(self, batch_size: int, gradient_step: int) -> None:
        if self.fused_learner and self._use_packed_batch():
            return self._gradient_step_fused(batch_size, gradient_step)
        return self._gradient_step_aten(batch_size, gradient_step)

    def _train_device_only(self, gradient_steps: int, batch_size: int) -> None:
        # SAC's, with the kernel path's own condition: a step the torch statements take accumulates, so its sums need the fill
        self._single_step = (gradient_steps == 1 and self.fused_learner and self._use_packed_batch() and self.ent_coef_optimizer is not None)
        if not self._single_step:
            self._loss_sum_buf.zero_()
        for gradient_step in range(gradient_steps):
            self._gradient_step(batch_size, gradient_step)

    def _gradient_step_fused(self, batch_size: int, gradient_step: int) -> None:
        s, pol, fa, blk = self._loss_sums, self.policy, self._fast_actor, self._critic_block
        (c_out, c_sum), (a_out, a_sum) = self._loss_slot("critic"), self._loss_slot("actor")
        pb, _, rd = self._sample(batch_size)
        n, b = self.cql_n_actions, batch_size
        # the 2B-row actor pass of SAC's packed-batch step; its head outputs [mean | raw log_std] of s and s' are handed out
        # (`params_out`), so the candidates need no second trunk pass. Without the pair pass (rocBLAS Linears, a single queued draw)
        # the two passes are SAC's and the parameters come from a second, gradient-free trunk pass over the 2B rows (its outputs are
        # fresh tensors of the caching allocator every step: only the pair path keeps every buffer of the step).
        params = self._cql_params
        if fa.pair_supported(pb):
            x_pi, log_prob, x_next, next_log_prob = fa.action_log_prob_pair(pb, params_out=params)
        else:
            x_pi, log_prob = fa.action_log_prob(rd.observations, xbuf=pb.x_pi.detach())
            with th.no_grad():
                x_next, next_log_prob = fa.action_log_prob(rd.next_observations, train_params=False, xbuf=pb.x_next)
                params = fa.dist_params(pb.x_pn[:, :pb.obs_dim], train_params=False)
        corr = self._cql_corr if self.cql_importance_sample else None
        x_cand = self._x_wide[b:]
        if self.cql_noise_queue:
            u, eps = self._draw_cql_noise(b, pb.act_dim)
            hip_ops.cql_candidates(rd.observations, params[:b], params[b:], n, x_cand, corr, u=u, eps=eps)
        else:
            # the algorithm's own Philox control words (`set_random_seed` reseeds them), CQL's stream tag in the counter
            hip_ops.cql_candidates(rd.observations, params[:b], params[b:], n, x_cand, corr, rng_ctl=self._device_rng())

        ent_opt = self.ent_coef_optimizer
        if ent_opt is not None:  # SAC's entropy-coefficient loss (ent_coef = exp(log_ent_coef) BEFORE the update), a launch of its own
            (ent_coef, ent_coef_sum), (e_out, e_sum) = self._loss_slot("ent_coef"), self._loss_slot("ent_coef_loss")
            hip_ops.sac_alpha(self.log_ent_coef.detach(), log_prob.detach(), self.target_entropy, self._ent_arena.grad[0:1], ent_coef,
                              loss_sum=e_sum, ent_coef_sum=ent_coef_sum, loss_out=e_out)
        else:
            ent_coef = self.ent_coef_tensor.reshape(1)
            s["ent_coef"] += ent_coef
        aux = self._loss_sum_buf[4:8] if self._single_step else self._aux_now
        q_all = blk.cql_step(self._x_wide, corr, not self.cql_importance_sample, x_next, rd, self.gamma, self.conservative_weight, self.cql_temp,
                             self._target_q, c_out, c_sum, aux, next_logp=next_log_prob if self.backup_entropy else None, ent_coef=ent_coef,
                             after_loss=self._ent_coef_step if ent_opt is not None and not self._ent_rides_critic else None)
        if not self._single_step:
            self._loss_sum_buf[4:8] += self._aux_now
        if ent_opt is not None and self._ent_rides_critic:
            self.critic.optimizer.step_with(ent_opt)
        else:
            self.critic.optimizer.step()

        blk.sac_actor_pass(x_pi, log_prob, ent_coef, a_out, a_sum)
        if gradient_step % self.target_update_interval == 0:
            self.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, self.tau))
        else:
            self.actor.optimizer.step()

        if self.debug_capture:
            self.last_train_tensors = blk.captured([q_all[0, :b], q_all[1, :b]], self._target_q, c_out, a_out, ent_coef=ent_coef.detach().clone(),
                                                   log_prob=log_prob.detach().clone(), x_cand=x_cand.clone(),
                                                   corr=None if corr is None else corr.clone(), q_all=q_all.clone(), aux=aux.clone())

    def _candidates_torch(self, obs, next_obs, u, eps):
        """(actions [B, 3N, A], corrections [B, 3N]) from the distribution parameters of s and s', ONCE per state (no repeated rows)"""
        n = self.cql_n_actions
        a_dim = u.shape[2]
        acts, corr = [u], [th.full(u.shape[:2], a_dim * math.log(0.5), dtype=u.dtype, device=u.device)]
        for o, e in ((obs, eps[:, :n]), (next_obs, eps[:, n:])):
            mean, log_std, _ = self.actor.get_action_dist_params(o)
            mu, sd = mean.unsqueeze(1), log_std.exp().unsqueeze(1)
            g = mu + sd * e
            a = th.tanh(g)
            lp = (-((g - mu) ** 2) / (2 * sd ** 2) - sd.log() - math.log(math.sqrt(2 * math.pi))).sum(dim=2)
            acts.append(a)
            corr.append(lp - th.log(1 - a ** 2 + 1e-6).sum(dim=2))
        return th.cat(acts, dim=1), th.cat(corr, dim=1)

    def _gradient_step_aten(self, batch_size: int, gradient_step: int) -> None:
        """The statement of the module docstring in plain torch on the nn.Modules (autograd losses): what configurations the kernel
        path does not cover run, and the A/B reference in tests."""
        s = self._loss_sums
        rd = self.replay_buffer.sample_into(self._batch(batch_size))
        n, w, T = self.cql_n_actions, self.conservative_weight, self.cql_temp
        b, a_dim = rd.actions.shape

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
            u, eps = self._draw_cql_noise(b, a_dim)
            cand, corr = self._candidates_torch(rd.observations, rd.next_observations, u, eps)
            next_q, _ = th.min(th.cat(self.critic_target(rd.next_observations, next_actions), dim=1), dim=1, keepdim=True)
            if self.backup_entropy:
                next_q = next_q - ent_coef * next_log_prob.reshape(-1, 1)
            target_q = rd.rewards + (1 - rd.dones) * self.gamma * next_q
            x_cand = th.cat([rd.observations.unsqueeze(1).expand(b, 3 * n, -1), cand], dim=2).reshape(b * 3 * n, -1)
            d = rd.observations.shape[1]

        q_data = self.critic(rd.observations, rd.actions)
        q_cand = self.critic(x_cand[:, :d], x_cand[:, d:])
        bellman = 0.5 * sum(F.mse_loss(q, target_q) for q in q_data)
        lse = []
        for qd, qc in zip(q_data, q_cand):
            c = qc.reshape(b, 3 * n)
            c = c - corr if self.cql_importance_sample else th.cat([c, qd], dim=1)
            lse.append(T * th.logsumexp(c / T, dim=1))
        cons = 0.5 * w * sum(l.mean() - qd.mean() for l, qd in zip(lse, q_data))
        critic_loss = bellman + cons
        s["critic"] += critic_loss.detach()
        aux = th.stack([bellman.detach(), cons.detach(), sum(l.mean() for l in lse).detach() / len(lse),
                        sum(q.mean() for q in q_data).detach() / len(q_data)])
        self._loss_sum_buf[4:8] += aux
        self.critic.optimizer.zero_grad()
        critic_loss.backward()
        self.critic.optimizer.step()

        q_values_pi = th.cat(self.critic(rd.observations, actions_pi), dim=1)
        min_qf_pi, _ = th.min(q_values_pi, dim=1, keepdim=True)
        actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
        s["actor"] += actor_loss.detach()
        self.actor.optimizer.zero_grad()
        actor_loss.backward()
        self.actor.optimizer.step()
        if gradient_step % self.target_update_interval == 0:
            self.policy.critic_target_arena.polyak_from(self.policy.critic_arena, self.tau)

        if self.debug_capture:
            self.last_train_tensors = dict(target_q=target_q.clone(), current_q=[q.detach().clone() for q in q_data],
                                           critic_loss=critic_loss.detach().clone(), actor_loss=actor_loss.detach().clone(),
                                           ent_coef=ent_coef.detach().clone(), log_prob=log_prob.detach().clone(), x_cand=x_cand.clone(),
                                           corr=corr.clone() if self.cql_importance_sample else None,
                                           q_all=th.stack([th.cat([qd, qc]).detach() for qd, qc in zip(q_data, q_cand)]), aux=aux.clone())

    def _train_host_only(self, gradient_steps: int) -> None:
        super()._train_host_only(gradient_steps)
        s = self._loss_sums  # read lazily, like the losses: no host synchronisation in the step
        self.logger.record("train/cql_loss", DeviceMean(s["cql"], gradient_steps))
        self.logger.record("train/bellman_loss", DeviceMean(s["bellman"], gradient_steps))
        self.logger.record("train/cql_lse", DeviceMean(s["lse"], gradient_steps))
        self.logger.record("train/q_data", DeviceMean(s["q_data"], gradient_steps))

    # ---- reference odds and ends -----------------------------------------------------------------------------------------------
    def _behavior_cloning_update(self, observations, actions) -> float:
        pass  # accepted, without effect (as BCQ)

    def _behavior_cloning_warmup(self, callback) -> None:
        pass

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "CQL",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return OfflineAlgorithm.learn(self, total_timesteps=total_timesteps, callback=callback, log_interval=log_interval,
                                      tb_log_name=tb_log_name, reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        d = dict(super()._extra_save_data(), conservative_weight=self.conservative_weight, cql_n_actions=self.cql_n_actions,
                 cql_temp=self.cql_temp, cql_importance_sample=self.cql_importance_sample, backup_entropy=self.backup_entropy,
                 behavior_cloning_warmup=self.behavior_cloning_warmup, n_eval_episodes=self.n_eval_episodes)
        if isinstance(self.dataset, str):
            d["dataset"] = self.dataset  # load() without dataset= reads it again
        return d

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "buffer_size", "batch_size", "tau", "gamma", "gradient_steps", "seed", "policy_kwargs", "ent_coef",
                "target_update_interval", "target_entropy", "conservative_weight", "cql_n_actions", "cql_temp", "cql_importance_sample",
                "backup_entropy", "behavior_cloning_warmup", "n_eval_episodes", "dataset")

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        ctor.pop("train_freq", None)  # the base class's (1, "step") placeholder is not a constructor argument here
        return super()._construct_for_load(env, device, ctor)
