"""SAC.train's gradient step on the row-chain kernels (csrc/cstr_chain.hip): 8 launches instead of 20 (10 under data-parallel).

    reference statement (core/sac/sac.py)                              launch
    :215 sample (gather) + :222 pi(obs) + :247 pi(next_obs)             cstr_sac_actor_chain_fwd_f32      (head left as partial sums)
    :250 target critics + :258 critics (actor head finalised inside)    cstr_q_chain_fwd_f32, 4 networks  (Q heads left as partial sums)
    :230-261 entropy-coefficient loss, TD target, critic loss, critic
             backward to dz                                             cstr_q_chain_bwd_f32, mode 1
    :266-267 critic dW / db (6 layers) + :240-243, :268 entropy-
             coefficient and critic Adam steps                          cstr_linear_bwd_weight_adam_sets_f32
    :273 critics on (obs, pi(obs))                                      cstr_q_chain_fwd_f32, 2 networks
    :275 actor loss + backward through the frozen critics to the action cstr_q_chain_bwd_f32, mode 2      (action gradient as partial sums)
    :279-280 backward of the squashed-Gaussian head and the actor       cstr_sac_actor_chain_bwd_f32
    :280 actor dW / db (3 layers) + :281 actor Adam step + :284-287
             soft update of the target critics                          cstr_linear_bwd_weight_adam_sets_f32

That is the step on one GPU; with the rollout launch in front of it an iteration is 9 launches. Data-parallel training puts a collective
between a gradient and its optimiser step, so each cstr_linear_bwd_weight_adam_sets_f32 launch becomes

    cstr_linear_bwd_weight_sets_f32 -> all-reduce of the arena's gradient -> cstr_adam_multi_f32

(10 launches; the soft update rides the actor's Adam launch, the entropy coefficient the critic's, or it all-reduces and steps in a
launch of its own in front of it). Batches of 32 rows and fewer and CSTR_WGRAD_ADAM=0 take the same form without the collectives.
TD3's step and MADDPG's critic steps are built on the same twin-critic block (`TwinCriticBlock`); their launches are listed in their
class docstrings. Shapes the chain kernels do not cover (other activations, widths that are not multiples of 4 or above 512, batches
that are not multiples of 16, a VecNormalize normaliser, n_critics != 2) stay on the per-layer fused path (core/common/fused.py).
CSTR_CHAIN=0 turns this path off.
"""
import os

import torch as th
from torch import nn

from core import _native as nv
from core.common import fused, hip_ops

USE_CHAIN = os.environ.get("CSTR_CHAIN", "1") != "0"
# single GPU: the dW / db launch applies the Adam step to the tiles it has reduced (cstr_linear_bwd_weight_adam_sets_f32): 8 launches
USE_WGRAD_ADAM = os.environ.get("CSTR_WGRAD_ADAM", "1") != "0"
# 16-column MFMA tiles per workgroup: actor forward, Q forward (4 networks), Q forward (2 networks), Q backward, actor backward
TILES = tuple(int(v) for v in os.environ.get("CSTR_CHAIN_TILES", "2,2,2,2,1").split(","))


# TD3's class-default nets are [400, 300]; A/B on MI355X (bench --algo td3, exact-width kernels, profiles/r03_chain_tiles_sweep_td3.txt):
# 2,2,2,2,2 0.0705 ms, 2,2,2,2,1 0.0712, 2,4,2,2,1 0.0781, one column group everywhere 0.1037
TD3_TILES = tuple(int(v) for v in os.environ.get("CSTR_CHAIN_TILES_TD3", "2,2,2,2,2").split(","))


def _adam_in_wgrad(model, B: int) -> bool:
    """The dW / db launch applies the Adam step to the tiles it has reduced: only when no collective stands between a gradient and
    its optimiser step (`model._grads_need_allreduce`), and above the batch size where that launch wins."""
    return USE_WGRAD_ADAM and B > 32 and not model._grads_need_allreduce()


def _q_layers(qnet: nn.Sequential):
    lin = [m for m in qnet if isinstance(m, nn.Linear)]
    return tuple((m.weight, m.bias) for m in lin)


def _is_q_mlp(qnet) -> bool:
    """Linear-ReLU-Linear-ReLU-Linear(., 1): the only Q network the chain kernels evaluate."""
    mods = list(qnet)
    if len(mods) != 5 or not all(isinstance(mods[i], nn.Linear) for i in (0, 2, 4)):
        return False
    return all(isinstance(mods[i], nn.ReLU) for i in (1, 3)) and mods[4].out_features == 1


def _q_dims_supported(qnet, d: int, a: int, batch_size: int) -> bool:
    """The (observation, action) layout and the widths of a Q network (`_is_q_mlp`) are ones the chain kernels cover at this batch size."""
    c1, c2 = qnet[0], qnet[2]
    return (d, a) in hip_ops.LAYOUTS and c1.in_features == d + a and hip_ops.chain_supported(c1.out_features, c2.out_features, batch_size)


def _pick_tiles(kdim: int, want: int, forward: bool = False) -> int:
    """The largest tile count <= `want` whose per-wave share of a K = kdim reduction fits in registers."""
    for t in (4, 2, 1):
        if t <= want and hip_ops.chain_tiles_ok(kdim, t, forward):
            return t
    return 1


class TwinCriticBlock:
    """A twin critic and its target on the row-chain kernels: the buffers and the launches of the critic step (four-network forward,
    TD root + backward to dz, the six dW / db sets) and of a policy pass through the first `n_pi` critics (forward on x_pi, loss root +
    backward to the action as partial sums). What differs between SAC, TD3 and MADDPG (roles, root arguments, what follows an unfused
    dW / db launch) is an argument or stays with the caller."""

    def __init__(self, q_networks, target_q_networks, D: int, A: int, B: int, tiles, dev, n_pi: int = 1, q_out=None):
        """tiles: wanted (4-network forward, policy-pass forward, backward) tile counts. q_out: where the TD root leaves Q1 / Q2 [2, B]
        (MADDPG hands in a row of the [n_agents, 2, B] tensor its train() reads)."""
        self.crit, self.targ = [_q_layers(q) for q in q_networks], [_q_layers(q) for q in target_q_networks]
        self.D, self.A, self.B, self.W, self.n_pi = D, A, B, D + A, n_pi
        H1, H2 = self.H1, self.H2 = q_networks[0][0].out_features, q_networks[0][2].out_features
        hip_ops.chain_check_nets(self.crit + self.targ, self.W, H1, H2)  # chain_net passes raw pointers: checked here, once
        t_q4, t_qpi, t_qb = tiles  # (a wave's share of the reduction must fit in registers: fewer tiles for wide layers)
        self.t_q4, self.t_qpi = _pick_tiles(H1, t_q4, True), _pick_tiles(H1, t_qpi, True)
        self.t_qb = _pick_tiles(H2, t_qb)
        self.n_q4, self.n_qpi = hip_ops.chain_colgroups(H2, self.t_q4), hip_ops.chain_colgroups(H2, self.t_qpi)
        self.n_gact = hip_ops.chain_colgroups(H1, self.t_qb)
        e = lambda *sh: th.empty(*sh, dtype=th.float32, device=dev)  # noqa: E731
        # per-network views (lists): every step reads them one network at a time, and indexing a tensor costs host time
        self.c_h1, self.c_h2 = list(e(2, B, H1)), list(e(2, B, H2))
        self.q_part4, self.q_part_pi = list(e(4, self.n_q4, B)), list(e(n_pi, self.n_qpi, B))
        self.q_out = e(2, B) if q_out is None else q_out
        self.gq, self.dz2, self.dz1 = e(2, B), e(2, B, H2), e(2, B, H1)
        self.qpi_out, self.gact_part = e(n_pi, B), e(n_pi, self.n_gact, B, A)
        self.b3s = [self.crit[0][2][1], self.crit[1][2][1], self.targ[0][2][1], self.targ[1][2][1]]

    PLAIN = (nv.CHAIN_ROLE_PLAIN, nv.CHAIN_ROLE_PLAIN)
    NEXT = (nv.CHAIN_ROLE_NEXT_STORE, nv.CHAIN_ROLE_NEXT)  # x_next's action columns are finalised from an actor head inside the launch

    def nets4(self, x_cur, x_next, roles=PLAIN, target_roles=NEXT):
        """The critics on x_cur (hidden layers kept for the backward) and the targets on x_next."""
        return [hip_ops.chain_net(self.crit[0], x_cur, self.c_h1[0], self.c_h2[0], self.q_part4[0], roles[0]),
                hip_ops.chain_net(self.crit[1], x_cur, self.c_h1[1], self.c_h2[1], self.q_part4[1], roles[1]),
                hip_ops.chain_net(self.targ[0], x_next, None, None, self.q_part4[2], target_roles[0]),
                hip_ops.chain_net(self.targ[1], x_next, None, None, self.q_part4[3], target_roles[1])]

    def pi_nets(self, x_pi, role: int = 0):
        return [hip_ops.chain_net(self.crit[g], x_pi, self.c_h1[g], self.c_h2[g], self.q_part_pi[g], role) for g in range(self.n_pi)]

    def back_nets(self, n: int = 2):
        return [hip_ops.chain_net(self.crit[g], None, self.c_h1[g], self.c_h2[g]) for g in range(n)]

    def forward(self, nets, tiles: int, fin=None) -> None:
        """One forward launch for `nets` (this block's `nets4` / `pi_nets`, or several same-shaped blocks' lists in a row)."""
        hip_ops.q_chain_fwd(nets, self.W, self.D, self.H1, self.H2, self.B, tiles, fin)

    def td_root(self, rd, gamma: float, scale: float, target_out, loss_out, loss_sum, **kw):
        """kw: next_logp, ent_coef, alpha, rng_advance, adam_advance of hip_ops.chain_root."""
        return hip_ops.chain_root("td", self.B, self.q_part4, self.b3s, self.n_q4, gamma=gamma, scale=scale, rew=rd.rewards, done=rd.dones,
                                  target_out=target_out, q_out=self.q_out, gq_out=self.gq, loss_out=loss_out, loss_sum=loss_sum, **kw)

    def pi_root(self, mode: str, **kw):
        """mode "sac_actor" (kw: ent_coef, logp) or "neg_mean"; kw: loss_out, loss_sum, adam_advance."""
        return hip_ops.chain_root(mode, self.B, self.q_part_pi, self.b3s[:self.n_pi], self.n_qpi, q_out=self.qpi_out, **kw)

    def td_backward(self, back, root) -> None:
        hip_ops.q_chain_bwd(back, root, self.W, self.D, self.H1, self.H2, self.t_qb, dz2=self.dz2, dz1=self.dz1)

    def pi_backward(self, back, root) -> None:
        hip_ops.q_chain_bwd(back, root, self.W, self.D, self.H1, self.H2, self.t_qb, gact_part=self.gact_part)

    def policy_pass(self, mode: str, x_pi, back, role: int = 0, fin=None, **root_kw) -> None:
        """The policy loss through the first `n_pi` (frozen) critics and its gradient w.r.t. the action, left in `gact_part`: 2 launches.
        back: `back_nets(n_pi)` (a step that ran `td_backward` passes the nets it built for it)."""
        self.forward(self.pi_nets(x_pi, role), self.t_qpi, fin)
        self.pi_backward(back, self.pi_root(mode, **root_kw))

    def sets(self, x_cur, fuse_opt: bool, opt_index: int = 0) -> list:
        """The six dW / db sets of the twin critic, for linear_bwd_weight_adam_sets (optimiser `opt_index` of its list) or
        linear_bwd_weight_sets."""
        B, sets = self.B, []
        for g in range(2):
            (w1, b1), (w2, b2), (w3, b3) = self.crit[g]
            if fuse_opt:
                sets += [(self.dz1[g], x_cur, w1, b1, opt_index, None), (self.dz2[g], self.c_h1[g], w2, b2, opt_index, None),
                         (self.gq[g].view(B, 1), self.c_h2[g], w3, b3, opt_index, None)]
            else:
                sets += [(self.dz1[g], x_cur, w1.grad, b1.grad), (self.dz2[g], self.c_h1[g], w2.grad, b2.grad),
                         (self.gq[g].view(B, 1), self.c_h2[g], w3.grad, b3.grad)]
        return sets

    @staticmethod
    def apply(blocks, x_cur, fuse_opt: bool, opts, flat=()) -> None:
        """The critic gradients of `blocks` in ONE launch. fuse_opt (`_adam_in_wgrad`): with the Adam steps of `opts` (one optimiser per
        block, step counters pre-advanced by the TD roots) and the `flat` segments inside. Otherwise gradients only: the caller
        all-reduces and steps behind it."""
        if fuse_opt:
            hip_ops.linear_bwd_weight_adam_sets([st for k, blk in enumerate(blocks) for st in blk.sets(x_cur, True, k)], opts, flat)
        else:
            hip_ops.linear_bwd_weight_sets([st for blk in blocks for st in blk.sets(x_cur, False)])

    def captured(self, target_q, critic_loss, actor_loss=None, **more) -> dict:
        """model.last_train_tensors of a debug_capture step."""
        B = self.B
        return dict(target_q=target_q.clone(), current_q=[self.q_out[0].clone().view(B, 1), self.q_out[1].clone().view(B, 1)],
                    critic_loss=critic_loss.clone(), actor_loss=None if actor_loss is None else actor_loss.clone(), **more)


class SacChain:
    """Buffers + launch sequence of one SAC gradient step on the chain kernels. Built once per (model, batch size)."""

    ROLES = (nv.CHAIN_ROLE_STORE_PI, nv.CHAIN_ROLE_PLAIN)  # the first critic's launch also finalises pi(obs): x_pi's action columns, params, logp_pi

    @staticmethod
    def supported(model, batch_size: int) -> bool:
        if not (USE_CHAIN and fused.USE_FUSED_LINEAR and model.fused_learner and model._use_packed_batch()):
            return False
        if getattr(model, "use_sde", False):  # gSDE actors run on the per-layer fused path
            return False
        if len(model.critic.q_networks) != 2:  # the chain root has twin slots: other n_critics run on the per-layer fused path
            return False
        fa = model._fast_actor
        layers = fa.latent.layers
        if len(layers) != 2 or any(act != fused.ACT_RELU for _, act in layers) or fa.head is None or not fa._hw.is_contiguous():
            return False
        if not all(_is_q_mlp(q) for q in list(model.critic.q_networks) + list(model.critic_target.q_networks)):
            return False
        (l1, _), (l2, _) = layers
        return (_q_dims_supported(model.critic.q_networks[0], l1.in_features, fa.act_dim, batch_size)
                and hip_ops.chain_supported(l1.out_features, l2.out_features, batch_size)
                and all(p.grad is not None for p in list(model.actor.parameters()) + list(model.critic.parameters())))

    def __init__(self, model, batch_size: int):
        fa, dev, B = model._fast_actor, model.device, batch_size
        (l1, _), (l2, _) = fa.latent.layers
        self.D, self.A, self.B = l1.in_features, fa.act_dim, B
        self.W = self.D + self.A
        self.aH1, self.aH2 = l1.out_features, l2.out_features
        t_act, t_q4, t_q2, t_qb, t_ab = TILES
        self.t_act, self.t_ab = _pick_tiles(self.aH1, t_act, True), _pick_tiles(self.aH2, t_ab)
        self.actor = hip_ops.sac_actor_desc(self.D, self.A, l1.weight, l1.bias, l2.weight, l2.bias, fa._hw, fa._hb)
        self.actor_layers = (l1, l2)
        self.block = TwinCriticBlock(model.critic.q_networks, model.critic_target.q_networks, self.D, self.A, B, (t_q4, t_q2, t_qb), dev, n_pi=2)
        e = lambda *sh: th.empty(*sh, dtype=th.float32, device=dev)  # noqa: E731
        A, H1, H2 = self.A, self.aH1, self.aH2
        self.n_head_parts = hip_ops.chain_colgroups(H2, self.t_act)
        self.a_h1, self.a_h2, self.head_part = e(B, H1), e(B, H2), e(self.n_head_parts, 2 * B, 2 * A)
        self.params, self.eps_all, self.logp_pi, self.logp_next = e(B, 2 * A), e(2 * B, A), e(B), e(B)
        self.g_params, self.dz2a, self.dz1a = e(B, 2 * A), e(B, H2), e(B, H1)
        # the merged (mu | log_std) head as (values, gradient, exp_avg, exp_avg_sq) views for the fused dW + Adam launch
        self._head_params = None
        aopt = model.actor.optimizer
        off = getattr(getattr(aopt, "arena", None), "offset_of", {})
        mu, ls = fa.actor.mu, fa.actor.log_std
        if id(mu.weight) in off and id(mu.bias) in off and hasattr(aopt, "exp_avg"):
            ow, ob, nw, nb = off[id(mu.weight)], off[id(mu.bias)], 2 * A * H2, 2 * A
            if off.get(id(ls.weight)) == ow + A * H2 and off.get(id(ls.bias)) == ob + A:
                self._head_params = ((fa._hw, fa._hwg, aopt.exp_avg[ow:ow + nw], aopt.exp_avg_sq[ow:ow + nw]),
                                     (fa._hb, fa._hbg, aopt.exp_avg[ob:ob + nb], aopt.exp_avg_sq[ob:ob + nb]))

    def step(self, model, pb, gather, gradient_step: int) -> None:
        s, pol, blk, B, D, A = model._loss_sums, model.policy, self.block, self.B, self.D, self.A
        fa = model._fast_actor
        (c_out, c_sum), (a_out, a_sum) = model._loss_slot("critic"), model._loss_slot("actor")
        rd = pb.samples
        dist = fa.actor.action_dist
        eps2 = None
        if dist.eps_queue:  # teacher-forced draws (tests): the pi(obs) tensor was queued first
            eps2 = th.cat((dist.draw_eps((B, A), model.device), dist.draw_eps((B, A), model.device)), dim=0).contiguous()
        elif fa.rng_ctl is None:
            fa.rng_ctl = hip_ops.new_rng_ctl(th.initial_seed(), model.device)
        # -- pi(obs) and pi(next_obs): gather + layers 1, 2 + head partials
        # Philox offset bookkeeping: the rollout launch in front of this step leaves its advance (n_envs draws) to the launches behind it;
        # the actor launch only READS the offset (its noise lanes add what is pending), the Q backward launch's loss workgroup advances it
        pending_ctl, pending = (None, 0)
        if gather is not None and gather[2] is not None:
            pending_ctl, pending = gather[2]
        if pending_ctl is not None and eps2 is None and pending_ctl.data_ptr() != fa.rng_ctl.data_ptr():
            raise RuntimeError("the rollout launch and the sampling head must share one Philox stream")
        noise = {} if eps2 is not None else dict(head_rng_ctl=fa.rng_ctl, head_rng_offset=pending, eps_all=self.eps_all)
        eps = self.eps_all if eps2 is None else eps2
        rng_total = None
        if eps2 is None:
            rng_total = (fa.rng_ctl, pending + 2 * B)
        elif pending_ctl is not None:
            rng_total = (pending_ctl, pending)
        if gather is not None:
            ring, idx, _, _ = gather
            hip_ops.sac_actor_chain_fwd(self.actor, B, pb.x_data, pb.x_pi, pb.x_next, rd.dones, rd.rewards, self.a_h1, self.a_h2, self.head_part,
                                        self.t_act, ring=ring, sample_idx=idx, advance_ring=True, **noise)
        else:
            hip_ops.sac_actor_chain_fwd(self.actor, B, None, pb.x_pi, pb.x_next, None, None, self.a_h1, self.a_h2, self.head_part, self.t_act, **noise)
        # -- critics on x_data, target critics on x_next (its action columns finalised inside the launch)
        fin = nv.SacHeadFin(self.head_part.data_ptr(), fa._hb.data_ptr(), eps.data_ptr(), self.n_head_parts, A, D, nv.CHAIN_HEAD_GAUSSIAN, 2 * B, B, 0.0, 0.0,
                            pb.x_pi.data_ptr(), pb.x_next.data_ptr(), self.params.data_ptr(), self.logp_pi.data_ptr(), self.logp_next.data_ptr())
        self._keep = eps2  # alive until the launches that read it have been issued (and recorded)
        blk.forward(blk.nets4(pb.x_data, pb.x_next, roles=self.ROLES), blk.t_q4, fin)
        # -- entropy-coefficient loss, TD target, critic loss and the critic backward down to dz1
        if model.ent_coef_optimizer is not None:
            (ent_coef, ent_coef_sum), (e_out, e_sum) = model._loss_slot("ent_coef"), model._loss_slot("ent_coef_loss")
            alpha = dict(log_alpha=model.log_ent_coef.detach(), logp_pi=self.logp_pi, target_entropy=model.target_entropy,
                         grad_out=model._ent_arena.grad[0:1], ent_coef_out=ent_coef, loss_out=e_out, loss_sum=e_sum, ent_coef_sum=ent_coef_sum)
        else:
            ent_coef, alpha = model.ent_coef_tensor.reshape(1), None
            s["ent_coef"] += ent_coef
        # one GPU: no collective between a gradient and its optimiser step -> the dW / db launch applies Adam to its tiles; the step
        # counters are advanced by the loss workgroup of the launch in front of it. The actor's launch also needs the merged head's
        # moment views: without them its optimiser steps (and advances its own counter) behind an unfused dW / db launch
        fuse_opt = _adam_in_wgrad(model, B)
        fuse_actor = fuse_opt and self._head_params is not None
        ent_opt = model.ent_coef_optimizer
        back = blk.back_nets()
        advance = ([model.critic.optimizer] + ([ent_opt] if ent_opt is not None else [])) if fuse_opt else ()
        blk.td_backward(back, blk.td_root(rd, model.gamma, 0.5, model._target_q, c_out, c_sum, next_logp=self.logp_next, ent_coef=ent_coef,
                                          alpha=alpha, rng_advance=rng_total, adam_advance=advance))
        blk.apply([blk], pb.x_data, fuse_opt, [model.critic.optimizer], [ent_opt._segment()] if fuse_opt and ent_opt is not None else [])
        if not fuse_opt:
            if ent_opt is not None and not model._ent_rides_critic:
                model._allreduce_grads(model._ent_arena)
                ent_opt.step()
            model._allreduce_grads(pol.critic_arena)
            if ent_opt is not None and model._ent_rides_critic:
                model.critic.optimizer.step_with(ent_opt)
            else:
                model.critic.optimizer.step()
        # -- actor loss through the (updated, frozen) critics
        blk.policy_pass("sac_actor", pb.x_pi, back, ent_coef=ent_coef, logp=self.logp_pi, loss_out=a_out, loss_sum=a_sum,
                        adam_advance=[model.actor.optimizer] if fuse_actor else ())
        hip_ops.sac_actor_chain_bwd(self.actor, blk.gact_part, 2, blk.n_gact, ent_coef, pb.x_pi, self.params, eps, self.a_h1, self.a_h2,
                                    self.g_params, self.dz2a, self.dz1a, B, self.t_ab)
        l1, l2 = self.actor_layers
        soft = gradient_step % model.target_update_interval == 0
        if fuse_actor:
            aopt = model.actor.optimizer
            sh = aopt.shadow
            hw_p, hb_p = self._head_params
            sets = [(self.dz1a, pb.x_pi[:, :D], l1.weight, l1.bias, 0, sh[0] if sh is not None and sh[4] is l1.weight else None),
                    (self.dz2a, self.a_h1, l2.weight, l2.bias, 0, sh[0] if sh is not None and sh[4] is l2.weight else None),
                    (self.g_params, self.a_h2, hw_p, hb_p, 0, None)]
            if not pol.critic_target_arena.same_layout(pol.critic_arena):
                raise ValueError("Iterables have different lengths")  # zip_strict's error (utils.py:447)
            flat = [("polyak", pol.critic_arena.flat, pol.critic_target_arena.flat, model.tau)] if soft else []
            hip_ops.linear_bwd_weight_adam_sets(sets, [aopt], flat)  # :279-281 and :284-287
        else:
            hip_ops.linear_bwd_weight_sets([(self.dz1a, pb.x_pi[:, :D], l1.weight.grad, l1.bias.grad), (self.dz2a, self.a_h1, l2.weight.grad, l2.bias.grad),
                                            (self.g_params, self.a_h2, fa._hwg, fa._hbg)])
            model._allreduce_grads(pol.actor_arena)
            if soft:  # :281 and :284-287 (disjoint arenas) in one launch
                model.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, model.tau))
            else:
                model.actor.optimizer.step()
        if model.debug_capture:
            model.last_train_tensors = blk.captured(model._target_q, c_out, a_out, ent_coef=ent_coef.detach().clone(), log_prob=self.logp_pi.clone())


class Td3Chain:
    """TD3.train's gradient step (core/td3/td3.py:154-211) on the chain kernels:

        critic step (every update)     target actor chain (next_obs rows, head as partial sums) -> Q chain, 4 networks (target actions +
                                       smoothing noise finalised inside) -> Q backward chain (TD target + critic loss inside) -> dW / db +
                                       Adam: 4 launches
        policy step (every 2nd update) actor chain (obs rows) -> Q chain, first critic on (obs, pi(obs)) -> Q backward chain (-mean(Q1))
                                       to the action -> actor backward chain -> dW / db + Adam + the soft updates of both targets: 5 launches
    Twin critics and deterministic 3-Linear actors only (DDPG's single critic stays on the per-layer path)."""

    @staticmethod
    def supported(model, batch_size: int) -> bool:
        if not (USE_CHAIN and fused.USE_FUSED_LINEAR and model.fused_learner and model._use_packed_batch()):
            return False
        if len(model.critic.q_networks) != 2:
            return False
        if not all(_is_q_mlp(q) for q in list(model.critic.q_networks) + list(model.critic_target.q_networks)):
            return False
        for actor in (model.actor, model.actor_target):
            mods = list(actor.mu)
            if (len(mods) != 6 or not all(isinstance(mods[i], nn.Linear) for i in (0, 2, 4)) or not all(isinstance(mods[i], nn.ReLU) for i in (1, 3))
                    or not isinstance(mods[5], nn.Tanh)):
                return False
        a1, a2, a3 = (model.actor.mu[i] for i in (0, 2, 4))
        return (_q_dims_supported(model.critic.q_networks[0], a1.in_features, a3.out_features, batch_size)
                and hip_ops.chain_supported(a1.out_features, a2.out_features, batch_size)
                and all(p.grad is not None for p in list(model.actor.parameters()) + list(model.critic.parameters())))

    def __init__(self, model, batch_size: int):
        dev, B = model.device, batch_size
        a1, a2, a3 = (model.actor.mu[i] for i in (0, 2, 4))
        t1, t2, t3 = (model.actor_target.mu[i] for i in (0, 2, 4))
        self.D, self.A, self.B = a1.in_features, a3.out_features, B
        self.W = self.D + self.A
        self.aH1, self.aH2 = a1.out_features, a2.out_features
        t_act, t_q4, t_q2, t_qb, t_ab = TD3_TILES
        self.t_act, self.t_ab = _pick_tiles(self.aH1, t_act, True), _pick_tiles(self.aH2, t_ab)
        self.actor = hip_ops.sac_actor_desc(self.D, self.A, a1.weight, a1.bias, a2.weight, a2.bias, a3.weight, a3.bias)
        self.tactor = hip_ops.sac_actor_desc(self.D, self.A, t1.weight, t1.bias, t2.weight, t2.bias, t3.weight, t3.bias)
        self.actor_layers, self.tactor_layers = (a1, a2, a3), (t1, t2, t3)
        self.block = TwinCriticBlock(model.critic.q_networks, model.critic_target.q_networks, self.D, self.A, B, (t_q4, t_q2, t_qb), dev)
        e = lambda *sh: th.empty(*sh, dtype=th.float32, device=dev)  # noqa: E731
        A, H1, H2 = self.A, self.aH1, self.aH2
        self.n_head = hip_ops.chain_colgroups(H2, self.t_act)
        self.head_part = e(self.n_head, B, A)
        self.eps = e(B, A)
        self.a_h1, self.a_h2 = e(B, H1), e(B, H2)
        self.g_params, self.dz2a, self.dz1a = e(B, A), e(B, H2), e(B, H1)

    def step(self, model, pb, gather, n_updates: int) -> None:
        pol, blk, B, D, A = model.policy, self.block, self.B, self.D, self.A
        rd = pb.samples
        c_out, c_sum = model._loss_slot("critic")
        queued = model.noise_queue.pop(0).to(model.device, th.float32).contiguous() if model.noise_queue else None  # teacher-forced, scaled
        rng = None if queued is not None else model._device_rng()
        noise = {} if queued is not None else dict(head_rng_ctl=rng, eps_all=self.eps)
        eps = self.eps if queued is None else queued
        sigma = model.target_policy_noise if queued is None else 1.0
        fuse_opt = _adam_in_wgrad(model, B)
        # -- critic step: target actor on next_obs (:171), four Q networks (:173, :179), TD target + loss + backward (:174-186)
        kw = dict(rows_mode=nv.CHAIN_ROWS_NEXT, head_n=A, **noise)
        if gather is not None:
            ring, idx, pending, _ = gather
            if pending is not None:
                raise RuntimeError("a deterministic actor's rollout launch draws nothing: no Philox advance can be pending")
            hip_ops.sac_actor_chain_fwd(self.tactor, B, pb.x_data, pb.x_pi, pb.x_next, rd.dones, rd.rewards, None, None, self.head_part, self.t_act,
                                        ring=ring, sample_idx=idx, advance_ring=True, **kw)
        else:
            hip_ops.sac_actor_chain_fwd(self.tactor, B, None, None, pb.x_next, None, None, None, None, self.head_part, self.t_act, **kw)
        t3 = self.tactor_layers[2]
        fin = nv.SacHeadFin(self.head_part.data_ptr(), t3.bias.data_ptr(), eps.data_ptr(), self.n_head, A, D, nv.CHAIN_HEAD_DETERMINISTIC, B, 0,
                            float(sigma), float(model.target_noise_clip), pb.x_pi.data_ptr(), pb.x_next.data_ptr(), None, None, None)
        self._keep = queued
        blk.forward(blk.nets4(pb.x_data, pb.x_next), blk.t_q4, fin)
        back = blk.back_nets()
        blk.td_backward(back, blk.td_root(rd, model.gamma, 1.0, model._target_q, c_out, c_sum, rng_advance=None if queued is not None else (rng, B),
                                          adam_advance=[model.critic.optimizer] if fuse_opt else ()))
        blk.apply([blk], pb.x_data, fuse_opt, [model.critic.optimizer])
        if not fuse_opt:
            model._allreduce_grads(pol.critic_arena)
            model.critic.optimizer.step()
        a_out = None
        if n_updates % model.policy_delay == 0:  # :192-206
            a_out, a_sum = model._loss_slot("actor")
            a1, a2, a3 = self.actor_layers
            hip_ops.sac_actor_chain_fwd(self.actor, B, None, pb.x_pi, None, None, None, self.a_h1, self.a_h2, self.head_part, self.t_act,
                                        rows_mode=nv.CHAIN_ROWS_OBS, head_n=A)
            fin2 = nv.SacHeadFin(self.head_part.data_ptr(), a3.bias.data_ptr(), None, self.n_head, A, D, nv.CHAIN_HEAD_DETERMINISTIC, B, 0, 0.0, 0.0,
                                 pb.x_pi.data_ptr(), None, None, None, None)
            blk.policy_pass("neg_mean", pb.x_pi, back[:1], role=nv.CHAIN_ROLE_PI, fin=fin2, loss_out=a_out, loss_sum=a_sum,
                            adam_advance=[model.actor.optimizer] if fuse_opt else ())
            hip_ops.sac_actor_chain_bwd(self.actor, blk.gact_part, 1, blk.n_gact, None, pb.x_pi, None, None, self.a_h1, self.a_h2, self.g_params,
                                        self.dz2a, self.dz1a, B, self.t_ab, kind=nv.CHAIN_HEAD_DETERMINISTIC)
            if not pol.actor_target_arena.same_layout(pol.actor_arena) or not pol.critic_target_arena.same_layout(pol.critic_arena):
                raise ValueError("Iterables have different lengths")  # zip_strict's error (utils.py:447)
            if fuse_opt:
                aopt, tau = model.actor.optimizer, model.tau
                sh = aopt.shadow
                shadow_of = lambda lin: sh[0] if sh is not None and sh[4] is lin.weight else None  # noqa: E731
                t1, t2, t3 = self.tactor_layers
                sets = [(self.dz1a, pb.x_pi[:, :D], a1.weight, a1.bias, 0, shadow_of(a1), (t1.weight.detach(), t1.bias.detach(), tau)),
                        (self.dz2a, self.a_h1, a2.weight, a2.bias, 0, shadow_of(a2), (t2.weight.detach(), t2.bias.detach(), tau)),
                        (self.g_params, self.a_h2, a3.weight, a3.bias, 0, shadow_of(a3), (t3.weight.detach(), t3.bias.detach(), tau))]
                hip_ops.linear_bwd_weight_adam_sets(sets, [aopt], [("polyak", pol.critic_arena.flat, pol.critic_target_arena.flat, tau)])  # :199-205
            else:
                hip_ops.linear_bwd_weight_sets([(self.dz1a, pb.x_pi[:, :D], a1.weight.grad, a1.bias.grad), (self.dz2a, self.a_h1, a2.weight.grad, a2.bias.grad),
                                                (self.g_params, self.a_h2, a3.weight.grad, a3.bias.grad)])
                model._allreduce_grads(pol.actor_arena)
                model.actor.optimizer.step_with(polyak=(pol.critic_arena, pol.critic_target_arena, model.tau),
                                                own_target=(pol.actor_target_arena.flat, model.tau))
        if model.debug_capture:
            model.last_train_tensors = blk.captured(model._target_q, c_out, a_out)


class MaddpgCriticChain:
    """The critic steps of MADDPG.train (core/maddpg/maddpg.py:146-164) on the chain kernels. Every agent's twin critic reads the SAME joint
    input (cat(all observations, all actions)) and its target the same next input, so
      * one agent's critic step = Q chain forward (critic + target, 4 networks) -> Q backward chain (TD target + loss inside) -> dW / db +
        Adam: 3 launches instead of 7;
      * a step WITHOUT a policy update = ONE forward launch for all agents' 4 x n_agents networks, a backward launch per agent and one
        dW / db + Adam launch per two agents.
    Centralised critics only (IDDPG's local critics read per-agent inputs and stay on the per-layer path)."""

    TARGET_ROLES = TwinCriticBlock.PLAIN  # x_next arrives complete: no actor head is finalised inside the launch

    @staticmethod
    def supported(model, batch_size: int) -> bool:
        C = model.critic
        if not (USE_CHAIN and fused.USE_FUSED_LINEAR and model.fused_learner and not C.local and C.n_critics == 2 and 4 * model.n_agents <= nv.CHAIN_MAX_NETS):
            return False
        from core.common.arena import FlatAdam

        if not all(isinstance(o, FlatAdam) for o in C.optimizer_list):
            return False
        if not all(_is_q_mlp(q) for nets in list(C.q_networks_list) + list(model.critic_target.q_networks_list) for q in nets):
            return False
        return (_q_dims_supported(C.q_networks_list[0][0], model.observation_space.shape[0], model.action_space.shape[0], batch_size)
                and all(p.grad is not None for p in C.parameters()))

    def __init__(self, model, batch_size: int):
        dev, B, n = model.device, batch_size, model.n_agents
        self.B, self.n = B, n
        self.D, self.A = model.observation_space.shape[0], model.action_space.shape[0]
        self.W = self.D + self.A
        t_act, t_q4, t_q2, t_qb, t_ab = TD3_TILES
        self.q_out = th.empty(n, 2, B, dtype=th.float32, device=dev)
        # one block per agent; its policy pass is through agent i's FIRST critic (:174-177)
        self.blocks = [TwinCriticBlock(model.critic.q_networks_list[i], model.critic_target.q_networks_list[i], self.D, self.A, B, (t_q4, t_q2, t_qb),
                                       dev, q_out=self.q_out[i]) for i in range(n)]
        # the critic-input gradient the per-layer actor backward reads (observation columns stay zero)
        self.g_x = th.zeros(B, self.W, dtype=th.float32, device=dev)

    def actor_loss_grad(self, model, i: int, x_pi) -> th.Tensor:
        """-mean(Q1_i(obs, pi(obs))) (:177) and its gradient w.r.t. the critic input: Q chain forward (first critic, frozen) -> Q backward
        chain to the action (partials) -> the partials' sum into the action columns of g_x: 3 launches instead of 6."""
        blk = self.blocks[i]
        blk.policy_pass("neg_mean", x_pi, blk.back_nets(1), loss_out=model._loss_now, loss_sum=model._loss_sums[f"actor{i}"])
        hip_ops.chain_sum_parts(blk.gact_part, self.g_x[:, self.D:])
        return self.g_x

    def _backward(self, model, i: int, rd, fuse_opt: bool) -> None:
        blk = self.blocks[i]
        blk.td_backward(blk.back_nets(), blk.td_root(rd, model.gamma, 1.0, model._target_q[i], model._loss_now, model._loss_sums[f"critic{i}"],
                                                     adam_advance=[model.critic.optimizer_list[i]] if fuse_opt else ()))

    def captured(self, model, i: int) -> dict:
        return self.blocks[i].captured(model._target_q[i], model._loss_now)

    def critic_step(self, model, i: int, x_cur, x_next, rd) -> None:
        """Agent i's critic step (:146-164): 3 launches."""
        fuse_opt, blk = _adam_in_wgrad(model, self.B), self.blocks[i]
        blk.forward(blk.nets4(x_cur, x_next, target_roles=self.TARGET_ROLES), blk.t_q4)
        self._backward(model, i, rd, fuse_opt)
        opt = model.critic.optimizer_list[i]
        blk.apply([blk], x_cur, fuse_opt, [opt])
        if not fuse_opt:
            model._allreduce_grads(model.policy.critic_slices[i])
            opt.step()

    def critic_steps_all(self, model, x_cur, x_next, rd, capture=None) -> None:
        """Every agent's critic step of an update WITHOUT a policy step: the agents' steps do not depend on each other (no soft update in
        between), so their 4 x n_agents networks share ONE forward launch; a backward launch per agent; a dW / db + Adam launch per two
        agents. The same kernels on the same operands as `critic_step`: bit-identical."""
        fuse_opt, blocks = _adam_in_wgrad(model, self.B), self.blocks
        blocks[0].forward([net for blk in blocks for net in blk.nets4(x_cur, x_next, target_roles=self.TARGET_ROLES)], blocks[0].t_q4)
        for i in range(self.n):
            self._backward(model, i, rd, fuse_opt)
            if capture is not None:
                capture.append(self.captured(model, i))
        opts = model.critic.optimizer_list
        for i0 in range(0, self.n, 2):
            TwinCriticBlock.apply(blocks[i0:i0 + 2], x_cur, fuse_opt, opts[i0:i0 + 2])
        if not fuse_opt:
            for i in range(self.n):
                model._allreduce_grads(model.policy.critic_slices[i])
            opts[0].step_with(*opts[1:])
