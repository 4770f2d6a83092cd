#!/usr/bin/env python3
"""Per-launch time of the SAC gradient step's row-chain kernels (csrc/cstr_chain.hip) at the bench shape, graph-replayed back-to-back
launches + HIP events, for every `tiles` setting; the per-layer launch they replace beside them. `chain_launches` is also what
bench.py's `kernels` section times.
    python tools/chain_probe.py [--batch 256]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch as th  # noqa: E402


def chain_launches(model, B: int, tiles=None) -> dict:
    """{name: (callable issuing ONE launch, algorithmic FLOPs of its MFMA work)} for the six chain launches of a SAC gradient step on
    `model` (state of the step's buffers as a real step leaves them: every launch is idempotent on it)."""
    from core import _native as nv
    from core.common import chain, hip_ops

    old = chain.TILES
    if tiles is not None:
        chain.TILES = tuple(tiles)
    try:
        c = chain.SacChain(model, B)
    finally:
        chain.TILES = old
    pb = model._packed_batch(B)
    if model.replay_buffer._predrawn is None:
        model.replay_buffer.sample_packed_into(pb)
    rd = pb.samples
    fa = model._fast_actor
    if fa.rng_ctl is None:
        fa.rng_ctl = hip_ops.new_rng_ctl(0, model.device)
    blk, D, A = c.block, c.D, c.A
    fin = nv.SacHeadFin(c.head_part.data_ptr(), fa._hb.data_ptr(), c.eps_all.data_ptr(), c.n_head_parts, A, D, nv.CHAIN_HEAD_GAUSSIAN, 2 * B, B, 0.0, 0.0,
                        pb.x_pi.data_ptr(), pb.x_next.data_ptr(), c.params.data_ptr(), c.logp_pi.data_ptr(), c.logp_next.data_ptr())
    # the step's own lists and roots (core/common/chain.py:TwinCriticBlock), without the RNG / Adam advances (idempotent)
    nets4 = blk.nets4(pb.x_data, pb.x_next, roles=c.ROLES)
    nets2, back = blk.pi_nets(pb.x_pi), blk.back_nets()
    ent = th.ones(1, device=model.device)
    loss = th.zeros(1, device=model.device)
    tq = th.zeros(B, 1, device=model.device)
    root = blk.td_root(rd, 0.99, 0.5, tq, loss, None, next_logp=c.logp_next, ent_coef=ent)
    aroot = blk.pi_root("sac_actor", ent_coef=ent, logp=c.logp_pi, loss_out=loss)
    actor_f = 2.0 * (D * c.aH1 + c.aH1 * c.aH2 + c.aH2 * 2 * A)
    q_f = 2.0 * (blk.W * blk.H1 + blk.H1 * blk.H2 + blk.H2)
    keep = (c, pb, fin, nets4, nets2, back, root, aroot, ent, loss, tq)  # alive as long as the callables
    return dict(
        sac_actor_chain_fwd=(lambda k=keep: hip_ops.sac_actor_chain_fwd(c.actor, B, None, pb.x_pi, pb.x_next, None, None, c.a_h1, c.a_h2, c.head_part, c.t_act,
                                                                        head_rng_ctl=fa.rng_ctl, eps_all=c.eps_all), actor_f * 2 * B),
        q_chain_fwd_4nets=(lambda k=keep: blk.forward(nets4, blk.t_q4, fin), q_f * 4 * B),
        q_chain_bwd_td=(lambda k=keep: blk.td_backward(back, root), 2.0 * blk.H1 * blk.H2 * 2 * B),
        q_chain_fwd_2nets=(lambda k=keep: blk.forward(nets2, blk.t_qpi), q_f * 2 * B),
        q_chain_bwd_actor=(lambda k=keep: blk.pi_backward(back, aroot), 2.0 * blk.H1 * blk.H2 * 2 * B),
        sac_actor_chain_bwd=(lambda k=keep: hip_ops.sac_actor_chain_bwd(c.actor, blk.gact_part, 2, blk.n_gact, ent, pb.x_pi, c.params, c.eps_all, c.a_h1,
                                                                        c.a_h2, c.g_params, c.dz2a, c.dz1a, B, c.t_ab), 2.0 * (c.aH1 * c.aH2 + 2 * A * c.aH2) * B))


def main():
    from bench import event_time_us
    from core.common import hip_ops
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n", type=int, default=200)
    args = ap.parse_args()
    B = args.batch
    model = SAC("MlpPolicy", CSTRVecEnv(4096), seed=0, batch_size=B)
    model.learn(4096 * 4)
    stream = th.cuda.current_stream()
    res = {}
    names = None
    for tiles in (1, 2, 4):
        fns = chain_launches(model, B, (tiles,) * 5)
        names = list(fns)
        for fn, _ in fns.values():
            fn()
        for name, (fn, _) in fns.items():
            res[(name, tiles)] = event_time_us(fn, args.n, stream, in_graph=True)
    print(f"chain kernels, batch {B}: us per graph-replayed launch at tiles = 1 / 2 / 4")
    for name in names:
        print(f"  {name:20s} " + " / ".join(f"{res[(name, t)]:6.2f}" for t in (1, 2, 4)))
    h = 256
    x = th.randn(B, h, device=model.device)
    w, bias = th.randn(h, h, device=model.device) / 16, th.zeros(h, device=model.device)
    us = event_time_us(lambda: hip_ops.linear_act_fwd(x, w, bias, 1), args.n, stream, in_graph=True)
    print(f"  reference: linear_act_fwd {B} x {h} x {h}: {us:.2f} us per launch")


if __name__ == "__main__":
    main()
