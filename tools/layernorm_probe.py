#!/usr/bin/env python3
"""LayerNorm / dropout critics (csrc/cstr_layernorm.hip) on the MI355X beside plain SAC. No pass / fail threshold. Class defaults
((256, 256), batch 256, 2 critics), 64 device envs, ONE process, the legs taking turns, median of `--rounds` rounds of `--steps`
iterations (one vec-step of rollout + one gradient step) between two device synchronisations:

  * SAC layer_norm=True, dropout_rate=0.01 and the same at p = 0, replayed from hipGraphs;
  * plain SAC on its per-layer step (the row-chain step switched off, as CSTR_CHAIN=0 does: the form the LayerNorm step is built on),
    replayed from hipGraphs;
  * the torch-statement path (`fused_learner = False`) of the LayerNorm model, eager: that path is not captured;
  * ABI calls (launching entry points) per gradient step of the LayerNorm and the plain per-layer step, eager;
  * device time per call of the two new entry points at SAC's hidden layer (G 2, M 256, K 256, N 256) and at the 32-row-block grid's
    other shapes, each recorded 64 times into one hipGraph and replayed (the backward's figure includes its finishing launch).

usage:  layernorm_probe.py [--rounds 5] [--steps 256] [--out profiles/layernorm_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)

BATCH, ENVS = 256, 64


def model(kind: str, graph: bool):
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    kw = {"ln": dict(layer_norm=True, dropout_rate=0.01), "ln0": dict(layer_norm=True), "plain": {}, "aten": dict(layer_norm=True, dropout_rate=0.01)}[kind]
    m = SAC("MlpPolicy", CSTRVecEnv(ENVS), seed=0, learning_starts=ENVS * 4, buffer_size=ENVS * 4096, policy_kwargs=kw)
    if kind == "aten":
        m.fused_learner = False
    elif graph:
        m.enable_graph_capture(True)
    m.learn(ENVS * 96)  # warm-up actions, allocator, graph warm-up iterations and captures
    return m


def timed(m, steps: int) -> float:
    import torch as th

    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    a.record()
    m.learn(ENVS * steps, reset_num_timesteps=False)
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / steps


def abi_calls(kind: str) -> int:
    import torch as th

    from core import _native as nv

    m = model(kind, graph=False)
    th.cuda.synchronize()
    before = nv.ABI_CALLS[0]
    m.train(1, BATCH)
    return nv.ABI_CALLS[0] - before


def graph_time(fn, rounds: int, reps: int = 64) -> float:
    """device time per call of `fn` (us): recorded `reps` times into one graph, median of `rounds` rounds of 8 replays"""
    import torch as th

    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(3):
            fn()
    th.cuda.current_stream().wait_stream(side)
    g = th.cuda.CUDAGraph()
    with th.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(4):
        g.replay()
    ts = []
    for _ in range(rounds):
        a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        a.record()
        for _ in range(8):
            g.replay()
        e.record()
        th.cuda.synchronize()
        ts.append(a.elapsed_time(e) * 1000.0 / (8 * reps))
    return statistics.median(ts)


def kernels_alone(rounds: int) -> list:
    import torch as th

    from core import _native as nv
    from core.common import hip_ops

    r = lambda *s: th.randn(*s, device="cuda")  # noqa: E731
    lines = []
    for G, M, K, N in ((2, 256, 256, 256), (2, 256, 6, 256), (2, 256, 400, 300), (2, 256, 512, 512)):
        x, w, b, gm, bt = r(G, M, K), r(G, N, K) / K ** 0.5, r(G, N), 1 + 0.1 * r(G, N), 0.1 * r(G, N)
        w_next, gz_next, w_head, gq = r(G, K, N) / N ** 0.5, r(G, M, K), r(G, 1, N), r(G, M, 1)
        ctl, word = th.zeros(nv.RNG_CTL_WORDS, dtype=th.int64, device="cuda"), th.zeros(1, dtype=th.int64, device="cuda")
        out = hip_ops.linear_ln_act_fwd(x, w, b, gm, bt, 1)
        gz, dg, db, parts = th.empty(G, M, N, device="cuda"), th.empty(G, N, device="cuda"), th.empty(G, N, device="cuda"), hip_ops.ln_parts(G, M, N, "cuda")
        zb = th.zeros(G, N, device="cuda")
        t = dict(
            fwd0=graph_time(lambda: hip_ops.linear_ln_act_fwd(x, w, b, gm, bt, 1, out=out), rounds),
            fwdp=graph_time(lambda: hip_ops.linear_ln_act_fwd(x, w, b, gm, bt, 1, 0.01, rng_ctl=ctl, advance=True, pass_out=word, out=out), rounds),
            plain=graph_time(lambda: hip_ops.linear_act_fwd(x, w, zb, 1), rounds),
            bwd0=graph_time(lambda: hip_ops.ln_linear_bwd_input(gz_next, w_next, *out, gm, 1, parts=parts, dgamma=dg, dbeta=db, out=gz), rounds),
            bwdp=graph_time(lambda: hip_ops.ln_linear_bwd_input(gz_next, w_next, *out, gm, 1, 0.01, rng_ctl=ctl, pass_ctr=word, parts=parts, dgamma=dg,
                                                                dbeta=db, out=gz), rounds),
            bwdf=graph_time(lambda: hip_ops.ln_linear_bwd_input(gz_next, w_next, *out, gm, 1, out=gz), rounds),
            head=graph_time(lambda: hip_ops.ln_linear_bwd_input(gq, w_head, *out, gm, 1, parts=parts, dgamma=dg, dbeta=db, out=gz), rounds),
            plain_bwd=graph_time(lambda: hip_ops.linear_bwd_input(gz_next, w_next, out[0], 1), rounds))
        lines.append(f"  G {G} M {M} K {K} N {N} ({G * ((M + 15) // 16)} workgroups): forward {t['fwd0']:.2f} us (p = 0.01: {t['fwdp']:.2f}; plain Linear + ReLU "
                     f"launch, one wave per 16 x 16 tile: {t['plain']:.2f}); backward from a {K}-wide consumer with d gamma / d beta {t['bwd0']:.2f} us "
                     f"(p = 0.01: {t['bwdp']:.2f}; frozen parameters, no finishing launch: {t['bwdf']:.2f}; plain input-gradient launch: "
                     f"{t['plain_bwd']:.2f}); backward from the scalar head {t['head']:.2f} us")
    return lines


def main() -> None:
    import torch as th

    from core.common import chain

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layernorm_probe.txt"))
    args = ap.parse_args()
    chain.USE_CHAIN = False  # plain SAC on its per-layer step; the LayerNorm critics never take the row-chain step
    legs = {k: model(k, graph=True) for k in ("ln", "ln0", "plain", "aten")}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, m in legs.items():  # the legs take turns
            ms[k].append(timed(m, args.steps if k != "aten" else max(args.steps // 8, 16)))
    med = {k: statistics.median(v) for k, v in ms.items()}
    calls = {k: abi_calls(k) for k in ("ln", "ln0", "plain")}
    names = dict(ln="SAC layer_norm=True, dropout_rate=0.01, hipGraph replay", ln0="SAC layer_norm=True, p = 0, hipGraph replay",
                 plain="plain SAC, per-layer step (row chain off), hipGraph replay", aten="LayerNorm model (p = 0.01), torch statements, eager")
    out = [f"LayerNorm / dropout critics beside plain SAC; class defaults, batch {BATCH}, {ENVS} device envs, {th.cuda.get_device_name(0)}",
           f"ms per iteration (one vec-step of rollout + one gradient step): median (max - min) of {args.rounds} rounds of {args.steps} iterations, "
           "one process, the legs taking turns (torch statements: an eighth of the iterations)"]
    for k in legs:
        st = legs[k].graph_status()
        out.append(f"  {names[k]:62s}: {med[k]:.4f} ms ({max(ms[k]) - min(ms[k]):.4f})  (replays {st['replays']}, error {st['error']})")
    out.append(f"kernel path against the torch statements of the same model: {med['aten'] / med['ln']:.1f} x faster; against plain per-layer SAC: "
               f"{med['ln'] / med['plain']:.2f} x the time (p = 0: {med['ln0'] / med['plain']:.2f} x)")
    out.append(f"ABI calls per gradient step, eager: LayerNorm p = 0.01 {calls['ln']}, p = 0 {calls['ln0']}, plain per-layer {calls['plain']}")
    out.append("device time per call, recorded 64 times into one hipGraph, median of rounds of 8 replays:")
    out += kernels_alone(args.rounds)
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
