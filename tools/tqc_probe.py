#!/usr/bin/env python3
"""TQC on the MI355X beside SAC, class defaults ((256, 256), batch 256, 2 critics x 25 atoms, 2 dropped per critic), 64 device envs:
ABI calls per gradient step, ms per iteration (one vec-step of rollout + one gradient step) with eager launches, replayed from
hipGraphs (1 and 8 iterations per graph) and on the torch statements (`fused_learner = False`, eager); SAC's per-layer step
(CSTR_CHAIN=0: the form TQC's step is built on) and SAC's row-chain step in the same run as baselines; and the two loss launches alone,
also at G = 5 (M = 125).

Every timed figure is the median over the rounds of `--alternations` processes per configuration, the configurations' processes taking
turns: one round = `--steps` iterations between two device synchronisations. Every child process runs under its own time limit.
The launches alone: each is recorded 64 times into one hipGraph and the graph replayed, so the figure is device time per call
(the critic loss is two launches) without the host's launch cost.

usage:  tqc_probe.py [--alternations 2] [--steps 512]            (writes the report to stdout)
        tqc_probe.py --child <algo>:<mode>                       (one configuration, one JSON line; used by the parent)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

SPECS = ("tqc:eager", "tqc:graph1", "tqc:graph8", "tqc:aten", "sac_perlayer:graph1", "sac_perlayer:eager", "sac:graph1")
BATCH, ENVS, ROUNDS, CHILD_LIMIT = 256, 64, 5, 240


def _model(algo: str, mode: str):
    from core.common.vec_env import CSTRVecEnv

    if algo == "tqc":
        from core.tqc import TQC as cls
    else:
        from core.sac import SAC as cls
    model = cls("MlpPolicy", CSTRVecEnv(ENVS), seed=0, learning_starts=ENVS * 4, buffer_size=ENVS * 4096)
    if mode.startswith("graph"):
        model.enable_graph_capture(True, unroll=int(mode[5:]))
    if mode == "aten":
        model.fused_learner = False
    return model


def _rounds(run_steps, steps: int) -> list:
    import torch as th

    out = []
    for _ in range(ROUNDS):
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        a.record()
        run_steps(steps)
        b.record()
        th.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def child(spec: str, steps: int) -> dict:
    import torch as th

    from core import _native as nv

    algo, mode = spec.split(":")
    out = dict(algo=algo, mode=mode, device=th.cuda.get_device_name(0))
    model = _model(algo, mode)
    model.learn(ENVS * 96)  # warm-up actions, allocator, graph warm-up iterations and captures
    if mode == "eager":
        th.cuda.synchronize()
        before = nv.ABI_CALLS[0]
        model.train(1, BATCH)
        out["launches"] = nv.ABI_CALLS[0] - before
    n = steps if mode != "aten" else max(steps // 4, 32)
    out["ms"] = _rounds(lambda k: model.learn(ENVS * k, reset_num_timesteps=False), n)
    st = model.graph_status()
    out.update(replays=st["replays"], eager_iterations=st["eager_iterations"], error=st["error"])
    return out


def _graph_time(fn, reps: int = 64) -> list:
    """device time per call of `fn` (us), recorded `reps` times into one graph"""
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
    for _ in range(ROUNDS):
        a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        a.record()
        for _ in range(8):
            g.replay()
        e.record()
        th.cuda.synchronize()
        ts.append(a.elapsed_time(e) * 1000.0 / (8 * reps))
    return ts


def launches_alone() -> dict:
    import torch as th

    from core.common import hip_ops

    out = {}
    b = BATCH
    r = lambda *s: th.randn(*s, device="cuda")  # noqa: E731
    for G, Nq, k in ((2, 25, 2), (5, 25, 2), (16, 16, 3)):
        z, zn, lp, rew, done, ec = r(G, b, Nq) - 3, r(G, b, Nq) - 3, r(b) - 1, -r(b, 1).abs(), th.zeros(b, 1, device="cuda"), th.full((1,), 0.2, device="cuda")
        gz, gzp, glp, zm = th.empty(G, b, Nq, device="cuda"), th.empty(G, b, Nq, device="cuda"), th.empty(b, device="cuda"), th.empty(b, device="cuda")
        y, ws = th.empty(b, G * Nq - k * G, device="cuda"), th.empty(3 * b, dtype=th.float64, device="cuda")
        lo, mo, la = th.zeros(1, device="cuda"), th.zeros(2, device="cuda"), th.zeros(1, device="cuda")
        out[f"critic G{G} Nq{Nq} k{k}"] = _graph_time(lambda: hip_ops.tqc_critic_loss(z, zn, lp, rew, done, ec, 0.99, k, gz, ws, loss_out=lo, target_out=y,
                                                                                         means_out=mo))
        out[f"actor G{G} Nq{Nq}"] = _graph_time(lambda: hip_ops.tqc_actor_loss(z, lp, ec, gzp, glp, loss_out=la, z_pi_mean=zm))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--child", default=None)
    ap.add_argument("--launches-alone", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.steps)))
        return
    if args.launches_alone:
        print(json.dumps(launches_alone()))
        return
    me = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps)]
    results = {s: [] for s in SPECS}
    for _ in range(args.alternations):
        for s in SPECS:  # the configurations' processes take turns; a failing child ends the probe
            env = dict(os.environ, CSTR_CHAIN="0") if s.startswith("sac_perlayer") else dict(os.environ)
            res = subprocess.run(me + ["--child", s], check=True, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT, env=env)
            results[s].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"{s}: {statistics.median(results[s][-1]['ms']):.4f} ms", file=sys.stderr, flush=True)
    alone = json.loads(subprocess.run(me + ["--launches-alone"], check=True, stdout=subprocess.PIPE, text=True,
                                      timeout=CHILD_LIMIT).stdout.strip().splitlines()[-1])
    first = results[SPECS[0]][0]
    print(f"TQC beside SAC; class defaults, batch {BATCH}, {ENVS} device envs, {first['device']}")
    print(f"ms per iteration (one vec-step of rollout + one gradient step): median (max - min) over {ROUNDS * args.alternations} rounds of "
          f"{args.steps} iterations from {args.alternations} alternating processes per configuration (torch statements: a quarter of the iterations)")
    names = {"tqc:eager": "TQC eager launches", "tqc:graph1": "TQC hipGraph replay, 1 iteration per graph", "tqc:graph8": "TQC hipGraph replay, 8 iterations per graph",
             "tqc:aten": "TQC torch statements, eager", "sac_perlayer:graph1": "SAC per-layer step (CSTR_CHAIN=0), replay, 1 per graph",
             "sac_perlayer:eager": "SAC per-layer step (CSTR_CHAIN=0), eager", "sac:graph1": "SAC row-chain step, replay, 1 per graph"}
    print(f"ABI calls per gradient step: TQC {results['tqc:eager'][0]['launches']}, SAC per-layer {results['sac_perlayer:eager'][0]['launches']}")
    med = {}
    for s in SPECS:
        rs = results[s]
        ms = [v for r in rs for v in r["ms"]]
        med[s] = statistics.median(ms)
        print(f"  {names[s]:54s}: {med[s]:.4f} ms ({max(ms) - min(ms):.4f})  (replays {rs[0]['replays']}, eager iterations "
              f"{rs[0]['eager_iterations']}, error {rs[0]['error']})")
    print(f"TQC's replayed iteration against SAC's per-layer one: {med['tqc:graph1'] / med['sac_perlayer:graph1']:.2f} x; "
          f"against the torch statements: {med['tqc:aten'] / med['tqc:graph1']:.1f} x faster")
    print("device time per call of the loss entry points at batch 256, recorded 64 times into one graph, median of 5 rounds of 8 replays:")
    for name, ts in alone.items():
        print(f"  {name:24s}: {statistics.median(ts):.2f} us")


if __name__ == "__main__":
    main()
