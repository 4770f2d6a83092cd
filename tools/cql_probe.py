#!/usr/bin/env python3
"""CQL on the MI355X beside TD3BC and BCQ, class defaults ((256, 256), batch 256, N = 10 candidates per kind: the critic step runs on
31 * 256 = 7936 rows): ABI launches per gradient step, ms per gradient step with eager launches, replayed from hipGraphs (1 and 8
gradient steps per graph) and on the torch-statement path (`fused_learner = False`, eager), the two new launches alone, and how the
critic step splits between the Linear kernels and the two new launches.

Every timed figure is the median over the rounds of `--alternations` processes per configuration, the configurations' processes taking
turns (a, b, c, ..., a, b, c, ...): one round = `--steps` gradient steps between two device synchronisations. The three algorithms run
their own learn() loops (OfflineAlgorithm: an iteration IS a gradient step). Every child process runs under its own time limit.
The launches alone: each is recorded 64 times into one hipGraph and the graph replayed, so the figure is device time per launch without
the host's launch cost: cstr_cql_candidates_f32 (drawn noise), cstr_cql_q_loss_f32, and PerLayerTwinCritic.cql_step as a whole (target
critics on B rows, the twin critic's forward and backward on 31 B rows, the loss launch between them).

usage:  cql_probe.py [--alternations 2] [--steps 512] [--rows 100000]            (writes the report to stdout)
        cql_probe.py --child <algo>:<mode>                                       (one configuration, one JSON line; used by the parent)
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

SPECS = ("cql:eager", "cql:graph1", "cql:graph8", "cql:aten", "td3bc:graph1", "bcq:graph1")
BATCH, ROUNDS, CHILD_LIMIT = 256, 5, 240


def _model(algo: str, rows: int, mode: str):
    from bcq_probe import dataset
    from core.common.vec_env import CSTRVecEnv

    if algo == "cql":
        from core.cql import CQL as cls
    elif algo == "td3bc":
        from core.td3bc import TD3BC as cls
    else:
        from core.bcq import BCQ as cls
    model = cls("MlpPolicy", CSTRVecEnv(1), dataset=dataset(rows, "cuda"), seed=0)
    if mode.startswith("graph"):
        model.enable_graph_capture(True, unroll=int(mode[5:]))
    if mode == "aten":
        model.fused_learner = False
    return model


def _abi_calls(fn) -> int:
    import torch as th

    from core import _native as nv

    th.cuda.synchronize()
    before = nv.ABI_CALLS[0]
    fn()
    return nv.ABI_CALLS[0] - before


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


def child(spec: str, steps: int, rows: int) -> dict:
    import torch as th

    algo, mode = spec.split(":")
    out = dict(algo=algo, mode=mode, device=th.cuda.get_device_name(0))
    model = _model(algo, rows, mode)
    model.learn(96)  # allocator, graph warm-up iterations and captures
    if mode == "eager":
        out["launches"] = _abi_calls(lambda: model.train(1, BATCH))
    out["ms"] = _rounds(lambda n: model.learn(n, reset_num_timesteps=False), steps if mode != "aten" else max(steps // 4, 32))
    st = model.graph_status()
    out.update(replays=st["replays"], eager_iterations=st["eager_iterations"], error=st["error"])
    return out


def launches_alone(rows: int) -> dict:
    """device time per launch (us), each recorded 64 times into one graph"""
    import torch as th

    from core.common import hip_ops

    model = _model("cql", rows, "eager")
    model.learn(8)
    b, n = BATCH, model.cql_n_actions
    pb, rd, blk = model._packed, model._packed.samples, model._critic_block
    params, corr, xw = model._cql_params, model._cql_corr, model._x_wide
    ent = th.ones(1, device="cuda")
    q_all = th.randn(2, (1 + 3 * n) * b, 1, device="cuda")
    gq, tq, lo, aux = th.empty_like(q_all), th.empty(b, 1, device="cuda"), th.zeros(1, device="cuda"), th.zeros(4, device="cuda")
    qt = th.randn(2, b, device="cuda")

    def candidates():
        hip_ops.cql_candidates(rd.observations, params[:b], params[b:], n, xw[b:], corr, rng_ctl=model._device_rng())

    def q_loss():
        hip_ops.cql_q_loss(q_all, corr, False, qt[0], qt[1], None, rd.rewards, rd.dones, ent, 0.99, 5.0, 1.0, tq, gq, lo, None, aux)

    def critic_step():
        blk.cql_step(xw, corr, False, pb.x_next, rd, 0.99, 5.0, 1.0, tq, lo, None, aux, ent_coef=ent)

    out = {}
    for name, fn, reps in (("candidates", candidates, 64), ("q_loss", q_loss, 64), ("critic_step", critic_step, 16)):
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
        out[name] = ts
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--child", default=None)
    ap.add_argument("--launches-alone", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.steps, args.rows)))
        return
    if args.launches_alone:
        print(json.dumps(launches_alone(args.rows)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--rows", str(args.rows)]
    results = {s: [] for s in SPECS}
    for _ in range(args.alternations):
        for s in SPECS:  # the configurations' processes take turns; a failing child ends the probe
            res = subprocess.run(me + ["--child", s], check=True, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
            results[s].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"{s}: {statistics.median(results[s][-1]['ms']):.4f} ms", file=sys.stderr, flush=True)
    alone = json.loads(subprocess.run(me + ["--launches-alone"], check=True, stdout=subprocess.PIPE, text=True,
                                      timeout=CHILD_LIMIT).stdout.strip().splitlines()[-1])
    first = results[SPECS[0]][0]
    print(f"CQL beside TD3BC and BCQ; class defaults, batch {BATCH}, N = 10 (critic step on {31 * BATCH} rows), dataset of {args.rows} rows, "
          f"{first['device']}")
    print(f"ms per gradient step: median (max - min) over {ROUNDS * args.alternations} rounds of {args.steps} steps from {args.alternations} "
          "alternating processes per configuration (torch statements: a quarter of the steps)")
    names = {"cql:eager": "CQL  eager launches", "cql:graph1": "CQL  hipGraph replay, 1 step per graph", "cql:graph8": "CQL  hipGraph replay, 8 steps per graph",
             "cql:aten": "CQL  torch statements, eager", "td3bc:graph1": "TD3BC hipGraph replay, 1 step per graph",
             "bcq:graph1": "BCQ  hipGraph replay, 1 step per graph"}
    print(f"CQL: ABI launches per gradient step {results['cql:eager'][0]['launches']}")
    med = {}
    for s in SPECS:
        rs = results[s]
        ms = [v for r in rs for v in r["ms"]]
        med[s] = statistics.median(ms)
        print(f"  {names[s]:42s}: {med[s]:.4f} ms ({max(ms) - min(ms):.4f})  (replays {rs[0]['replays']}, eager iterations "
              f"{rs[0]['eager_iterations']}, error {rs[0]['error']})")
    faster = "faster" if med["cql:graph1"] < med["cql:aten"] else "NOT faster"
    print(f"the replayed fused step is {faster} than the eager torch-statement step: {med['cql:graph1']:.4f} ms against {med['cql:aten']:.4f} ms")
    us = {k: statistics.median(v) for k, v in alone.items()}
    print("device time per launch, each recorded 64 times (the critic step 16 times) into one graph, median of 5 rounds of 8 replays:")
    print(f"  cstr_cql_candidates_f32 (7680 rows, drawn noise) : {us['candidates']:.2f} us")
    print(f"  cstr_cql_q_loss_f32 (256 states x 2 critics x 30): {us['q_loss']:.2f} us")
    print(f"  the critic step (targets on 256 rows, forward + backward on 7936 rows, the loss launch): {us['critic_step']:.2f} us, of which the "
          f"Linear kernels {us['critic_step'] - us['q_loss']:.2f} us ({100 * (1 - us['q_loss'] / us['critic_step']):.0f} %)")


if __name__ == "__main__":
    main()
