#!/usr/bin/env python3
"""IQL on the MI355X beside TD3BC, CQL and BCQ, class defaults ((256, 256), batch 256): ABI launches per gradient step, ms per gradient
step with eager launches, replayed from hipGraphs (1 and 8 gradient steps per graph) and on the torch-statement path
(`fused_learner = False`, eager), and the loss launch alone.

Every timed figure is the median over the rounds of `--alternations` processes per configuration, the configurations' processes taking
turns (a, b, c, ..., a, b, c, ...): one round = `--steps` gradient steps between two device synchronisations. The four algorithms run
their own learn() loops (OfflineAlgorithm: an iteration IS a gradient step). Every child process runs under its own time limit.
The launch alone: cstr_iql_loss_f32 is recorded 64 times into one hipGraph and the graph replayed, so the figure is device time per
launch without the host's launch cost.

usage:  iql_probe.py [--alternations 2] [--steps 512] [--rows 100000]            (writes the report to stdout)
        iql_probe.py --child <algo>:<mode>                                       (one configuration, one JSON line; used by the parent)
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

SPECS = ("iql:eager", "iql:graph1", "iql:graph8", "iql:aten", "td3bc:graph1", "cql:graph1", "bcq:graph1")
BATCH, ROUNDS, CHILD_LIMIT = 256, 5, 240


def _model(algo: str, rows: int, mode: str):
    from bcq_probe import dataset
    from core.common.vec_env import CSTRVecEnv

    if algo == "iql":
        from core.iql import IQL as cls
    elif algo == "cql":
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


def launch_alone(rows: int) -> dict:
    """device time of the loss launch (us), recorded 64 times into one graph"""
    import torch as th

    from core.common import hip_ops

    model = _model("iql", rows, "eager")
    model.learn(8)
    b = BATCH
    rd = model._packed.samples
    r = lambda *s: th.randn(*s, device="cuda")  # noqa: E731
    qt, v2, q, params = r(2, b) - 3, r(2 * b) - 3, r(2, b) - 3, r(b, 4) * 0.5
    g_v, gq, g_params, tq, adv, logp = th.empty(b, device="cuda"), th.empty(2, b, device="cuda"), th.empty(b, 4, device="cuda"), \
        th.empty(b, device="cuda"), th.empty(b, device="cuda"), th.empty(b, device="cuda")
    lo, aux = th.zeros(3, device="cuda"), th.zeros(6, device="cuda")

    def loss():
        hip_ops.iql_loss(qt[0], qt[1], v2[:b], v2[b:], q[0], q[1], params, rd.actions, rd.rewards, rd.dones, 0.99, 0.7, 3.0, 100.0, g_v=g_v,
                         gq1=gq[0], gq2=gq[1], g_params=g_params, loss_out=lo, aux=aux, target_out=tq, adv_out=adv, logp_out=logp)

    reps = 64
    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(3):
            loss()
    th.cuda.current_stream().wait_stream(side)
    g = th.cuda.CUDAGraph()
    with th.cuda.graph(g):
        for _ in range(reps):
            loss()
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
    return dict(loss=ts)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--child", default=None)
    ap.add_argument("--launch-alone", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.steps, args.rows)))
        return
    if args.launch_alone:
        print(json.dumps(launch_alone(args.rows)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--rows", str(args.rows)]
    results = {s: [] for s in SPECS}
    for _ in range(args.alternations):
        for s in SPECS:  # the configurations' processes take turns; a failing child ends the probe
            res = subprocess.run(me + ["--child", s], check=True, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
            results[s].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"{s}: {statistics.median(results[s][-1]['ms']):.4f} ms", file=sys.stderr, flush=True)
    alone = json.loads(subprocess.run(me + ["--launch-alone"], check=True, stdout=subprocess.PIPE, text=True,
                                      timeout=CHILD_LIMIT).stdout.strip().splitlines()[-1])
    first = results[SPECS[0]][0]
    print(f"IQL beside TD3BC, CQL and BCQ; class defaults, batch {BATCH}, dataset of {args.rows} rows, {first['device']}")
    print(f"ms per gradient step: median (max - min) over {ROUNDS * args.alternations} rounds of {args.steps} steps from {args.alternations} "
          "alternating processes per configuration (torch statements: a quarter of the steps)")
    names = {"iql:eager": "IQL  eager launches", "iql:graph1": "IQL  hipGraph replay, 1 step per graph", "iql:graph8": "IQL  hipGraph replay, 8 steps per graph",
             "iql:aten": "IQL  torch statements, eager", "td3bc:graph1": "TD3BC hipGraph replay, 1 step per graph",
             "cql:graph1": "CQL  hipGraph replay, 1 step per graph", "bcq:graph1": "BCQ  hipGraph replay, 1 step per graph"}
    print(f"IQL: ABI launches per gradient step {results['iql:eager'][0]['launches']}")
    med = {}
    for s in SPECS:
        rs = results[s]
        ms = [v for r in rs for v in r["ms"]]
        med[s] = statistics.median(ms)
        print(f"  {names[s]:42s}: {med[s]:.4f} ms ({max(ms) - min(ms):.4f})  (replays {rs[0]['replays']}, eager iterations "
              f"{rs[0]['eager_iterations']}, error {rs[0]['error']})")
    faster = "faster" if med["iql:graph1"] < med["iql:aten"] else "NOT faster"
    print(f"the replayed fused step is {faster} than the eager torch-statement step: {med['iql:graph1']:.4f} ms against {med['iql:aten']:.4f} ms")
    print(f"IQL's replayed step against CQL's: {med['iql:graph1'] / med['cql:graph1']:.2f} x")
    us = statistics.median(alone["loss"])
    print("device time of the loss launch, recorded 64 times into one graph, median of 5 rounds of 8 replays:")
    print(f"  cstr_iql_loss_f32 (256 rows, A = 2, every output): {us:.2f} us")


if __name__ == "__main__":
    main()
