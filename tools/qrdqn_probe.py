#!/usr/bin/env python3
"""QR-DQN on the MI355X beside DQN, class defaults (train_freq 4, batch 32, nets [64, 64], 200 atoms) on CSTRVecEnv(4096,
discrete_actions=5). No pass / fail threshold. One process per configuration, each under its own time limit:

  * milliseconds per iteration (one iteration = train_freq vec-steps and one gradient step) and env-steps/s with eager launches and
    replayed from a hipGraph holding one and eight iterations, for QR-DQN and for DQN in the same run; the ABI calls of one iteration.
    learning_starts is lowered to one iteration so that the measured iterations are steady-state ones. Wall clock over `--iterations`
    iterations between two device synchronisations, median of five rounds;
  * device time per call of the fold launch and of the loss entry point (two launches) at (levels, atoms) = (5, 200), (16, 25),
    (16, 200), batch 32, hidden width 64: each recorded 64 times into one hipGraph and the graph replayed;
  * one vec-step at `--envs` envs through the folded head (fold launch, trunk, one [M, H] Linear) beside the same vec-step through the
    full quantile layer and a torch mean over the atoms ([envs, atoms * M] written and re-read), at (5, 200) and (16, 200): 16
    vec-steps recorded into one hipGraph, device time per vec-step.

usage:  qrdqn_probe.py [--envs 4096] [--iterations 300]          (writes the report to stdout)
        qrdqn_probe.py --child <spec>                             (one configuration, one JSON line; used by the parent)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)

ITER_SPECS = ("qrdqn:eager", "qrdqn:graph1", "qrdqn:graph8", "dqn:eager", "dqn:graph1", "dqn:graph8")
SHAPES = ((5, 200), (16, 25), (16, 200))
VEC_SHAPES = ((5, 200), (16, 200))
ROUNDS, CHILD_LIMIT = 5, 240


def _model(algo: str, envs: int, levels: int, **kw):
    from core.common.logger import Logger
    from core.common.vec_env import CSTRVecEnv

    if algo == "qrdqn":
        from core.qrdqn import QRDQN as cls
    else:
        from core.dqn import DQN as cls
    model = cls("MlpPolicy", CSTRVecEnv(envs, discrete_actions=levels), seed=0, learning_starts=envs, **kw)
    model.set_logger(Logger(folder=None, output_formats=[]))
    return model


def iteration_child(spec: str, envs: int, iterations: int) -> dict:
    import torch as th

    from core import _native as nv

    algo, mode = spec.split(":")
    model = _model(algo, envs, 5)
    unroll = int(mode[5:]) if mode.startswith("graph") else 1
    if mode.startswith("graph"):
        model.enable_graph_capture(True, unroll=unroll)
    per_iter = model.train_freq.frequency * envs
    model.learn(per_iter * (16 + 8 * unroll))  # warm-up bodies, captures, allocator
    rounds = []
    for _ in range(ROUNDS):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        model.learn(per_iter * iterations, reset_num_timesteps=False)
        th.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3 / iterations)
    st = model.graph_status()
    out = dict(ms=rounds, per_iter=per_iter, device=th.cuda.get_device_name(0), graphs=st["graphs"], replays=st["replays"],
               eager_iterations=st["eager_iterations"], error=st["error"], fused=bool(model.fused_learner))
    if mode == "eager":
        c0 = nv.ABI_CALLS[0]
        model.learn(per_iter, reset_num_timesteps=False)
        out["abi_calls"] = nv.ABI_CALLS[0] - c0
    return out


def _graph_time(fn, reps: int) -> list:
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


def launches_child() -> dict:
    import torch as th

    from core.common import hip_ops

    out, b, h = {}, 32, 64
    r = lambda *s: th.randn(*s, device="cuda")  # noqa: E731
    for K, Nq in SHAPES:
        M = K * K
        w, bias, w_mean, b_mean = r(Nq * M, h), r(Nq * M), th.empty(M, h, device="cuda"), th.empty(M, device="cuda")
        out[f"fold K{K} Nq{Nq}"] = _graph_time(lambda: hip_ops.qrdqn_fold_head(w, bias, M, w_mean, b_mean), 64)
        z, zn, valve = r(b, Nq * M) - 3, r(b, Nq * M) - 3, th.full((b, 2), -1.0, device="cuda")
        rew, done, gz = -r(b, 1).abs(), th.zeros(b, 1, device="cuda"), th.empty(b, Nq * M, device="cuda")
        ws, lo = th.empty(b, dtype=th.float64, device="cuda"), th.zeros(1, device="cuda")
        out[f"loss K{K} Nq{Nq}"] = _graph_time(lambda: hip_ops.qrdqn_loss(z, zn, valve, rew, done, 0.99, K, Nq, gz, ws, loss_out=lo), 64)
    return out


def vecstep_child(envs: int, levels: int, atoms: int, full: bool) -> dict:
    import torch as th

    model = _model("qrdqn", envs, levels, policy_kwargs=dict(n_quantiles=atoms))
    model.learn(envs * 8)
    if full:  # the literal statement: the whole quantile layer, then the mean over the atoms
        m = levels * levels

        def q_values(obs):
            with th.no_grad():
                return model._fast_q(obs, train_params=False).view(obs.shape[0], atoms, m).mean(dim=1)

        model._q_values = q_values
    model._write_eps([0.05])
    slot = model._eps_slots[0:1]
    with th.cuda.device(model.device):
        ts = _graph_time(lambda: model._device_vec_step(slot), 16)
    return dict(us=ts)


def _run_child(me: list, spec: str) -> dict:
    res = subprocess.run(me + ["--child", spec], check=True, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        kind = args.child.split(":")
        if kind[0] == "launches":
            out = launches_child()
        elif kind[0] == "vecstep":
            out = vecstep_child(args.envs, int(kind[1]), int(kind[2]), kind[3] == "full")
        else:
            out = iteration_child(args.child, args.envs, args.iterations)
        print(json.dumps(out))
        return
    me = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--iterations", str(args.iterations)]
    results = {}
    for s in ITER_SPECS:  # a failing child ends the probe
        results[s] = _run_child(me, s)
        print(f"{s}: {statistics.median(results[s]['ms']):.4f} ms", file=sys.stderr, flush=True)
    print(f"QR-DQN beside DQN, class defaults, {args.envs} envs, 5 x 5 valve levels, {results[ITER_SPECS[0]]['device']}")
    print(f"ms per iteration (4 vec-steps + one gradient step), median of {ROUNDS} rounds of {args.iterations} iterations, wall clock:")
    labels = {"eager": "eager", "graph1": "graph, 1 iteration", "graph8": "graph, 8 iterations"}
    for s in ITER_SPECS:
        algo, mode = s.split(":")
        r = results[s]
        ms = statistics.median(r["ms"])
        line = f"  {algo.upper():6s} {labels[mode]:20s}: {ms:.4f} ms / iteration ({r['per_iter'] / ms * 1e3:.3g} env-steps/s)"
        if mode == "eager":
            line += f"; {r['abi_calls']} ABI calls / iteration; kernel path {r['fused']}"
        else:
            line += f"; graphs {r['graphs']}, replays {r['replays']}, eager iterations {r['eager_iterations']}, error {r['error']}"
        print(line)
    alone = _run_child(me, "launches")
    print("device time per call at batch 32, hidden width 64, recorded 64 times into one graph, median of 5 rounds of 8 replays:")
    for name, ts in alone.items():
        print(f"  {name:16s}: {statistics.median(ts):.2f} us")
    print(f"one vec-step at {args.envs} envs, 16 recorded into one graph, device time per vec-step, median of 5 rounds of 8 replays:")
    for K, Nq in VEC_SHAPES:
        fold = statistics.median(_run_child(me, f"vecstep:{K}:{Nq}:fold")["us"])
        full = statistics.median(_run_child(me, f"vecstep:{K}:{Nq}:full")["us"])
        print(f"  K{K} Nq{Nq}: folded head {fold:.1f} us; full quantile layer + torch mean ({args.envs * Nq * K * K * 4 / 1e6:.0f} MB of atoms) "
              f"{full:.1f} us; {full / fold:.1f} x")


if __name__ == "__main__":
    main()
