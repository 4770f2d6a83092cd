#!/usr/bin/env python3
"""TD3+BC on the MI355X beside BCQ and the online TD3's per-layer gradient step, class defaults ((400, 300), batch 256): ABI launches per
gradient step (without / with the delayed actor step), ms per gradient step with eager launches and replayed from hipGraphs (one graph
per residue of the update counter; 1 and 8 gradient steps per graph), and the distance between `evaluate_policy_fused` and
`evaluate_policy` for a TD3BC model with and without the folded state normalisation next to a plain TD3's.

Every timed figure is the median over the rounds of `--alternations` processes per configuration, the configurations' processes taking
turns (a, b, c, ..., a, b, c, ...): one round = `--steps` gradient steps between two device synchronisations. TD3BC and BCQ run their own
learn() loops (OfflineAlgorithm: an iteration IS a gradient step). The online TD3 has a rollout in its iteration, so its gradient step
is timed alone: train(1, 256) calls on a filled buffer with the row-chain kernels switched off (the per-layer path TD3BC shares), and,
for the replayed figures, the same call recorded by this tool into one graph per residue.

usage:  td3bc_probe.py [--alternations 2] [--steps 512] [--rows 100000]            (writes the report to stdout)
        td3bc_probe.py --child <algo>:<mode>                                       (one configuration, one JSON line; used by the parent)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)

ALGOS, MODES, BATCH, ROUNDS = ("td3bc", "bcq", "td3"), ("eager", "graph1", "graph8"), 256, 5


def dataset(rows: int, device):
    from bcq_probe import dataset as bcq_dataset

    return bcq_dataset(rows, device)


def _offline(algo: str, rows: int, mode: str):
    from core.common.vec_env import CSTRVecEnv

    if algo == "td3bc":
        from core.td3bc import TD3BC as cls
    else:
        from core.bcq import BCQ as cls
    model = cls("MlpPolicy", CSTRVecEnv(1), dataset=dataset(rows, "cuda"), seed=0)
    if mode != "eager":
        model.enable_graph_capture(True, unroll=int(mode[5:]))
    return model


def _online_td3():
    """TD3 with a filled buffer, per-layer gradient steps (the path TD3BC shares)"""
    from core.common import chain
    from core.common.vec_env import CSTRVecEnv
    from core.td3 import TD3

    chain.USE_CHAIN = False
    model = TD3("MlpPolicy", CSTRVecEnv(64), seed=0, batch_size=BATCH, buffer_size=64 * 512, learning_starts=64 * 16)
    model.learn(64 * 32)
    assert model.fused_learner and model._chain_for(BATCH) is None
    model._n_updates -= model._n_updates % 2
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
    if algo in ("td3bc", "bcq"):
        model = _offline(algo, rows, mode)
        model.learn(96)  # allocator, graph warm-up iterations and captures
        if mode == "eager":
            assert model._n_updates % 2 == 0
            out["launches"] = [_abi_calls(lambda: model.train(1, BATCH)), _abi_calls(lambda: model.train(1, BATCH))]
        out["ms"] = _rounds(lambda n: model.learn(n, reset_num_timesteps=False), steps)
        st = model.graph_status()
        out.update(replays=st["replays"], eager_iterations=st["eager_iterations"], error=st["error"])
        return out
    model = _online_td3()

    def one():
        model._train_device_only(1, BATCH)
        model._n_updates += 1

    model.policy.set_training_mode(True)
    for _ in range(8):
        one()
    if mode == "eager":
        out["launches"] = [_abi_calls(one), _abi_calls(one)]
        out["ms"] = _rounds(lambda n: [one() for _ in range(n)], steps)
        return out
    unroll = int(mode[5:])
    graphs = []
    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(4):
            one()
    th.cuda.current_stream().wait_stream(side)
    for _ in range(2 if unroll % 2 else 1):  # one graph per residue of the update counter an unrolled body starts at
        g = th.cuda.CUDAGraph()
        with th.cuda.graph(g):
            for _ in range(unroll):
                one()
        graphs.append(g)
    assert steps % (unroll * len(graphs)) == 0

    def replay(n):
        for _ in range(n // (unroll * len(graphs))):
            for g in graphs:
                g.replay()

    replay(unroll * len(graphs) * 4)
    out["ms"] = _rounds(replay, steps)
    return out


def eval_distances() -> list:
    """worst |evaluate_policy_fused - evaluate_policy| episode return: plain TD3, TD3BC raw, TD3BC with the folded normalisation"""
    import numpy as np

    from core.common.evaluation import evaluate_policy, evaluate_policy_fused
    from core.common.vec_env import CSTRVecEnv
    from core.td3 import TD3
    from core.td3bc import TD3BC

    class Short(CSTRVecEnv):
        max_steps = 20

    def both(model):
        rets = []
        for fn in (evaluate_policy, evaluate_policy_fused):
            env = Short(4)
            env.seed(21)
            rets.append(np.asarray(fn(model, env, n_eval_episodes=8, return_episode_rewards=True, warn=False)[0], np.float64))
        return float(np.abs(rets[0] - rets[1]).max()), float(rets[0].mean())

    pk = dict(net_arch=[64, 64])
    lines = []
    d, mean = both(TD3("MlpPolicy", CSTRVecEnv(1), seed=0, policy_kwargs=pk))
    lines.append(f"  plain TD3                       : {d:.3e} (returns around {mean:.3f})")
    for normalize in (False, True):
        m = TD3BC("MlpPolicy", CSTRVecEnv(1), dataset=dataset(4096, "cuda"), seed=0, batch_size=64, policy_kwargs=pk, normalize_states=normalize)
        d, mean = both(m)
        lines.append(f"  TD3BC normalize_states={str(normalize):5s}    : {d:.3e} (returns around {mean:.3f})")
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--child", default=None)
    ap.add_argument("--eval-distances", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.steps, args.rows)))
        return
    if args.eval_distances:
        print("\n".join(eval_distances()))
        return
    specs = [f"{a}:{m}" for a in ALGOS for m in MODES]
    results = {s: [] for s in specs}
    for _ in range(args.alternations):
        for s in specs:  # the configurations' processes take turns; a failing child ends the probe
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s, "--steps", str(args.steps), "--rows", str(args.rows)],
                                 check=True, stdout=subprocess.PIPE, text=True, timeout=240)
            results[s].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f"{s}: {statistics.median(results[s][-1]['ms']):.4f} ms", file=sys.stderr, flush=True)
    first = results[specs[0]][0]
    print(f"TD3+BC beside BCQ and the online TD3's per-layer gradient step; class defaults, batch {BATCH}, dataset of {args.rows} rows, {first['device']}")
    print(f"ms per gradient step: median (max - min) over {ROUNDS * args.alternations} rounds of {args.steps} steps from {args.alternations} "
          "alternating processes per configuration")
    names = dict(td3bc="TD3BC", bcq="BCQ", td3="TD3 (online, per-layer gradient step alone)")
    modes = dict(eager="eager launches", graph1="hipGraph replay, 1 step per graph", graph8="hipGraph replay, 8 steps per graph")
    for a in ALGOS:
        lau = results[f"{a}:eager"][0]["launches"]
        print(f"{names[a]}: ABI launches per gradient step {lau[0]} without / {lau[1]} with the delayed actor step")
        for m in MODES:
            rs = results[f"{a}:{m}"]
            ms = [v for r in rs for v in r["ms"]]
            extra = ""
            if "replays" in rs[0]:
                extra = f"  (replays {rs[0]['replays']}, eager iterations {rs[0]['eager_iterations']}, error {rs[0]['error']})"
            print(f"  {modes[m]:36s}: {statistics.median(ms):.4f} ms ({max(ms) - min(ms):.4f}){extra}")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval-distances"], check=True, stdout=subprocess.PIPE, text=True, timeout=240)
    print("worst |evaluate_policy_fused - evaluate_policy| episode return, (64, 64) networks, 8 episodes of 20 steps on 4 envs:")
    print(res.stdout.rstrip())


if __name__ == "__main__":
    main()
