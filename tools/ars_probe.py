#!/usr/bin/env python3
"""ARS on the MI355X. No pass / fail threshold. One process per configuration, each under its own time limit:

  * milliseconds per update on the kernel path (one population launch, one update launch, one read of six doubles) for LinearPolicy and
    MlpPolicy [64, 64] at n_delta in {8, 256, 2048} on CSTRVecEnv(2 * n_delta) (every candidate in parallel), class defaults otherwise
    (400-step episodes, n_eval_episodes 1). Wall clock over `--updates` updates between two device synchronisations, median of five
    rounds; env-steps/s from the same rounds;
  * device time of each of the two launches in the same configurations (HIP events around the call, median of `--updates` calls);
  * the same update on the published-statement path (`fused_learner = False`: 2 n_delta sequential evaluate_policy calls, the update in
    torch) at n_delta = 8, the only comparison that exists.

usage:  ars_probe.py [--updates 20]            (writes the report to stdout)
        ars_probe.py --child <spec>            (one configuration, one JSON line; used by the parent)
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

SPECS = tuple(f"{pol}:{nd}:kernel" for pol in ("LinearPolicy", "MlpPolicy") for nd in (8, 256, 2048)) + ("LinearPolicy:8:published", "MlpPolicy:8:published")
ROUNDS, CHILD_LIMIT = 5, 240


def child(spec: str, updates: int) -> dict:
    import torch as th

    from core import ARS
    from core.common.logger import Logger
    from core.common.vec_env import CSTRVecEnv

    policy, nd, path = spec.split(":")
    nd = int(nd)
    model = ARS(policy, CSTRVecEnv(2 * nd), n_delta=nd, seed=0, zero_policy=False)
    model.set_logger(Logger(folder=None, output_formats=[]))
    assert model.fused_learner
    model.fused_learner = path == "kernel"
    if path != "kernel":
        updates = 2
    per_update = 2 * nd * int(model.env.coef.max_steps)
    model.learn(per_update * 2)  # warm-up: allocator, first launches
    rounds = []
    for _ in range(ROUNDS if path == "kernel" else 2):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        before = model._n_updates
        model.learn(per_update * updates, reset_num_timesteps=False)
        th.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3 / max(model._n_updates - before, 1))
    out = dict(ms=rounds, per_update=per_update, device=th.cuda.get_device_name(0), fused=bool(model.fused_learner), n_params=model.n_params)
    if path == "kernel":  # device time of the two launches
        from core.common import hip_ops

        real = hip_ops.ars_population, hip_ops.ars_update
        times = {"population": [], "update": []}

        def timed(name, fn):
            def run(*a, **k):
                e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                e0.record()
                fn(*a, **k)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
            return run

        hip_ops.ars_population, hip_ops.ars_update = timed("population", real[0]), timed("update", real[1])
        try:
            model.learn(per_update * updates, reset_num_timesteps=False)
        finally:
            hip_ops.ars_population, hip_ops.ars_update = real
        out["population_us"], out["update_us"] = statistics.median(times["population"]), statistics.median(times["update"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.updates)))
        return
    print(f"ARS probe: {a.updates} updates per round, median of {ROUNDS} rounds; CSTRVecEnv(2 * n_delta), 400-step episodes, n_eval_episodes 1")
    for spec in SPECS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, "--updates", str(a.updates)], capture_output=True,
                               text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{spec}: no result within {CHILD_LIMIT} s; stopping")
            break
        if r.returncode != 0:
            print(f"{spec}: child failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
            break
        d = json.loads(r.stdout.strip().splitlines()[-1])
        ms = statistics.median(d["ms"])
        line = (f"{spec:28s} P = {d['n_params']:5d}  {ms:10.3f} ms / update  (rounds {', '.join(f'{x:.3f}' for x in d['ms'])})  "
                f"{d['per_update'] / ms * 1e3:14.0f} env-steps/s")
        if "population_us" in d:
            line += f"  device: population {d['population_us']:.1f} us, update {d['update_us']:.1f} us"
        print(line, flush=True)
    print("device:", d.get("device") if "d" in dir() else "?")


if __name__ == "__main__":
    main()
