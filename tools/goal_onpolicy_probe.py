#!/usr/bin/env python3
"""Times PPO and A2C on the goal face beside the Box face. Starts profiles/goal_onpolicy_probe.txt afresh (header and conditions
included).

    python tools/goal_onpolicy_probe.py

Two sections:
  * per-launch times of cstr_goal_rollout_add_f32 / cstr_goal_ppo_gather_f32 (6-float rows as three float2) beside
    cstr_rollout_add_f32 / cstr_ppo_gather_f32 on a width-4 buffer (one float4), same shapes and operands;
  * the eager iteration time (one rollout + train()) of PPO (32 envs x 64 steps, batch 512) and A2C (4096 envs x 5 steps) with
    "MultiInputPolicy" on CSTRVecEnv(goal_conditioned=True) beside "MlpPolicy" on the Box face.

Protocol: warm-up runs first; a launch is timed as a batch of back-to-back launches between two device synchronisations, divided by
the batch length (the add's buffer is reset between batches, outside the timed region); an iteration is timed between two device
synchronisations; the median of the repetitions is reported with the fastest and slowest beside it.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd"), ROOT):
    if p not in sys.path:
        sys.path.append(p)

import torch as th  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "goal_onpolicy_probe.txt")
GOAL_RANGE = (0.10, 0.40)
DEV = "cuda:0"


def emit(line: str) -> None:
    print(line)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def stats(xs: list) -> str:
    return f"median {statistics.median(xs) * 1e6:9.2f} us  (min {min(xs) * 1e6:9.2f}, max {max(xs) * 1e6:9.2f})"


def timed_batches(fn, per_batch: int, reps: int, warmup: int, before=None) -> list:
    out = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(per_batch):
            fn()
        th.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) / per_batch)
    return out


def probe_launches(reps: int, warmup: int) -> None:
    from core.common import hip_ops as ops

    emit("# -- launches: add (one row of n_envs) and gather (batch rows), goal face (obs_dim 6) beside the Box face (obs_dim 4)")
    for n, T in ((32, 64), (4096, 5), (65536, 5)):
        z = lambda *s: th.randn(*s, device=DEV)  # noqa: E731
        operands = dict(act=z(n, 2), rew=z(n), val=z(n), logp=z(n), tout=(th.rand(n, device=DEV) < 0.1).float(), tv=z(n))
        operands["done"] = operands["tout"].clone()
        for face, d in (("goal", 6), ("box", 4)):
            rb = ops.DeviceRollout(T, n, d, 2, DEV, goal=face == "goal")
            obs, start = z(n, d), th.ones(n, device=DEV)
            ep_ret, ep_len, st = th.zeros(n, device=DEV), th.zeros(n, dtype=th.int32, device=DEV), th.zeros(4, dtype=th.float64, device=DEV)
            add = ops.goal_rollout_add if face == "goal" else ops.rollout_add
            o = operands
            ts = timed_batches(lambda: add(rb, obs, o["act"], o["rew"], start, o["val"], o["logp"], o["tout"], o["tv"], 0.99, o["done"], ep_ret, ep_len, st),
                               T, reps, warmup, before=rb.ctl.zero_)
            emit(f"add    {face:4s} n_envs {n:6d} rows {T:3d}: {stats(ts)}")
        for batch in sorted({min(512, n * T), n * T}):
            idx = th.randperm(n * T, device=DEV)[:batch].contiguous()
            for face, d in (("goal", 6), ("box", 4)):
                rb = ops.DeviceRollout(T, n, d, 2, DEV, goal=face == "goal")
                e = lambda *s: th.empty(*s, device=DEV)  # noqa: E731
                out = (e(batch, d), e(batch, 2), e(batch), e(batch), e(batch), e(batch))
                gather = ops.goal_ppo_gather if face == "goal" else ops.ppo_gather
                ts = timed_batches(lambda: gather(rb, idx, *out), 20, reps, warmup)
                emit(f"gather {face:4s} n_envs {n:6d} rows {T:3d} batch {batch:7d}: {stats(ts)}")


def probe_iterations(reps: int, warmup: int) -> None:
    from core.a2c import A2C
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    emit("# -- eager iterations (collect_rollouts + train), seeded models at the class-default widths")
    cases = (("PPO", PPO, 32, dict(n_steps=64, batch_size=512)), ("A2C", A2C, 4096, dict(n_steps=5)))
    for name, cls, n, kw in cases:
        for face in ("goal", "box"):
            env = CSTRVecEnv(n, device=DEV, goal_conditioned=True, goal_range=GOAL_RANGE) if face == "goal" else CSTRVecEnv(n, device=DEV)
            model = cls("MultiInputPolicy" if face == "goal" else "MlpPolicy", env, seed=0, device=DEV, **kw)
            assert model.fused_learner and model._device_rollout()
            _, cb = model._setup_learn(10 ** 9, None)

            def iteration():
                model.collect_rollouts(model.env, cb, model.rollout_buffer, model.n_steps)
                model.train()

            ts = timed_batches(iteration, 1, reps, warmup)
            ms = [t * 1e3 for t in ts]
            emit(f"{name} {face:4s} {n:5d} envs x {kw['n_steps']:3d} steps: median {statistics.median(ms):8.3f} ms  (min {min(ms):8.3f}, max {max(ms):8.3f})"
                 f"  = {n * kw['n_steps'] / statistics.median(ts):12.0f} env steps/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()  # a fresh file: the lines of an older run are not mixed with this one's
    emit(f"# tools/goal_onpolicy_probe.py on {th.cuda.get_device_name(0)}, torch {th.__version__}")
    emit(f"# reps {args.reps}, warm-up {args.warmup}; every timed region between two device synchronisations; times are wall-clock and include")
    emit("# the host's launch overhead (the add and gather launches are latency-bound at these sizes)")
    probe_launches(args.reps, args.warmup)
    probe_iterations(args.reps, args.warmup)
