#!/usr/bin/env python3
"""The Categorical head on the MI355X: microseconds per launch of cstr_categorical_act_f32 / cstr_categorical_loss_f32, and the PPO
iteration (one rollout + train()) on the Discrete valve face next to the Gaussian PPO's on the Box face with the same trunks.

A record, not a gate: the code before this head cannot run the discrete case, so there is no earlier figure to hold it to.

usage:
  categorical_probe.py [--rows 4096] [--launches 200] [--envs 32] [--iterations 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)


def timed(fn, reps: int) -> float:
    """milliseconds per call: `reps` calls between two events, the median of five such rounds"""
    import torch as th

    out = []
    for _ in range(5):
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        th.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return sorted(out)[2]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=20)
    args = ap.parse_args()
    import torch as th

    from core.common import hip_ops as ops
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    dev = "cuda:0"
    print(f"python tools/categorical_probe.py   ({th.cuda.get_device_name(0)}; a record, not a gate: the discrete face has no earlier figure)")
    n = args.rows
    for levels in (5, 16):
        m = levels * levels
        g = th.Generator(device=dev).manual_seed(0)
        z = th.randn(n, m, device=dev, generator=g)
        idx, valve, logp = th.empty(n, 1, device=dev), th.empty(n, 2, device=dev), th.empty(n, device=dev)
        ctl = ops.new_rng_ctl(1, dev)
        act = lambda: ops.categorical_act(z, levels, idx, rng_ctl=ctl, valve_out=valve, log_prob=logp)  # noqa: E731
        act()
        e = lambda: th.randn(n, device=dev, generator=g)  # noqa: E731
        values, adv, ret = e(), e(), e()
        old_lp = logp.clone()
        g_z, g_v, ws, scal = th.empty(n, m, device=dev), th.empty(n, device=dev), ops.new_ppo_workspace(dev), th.zeros(6, device=dev)
        loss = lambda: ops.categorical_loss(ops.CAT_PPO, z, levels, idx, values, adv, ret, True, 0.01, 0.5, g_z, g_v, ws,  # noqa: E731
                                            old_log_prob=old_lp, clip_range=0.2, scalars_out=scal)
        loss()
        print(f"  rows {n}, n_actions {m:3d}: cstr_categorical_act_f32 {1e3 * timed(act, args.launches):7.2f} us / launch, "
              f"cstr_categorical_loss_f32 {1e3 * timed(loss, args.launches):7.2f} us / launch (wrapper included)")
    kw = dict(n_steps=64, batch_size=512, n_epochs=4, seed=0, device=dev)
    for name, env in (("Categorical, Discrete(25)", CSTRVecEnv(args.envs, discrete_actions=5, device=dev)), ("Gaussian, Box(2)", CSTRVecEnv(args.envs, device=dev))):
        model = PPO("MlpPolicy", env, **kw)
        assert model.fused_learner and model._device_rollout()
        _, cb = model._setup_learn(10 ** 9, None)

        def iteration():
            model.collect_rollouts(model.env, cb, model.rollout_buffer, model.n_steps)
            model.train()

        iteration()  # warm-up: allocator, step buffers
        ms = timed(iteration, args.iterations)
        print(f"  PPO iteration, {name:26s}: {ms:8.3f} ms ({args.envs} envs, n_steps 64, batch 512, 4 epochs, class-default nets; "
              f"{args.envs * 64 / ms * 1e3:.3g} env-steps/s)")
