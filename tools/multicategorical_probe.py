#!/usr/bin/env python3
"""The MultiCategorical head on the MI355X: microseconds per launch of cstr_multicategorical_act_f32 / cstr_multicategorical_loss_f32
beside the Categorical head's two launches at the same rows and the same K per valve, and the eager PPO and A2C iteration (one rollout
+ train()) on the MultiDiscrete([K, K]) face beside the Discrete(K * K) face with the same trunks.

A record, not a gate. Every figure is the median of `--rounds` rounds of `--launches` calls between two device events, after a
warm-up round; the spread is the least and the greatest round. The two heads alternate round by round, so a drift of the machine
meets both.

usage:
  multicategorical_probe.py [--rows 4096] [--launches 500] [--rounds 9] [--envs 32] [--iterations 10]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)


def one_round(fn, reps: int) -> float:
    """milliseconds per call: `reps` calls between two device events"""
    import torch as th

    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns: dict, reps: int, rounds: int) -> dict:
    """name -> (median, least, greatest) milliseconds per call; one warm-up round each, then the functions take turns"""
    for fn in fns.values():
        one_round(fn, max(reps // 4, 1))
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(one_round(fn, reps))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in out.items()}


def us(t) -> str:
    return f"{1e3 * t[0]:7.2f} us [{1e3 * t[1]:.2f} .. {1e3 * t[2]:.2f}]"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=10)
    args = ap.parse_args()
    import torch as th

    from core.a2c import A2C
    from core.common import hip_ops as ops
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    dev = "cuda:0"
    print(f"python tools/multicategorical_probe.py   ({th.cuda.get_device_name(0)}; a record, not a gate; median [least .. greatest] of "
          f"{args.rounds} rounds of {args.launches} launches, wrapper included, the two heads alternating)")
    n = args.rows
    for K in (5, 16):
        g = th.Generator(device=dev).manual_seed(0)
        e = lambda *s: th.randn(*s, device=dev, generator=g)  # noqa: E731
        values, adv, ret = e(n), e(n), e(n)
        ws, scal = ops.new_ppo_workspace(dev), th.zeros(6, device=dev)
        # the MultiCategorical head: 2 K logits
        zm = e(n, 2 * K)
        pair, valve_m, logp_m = th.empty(n, 2, device=dev), th.empty(n, 2, device=dev), th.empty(n, device=dev)
        ctl_m = ops.new_rng_ctl(1, dev)
        m_act = lambda: ops.multicategorical_act(zm, (K, K), pair, rng_ctl=ctl_m, valve_out=valve_m, log_prob=logp_m)  # noqa: E731
        m_act()
        old_m, gm, gv_m = logp_m.clone(), th.empty(n, 2 * K, device=dev), th.empty(n, device=dev)
        m_loss = lambda: ops.multicategorical_loss(ops.CAT_PPO, zm, (K, K), pair, values, adv, ret, True, 0.01, 0.5, gm, gv_m, ws,  # noqa: E731
                                                   old_log_prob=old_m, clip_range=0.2, scalars_out=scal)
        # the Categorical head: K * K logits
        zc = e(n, K * K)
        idx, valve_c, logp_c = th.empty(n, 1, device=dev), th.empty(n, 2, device=dev), th.empty(n, device=dev)
        ctl_c = ops.new_rng_ctl(1, dev)
        c_act = lambda: ops.categorical_act(zc, K, idx, rng_ctl=ctl_c, valve_out=valve_c, log_prob=logp_c)  # noqa: E731
        c_act()
        old_c, gc, gv_c = logp_c.clone(), th.empty(n, K * K, device=dev), th.empty(n, device=dev)
        c_loss = lambda: ops.categorical_loss(ops.CAT_PPO, zc, K, idx, values, adv, ret, True, 0.01, 0.5, gc, gv_c, ws,  # noqa: E731
                                              old_log_prob=old_c, clip_range=0.2, scalars_out=scal)
        t = alternate({"m_act": m_act, "c_act": c_act, "m_loss": m_loss, "c_loss": c_loss}, args.launches, args.rounds)
        print(f"  rows {n}, K {K:2d}: cstr_multicategorical_act_f32  ({2 * K:3d} logits) {us(t['m_act'])}   cstr_categorical_act_f32  ({K * K:3d} logits) {us(t['c_act'])}")
        print(f"  rows {n}, K {K:2d}: cstr_multicategorical_loss_f32 ({2 * K:3d} logits) {us(t['m_loss'])}   cstr_categorical_loss_f32 ({K * K:3d} logits) {us(t['c_loss'])}")

    def iteration_of(cls, env, **kw):
        model = cls("MlpPolicy", env, seed=0, device=dev, **kw)
        assert model.fused_learner and model._device_rollout()
        _, cb = model._setup_learn(10 ** 9, None)

        def iteration():
            model.collect_rollouts(model.env, cb, model.rollout_buffer, model.n_steps)
            model.train()

        return iteration

    for cls, kw, what in ((PPO, dict(n_steps=64, batch_size=512, n_epochs=4), "n_steps 64, batch 512, 4 epochs"), (A2C, dict(n_steps=5), "n_steps 5")):
        fns = {"MultiCategorical, MultiDiscrete([5, 5])": iteration_of(cls, CSTRVecEnv(args.envs, multi_discrete_actions=5, device=dev), **kw),
               "Categorical, Discrete(25)": iteration_of(cls, CSTRVecEnv(args.envs, discrete_actions=5, device=dev), **kw)}
        t = alternate(fns, args.iterations, args.rounds)
        for name, v in t.items():
            print(f"  {cls.__name__} iteration, {name:40s}: {v[0]:8.3f} ms [{v[1]:.3f} .. {v[2]:.3f}] ({args.envs} envs, {what}, class-default nets; "
                  f"{args.envs * kw['n_steps'] / v[0] * 1e3:.3g} env-steps/s)")
