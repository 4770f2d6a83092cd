#!/usr/bin/env python3
"""A2C on the MI355X, class defaults (n_steps 5, RMSprop, nets [64, 64]): ABI calls and milliseconds per iteration (eager launches;
A2C has no hipGraph replay), the gradient step with the buffer evaluated in place next to what `get(None)` alone would add to it
(host permutation, its H2D copy, the gather launch), and the fused clip + RMSprop step against cstr_grad_clip_f32 followed by the
unclipped step on the policy's own arena. Then train() under three optimisers: FlatRMSprop (the default), FlatRMSpropTFLike
(optimizer_class=RMSpropTFLike, eps 1e-5) and RMSpropTFLike itself on the arena's parameter views (a subclass of it, which
make_optimizer treats as any foreign class: the torch-statement path, get(None) included, one ATen launch per tensor and operation).

An ABI call is one kernel launch, except the clipped RMSprop steps and the gradient clip, which are two each.

usage:
  a2c_probe.py [--envs 4096] [--iterations 200]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)


def timed(fn, reps: int) -> float:
    """milliseconds per call, `reps` calls between two events"""
    import torch as th

    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / reps


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    args = ap.parse_args()
    import torch as th

    from core import _native as nv
    from core.a2c import A2C
    from core.common import hip_ops
    from core.common.vec_env import CSTRVecEnv

    model = A2C("MlpPolicy", CSTRVecEnv(args.envs), seed=0)
    _, cb = model._setup_learn(10 ** 9, None)
    collect = lambda: model.collect_rollouts(model.env, cb, model.rollout_buffer, model.n_steps)  # noqa: E731

    def iteration():
        collect()
        model.train()

    for _ in range(3):
        iteration()  # warm-up: allocator, step buffers
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    reps = max(args.iterations // 5, 1)
    ms_iter = med([timed(iteration, reps) for _ in range(5)])
    c0 = nv.ABI_CALLS[0]
    collect()
    c1 = nv.ABI_CALLS[0]
    model.train()
    c2 = nv.ABI_CALLS[0]
    rb = model.rollout_buffer
    get_none = lambda: next(iter(rb.get(None)))  # noqa: E731  what the reference's row order costs: permutation, H2D copy, gather
    get_none()
    t_train, t_get = [], []
    for _ in range(5):  # alternating inside one process
        t_train.append(timed(model.train, reps))
        t_get.append(timed(get_none, reps))
    ms_train, ms_get = med(t_train), med(t_get)
    # the optimiser alone, on the policy's own arena (about 1e4 floats: launch-bound)
    arena, opt, ws = model.policy.arena, model.policy.optimizer, model._ws
    th.manual_seed(0)
    arena.grad.normal_()
    g = opt.param_groups[0]
    fused = lambda: hip_ops.rmsprop(arena.flat, arena.grad, opt.square_avg, opt.lr_dev, g["alpha"], g["eps"], 0.5, ws, model._grad_norm)  # noqa: E731

    def separate():
        hip_ops.grad_clip(arena.grad, 0.5, ws, model._grad_norm)
        hip_ops.rmsprop(arena.flat, arena.grad, opt.square_avg, opt.lr_dev, g["alpha"], g["eps"], None)

    fused(), separate()
    t_fused, t_sep = [], []
    for _ in range(5):
        t_fused.append(timed(fused, 500))
        t_sep.append(timed(separate, 500))
    ms_fused, ms_sep = med(t_fused), med(t_sep)
    steps = args.envs * model.n_steps
    print(f"A2C, class defaults, {args.envs} envs, n_steps {model.n_steps}, arena {arena.numel} floats, {th.cuda.get_device_name(0)}")
    print(f"  iteration      : {ms_iter:.4f} ms ({steps / ms_iter * 1e3:.3g} env-steps/s), {c2 - c0} ABI calls = {c1 - c0} rollout + {c2 - c1} train()")
    print(f"  train()        : {ms_train:.4f} ms in place ({c2 - c1} ABI calls); get(None) alone, which it does not call: {ms_get:.4f} ms "
          "(host permutation, H2D copy, 1 gather launch)")
    print(f"  clip + RMSprop : fused {ms_fused * 1e3:.2f} us (2 launches), cstr_grad_clip_f32 + unclipped step {ms_sep * 1e3:.2f} us (3 launches)")
    # train() under the three optimisers, each model warmed up by three iterations of its own, alternating inside this process
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    class ForeignRMSpropTFLike(RMSpropTFLike):
        """not `RMSpropTFLike` itself, so it runs as any optimiser class a caller passes does"""

    def build(pk):
        m = A2C("MlpPolicy", CSTRVecEnv(args.envs), seed=0, policy_kwargs=pk)
        _, c = m._setup_learn(10 ** 9, None)
        for _ in range(3):
            m.collect_rollouts(m.env, c, m.rollout_buffer, m.n_steps)
            m.train()
        return m

    tf_kw = dict(optimizer_kwargs=dict(eps=1e-5))
    models = [("FlatRMSprop (default)", model), ("FlatRMSpropTFLike", build(dict(optimizer_class=RMSpropTFLike, **tf_kw))),
              ("RMSpropTFLike on the arena views", build(dict(optimizer_class=ForeignRMSpropTFLike, **tf_kw)))]
    times = {name: [] for name, _ in models}
    for _ in range(5):
        for name, m in models:
            times[name].append(timed(m.train, reps))
    print("  train() by optimiser             optimizer class                fused_learner  ABI calls  ms per train()")
    for name, m in models:
        c0 = nv.ABI_CALLS[0]
        m.train()
        calls = nv.ABI_CALLS[0] - c0
        print(f"  {name:<32s} {type(m.policy.optimizer).__name__:<30s} {str(m.fused_learner):<14s} {calls:<10d} {med(times[name]):.4f}")
