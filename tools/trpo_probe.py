#!/usr/bin/env python3
"""TRPO on the MI355X. No pass / fail threshold. One process per size, each under its own time limit, the next one only after the last
one succeeded:

  * milliseconds per train() on the kernel path and on the torch path (`fused_learner = False`: the published statements, the
    Fisher-vector product by double backward) of the SAME model on the SAME filled rollout buffer in the same process, alternating,
    every round from the same weights and optimiser state. Class defaults on CSTRVecEnv(8): R = 16384 rows (n_steps 2048), and a second
    size R = 2048 (n_steps 256). Wall clock between two device synchronisations; two warm-up rounds per path, median of `--rounds`;
  * device time per Fisher-vector product (tangent pass, head metric, backward, the CG launch; HIP events around the calls, median
    of 50) and per tangent-layer launch (each of the actor's three layers);
  * ABI calls (launching entry points) per product and per train().

usage:  trpo_probe.py [--rounds 5] [--out profiles/trpo_probe.txt]
        trpo_probe.py --child <rows>            (one size, one JSON line; used by the parent)
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)

SIZES = (16384, 2048)
N_ENVS, CHILD_LIMIT = 8, 420


def _events(fn, reps: int = 50) -> float:
    import torch as th

    fn()
    th.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def child(rows: int, rounds: int) -> dict:
    import torch as th

    from core import TRPO
    from core import _native as nv
    from core.common import hip_ops
    from core.common.logger import Logger
    from core.common.vec_env import CSTRVecEnv

    model = TRPO("MlpPolicy", CSTRVecEnv(N_ENVS), n_steps=rows // N_ENVS, seed=0)
    model.set_logger(Logger(folder=None, output_formats=[]))
    assert model.fused_learner
    _, cb = model._setup_learn(rows, None)
    assert model.collect_rollouts(model.env, cb, model.rollout_buffer, model.n_steps)
    arena, opt = model.policy.arena, model.policy.optimizer
    state = (arena.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ctl.clone())

    def one(fused: bool):
        for dst, src in zip((arena.flat, opt.exp_avg, opt.exp_avg_sq, opt.ctl), state):
            dst.copy_(src)
        model.fused_learner = fused
        th.cuda.synchronize()
        calls, t0 = nv.ABI_CALLS[0], time.perf_counter()
        model.train()
        th.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, nv.ABI_CALLS[0] - calls, model.logger.name_to_value["train/is_line_search_success"]

    for _ in range(2):  # warm-up of both paths: allocator, first launches, autograd's graphs
        one(True), one(False)
    ms = {True: [], False: []}
    for _ in range(rounds):
        for fused in (True, False):
            t, calls, ok = one(fused)
            ms[fused].append(t)
            if fused:
                train_calls, success = calls, ok
    # one product in isolation, on the kernel path's own buffers
    model.fused_learner = True
    with th.cuda.device(model.device):
        obs = model._batch()[0]
        acts = model._actor_forward(obs)
        head, b, vec = model._head_of(model._fast), model._rows(obs.shape[0]), model._vec
        hip_ops.trpo_x0(vec["p"], model._mask, 1.0, model._x0_stream())
        vec["g"].copy_(vec["p"])

        def product():
            model._fvp_fused(vec["p"], acts, head, b)
            hip_ops.trpo_cg_step(nv.TRPO_CG_INIT, vec["x"], vec["r"], vec["theta0"], arena.grad, vec["g"], model.cg_damping, 1e-10, model._ctl)

        arena.grad.zero_()
        calls = nv.ABI_CALLS[0]
        product()
        fvp_calls = nv.ABI_CALLS[0] - calls
        fvp_us = _events(product)
        tangent_us, x_dot = [], None
        for i, (lin, act) in enumerate(model._fast.pi_layers):
            w = lin.weight.detach()
            args = (acts[i], x_dot, w, th.ones_like(w), th.ones_like(lin.bias.detach()), acts[i + 1], act)
            tangent_us.append((tuple(w.shape), _events(lambda a=args: hip_ops.linear_tangent_fwd(*a))))
            x_dot = hip_ops.linear_tangent_fwd(*args)
        arena.grad.zero_()
    return dict(rows=rows, kernel_ms=ms[True], torch_ms=ms[False], train_calls=train_calls, fvp_calls=fvp_calls, fvp_us=fvp_us,
                tangent_us=tangent_us, line_search_success=success, device=th.cuda.get_device_name(0), n_actor=model._n_actor,
                products=model.cg_max_steps + 2, critic_minibatches=model.n_critic_updates * -(-rows // model.batch_size))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trpo_probe.txt"))
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rounds)))
        return
    lines = [f"TRPO probe, {datetime.date.today().isoformat()}: class defaults on CSTRVecEnv({N_ENVS}) (batch_size 128, cg_max_steps 15, n_critic_updates 10, "
             f"MlpPolicy [64, 64] tanh), one filled rollout buffer, every round from the same weights; median of {a.rounds} rounds after 2 warm-up rounds per path"]
    d = None
    for rows in SIZES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows), "--rounds", str(a.rounds)], capture_output=True,
                               text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"R = {rows}: no result within {CHILD_LIMIT} s; stopping")
            break
        if r.returncode != 0:
            lines.append(f"R = {rows}: child failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
            break
        d = json.loads(r.stdout.strip().splitlines()[-1])
        k, t = statistics.median(d["kernel_ms"]), statistics.median(d["torch_ms"])
        lines.append(f"R = {rows:5d}  train(): kernel path {k:9.2f} ms (rounds {', '.join(f'{x:.2f}' for x in d['kernel_ms'])}), torch path {t:9.2f} ms "
                     f"(rounds {', '.join(f'{x:.2f}' for x in d['torch_ms'])}), torch / kernel = {t / k:.2f}")
        lines.append(f"           {d['products']} Fisher-vector products over {d['n_actor']} actor parameters, {d['critic_minibatches']} critic minibatches, "
                     f"line search success {d['line_search_success']}; ABI calls: {d['fvp_calls']} per product (CG launch included), {d['train_calls']} per train()")
        lines.append(f"           device time: {d['fvp_us']:.1f} us per product; tangent layers "
                     + ", ".join(f"{tuple(s)}: {us:.1f} us" for s, us in d["tangent_us"]))
        print("\n".join(lines[-3:]), flush=True)
    lines.append(f"device: {d['device'] if d else '?'}")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(lines[0] + "\n" + lines[-1])


if __name__ == "__main__":
    main()
