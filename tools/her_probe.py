#!/usr/bin/env python3
"""HER launches on the MI355X, at the shape of a 1 M-transition buffer on 4096 envs (a 244 x 4096 ring): microseconds per launch of
  * cstr_her_sample_f32 at B = 256 for the three strategies, beside cstr_replay_sample_mt19937_f32 at the same shape (existing code);
  * cstr_her_add_f32 beside cstr_replay_add_f32, both through their hip_ops wrappers on prepared tensors;
  * step_device on the goal face (cstr_goal_vec_step_f32) beside step_device on the Box face (cstr_vec_step_f32 + cstr_reset_draw_f32
    and two device copies): wrapper calls, not kernel times;
  * the goal face's fused collect launch (cstr_goal_collect_step_f32) beside the sequence it replaces: the element-wise action chain,
    the row copy, step_device, add_device and the statistics ops of CSTR_HER_FUSED_COLLECT=0;
  * the SAC iteration (one vec-step + one gradient step, class defaults, per-layer learner) with HER on the goal face: eager with
    CSTR_HER_FUSED_COLLECT 0 and 1, replayed from hipGraphs at unroll 1 and 8 (with the graph's launches per iteration from
    `graph_status()`), beside the eager Box face (CSTR_CHAIN=0).

Every figure is host wall-clock per Python call, not a kernel duration: the time of `--launches` back-to-back calls (200 iterations)
between two device synchronisations, divided by their number, median of five rounds. The kernels are launch-latency-bound, so this is
the per-launch cost inside a stream of launches. There is no pass / fail threshold.

Every iteration figure comes from a process of its own (`--iteration MODE` is what such a process runs). With `--parent TREE`, a built
checkout of the parent commit, that tree's eager goal-face iteration is measured too, by the same code importing the package from TREE,
in processes that alternate with this tree's (parent, this, parent, this, ...; `--alternations` of each): a figure is then the median of
all rounds of its processes, its spread their max - min, and the two comparisons with the parent are printed with both.

Episodes are shortened to 100 steps with uneven starts so that the ring holds finished episodes of every phase (a 400-step episode is
longer than the 244-row ring).

usage:
  her_probe.py [--envs 4096] [--rows 244] [--batch 256] [--launches 2000] [--parent TREE] [--alternations 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERATION_MODES = ("eager", "eager-elementwise", "replay1", "replay8", "box")


def use_tree(root: str) -> None:
    for p in (root, os.path.join(root, "pytorch-rl-enhancedstablebaselines_amd")):
        sys.path.insert(0, p)


def timed(fn, launches: int) -> float:
    import torch as th

    for _ in range(20):
        fn()
    rounds = []
    for _ in range(5):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            fn()
        th.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e6 / launches)
    return sorted(rounds)[2]


def sac_iteration(mode: str, n: int) -> dict:
    """us per SAC iteration (one vec-step + one gradient step) at the class defaults, per-layer learner (no row chain): five rounds of 200"""
    import torch as th

    from core import _native as nv
    from core.common import chain
    from core.common import off_policy_algorithm as opa
    from core.common.logger import Logger
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer
    from core.sac import SAC

    chain.USE_CHAIN = False  # CSTR_CHAIN=0: the same per-layer learner on both faces
    goal = mode != "box"
    if mode == "eager-elementwise":
        opa.HER_FUSED_COLLECT = False
    env = CSTRVecEnv(n, goal_conditioned=True, goal_range=(0.10, 0.40)) if goal else CSTRVecEnv(n)
    env.coef = nv.default_coef(0.20, 0.05, 0.45, 100)
    kw = dict(replay_buffer_class=HerReplayBuffer) if goal else {}
    model = SAC("MultiInputPolicy" if goal else "MlpPolicy", env, seed=0, learning_starts=n * 110, **kw)
    model.set_logger(Logger(folder=None, output_formats=[]))
    if mode.startswith("replay"):
        model.enable_graph_capture(True, unroll=int(mode[len("replay"):]))
    model.learn(n * 150)
    rounds = []
    for _ in range(5):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        model.learn(n * 200, reset_num_timesteps=False)
        th.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e6 / 200)
    st = model.graph_status()
    if mode.startswith("replay") and not (st["active"] and st["error"] is None and st["replays"] >= 1000):
        raise RuntimeError(f"the iterations were not replayed: {st}")
    return dict(rounds=rounds, replays=st["replays"], launches=st["abi_launches_per_iteration"])


def iteration_process(tree: str, mode: str, n: int) -> dict:
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--iteration", mode, "--envs", str(n)], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def summary(runs: list) -> tuple:
    """(median of all rounds, max - min of all rounds) of one configuration's processes"""
    rounds = sorted(r for run in runs for r in run["rounds"])
    return rounds[len(rounds) // 2], rounds[-1] - rounds[0]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=244)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its eager goal-face iteration is measured in alternation")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--iteration", choices=ITERATION_MODES, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    use_tree(args.tree)
    if args.iteration is not None:  # one configuration's process
        print(json.dumps(sac_iteration(args.iteration, args.envs)))
        sys.exit(0)
    import numpy as np
    import torch as th

    from core import _native as nv
    from core.common.buffers import ReplayBuffer
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer
    from core.her.goal_selection_strategy import KEY_TO_GOAL_STRATEGY

    n, rows, B = args.envs, args.rows, args.batch
    print(f"HER launches, {rows} x {n} ring, batch {B}, {th.cuda.get_device_name(0)}; us per launch, median of 5 rounds of {args.launches}")
    genv, benv = CSTRVecEnv(n, goal_conditioned=True, goal_range=(0.10, 0.40)), CSTRVecEnv(n)
    for env in (genv, benv):
        env.coef = nv.default_coef(0.20, 0.05, 0.45, 100)
        env.seed(0)
        env.reset_device()
        env.step_count.copy_(th.from_numpy(np.random.default_rng(0).integers(0, 100, n).astype(np.int32)))
    her = HerReplayBuffer(rows * n, genv.observation_space, genv.action_space, genv, n_envs=n)
    rb = ReplayBuffer(rows * n, benv.observation_space, benv.action_space, n_envs=n)
    her.seed_sampler(0), rb.seed_sampler(0)
    act = (th.rand(n, 2, device="cuda") * 2 - 1).contiguous()
    flat = genv.flat.clone()
    for _ in range(rows + 50):  # fill both rings through one wrap
        flat.copy_(genv.flat)
        _, rew, done, tout, nxt = genv.step_device(act)
        her.add_device(flat, nxt, act, rew, done, tout)
        prev = benv.obs.clone()
        _, rew_b, done_b, tout_b, nxt_b = benv.step_device(act)
        rb.add(prev, nxt_b, act, rew_b, done_b, tout_b)
    print(f"  valid transitions: {int((her.ep_length > 0).sum())} of {rows * n}")
    out, out_b = her.alloc_batch(B), rb.alloc_batch(B)
    for strategy in ("future", "final", "episode"):
        her.goal_selection_strategy = KEY_TO_GOAL_STRATEGY[strategy]
        print(f"  cstr_her_sample_f32 ({strategy:7s}, {her.nb_virtual(B)} virtual)   : {timed(lambda: her.sample_into(out), args.launches):8.2f}")
    from core.common import hip_ops

    print(f"  cstr_replay_sample_mt19937_f32 (same shape)      : {timed(lambda: rb.sample_into(out_b), args.launches):8.2f}")
    print(f"  cstr_her_add_f32 (hip_ops.her_add)               : {timed(lambda: hip_ops.her_add(her.ring, her.her, flat, nxt, act, rew, done, tout), args.launches):8.2f}")
    print(f"  cstr_replay_add_f32 (hip_ops.replay_add)         : {timed(lambda: hip_ops.replay_add(rb.ring, prev, nxt_b, act, rew_b, done_b, tout_b), args.launches):8.2f}")
    print(f"  step_device, goal face (1 launch)                : {timed(lambda: genv.step_device(act), args.launches):8.2f}")
    print(f"  step_device, Box face (2 launches + 2 copies)    : {timed(lambda: benv.step_device(act), args.launches):8.2f}")

    # the vec-step behind the policy output `act`: one launch against the launches of CSTR_HER_FUSED_COLLECT=0 (off_policy_algorithm.py)
    lo, hi = th.full((2,), -1.0, device="cuda"), th.full((2,), 1.0, device="cuda")
    ep_return, ep_len = th.zeros(n, device="cuda"), th.zeros(n, device="cuda")
    ep_stats = th.zeros(4, dtype=th.float64, device="cuda")
    adv = th.zeros(nv.RNG_CTL_WORDS, dtype=th.int64, device="cuda")

    def elementwise_collect():
        adv[1] += n
        v = lo + (0.5 * (act + 1.0) * (hi - lo))
        sc = (2.0 * ((v - lo) / (hi - lo)) - 1.0).contiguous()
        ea = (lo + (0.5 * (sc + 1.0) * (hi - lo))).contiguous()
        flat.copy_(genv.flat)
        _, r, d, to, nx = genv.step_device(ea)
        her.add_device(flat, nx, sc, r, d, to)
        ret, length = ep_return + r, ep_len + 1.0
        ep_stats[0] += d.sum().double()
        ep_stats[1] += (ret * d).sum().double()
        ep_stats[2] += (length * d).sum().double()
        ep_return.copy_(ret * (1.0 - d))
        ep_len.copy_(length * (1.0 - d))

    def fused_collect():
        genv.collect_step_device(her.ring, her.her, act, 1, [-1.0, -1.0], [1.0, 1.0], ep_return=ep_return, ep_stats=ep_stats, rng_advance=(adv, n))

    print(f"  collect step, goal face, element-wise sequence   : {timed(elementwise_collect, args.launches):8.2f}")
    print(f"  collect step, goal face, cstr_goal_collect_step  : {timed(fused_collect, args.launches):8.2f}")
    del her, rb, genv, benv
    th.cuda.synchronize()

    # iterations: a process per configuration and repetition, the parent's (if given) alternating with this tree's
    modes = ("eager", "eager-elementwise", "replay1", "replay8")
    runs = {m: [] for m in modes + ("parent",)}
    reps = args.alternations if args.parent else 1
    for _ in range(reps):
        if args.parent:
            runs["parent"].append(iteration_process(args.parent, "eager", n))
        for m in modes:
            runs[m].append(iteration_process(ROOT, m, n))
    box = iteration_process(ROOT, "box", n)
    print(f"SAC iteration, us; median and spread (max - min) of {5 * reps} rounds of 200 iterations from {reps} process(es) per line")
    label = {"parent": "parent commit, eager, goal face + HER", "eager": "eager, goal face + HER (fused collect launch)",
             "eager-elementwise": "eager, goal face + HER, CSTR_HER_FUSED_COLLECT=0", "replay1": "replayed, goal face + HER, unroll 1",
             "replay8": "replayed, goal face + HER, unroll 8"}
    fig = {}
    for m in (("parent",) if args.parent else ()) + modes:
        fig[m] = summary(runs[m])
        extra = f"   launches per iteration {runs[m][0]['launches']}" if m.startswith("replay") else ""
        per_process = " ".join(f"{sorted(run['rounds'])[2]:.0f}" for run in runs[m])
        print(f"  {label[m]:49s}: {fig[m][0]:8.2f}  spread {fig[m][1]:7.2f}   per process {per_process}{extra}")
    print(f"  {'eager, Box face, CSTR_CHAIN=0':49s}: {summary([box])[0]:8.2f}  spread {summary([box])[1]:7.2f}")
    if args.parent:
        (p, sp), (e, se), (r, sr) = fig["parent"], fig["eager"], fig["replay1"]
        print(f"  replayed (unroll 1) against the parent's eager iteration: {p - r:+.2f} us faster, spread {max(sp, sr):.2f}: "
              f"{'beyond' if p - r > max(sp, sr) else 'WITHIN'} the spread")
        print(f"  eager with the fused launch against the parent's eager iteration: {p - e:+.2f} us faster, spread {max(sp, se):.2f}: "
              f"{'not slower' if e - p <= max(sp, se) else 'SLOWER'} by more than the spread")
