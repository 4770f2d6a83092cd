#!/usr/bin/env python3
"""n-step returns on the MI355X. Two sections, written to profiles/nstep_probe.txt; the numbers are recorded, nothing is asserted.

1. Device time per call (device events around `--calls` back-to-back calls, median of five rounds) of the three n-step launches at
   n_steps 3 and 8 beside their one-step counterparts, on the class-default ring (4096 envs, 1 M slots, full), batch 256.
2. Milliseconds per iteration of SAC at class defaults on CSTRVecEnv(4096), replayed from hipGraphs: n_steps 1, 3 and 8 on this tree
   and, with `--parent-tree`, the one-step model of a checkout of the parent commit (its library built), taking turns. A turn is a
   fresh child process (`--turn`) that imports `core` from its tree, warms up 24 iterations and times `--iterations` iterations between
   two device synchronisations; five rounds of turns, the median per configuration.

usage:
  nstep_probe.py [--envs 4096] [--iterations 400] [--calls 200] [--parent-tree DIR] [--out profiles/nstep_probe.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def use_tree(root: str) -> None:
    for p in (root, os.path.join(root, "pytorch-rl-enhancedstablebaselines_amd")):
        sys.path.insert(0, p)


def device_us(fn, calls: int) -> float:
    import torch as th

    for _ in range(10):
        fn()
    rounds = []
    for _ in range(5):
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        th.cuda.synchronize()
        rounds.append(a.elapsed_time(b) * 1e3 / calls)
    return sorted(rounds)[2]


def launches(envs: int, calls: int, batch: int, lines: list) -> None:
    import torch as th

    from core.common import hip_ops
    from core.common.buffers import NStepReplayBuffer
    from core.common.spaces import Box

    g = th.Generator(device="cuda:0").manual_seed(0)
    idx = None
    for n in (1, 3, 8):
        rb = NStepReplayBuffer(1_000_000, Box(-1, 1, (4,)), Box(-1, 1, (2,)), device="cuda:0", n_envs=envs, n_steps=n, gamma=0.99)
        rows = rb.buffer_size
        rb._adds = 3 * rows
        rb.ring.ctl.copy_(th.tensor([7, 1, 0, 3 * rows]))
        rb.rewards.copy_(th.randn(rows, envs, device="cuda:0", generator=g))
        rb.dones.copy_((th.rand(rows, envs, device="cuda:0", generator=g) < 0.0025).float())  # 400-step episodes
        rb.seed_sampler(0)
        if idx is None:
            idx = th.stack([th.randint(0, rows, (batch,), device="cuda:0", generator=g), th.randint(0, envs, (batch,), device="cuda:0", generator=g)]).int().contiguous()
        out, pb = rb.alloc_batch(batch), rb.alloc_packed_batch(batch)
        s = pb.samples

        def gather():
            if n == 1:
                hip_ops.replay_gather_packed(rb.ring, idx, batch, pb.x_data, pb.x_next, pb.x_pi, s.dones, s.rewards)
            else:
                hip_ops.replay_gather_nstep_packed(rb.ring, idx, batch, n, rb.gamma, pb.x_data, pb.x_next, pb.x_pi, s.dones, s.rewards, s.discounts, s.fold)

        lines.append(f"  n_steps {n}: sample {device_us(lambda: rb.sample_into(out), calls):7.2f} us, packed sample "
                     f"{device_us(lambda: rb.sample_packed_into(pb), calls):7.2f} us, gather of drawn indices {device_us(gather, calls):7.2f} us")


def turn(envs: int, iterations: int, n_steps: int) -> None:
    """the child process of one turn: prints `ms launches replays error`"""
    import torch as th

    from core.common.logger import Logger
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    m = SAC("MlpPolicy", CSTRVecEnv(envs), seed=0, learning_starts=envs, **(dict(n_steps=n_steps) if n_steps > 1 else {}))
    m.set_logger(Logger(folder=None, output_formats=[]))
    m.enable_graph_capture(True)
    m.learn(envs * 24)  # warm-up bodies, captures, allocator
    th.cuda.synchronize()
    t0 = time.perf_counter()
    m.learn(envs * iterations, reset_num_timesteps=False)
    th.cuda.synchronize()
    st = m.graph_status()
    print("TURN", (time.perf_counter() - t0) * 1e3 / iterations, st["abi_launches_per_iteration"], st["replays"], st["error"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_probe.txt"))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--turn", type=int, default=0, help="child mode: one timed turn of SAC with this n_steps")
    ap.add_argument("--tree", default=ROOT, help="child mode: the tree `core` is imported from")
    args = ap.parse_args()
    use_tree(args.tree)
    if args.turn:
        turn(args.envs, args.iterations, args.turn)
        sys.exit(0)
    import subprocess

    import torch as th

    lines = [f"n-step returns, {th.cuda.get_device_name(0)}; tools/nstep_probe.py --envs {args.envs} --iterations {args.iterations} --calls {args.calls}",
             f"launches: class-default ring, {args.envs} envs, full, batch {args.batch}; device time per call (n_steps 1 = the one-step launches)"]
    launches(args.envs, args.calls, args.batch, lines)
    configs = [("this tree, n_steps 1", ROOT, 1), ("this tree, n_steps 3", ROOT, 3), ("this tree, n_steps 8", ROOT, 8)]
    if args.parent_tree:
        configs.insert(0, ("parent commit, one-step", os.path.abspath(args.parent_tree), 1))
    rounds, last = {c[0]: [] for c in configs}, {}
    for _ in range(5):
        for name, tree, n in configs:  # taking turns
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--turn", str(n), "--tree", tree, "--envs", str(args.envs),
                                  "--iterations", str(args.iterations)], check=True, capture_output=True, text=True, timeout=120).stdout
            fields = [ln for ln in out.splitlines() if ln.startswith("TURN")][-1].split(None, 2)
            rounds[name].append(float(fields[1]))
            last[name] = fields[2]
    lines.append(f"SAC, class defaults, {args.envs} envs, replayed from hipGraphs: ms / iteration, median of five rounds taking turns "
                 "(a fresh process per turn); then abi_launches_per_iteration, replays, error of the last turn")
    for name, _, _ in configs:
        lines.append(f"  {name:24s}: {sorted(rounds[name])[2]:.4f} ms (rounds {' '.join(f'{r:.4f}' for r in rounds[name])}); {last[name]}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)
