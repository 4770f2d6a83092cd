#!/usr/bin/env python3
"""RecurrentPPO on the MI355X: train() on the kernel path against the torch-statement path of the same model on the same filled buffer
(one process, alternating, median of five rounds), at the class defaults and at CSTRVecEnv(4096), n_steps=64, batch_size=16384; and device
time per call of the two LSTM launches against torch.nn.LSTM (MIOpen) forward and forward + backward at the same shapes.

usage:
  rppo_probe.py [--out profiles/rppo_probe.txt] [--epochs 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)


def timed(fn, reps: int = 1) -> float:
    import torch as th

    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / reps


def med(v):
    return sorted(v)[len(v) // 2]


def train_ab(envs: int, n_steps: int, batch: int, epochs: int, lines: list) -> None:
    from core.common.vec_env import CSTRVecEnv
    from core.ppo_recurrent import RecurrentPPO

    model = RecurrentPPO("MlpLstmPolicy", CSTRVecEnv(envs), n_steps=n_steps, batch_size=batch, n_epochs=epochs, seed=0)
    _, cb = model._setup_learn(10 ** 9, None)
    model.collect_rollouts(model.env, cb, model.rollout_buffer, n_steps)
    ms = {True: [], False: []}
    for fused in (True, False):  # warm-up: allocator, step buffers
        model.fused_learner = fused
        model.train()
    for _ in range(5):
        for fused in (True, False):
            model.fused_learner = fused
            ms[fused].append(timed(model.train))
    k, t = med(ms[True]), med(ms[False])
    lines.append(f"train(), {envs} envs x {n_steps} steps, batch {batch}, {epochs} epochs, H 256: kernel path {k:.2f} ms, torch statements {t:.2f} ms "
                 f"(x{t / k:.2f}; median of 5 alternating rounds)")


def launch_ab(n_seg: int, length: int, lines: list, h: int = 256, k: int = 4) -> None:
    import torch as th

    from core.common import hip_ops

    dev = "cuda:0"
    r = n_seg * length
    g = th.Generator(device=dev).manual_seed(0)
    rn = lambda *s: th.randn(*s, device=dev, generator=g)  # noqa: E731
    x, es, dout = rn(r, k), th.zeros(r, device=dev), rn(r, h)
    w = (rn(4 * h, k) / 2, rn(4 * h, h) / 16, 0.1 * rn(4 * h), 0.1 * rn(4 * h))
    sh, sc = rn(n_seg, h), rn(n_seg, h)
    segs = hip_ops.LstmSegments([(i * length, length, i) for i in range(n_seg)], dev)
    e = lambda *s: th.empty(*s, device=dev)  # noqa: E731
    out, gates, c_seq, h_prev, dgates = e(r, h), e(r, 4 * h), e(r, h), e(r, h), e(r, 4 * h)
    hn, cn, dh0, dc0 = e(n_seg, h), e(n_seg, h), e(n_seg, h), e(n_seg, h)
    fwd = lambda: hip_ops.lstm_seq_fwd(x, es, *w, sh, sc, segs, hn, cn, out=out, gates=gates, c_seq=c_seq, h_prev=h_prev)  # noqa: E731
    bwd = lambda: hip_ops.lstm_seq_bwd(dout, gates, c_seq, sc, es, w[1], segs, dgates, dh0, dc0)  # noqa: E731
    lstm = th.nn.LSTM(k, h).to(dev)
    xs, douts = x.view(n_seg, length, k).transpose(0, 1).contiguous(), dout.view(n_seg, length, h).transpose(0, 1).contiguous()
    st = (sh[None].contiguous(), sc[None].contiguous())

    def lib_fwd():
        with th.no_grad():
            lstm(xs, st)

    def lib_both():
        y, _ = lstm(xs, st)
        y.backward(douts)

    for f in (fwd, bwd, lib_fwd, lib_both):
        f()
    reps = 20
    a, b, c, d = timed(fwd, reps), timed(bwd, reps), timed(lib_fwd, reps), timed(lib_both, reps)
    lines.append(f"{n_seg} segments x {length} steps, H {h}, K {k}: cstr_lstm_seq_fwd_f32 {a * 1e3:.0f} us, cstr_lstm_seq_bwd_f32 {b * 1e3:.0f} us; "
                 f"nn.LSTM forward {c * 1e3:.0f} us, forward + backward (with its weight gradients) {d * 1e3:.0f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rppo_probe.txt"))
    ap.add_argument("--epochs", type=int, default=2)
    args = ap.parse_args()
    import torch as th

    lines = [f"RecurrentPPO probe, {th.cuda.get_device_name(0)} (tools/rppo_probe.py)"]
    train_ab(1, 128, 128, args.epochs, lines)  # the class defaults on one env: a chunk is one or two segments
    train_ab(4096, 64, 16384, args.epochs, lines)
    for n_seg, length in ((1, 128), (16, 64), (256, 64), (4096, 1)):
        launch_ab(n_seg, length, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)
