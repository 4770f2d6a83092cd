"""The LSTM sequence kernels on the MI355X (csrc/cstr_lstm.hip) against a plain torch step loop with the reset multiply, in float64 on the
CPU: forward outputs, final states and saved tensors; backward dgates and the gradient of the initial state; dW_ih, dW_hh and db through the
existing weight-gradient launch against float64 autograd.

The bar, per tensor: max |kernel - fp64| <= 4 x max |float32 ATen on the CPU (the same loop) - fp64|. A repeated launch leaves the same
bits; the sentinel bands behind every output stay untouched, and so do the rows that belong to no segment.
A recorded run (`-s`: every figure) is profiles/lstm_gpu_tests.txt."""
import numpy as np
import pytest
import torch as th

from _sentinel_bufs import DEV, SENT, Bufs

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 9, 40)  # ragged within one workgroup's 16 segments
# (H, K, segments, force_stream): 17 segments = a partial second workgroup; weight_hh is LDS-resident up to H = 80 in the forward and up to
# H = 96 in the backward, streamed above (80 / 96 / 112: both sides of both thresholds); the last case streams at a resident width
CASES = [(h, k, s, False) for h in (16, 48, 256) for k in (4, 7) for s in (1, 17)] + [(80, 4, 17, False), (96, 4, 17, False), (112, 4, 17, False), (16, 7, 17, True)]


def problem(H, K, S):
    gen = th.Generator().manual_seed(1000 * H + 10 * K + S)
    r = lambda *s: th.randn(*s, generator=gen)  # noqa: E731
    lens = [9] if S == 1 else [LENGTHS[s % 4] for s in range(S)]
    table, row = [], 1  # row 0 and one row behind every fourth segment belong to no segment
    init = th.randperm(S + 3, generator=gen)[:S].tolist()
    for s, n in enumerate(lens):
        table.append((row, n, init[s]))
        row += n + (s % 4 == 3)
    R = row + 1
    es = th.zeros(R)
    for s, (f, n, _) in enumerate(table):  # resets at the first step, the last step, two steps in a row, none
        kind = (s // 4) % 4 if S > 1 else 2
        if kind == 0:
            es[f] = 1
        elif kind == 1:
            es[f + n - 1] = 1
        elif kind == 2 and n > 2:
            es[f + n // 2] = es[f + n // 2 + 1] = 1
    w = dict(w_ih=r(4 * H, K) / np.sqrt(K), w_hh=r(4 * H, H) / np.sqrt(H), b_ih=0.1 * r(4 * H), b_hh=0.1 * r(4 * H))
    return dict(table=table, R=R, es=es, x=r(R, K), dout=r(R, H), state_h=0.5 * r(S + 3, H), state_c=0.5 * r(S + 3, H), **w)


def step_loop(p, dtype):
    """nn.LSTM's statement per step, h and c multiplied by 1 - episode_start first; every tensor the kernels produce, autograd's gradients"""
    t = {k: v.to(dtype).clone().requires_grad_(k in ("w_ih", "w_hh", "b_ih", "b_hh", "state_h", "state_c"))
         for k, v in p.items() if isinstance(v, th.Tensor)}
    H = p["w_hh"].shape[1]
    rows = {k: {} for k in ("out", "gates", "c_seq", "h_prev", "z")}
    hn, cn = [], []
    for f, n, i0 in p["table"]:
        h, c = t["state_h"][i0], t["state_c"][i0]
        for r in range(f, f + n):
            h, c = h * (1 - t["es"][r]), c * (1 - t["es"][r])
            z = t["w_ih"] @ t["x"][r] + t["b_ih"] + t["w_hh"] @ h + t["b_hh"]
            i, fg, g, o = th.sigmoid(z[:H]), th.sigmoid(z[H:2 * H]), th.tanh(z[2 * H:3 * H]), th.sigmoid(z[3 * H:])
            rows["h_prev"][r], rows["z"][r] = h, z
            c = fg * c + i * g
            h = o * th.tanh(c)
            rows["out"][r], rows["gates"][r], rows["c_seq"][r] = h, th.cat([i, fg, g, o]), c
        hn.append(h), cn.append(c)
    order = sorted(rows["z"])
    loss = sum((rows["out"][r] * t["dout"][r]).sum() for r in order)
    grads = th.autograd.grad(loss, [rows["z"][r] for r in order] + [t[k] for k in ("w_ih", "w_hh", "b_ih", "state_h", "state_c")])
    i0 = [s[2] for s in p["table"]]
    res = {k: th.stack([v[r] for r in order]).detach() for k, v in rows.items() if k != "z"}
    res.update(hn=th.stack(hn).detach(), cn=th.stack(cn).detach(), dgates=th.stack(grads[:len(order)]), dw_ih=grads[-5], dw_hh=grads[-4],
               db=grads[-3], dh0=grads[-2][i0], dc0=grads[-1][i0])
    return res, order


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(H, K, S):
        if (H, K, S) not in cache:
            p = problem(H, K, S)
            cache[(H, K, S)] = (p, *step_loop(p, th.float64), step_loop(p, th.float32)[0])
        return cache[(H, K, S)]
    return get


@pytest.mark.parametrize("H,K,S,stream", CASES)
def test_forward_and_backward_against_fp64(references, H, K, S, stream):
    from core.common import hip_ops

    p, ref, order, aten = references(H, K, S)
    R, dev = p["R"], lambda v: v.to(DEV).contiguous()  # noqa: E731
    segs = hip_ops.LstmSegments(p["table"], DEV)
    ins = {k: dev(p[k]) for k in ("x", "es", "w_ih", "w_hh", "b_ih", "b_hh", "state_h", "state_c", "dout")}
    b = Bufs()
    for name, cols in (("out", H), ("gates", 4 * H), ("c_seq", H), ("h_prev", H), ("dgates", 4 * H)):
        b.new(name, R, cols)
    for name in ("hn", "cn", "dh0", "dc0"):
        b.new(name, S, H)
    b.new("dw_ih", 4 * H, K), b.new("dw_hh", 4 * H, H), b.new("db", 4 * H)
    o = {k: f[:n] for k, (f, n) in b.flat.items()}
    view = lambda k, cols: o[k].view(-1, cols)  # noqa: E731

    def launch():
        hip_ops.lstm_seq_fwd(ins["x"], ins["es"], ins["w_ih"], ins["w_hh"], ins["b_ih"], ins["b_hh"], ins["state_h"], ins["state_c"], segs,
                             view("hn", H), view("cn", H), out=view("out", H), gates=view("gates", 4 * H), c_seq=view("c_seq", H),
                             h_prev=view("h_prev", H), force_stream=stream)
        hip_ops.lstm_seq_bwd(ins["dout"], view("gates", 4 * H), view("c_seq", H), ins["state_c"], ins["es"], ins["w_hh"], segs,
                             view("dgates", 4 * H), view("dh0", H), view("dc0", H), force_stream=stream)
        # the existing weight-gradient launch on the segment rows (a contiguous copy: the rows of no segment hold the sentinel)
        dz = view("dgates", 4 * H)[order].contiguous()
        hip_ops.linear_bwd_weight(dz, view("h_prev", H)[order].contiguous(), view("dw_hh", H))
        hip_ops.linear_bwd_weight(dz, ins["x"][order].contiguous(), view("dw_ih", K), o["db"])

    launch()
    b.check(written=("hn", "cn", "dh0", "dc0", "dw_ih", "dw_hh", "db"))
    snap = b.snapshot()
    launch()
    b.check()
    b.same_as(snap)
    rest = np.setdiff1d(np.arange(R), order)
    tag = f"H{H} K{K} S{S}{' streamed' if stream else ''}"
    for name in ("out", "gates", "c_seq", "h_prev", "dgates", "hn", "cn", "dh0", "dc0", "dw_ih", "dw_hh", "db"):
        got = o[name].view(-1, ref[name].shape[-1]) if ref[name].dim() == 2 else o[name]
        if name in ("out", "gates", "c_seq", "h_prev", "dgates"):
            assert bool((got[rest] == SENT).all()), f"{name}: a row of no segment was written"
            got = got[order]
        ek = float((got.cpu().double() - ref[name]).abs().max())
        ea = float((aten[name].double() - ref[name]).abs().max())
        print(f"{tag} {name}: kernel {ek:.3e} aten {ea:.3e} ratio {ek / ea if ea else 0.0:.2f}")
        assert ek <= 4.0 * ea, f"{tag} {name}: kernel error {ek:.3e} above 4 x ATen's {ea:.3e}"


def test_rollout_mode_is_the_training_mode_step():
    """length-1 segments, one per env, nothing stored but the new state: the bits of the training mode's first step"""
    from core.common import hip_ops

    N, K, H = 21, 4, 48
    gen = th.Generator().manual_seed(5)
    r = lambda *s: th.randn(*s, generator=gen).to(DEV)  # noqa: E731
    x, es = r(N, K), (th.rand(N, generator=gen) < 0.3).float().to(DEV)
    w = (r(4 * H, K) / 2, r(4 * H, H) / 7, 0.1 * r(4 * H), 0.1 * r(4 * H))
    sh, sc = r(N, H), r(N, H)
    segs = hip_ops.LstmSegments([(i, 1, i) for i in range(N)], DEV)
    b = Bufs()
    hn, cn, hn2, cn2, out = (b.new(k, N, H) for k in ("hn", "cn", "hn2", "cn2", "out"))
    gates, c_seq, h_prev = b.new("gates", N, 4 * H), b.new("c_seq", N, H), b.new("h_prev", N, H)
    hip_ops.lstm_seq_fwd(x, es, *w, sh, sc, segs, hn, cn)
    hip_ops.lstm_seq_fwd(x, es, *w, sh, sc, segs, hn2, cn2, out=out, gates=gates, c_seq=c_seq, h_prev=h_prev)
    b.check(written=tuple(b.flat))
    assert th.equal(hn, hn2) and th.equal(cn, cn2) and th.equal(out, hn) and th.equal(c_seq, cn)
    assert th.equal(h_prev, sh * (1 - es)[:, None])
