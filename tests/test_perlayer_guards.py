"""The per-layer kernels of csrc/cstr_mlp.hip under guard: every output sits between two sentinel bands (tests/_sentinel_bufs.py:
GuardedBufs), strided outputs are column blocks of wider sentinel-filled matrices, every input is checked to be bit-unchanged, every
launch is repeated and must leave the same bits, and every value is compared with a float64 reference written here with plain torch
ops (the formulas of tests/test_hip_mlp_glue.py, at its tolerances).

Next to each entry point's case table stands what its dispatcher (the `extern "C"` function at the end of cstr_mlp.hip) tests; the table
launches both sides of every condition: shape conditions at the smallest sizes that straddle the 16 x 16 MFMA tile / the 64-column
ownership / the split-K and WAVES thresholds, alignment conditions with ONE operand moved 4 bytes off its 16-byte boundary
(`misalign=1`) at a vector-friendly shape. A misaligned launch is compared bit for bit with the same launch on aligned copies wherever
the scalar and the vector body sum in the same order (stated per entry point), and the dispatchers that refuse misalignment must
refuse and leave every output byte alone.

The `BUF = false` template bodies (plain global loads instead of buffer-descriptor loads, taken from 2^28 floats per operand) are
launched at the end of the file: a 17-row matrix whose rows lie 2^24 floats apart reaches the threshold with 1.1 GiB of address space
of which only the used columns are ever touched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch as th

from conftest import rel_err
from _sentinel_bufs import SENT, GuardedBufs

pytestmark = pytest.mark.gpu

E_BADARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ops():
    assert th.cuda.is_available()
    from core.common import hip_ops

    return hip_ops


def _gen(*key):
    return th.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _act64(t, act):
    return th.relu(t) if act == 1 else (th.tanh(t) if act == 2 else t)


def _dact64(y, act):
    """act'(pre-activation) expressed through the layer's OUTPUT y, as the backward kernels take it"""
    y = y.double()
    return (y > 0).double() if act == 1 else ((1.0 - y * y) if act == 2 else th.ones_like(y))


def _outputs(act, pre):
    """a layer's output y = act(pre) as float32: what the backward kernels read to form act'"""
    return _act64(pre.double(), act).float()


def _cpu(t):
    return t.detach().cpu().numpy()


def twice(b, launch, written=(), inplace=()):
    """launch, all guards; the same launch from the same inputs again: all guards, the same bits"""
    saved = [(t, t.clone()) for t in inplace]
    launch()
    b.check(written)
    snap = b.snapshot()
    for t, s in saved:
        t.copy_(s)
    launch()
    b.check(written)
    b.same_as(snap)


def refused(b, rc_call, code, outputs):
    """the dispatcher refuses (no launch): the given return code, and every byte of the outputs still the sentinel"""
    rc = rc_call()
    th.cuda.synchronize()
    assert rc == code, rc
    b.check()
    for t in outputs:
        assert bool((t == SENT).all())


def _x_operand(b, name, xv, mode, mis=0):
    """x [G, M, K] (values xv, float32 CPU) as the dispatcher's stride cases: contiguous, rows ld = K + 3 / K + 4 floats apart (column
    block of a wider guarded matrix), stride-0 group dimension, groups M * K + 1 floats apart"""
    G, M, K = xv.shape
    if mode == "contig":
        return b.put_ro(name, xv, misalign=mis)
    if mode in ("ld+3", "ld+4"):
        ld = K + int(mode[-1])
        return b.put_ro_cols(name, xv.reshape(G * M, K), ld, 1 if mode == "ld+3" else 4, misalign=mis).view(G, M, K)
    if mode == "shared":
        return b.put_ro(name, xv[0], misalign=mis).unsqueeze(0).expand(G, -1, -1)
    assert mode == "gs+1"
    gs = M * K + 1
    flat = th.zeros((G - 1) * gs + M * K)
    for g in range(G):
        flat[g * gs:g * gs + M * K] = xv[g].reshape(-1)
    return b.put_ro(name, flat, misalign=mis).as_strided((G, M, K), (gs, K, 1))


# ------------------------------------------------------------------------------------------------------------ bias + activation
# cstr_bias_act_fwd_f32: (n & 3) == 0 && aligned16(y) && aligned16(bias) -> float4 body, else scalar body; act 0 / 1 / 2. Element-wise:
# the two bodies give the same bits.
BIAS_ACT_FWD = [  # G, M, N, act, misaligned operand
    (1, 1, 1, 1, None), (1, 15, 3, 2, None), (2, 17, 16, 1, None), (3, 33, 36, 0, None), (1, 65, 65, 2, None), (2, 5, 17, 1, None),
    (2, 17, 16, 1, "y"), (2, 17, 16, 2, "bias"), (3, 33, 36, 2, "y")]


def _run_bias_act_fwd(ops, G, M, N, act, mis):
    g = _gen(G, M, N, act)
    z, bias = th.randn(G, M, N, generator=g), th.randn(G, N, generator=g)
    b = GuardedBufs()
    y, bb = b.put("y", z, misalign=int(mis == "y")), b.put_ro("bias", bias, misalign=int(mis == "bias"))
    twice(b, lambda: ops.bias_act_fwd_(y, bb, act), inplace=(y,))
    return y.clone(), _act64(z.double() + bias.double()[:, None, :], act)


@pytest.mark.parametrize("G,M,N,act,mis", BIAS_ACT_FWD)
def test_bias_act_fwd(ops, G, M, N, act, mis):
    y, ref = _run_bias_act_fwd(ops, G, M, N, act, mis)
    assert rel_err(_cpu(y), ref.numpy(), 1.0) < 1e-6
    if mis:
        assert th.equal(y, _run_bias_act_fwd(ops, G, M, N, act, None)[0])


# cstr_bias_act_bwd_f32: groups == 1 -> cstr_bias_act_bwd_rows_f32; m >= 64 -> 16 waves, else 4; act; gbias optional; a workgroup owns
# 64 columns (n = 1, 33, 64, 65); gz == gy allowed with act 0 (fused.py's bias gradient of a layer without activation: nothing to write
# but gbias). No alignment term.
BIAS_ACT_BWD = [  # G, M, N, act, in place
    (2, 1, 1, 1, False), (3, 15, 65, 2, False), (2, 65, 33, 0, False), (2, 64, 17, 1, False), (1, 17, 36, 2, False), (2, 63, 3, 1, False),
    (2, 33, 64, 0, False), (2, 65, 33, 0, True), (3, 17, 65, 0, True), (1, 33, 16, 0, True)]


@pytest.mark.parametrize("G,M,N,act,inplace", BIAS_ACT_BWD)
def test_bias_act_bwd(ops, G, M, N, act, inplace):
    g = _gen(G, M, N, act, 1)
    gy, yv = th.randn(G, M, N, generator=g), _outputs(act, th.randn(G, M, N, generator=g))
    ref = gy.double() * _dact64(yv, act)
    b = GuardedBufs()
    d_y = b.put_ro("y", yv) if act else None
    gb = b.new("gbias", G, N)
    if inplace:
        d_gy = b.put_ro("gy", gy)  # act 0, gz == gy: the kernel must not store to it at all
        twice(b, lambda: ops.bias_act_bwd(d_gy, d_y, act, d_gy, gb), ("gbias",))
    else:
        d_gy, gz = b.put_ro("gy", gy), b.new("gz", G, M, N)
        twice(b, lambda: ops.bias_act_bwd(d_gy, d_y, act, gz, gb), ("gz", "gbias"))
        assert rel_err(_cpu(gz), ref.numpy(), 1.0) < 1e-6
        gz2 = b.new("gz_alone", G, M, N)
        twice(b, lambda: ops.bias_act_bwd(d_gy, d_y, act, gz2, None), ("gz_alone",))  # frozen parameters: no gbias
        assert th.equal(gz2, gz)
    assert rel_err(_cpu(gb), ref.sum(1).numpy(), float(M) ** 0.5) < 2e-6


# cstr_bias_act_bwd_rows_f32: ldg >= n, ldy >= n (column blocks of wider matrices); gz == gy needs ldg == n; m >= 64; act.
BIAS_ACT_BWD_ROWS = [  # M, N, act, ldg - N, ldy - N
    (17, 36, 2, 3, 5), (65, 65, 1, 1, 0), (1, 3, 0, 2, 0), (64, 16, 1, 0, 4), (15, 1, 2, 7, 7), (33, 64, 0, 1, 0)]


@pytest.mark.parametrize("M,N,act,eg,ey", BIAS_ACT_BWD_ROWS)
def test_bias_act_bwd_rows(ops, M, N, act, eg, ey):
    from core import _native as nv

    g = _gen(M, N, act, 2)
    gy, yv = th.randn(M, N, generator=g), _outputs(act, th.randn(M, N, generator=g))
    ref = gy.double() * _dact64(yv, act)
    b = GuardedBufs()
    d_gy = b.put_ro_cols("gy", gy, N + eg, eg // 2)
    d_y = b.put_ro_cols("y", yv, N + ey, ey) if act else None
    gz, gb = b.new("gz", M, N), b.new("gbias", N)
    twice(b, lambda: ops.bias_act_bwd_rows(d_gy, d_y, act, gz, gb), ("gz", "gbias"))
    assert rel_err(_cpu(gz), ref.numpy(), 1.0) < 1e-6
    assert rel_err(_cpu(gb), ref.sum(0).numpy(), float(M) ** 0.5) < 2e-6
    if eg:  # in place on a strided gy: refused, nothing written
        rc = lambda: nv.lib().cstr_bias_act_bwd_rows_f32(nv.ptr(d_gy), C.c_int64(N + eg), nv.ptr(d_y), C.c_int64(N + ey), C.c_int(act), nv.ptr(d_gy),  # noqa: E731
                                                         nv.ptr(gb), C.c_int64(M), C.c_int64(N), nv.stream_ptr())
        snap = b.snapshot()
        assert rc() == E_BADARG
        b.check()
        b.same_as(snap)


# --------------------------------------------------------------------------------------------------------------- Linear forward
# cstr_linear_act_fwd_f32:
#   vec   = (k & 3) == 0 && (ldx & 3) == 0 && (x_group_stride & 3) == 0 && aligned16(x) && aligned16(w)   -> 16-byte / dword operand loads
#   buf   = m * ldx < 2^28 && n * k < 2^28                      -> buffer-descriptor / plain loads (false: test_buf_false_* below)
#   split = k > 32 && tiles * groups <= 2048                    -> 4 waves (split-K) / 1 wave
#   act 0 / 1 / 2; grid = ceil(n / 16) x ceil(m / 16) x groups.
# The scalar body loads the same four values per quad and feeds the same MFMA sequence: bit-identical to the vector body.
LINEAR_FWD = [  # G (0: 2-D operands), M, N, K, act, x layout, misaligned operand
    (0, 17, 17, 36, 1, "contig", None), (0, 17, 17, 32, 2, "contig", None), (0, 1, 1, 1, 0, "contig", None), (0, 15, 3, 3, 1, "contig", None),
    (0, 33, 16, 4, 2, "contig", None), (0, 65, 65, 68, 1, "contig", None), (0, 65, 33, 33, 2, "contig", None), (0, 17, 36, 6, 0, "contig", None),
    (0, 33, 65, 17, 1, "contig", None), (2, 17, 17, 36, 1, "contig", None), (3, 15, 33, 6, 2, "contig", None), (2, 33, 17, 36, 1, "shared", None),
    (0, 17, 17, 36, 1, "ld+3", None), (0, 17, 17, 36, 1, "ld+4", None), (2, 17, 17, 36, 2, "ld+4", None), (2, 15, 17, 36, 1, "gs+1", None),
    (0, 16401, 17, 36, 1, "contig", None),  # 2 x 1026 tiles > 2048: one wave per tile although k > 32
    (0, 17, 17, 36, 1, "contig", "x"), (0, 17, 17, 36, 1, "contig", "w"), (2, 17, 17, 36, 2, "ld+4", "x"), (0, 65, 65, 68, 0, "contig", "w")]


def _linear_ref(xv, w, bias, act):
    return _act64(th.einsum("gmk,gnk->gmn", xv.double(), w.double()) + bias.double()[:, None, :], act)


def _run_linear_fwd(ops, G, M, N, K, act, mode, mis):
    gg = max(G, 1)
    g = _gen(G, M, N, K, act)
    xv, w, bias = th.randn(gg, M, K, generator=g), th.randn(gg, N, K, generator=g) / K ** 0.5, th.randn(gg, N, generator=g)
    if mode == "shared":
        xv = xv[:1].expand(gg, -1, -1).contiguous()
    b = GuardedBufs()
    x = _x_operand(b, "x", xv, mode, int(mis == "x"))
    d_w, d_b = b.put_ro("w", w, misalign=int(mis == "w")), b.put_ro("bias", bias)
    y = b.new("y", gg, M, N)
    if G == 0:
        twice(b, lambda: ops.linear_act_fwd(x[0], d_w[0], d_b[0], act, out=y[0]), ("y",))
    else:
        twice(b, lambda: ops.linear_act_fwd(x, d_w, d_b, act, out=y), ("y",))
    return y.clone(), _linear_ref(xv, w, bias, act)


@pytest.mark.parametrize("G,M,N,K,act,mode,mis", LINEAR_FWD)
def test_linear_act_fwd(ops, G, M, N, K, act, mode, mis):
    y, ref = _run_linear_fwd(ops, G, M, N, K, act, mode, mis)
    assert rel_err(_cpu(y), ref.numpy(), max(1.0, float(ref.abs().max()))) < 2e-6
    if mis:
        assert th.equal(y, _run_linear_fwd(ops, G, M, N, K, act, mode, None)[0])


# cstr_linear_act_fwd_sets_f32 (pointer table, one shape): vec = (k & 3) == 0 && every set: (ldx & 3) == 0 && aligned16(x) && aligned16(w);
# buf = every set: m * ldx < 2^28 && n * k < 2^28; split = k > 32 && tiles * min(sets, 4) <= 2048; y has its own row stride ldy.
# Same tile code as cstr_linear_act_fwd_f32: scalar and vector bodies bit-identical.
LINEAR_FWD_SETS = [  # sets, M, N, K, act, x layout, misaligned operand (of the LAST set)
    (1, 17, 17, 36, 1, "contig", None), (3, 15, 3, 6, 2, "contig", None), (2, 33, 17, 33, 0, "contig", None), (2, 65, 16, 32, 1, "contig", None),
    (2, 17, 17, 36, 1, "ld+3", None), (2, 17, 17, 36, 2, "ld+4", None), (1, 16401, 17, 36, 1, "contig", None),
    (2, 17, 17, 36, 1, "contig", "x"), (2, 17, 17, 36, 1, "contig", "w")]


def _run_linear_fwd_sets(ops, S, M, N, K, act, mode, mis):
    g = _gen(S, M, N, K, act, 3)
    b = GuardedBufs()
    sets, refs, ys = [], [], []
    for i in range(S):
        xv, w, bias = th.randn(1, M, K, generator=g), th.randn(1, N, K, generator=g) / K ** 0.5, th.randn(1, N, generator=g)
        last = i == S - 1
        x = _x_operand(b, f"x{i}", xv, mode, int(last and mis == "x"))[0]
        y = b.new_cols(f"y{i}", M, N + 5, 2 + i, N)  # a column block of a wider matrix (MADDPG's joint action)
        sets.append((x, b.put_ro(f"w{i}", w[0], misalign=int(last and mis == "w")), b.put_ro(f"b{i}", bias[0]), y))
        refs.append(_linear_ref(xv, w, bias, act)[0])
        ys.append(y)
    twice(b, lambda: ops.linear_act_fwd_sets(sets, act), tuple(f"y{i}" for i in range(S)))
    return [y.clone() for y in ys], refs


@pytest.mark.parametrize("S,M,N,K,act,mode,mis", LINEAR_FWD_SETS)
def test_linear_act_fwd_sets(ops, S, M, N, K, act, mode, mis):
    ys, refs = _run_linear_fwd_sets(ops, S, M, N, K, act, mode, mis)
    for y, ref in zip(ys, refs):
        assert rel_err(_cpu(y), ref.numpy(), max(1.0, float(ref.abs().max()))) < 2e-6
    if mis:
        for y, y0 in zip(ys, _run_linear_fwd_sets(ops, S, M, N, K, act, mode, None)[0]):
            assert th.equal(y, y0)


# cstr_linear_smooth_fwd_f32: REFUSES n > 16, k <= 32, ceil(m / 16) > 2048, m * ldx >= 2^28 (CSTR_E_UNSUPPORTED);
# vec = (k & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(w); act; out has a row stride. Same loads / MFMA order in both bodies.
LINEAR_SMOOTH = [  # M, N, K, act, x layout, misaligned operand
    (1, 1, 33, 0, "contig", None), (15, 3, 36, 2, "contig", None), (17, 16, 68, 1, "contig", None), (33, 2, 36, 2, "contig", None),
    (65, 4, 260, 2, "contig", None), (17, 3, 36, 2, "ld+3", None), (17, 3, 36, 2, "ld+4", None),
    (15, 3, 36, 2, "contig", "x"), (15, 3, 36, 2, "contig", "w")]


def _run_linear_smooth(ops, M, N, K, act, mode, mis):
    g = _gen(M, N, K, act, 4)
    xv, w, bias = th.randn(1, M, K, generator=g), th.randn(N, K, generator=g) / K ** 0.5, th.randn(N, generator=g) * 0.1
    noise = th.randn(M, N, generator=g) * 0.4
    b = GuardedBufs()
    x = _x_operand(b, "x", xv, mode, int(mis == "x"))[0]
    d_w, d_b, d_n = b.put_ro("w", w, misalign=int(mis == "w")), b.put_ro("bias", bias), b.put_ro("noise", noise)
    out = b.new_cols("out", M, N + 4, 3, N)
    twice(b, lambda: ops.linear_smooth_fwd(x, d_w, d_b, act, d_n, None, 0.2, 0.5, out), ("out",))
    ref = (_linear_ref(xv, w[None], bias[None], act)[0] + noise.double().clamp(-0.5, 0.5)).clamp(-1.0, 1.0)
    return out.clone(), ref


@pytest.mark.parametrize("M,N,K,act,mode,mis", LINEAR_SMOOTH)
def test_linear_smooth_fwd(ops, M, N, K, act, mode, mis):
    out, ref = _run_linear_smooth(ops, M, N, K, act, mode, mis)
    assert rel_err(_cpu(out), ref.numpy(), max(1.0, float(ref.abs().max()))) < 2e-6
    if mis:
        assert th.equal(out, _run_linear_smooth(ops, M, N, K, act, mode, None)[0])


@pytest.mark.parametrize("M,N,K", [(17, 17, 36), (17, 3, 32)])
def test_linear_smooth_fwd_refuses_other_shapes(ops, M, N, K):
    from core import _native as nv

    b = GuardedBufs()
    x, w, bias, noise = b.put_ro("x", th.ones(M, K)), b.put_ro("w", th.ones(N, K)), b.put_ro("bias", th.ones(N)), b.put_ro("noise", th.ones(M, N))
    out = b.new("out", M, N)
    refused(b, lambda: nv.lib().cstr_linear_smooth_fwd_f32(nv.ptr(x), C.c_int64(K), nv.ptr(w), nv.ptr(bias), C.c_int(1), nv.ptr(noise), None,
                                                           C.c_float(0.2), C.c_float(0.5), nv.ptr(out), C.c_int64(N), C.c_int64(M), C.c_int64(N),
                                                           C.c_int64(K), nv.stream_ptr()), E_UNSUPPORTED, (out,))


# -------------------------------------------------------------------------------------------------------------- Linear backward
# cstr_linear_bwd_input_f32: vec = (n & 3) == 0 && aligned16(gz); buf = m * n, n * k, m * k < 2^28 (false: test_buf_false_bwd_input);
# n > 32 -> 4 waves split the reduction over n, else 1; sum_groups -> one grid slice sums the groups; act; the reduction runs over N in
# 16-wide chunks, the tile is 16 (m) x 16 (k). Both bodies load the same quads of gz: bit-identical.
LINEAR_BWD_INPUT = [  # G (0: 2-D), M, N, K, act, sum_groups, misaligned operand
    (0, 17, 36, 17, 1, False, None), (0, 17, 32, 4, 2, False, None), (0, 1, 1, 1, 0, False, None), (0, 15, 33, 3, 1, False, None),
    (0, 33, 17, 68, 2, False, None), (0, 65, 65, 33, 1, False, None), (0, 33, 16, 36, 0, False, None), (0, 15, 3, 6, 2, False, None),
    (2, 17, 36, 6, 0, False, None), (3, 15, 16, 17, 2, True, None), (2, 33, 33, 36, 1, True, None), (1, 17, 36, 32, 1, True, None),
    (0, 17, 36, 17, 1, False, "gz"), (0, 17, 32, 4, 2, False, "gz"), (2, 17, 36, 6, 1, True, "gz")]


def _bwd_input(gz, w, y, act, dz, G, sum_groups, M, N, K):
    from core import _native as nv

    nv.check(nv.lib().cstr_linear_bwd_input_f32(nv.ptr(gz), nv.ptr(w), nv.ptr(y if act else None), C.c_int(act), nv.ptr(dz), C.c_int64(G),
                                                C.c_int(int(sum_groups)), C.c_int64(M), C.c_int64(N), C.c_int64(K), nv.stream_ptr()),
             "cstr_linear_bwd_input_f32")


def _run_linear_bwd_input(G, M, N, K, act, sum_groups, mis):
    gg, go = max(G, 1), 1 if sum_groups else max(G, 1)
    g = _gen(G, M, N, K, act, 5)
    gz, w = th.randn(gg, M, N, generator=g), th.randn(gg, N, K, generator=g) / N ** 0.5
    yv = _outputs(act, th.randn(go, M, K, generator=g))
    dx = th.einsum("gmn,gnk->gmk", gz.double(), w.double())
    ref = (dx.sum(0, keepdim=True) if sum_groups else dx) * _dact64(yv, act)
    b = GuardedBufs()
    d_gz, d_w, d_y = b.put_ro("gz", gz, misalign=int(mis == "gz")), b.put_ro("w", w), b.put_ro("y", yv)
    dz = b.new("dz", go, M, K)
    twice(b, lambda: _bwd_input(d_gz, d_w, d_y, act, dz, gg, sum_groups, M, N, K), ("dz",))
    return dz.clone(), ref


@pytest.mark.parametrize("G,M,N,K,act,sum_groups,mis", LINEAR_BWD_INPUT)
def test_linear_bwd_input(ops, G, M, N, K, act, sum_groups, mis):
    dz, ref = _run_linear_bwd_input(G, M, N, K, act, sum_groups, mis)
    assert rel_err(_cpu(dz), ref.numpy(), max(1.0, float(ref.abs().max()))) < 2e-6
    if mis:
        assert th.equal(dz, _run_linear_bwd_input(G, M, N, K, act, sum_groups, None)[0])


# cstr_linear_bwd_weight_f32: m > 32 -> 4 waves split the rows, else 1; buf = m * n < 2^28 && m * ldx < 2^28 (false:
# test_buf_false_bwd_weight); db optional; x with row / group strides. No alignment term (dword loads only).
LINEAR_BWD_WEIGHT = [  # G (0: 2-D), M, N, K, x layout
    (0, 33, 17, 36, "contig"), (0, 32, 17, 36, "contig"), (0, 1, 1, 1, "contig"), (0, 15, 3, 3, "contig"), (0, 17, 16, 4, "contig"),
    (0, 65, 65, 68, "contig"), (0, 33, 36, 17, "contig"), (2, 17, 33, 6, "contig"), (3, 65, 17, 32, "contig"), (2, 33, 17, 36, "shared"),
    (0, 33, 17, 36, "ld+3"), (2, 17, 17, 36, "ld+4"), (2, 33, 3, 6, "gs+1")]


@pytest.mark.parametrize("G,M,N,K,mode", LINEAR_BWD_WEIGHT)
def test_linear_bwd_weight(ops, G, M, N, K, mode):
    gg = max(G, 1)
    g = _gen(G, M, N, K, 6)
    dzv, xv = th.randn(gg, M, N, generator=g), th.randn(gg, M, K, generator=g)
    if mode == "shared":
        xv = xv[:1].expand(gg, -1, -1).contiguous()
    ref_w, ref_b = th.einsum("gmn,gmk->gnk", dzv.double(), xv.double()), dzv.double().sum(1)
    b = GuardedBufs()
    x, dz = _x_operand(b, "x", xv, mode), b.put_ro("dz", dzv)
    dw, db, dw2 = b.new("dw", gg, N, K), b.new("db", gg, N), b.new("dw_alone", gg, N, K)
    s = (lambda t: t[0]) if G == 0 else (lambda t: t)  # noqa: E731
    twice(b, lambda: ops.linear_bwd_weight(s(dz), s(x), s(dw), s(db)), ("dw", "db"))
    twice(b, lambda: ops.linear_bwd_weight(s(dz), s(x), s(dw2), None), ("dw_alone",))
    scale = float(M) ** 0.5
    assert rel_err(_cpu(dw), ref_w.numpy(), scale) < 2e-6 and rel_err(_cpu(db), ref_b.numpy(), scale) < 2e-6
    assert th.equal(dw2, dw)


# cstr_linear_bwd_weight_sets_f32: the grid covers the LARGEST set (smaller sets' surplus workgroups return); min m > 32 -> 4 waves;
# buf = every set below 2^28. Same tile code as cstr_linear_bwd_weight_f32 -> the same bits as one launch per set.
@pytest.mark.parametrize("M", [17, 33, 65])
def test_linear_bwd_weight_sets(ops, M):
    g = _gen(M, 7)
    b = GuardedBufs()
    sets, singles = [], []
    for i, (N, K, mode) in enumerate([(17, 36, "contig"), (3, 6, "ld+3"), (65, 68, "ld+4"), (1, 1, "contig"), (16, 33, "contig")]):
        dzv, xv = th.randn(M, N, generator=g), th.randn(1, M, K, generator=g)
        x, dz = _x_operand(b, f"x{i}", xv, mode)[0], b.put_ro(f"dz{i}", dzv)
        dw, db = b.new(f"dw{i}", N, K), (None if i == 1 else b.new(f"db{i}", N))
        rw, rb = b.new(f"rw{i}", N, K), (None if i == 1 else b.new(f"rb{i}", N))
        ops.linear_bwd_weight(dz, x, rw, rb)
        sets.append((dz, x, dw, db))
        singles.append((rw, rb, th.einsum("mn,mk->nk", dzv.double(), xv[0].double()), dzv.double().sum(0)))
    names = tuple(f"dw{i}" for i in range(5)) + tuple(f"db{i}" for i in (0, 2, 3, 4))
    twice(b, lambda: ops.linear_bwd_weight_sets(sets), names)
    for (_, _, dw, db), (rw, rb, ref_w, ref_b) in zip(sets, singles):
        assert th.equal(dw, rw) and (db is None or th.equal(db, rb))
        assert rel_err(_cpu(dw), ref_w.numpy(), float(M) ** 0.5) < 2e-6
        assert db is None or rel_err(_cpu(db), ref_b.numpy(), float(M) ** 0.5) < 2e-6


# ------------------------------------------------------------------------------------------------- hidden layer + scalar head
# cstr_hidden_head_fwd_f32: v4 = (k & 3) == 0 && aligned16(z) && aligned16(b1) && aligned16(w2); grid = ceil(rows / 4) workgroups of 4
# waves, a wave per row; the float4 body strides 256 columns per pass, the scalar body 64. y = act(z + b1) is element-wise (the same
# bits in both bodies); q sums 4-column groups in the float4 body and single columns in the scalar one: two summation orders, so a
# misaligned launch is compared with float64 (and its y with the aligned launch's bits).
HIDDEN_HEAD_FWD = [  # G, M, K, act, misaligned operand
    (1, 1, 1, 0, None), (1, 15, 36, 1, None), (2, 17, 33, 2, None), (3, 33, 68, 1, None), (1, 65, 4, 2, None), (2, 5, 17, 0, None),
    (1, 3, 260, 1, None), (1, 3, 65, 2, None), (2, 6, 6, 1, None),
    (3, 33, 68, 1, "z"), (3, 33, 68, 2, "b1"), (3, 33, 68, 1, "w2"), (1, 3, 260, 0, "z")]


def _run_hidden_head_fwd(ops, G, M, K, act, mis):
    g = _gen(G, M, K, act, 8)
    z, b1 = th.randn(G, M, K, generator=g), th.randn(G, K, generator=g) * 0.3
    w2, b2 = th.randn(G, K, generator=g) / K ** 0.5, th.randn(G, generator=g)
    b = GuardedBufs()
    y = b.put("z", z, misalign=int(mis == "z"))
    d_b1, d_w2, d_b2 = b.put_ro("b1", b1, misalign=int(mis == "b1")), b.put_ro("w2", w2, misalign=int(mis == "w2")), b.put_ro("b2", b2)
    q = b.new("q", G, M, 1)
    twice(b, lambda: ops.hidden_head_fwd_(y, d_b1, act, d_w2, d_b2, q), ("q",), inplace=(y,))
    yd = _act64(z.double() + b1.double()[:, None, :], act)
    return y.clone(), q.clone(), yd, (yd * w2.double()[:, None, :]).sum(-1) + b2.double()[:, None]


@pytest.mark.parametrize("G,M,K,act,mis", HIDDEN_HEAD_FWD)
def test_hidden_head_fwd(ops, G, M, K, act, mis):
    y, q, yd, qd = _run_hidden_head_fwd(ops, G, M, K, act, mis)
    assert rel_err(_cpu(y), yd.numpy(), 1.0) < 1e-6
    assert rel_err(_cpu(q).reshape(G, M), qd.numpy(), 1.0) < 3e-6
    if mis:
        assert th.equal(y, _run_hidden_head_fwd(ops, G, M, K, act, None)[0])


# cstr_hidden_head_bwd_f32: m >= 64 -> 16 waves, else 4; gb1, gw2, gb2 all or none; a workgroup owns 64 columns (k = 1, 17, 64, 65);
# groups on grid.y. No alignment term.
HIDDEN_HEAD_BWD = [  # G, M, K, act
    (1, 1, 1, 1), (2, 15, 65, 2), (1, 64, 33, 0), (3, 65, 17, 1), (2, 63, 64, 2), (1, 17, 36, 1), (2, 33, 3, 0)]


@pytest.mark.parametrize("G,M,K,act", HIDDEN_HEAD_BWD)
def test_hidden_head_bwd(ops, G, M, K, act):
    g = _gen(G, M, K, act, 9)
    yv = _outputs(act, th.randn(G, M, K, generator=g))
    w2, gq = th.randn(G, K, generator=g) / K ** 0.5, th.randn(G, M, generator=g)
    ref_dz = gq.double()[:, :, None] * w2.double()[:, None, :] * _dact64(yv, act)
    b = GuardedBufs()
    d_y, d_w2, d_gq = b.put_ro("y", yv), b.put_ro("w2", w2), b.put_ro("gq", gq)
    dz, gb1, gw2, gb2, dz2 = b.new("dz", G, M, K), b.new("gb1", G, K), b.new("gw2", G, K), b.new("gb2", G), b.new("dz_alone", G, M, K)
    twice(b, lambda: ops.hidden_head_bwd(d_gq, d_y, act, d_w2, dz, gb1, gw2, gb2), ("dz", "gb1", "gw2", "gb2"))
    twice(b, lambda: ops.hidden_head_bwd(d_gq, d_y, act, d_w2, dz2), ("dz_alone",))
    scale = float(M) ** 0.5
    assert rel_err(_cpu(dz), ref_dz.numpy(), 1.0) < 1e-6 and th.equal(dz, dz2)
    assert rel_err(_cpu(gb1), ref_dz.sum(1).numpy(), scale) < 2e-6
    assert rel_err(_cpu(gw2), (gq.double()[:, :, None] * yv.double()).sum(1).numpy(), scale) < 2e-6
    assert rel_err(_cpu(gb2), gq.double().sum(1).numpy(), scale) < 2e-6


# ------------------------------------------------------------------------------------------------------ squashed Gaussian heads
def _squashed64(mean, log_std_raw, eps):
    """distributions.py:161-260 in float64 (tests/test_hip_mlp_glue.py: ref_squashed)"""
    std = th.clamp(log_std_raw, -20, 2).exp()
    u = mean + std * eps
    a = th.tanh(u)
    lp = (-((u - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))).sum(dim=1)
    return a, lp - th.sum(th.log(1 - a ** 2 + 1e-6), dim=1), u


def _head_inputs(g, B, A):
    """mean, raw log_std, eps: log_std in [-1, 1] (the kernel forms u - mean in float32: with std >= 0.37 that difference keeps its digits),
    plus one entry above and one below the clamp range, both at mean 0 (where u - mean is exact)"""
    mean, ls = (th.randn(B, A, generator=g) * 0.5).clamp(-1.0, 1.0), th.rand(B, A, generator=g) * 2 - 1
    eps = th.randn(B, A, generator=g)
    ls[0, 0], mean[0, 0] = 3.0, 0.0
    ls[-1, -1], mean[-1, -1] = (-25.0, 0.0) if B * A > 1 else (3.0, 0.0)
    return mean, ls, eps


def _logp64_of_action(mean, log_std_raw, eps, action):
    """The log-prob in float64 with the tanh correction taken from the action the launch RETURNED (float32): where tanh saturates,
    log(1 - a^2 + 1e-6) is a function of the last bits of a (a = 1.0f from |u| = 9 on: log(1e-6) against the exact -13.4), so a float64
    reference that recomputes a cannot be compared there at any useful bound. The action itself is compared at 1e-6 beside this."""
    std = th.clamp(log_std_raw, -20, 2).exp()
    u = mean + std * eps
    lp = (-((u - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))).sum(dim=1)
    return lp - th.sum(th.log(1 - action.double().cpu() ** 2 + 1e-6), dim=1)


def _check_head_fwd(action, logp, mean, ls, eps, a_tol=1e-6, lp_tol=5e-5):
    """the bars of test_squashed_gaussian_fwd_bwd: tanh output 1e-6; log-prob 5e-5 on every row and 5e-6 on the rows away from tanh's
    saturation (|u| < 3).
    The 5e-6 bar stands there between two FLOAT32 evaluations of the same statements (the kernel's and torch's) on that test's batch. It
    is not a bound a correct kernel keeps on the calm rows in general: a is a float32 (spacing 2^-24 below 1), and
    d log(1 - a^2 + 1e-6) / da = 2a / (1 - a^2) reaches 2 / (1 - tanh(3)^2) = 203 at the edge of the calm rows, so an action that is right
    to ONE unit in its last place moves its row's log-prob by up to 203 * 2^-24 = 1.2e-5 per action dimension. Measured on this file's
    batches: 6.9e-6 at [257-4] and 6.8e-6 at [1025-2-36] against float64, 9.6e-6 at [1025-2-36] against torch's float32 evaluation. The
    calm rows are therefore held to the 5e-5 bar against float64, like every row (the first comparison below, whose correction term
    comes from the returned action, covers the saturated rows at the same bar)."""
    a64, lp64, u64 = _squashed64(mean.double(), ls.double(), eps.double())
    assert rel_err(_cpu(action), a64.numpy(), 1.0) < a_tol
    if logp is not None:
        calm = (u64.abs().max(dim=1).values < 3).numpy()
        assert rel_err(_cpu(logp), _logp64_of_action(mean.double(), ls.double(), eps.double(), action).numpy(), 1.0) < lp_tol
        assert rel_err(_cpu(logp)[calm], lp64.numpy()[calm], 1.0) < 5e-5


def _grads64(mean, ls, eps, ga, gl):
    m64, l64 = mean.double().requires_grad_(True), ls.double().requires_grad_(True)
    a64, lp64, u64 = _squashed64(m64, l64, eps.double())
    th.autograd.backward([a64, lp64], [ga.double(), gl.double()])
    return m64.grad, l64.grad, u64.detach()


def _check_head_bwd(g_mean, g_ls, mean, ls, eps, ga, gl):
    """the bars of test_squashed_gaussian_fwd_bwd: finite everywhere, 3e-5 (floor 1e-2) away from saturation, exactly 0 outside the clamp"""
    gm64, gl64, u64 = _grads64(mean, ls, eps, ga, gl)
    ok = (u64.abs() < 5.0).numpy()
    gm, gls = _cpu(g_mean), _cpu(g_ls)
    assert np.isfinite(gm).all() and np.isfinite(gls).all()
    assert rel_err(gm[ok], gm64.numpy()[ok], 1e-2) < 3e-5 and rel_err(gls[ok], gl64.numpy()[ok], 1e-2) < 3e-5
    outside = ((ls > 2) | (ls < -20)).numpy()
    assert outside.any() and np.all(gls[outside] == 0.0)


# cstr_squashed_gaussian_fwd_f32 / _bwd_f32: flat grid-stride kernels, no alignment term; in_stride = A (separate tensors) or 2A (the two
# halves of a merged head's output); g_action with its own row stride, g_action / g_logp optional.
@pytest.mark.parametrize("B,A,merged", [(1, 1, False), (17, 2, True), (65, 3, True), (257, 4, False), (33, 2, False)])
def test_squashed_gaussian_fwd_bwd_guarded(ops, B, A, merged):
    g = _gen(B, A, 10)
    mean, ls, eps = _head_inputs(g, B, A)
    ga, gl = th.randn(B, A, generator=g), th.randn(B, generator=g)
    b = GuardedBufs()
    if merged:
        p = b.put_ro("params", th.cat((mean, ls), dim=1))
        d_mean, d_ls = p[:, :A], p[:, A:]
        gp = b.new("g_params", B, 2 * A)
        g_mean, g_ls, gnames = gp[:, :A], gp[:, A:], ("g_params",)
    else:
        d_mean, d_ls = b.put_ro("mean", mean), b.put_ro("log_std", ls)
        g_mean, g_ls, gnames = b.new("g_mean", B, A), b.new("g_log_std", B, A), ("g_mean", "g_log_std")
    d_eps, action, logp = b.put_ro("eps", eps), b.new("action", B, A), b.new("logp", B)
    twice(b, lambda: ops.squashed_gaussian_fwd(d_mean, d_ls, d_eps, action, logp), ("action", "logp"))
    _check_head_fwd(action, logp, mean, ls, eps)
    a2 = b.new("action_alone", B, A)
    twice(b, lambda: ops.squashed_gaussian_fwd(d_mean, d_ls, d_eps, a2, None), ("action_alone",))
    assert th.equal(a2, action)
    d_ga, d_gl = b.put_ro_cols("g_action", ga, A + 3, 2), b.put_ro("g_logp", gl)
    a_ro = b.put_ro("action_in", action)
    twice(b, lambda: ops.squashed_gaussian_bwd(d_ga, d_gl, a_ro, d_ls, d_eps, g_mean, g_ls), gnames)
    _check_head_bwd(g_mean, g_ls, mean, ls, eps, ga, gl)


# cstr_gaussian_head_fwd_f32 (eps given): 64 rows per workgroup, grid capped at 4096; bias optional; action_stride; no alignment term.
# cstr_gaussian_head_bwd_f32: ONE workgroup of 256 lanes strides the batch (b = 257: a second pass); g_action / g_bias optional, strides.
@pytest.mark.parametrize("B,A,with_bias", [(1, 1, True), (17, 2, True), (65, 3, True), (257, 4, True), (15, 2, False)])
def test_gaussian_head_fwd_bwd_guarded(ops, B, A, with_bias):
    g = _gen(B, A, 11)
    mean, ls, eps = _head_inputs(g, B, A)
    bias = th.randn(2 * A, generator=g) * 0.2 if with_bias else th.zeros(2 * A)
    z = th.cat((mean, ls), dim=1) - bias  # float32: z + bias gives mean / ls back to an ulp; the reference uses the kernel's own sum
    ga, gl = th.randn(B, A, generator=g), th.randn(B, generator=g)
    b = GuardedBufs()
    params, d_eps = b.put("params", z), b.put_ro("eps", eps)
    d_bias = b.put_ro("bias", bias) if with_bias else None
    action, logp = b.new_cols("action", B, A + 5, 4, A), b.new("logp", B)
    twice(b, lambda: ops.gaussian_head_fwd_(params, d_bias, d_eps, None, action, logp), ("action", "logp"), inplace=(params,))
    pb = (z + bias) if with_bias else z  # one float32 addition per element: the kernel's must be the same bits
    assert th.equal(params.cpu(), pb)
    _check_head_fwd(action, logp, pb[:, :A], pb[:, A:], eps)
    d_ga, d_gl = b.put_ro_cols("g_action", ga, A + 3, 1), b.put_ro("g_logp", gl)
    p_ro = b.put_ro("params_in", params)
    gp, gb = b.new("g_params", B, 2 * A), b.new("g_bias", 2 * A)
    twice(b, lambda: ops.gaussian_head_bwd(d_ga, d_gl, action, p_ro, d_eps, gp, gb), ("g_params", "g_bias"))
    _check_head_bwd(gp[:, :A], gp[:, A:], pb[:, :A], pb[:, A:], eps, ga, gl)
    assert rel_err(_cpu(gb), _cpu(gp).astype(np.float64).sum(0), float(B) ** 0.5) < 2e-6
    gp2 = b.new("g_params_alone", B, 2 * A)
    twice(b, lambda: ops.gaussian_head_bwd(d_ga, d_gl, action, p_ro, d_eps, gp2, None), ("g_params_alone",))
    assert th.equal(gp2, gp)


# cstr_gaussian_head_bwd_input_f32: the KERNEL picks its body: vec = (width & 3) == 0 && (ldh & 3) == 0 && w, hidden, dz 16-byte aligned;
# 4 rows per workgroup, a wave per row; the float4 body strides 256 columns per pass. Both bodies run the same fma chain per column
# (j ascending): bit-identical.
HEAD_BWD_INPUT = [  # B, A, H, act, ldh - H, misaligned operand
    (1, 1, 1, 0, 0, None), (15, 2, 36, 1, 0, None), (17, 3, 33, 2, 0, None), (33, 4, 260, 1, 4, None), (5, 2, 68, 2, 3, None), (6, 2, 6, 1, 0, None),
    (15, 2, 36, 1, 0, "w"), (15, 2, 36, 2, 0, "hidden"), (15, 2, 36, 1, 0, "dz"), (33, 4, 260, 2, 4, "hidden")]


def _run_head_bwd_input(ops, B, A, H, act, eh, mis):
    g = _gen(B, A, H, act, 12)
    mean, ls, eps = _head_inputs(g, B, A)
    ga, gl = th.randn(B, A, generator=g), th.randn(B, generator=g)
    w, hid = th.randn(2 * A, H, generator=g) / H ** 0.5, _outputs(act, th.randn(B, H, generator=g))
    action = _squashed64(mean.double(), ls.double(), eps.double())[0].float()
    b = GuardedBufs()
    d_ga, d_gl, d_a = b.put_ro_cols("g_action", ga, A + 3, 3), b.put_ro("g_logp", gl), b.put_ro_cols("action", action, A + 4, 4)
    d_p, d_eps, d_w = b.put_ro("params", th.cat((mean, ls), dim=1)), b.put_ro("eps", eps), b.put_ro("w", w, misalign=int(mis == "w"))
    d_h = b.put_ro_cols("hidden", hid, H + eh, 0, misalign=int(mis == "hidden"))
    gp, dz = b.new("g_params", B, 2 * A), b.new("dz", B, H, misalign=int(mis == "dz"))
    twice(b, lambda: ops.gaussian_head_bwd_input(d_ga, d_gl, d_a, d_p, d_eps, d_w, d_h, act, gp, dz), ("g_params", "dz"))
    return gp.clone(), dz.clone(), (mean, ls, eps, ga, gl, w, hid)


@pytest.mark.parametrize("B,A,H,act,eh,mis", HEAD_BWD_INPUT)
def test_gaussian_head_bwd_input(ops, B, A, H, act, eh, mis):
    gp, dz, (mean, ls, eps, ga, gl, w, hid) = _run_head_bwd_input(ops, B, A, H, act, eh, mis)
    _check_head_bwd(gp[:, :A], gp[:, A:], mean, ls, eps, ga, gl)
    ref_dz = (gp.double().cpu() @ w.double()) * _dact64(hid, act)  # the product in float64, of the launch's own g_params
    assert rel_err(_cpu(dz), ref_dz.numpy(), max(1.0, float(ref_dz.abs().max()))) < 2e-6
    if mis:
        gp0, dz0, _ = _run_head_bwd_input(ops, B, A, H, act, eh, None)
        assert th.equal(gp, gp0) and th.equal(dz, dz0)


# cstr_gaussian_head_gemm_fwd_f32: REFUSES (k & 3), (ldh & 3), hidden / w not 16-byte aligned, act_dim > 4 (CSTR_E_UNSUPPORTED);
# batch <= 1024 -> 4 rows (waves) per workgroup, else 16; a wave per row, 16-byte loads striding 256 columns.
@pytest.mark.parametrize("B,A,K,eh", [(1, 1, 4, 0), (17, 2, 36, 4), (33, 4, 68, 0), (1025, 2, 36, 0), (15, 3, 260, 8)])
def test_gaussian_head_gemm_fwd(ops, B, A, K, eh):
    g = _gen(B, A, K, 13)
    hid = th.randn(B, K, generator=g)
    w, bias, eps = th.randn(2 * A, K, generator=g) / K ** 0.5, th.randn(2 * A, generator=g) * 0.1, th.randn(B, A, generator=g)
    w[A:] *= 0.5  # log_std rows: |raw| stays well inside [-1, 1] in most rows (see _head_inputs)
    b = GuardedBufs()
    d_h, d_w, d_b, d_eps = b.put_ro_cols("hidden", hid, K + eh, 0), b.put_ro("w", w), b.put_ro("bias", bias), b.put_ro("eps", eps)
    params, action, logp = b.new("params", B, 2 * A), b.new_cols("action", B, A + 3, 3, A), b.new("logp", B)
    twice(b, lambda: ops.gaussian_head_gemm_fwd(d_h, d_w, d_b, params, d_eps, None, action, logp), ("params", "action", "logp"))
    ref_p = hid.double() @ w.double().t() + bias.double()
    assert rel_err(_cpu(params), ref_p.numpy(), 1.0) < 2e-6
    p = params.cpu()  # the sampling arithmetic on the launch's own (float32) head outputs
    _check_head_fwd(action, logp, p[:, :A], p[:, A:], eps)
    a64 = _squashed64(ref_p[:, :A], ref_p[:, A:], eps.double())[0]
    assert rel_err(_cpu(action), a64.numpy(), 1.0) < 5e-6


@pytest.mark.parametrize("what", ["k", "ldh", "hidden", "w"])
def test_gaussian_head_gemm_fwd_refuses_unaligned_operands(ops, what):
    from core import _native as nv

    B, A, K = 17, 2, 38 if what == "k" else 36
    ldh = K + (3 if what == "ldh" else 0)
    b = GuardedBufs()
    d_h = b.put_ro_cols("hidden", th.ones(B, K), ldh, 0, misalign=int(what == "hidden"))
    d_w, d_b, d_eps = b.put_ro("w", th.ones(2 * A, K), misalign=int(what == "w")), b.put_ro("bias", th.ones(2 * A)), b.put_ro("eps", th.ones(B, A))
    params, action, logp = b.new("params", B, 2 * A), b.new("action", B, A), b.new("logp", B)
    refused(b, lambda: nv.lib().cstr_gaussian_head_gemm_fwd_f32(nv.ptr(d_h), C.c_int64(ldh), nv.ptr(d_w), nv.ptr(d_b), nv.ptr(params), nv.ptr(d_eps), None,
                                                                nv.ptr(action), C.c_int64(A), nv.ptr(logp), C.c_int64(B), C.c_int(A), C.c_int64(K),
                                                                nv.stream_ptr()), E_UNSUPPORTED, (params, action, logp))


# ------------------------------------------------------------------------------------------------------------- policy network
# cstr_policy_swizzle_f32: REFUSES (k & 3), w / out not 16-byte aligned (CSTR_E_UNSUPPORTED); one thread per 16-byte entry, partial tiles
# and chunks zero-filled.
def _swizzle_ref(w):
    n, k = w.shape
    kc = -(-k // 16)
    out = np.zeros((-(-n // 16), kc, 64, 4), np.float32)
    for tile in range(out.shape[0]):
        for chunk in range(kc):
            for lane in range(64):
                row, col = 16 * tile + (lane & 15), 16 * chunk + 4 * (lane >> 4)
                if row < n and col < k:
                    out[tile, chunk, lane] = w[row, col:col + 4]
    return out.reshape(-1)


@pytest.mark.parametrize("N,K", [(1, 4), (17, 36), (33, 68), (16, 16), (15, 20)])
def test_policy_swizzle(ops, N, K):
    w = th.randn(N, K, generator=_gen(N, K, 14))
    b = GuardedBufs()
    d_w, out = b.put_ro("w", w), b.new("out", ops.swizzled_numel(N, K))
    twice(b, lambda: ops.policy_swizzle(d_w, out))  # (zero fill: "every element written" is the comparison below)
    assert np.array_equal(_cpu(out), _swizzle_ref(w.numpy()))


@pytest.mark.parametrize("what", ["k", "w", "out"])
def test_policy_swizzle_refuses_unaligned_operands(ops, what):
    from core import _native as nv

    N, K = 17, 38 if what == "k" else 36
    b = GuardedBufs()
    d_w = b.put_ro("w", th.ones(N, K), misalign=int(what == "w"))
    out = b.new("out", ops.swizzled_numel(N, K), misalign=int(what == "out"))
    refused(b, lambda: nv.lib().cstr_policy_swizzle_f32(nv.ptr(d_w), C.c_int64(N), C.c_int64(K), nv.ptr(out), nv.stream_ptr()), E_UNSUPPORTED, (out,))


# cstr_policy_rows_fwd_f32:
#   REFUSES k0 > 256, (h1 & 3), (h2 & 3), LDS > 64 KB, w2 / w3 not 16-byte aligned (CSTR_E_UNSUPPORTED), w2_swizzled misaligned (CSTR_E_BADARG)
#   vec0 = (k0 & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(w1)   -> first layer from 16-byte / dword loads (same values, same
#          k order: bit-identical)
#   tile-major W2 given && h1, h2 <= 512 -> the pipelined kernel (split-K head), else the first kernel (shuffle-tree head)
#   pipelined: k0 <= 16 / larger; h1, h2 <= 256 ("small") / larger;  head 0 (squashed Gaussian, eps given) / head 1 (deterministic)
POLICY_ROWS = [  # M, K0, H1, H2, A, act, tile-major W2, x layout, misaligned operand
    (1, 4, 16, 16, 1, 1, False, "contig", None), (15, 3, 36, 20, 2, 2, False, "contig", None), (17, 4, 32, 32, 2, 1, True, "contig", None),
    (33, 20, 36, 68, 4, 1, True, "contig", None), (17, 8, 260, 36, 2, 2, True, "contig", None), (65, 6, 64, 32, 3, 0, True, "contig", None),
    (17, 4, 32, 32, 2, 1, True, "ld+3", None), (17, 4, 32, 32, 2, 1, False, "ld+4", None), (17, 8, 520, 16, 2, 1, True, "contig", None),
    (17, 4, 32, 32, 2, 1, True, "contig", "x"), (17, 4, 32, 32, 2, 1, True, "contig", "w1"), (17, 4, 32, 32, 2, 2, False, "contig", "x"),
    (17, 4, 32, 32, 2, 2, False, "contig", "w1")]


def _policy_operands(b, ops, M, K0, H1, H2, A, swz, mode, mis, n_out):
    g = _gen(M, K0, H1, H2, A, 15)
    r = lambda *sh: th.randn(*sh, generator=g)  # noqa: E731
    v = dict(x=r(1, M, K0), w1=r(H1, K0) / K0 ** 0.5, b1=r(H1) * 0.1, w2=r(H2, H1) / H1 ** 0.5, b2=r(H2) * 0.1,
             w3=r(2 * A, H2) / H2 ** 0.5 * 0.5, b3=r(2 * A) * 0.1, eps=r(M, A))
    d = dict(x=_x_operand(b, "x", v["x"], mode, int(mis == "x"))[0])
    for k in ("w1", "b1", "w2", "b2", "eps"):
        d[k] = b.put_ro(k, v[k], misalign=int(mis == k))
    d["w3"], d["b3"] = b.put_ro("w3", v["w3"][:n_out], misalign=int(mis == "w3")), b.put_ro("b3", v["b3"][:n_out])
    d["swz"] = None
    if swz:
        s = b.new("w2_swz", ops.swizzled_numel(H2, H1), misalign=int(mis == "w2_swz"))
        if mis not in ("w2", "w2_swz"):
            ops.policy_swizzle(d["w2"], s)
            b.freeze("w2_swz")
        d["swz"] = s
    return v, d


def _run_policy_rows(ops, M, K0, H1, H2, A, act, swz, mode, mis):
    outs = []
    for head in (0, 1):
        b = GuardedBufs()
        n_out = 2 * A if head == 0 else A
        v, d = _policy_operands(b, ops, M, K0, H1, H2, A, swz, mode, mis, n_out)
        action = b.new_cols("action", M, A + 5, 5, A)
        if head == 0:
            logp = b.new("logp", M)
            twice(b, lambda: ops.policy_rows_fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["w3"], d["b3"], act, 0, 0, action, eps=d["eps"],
                                                 logp=logp, w2_swz=d["swz"]), ("action", "logp"))
            outs += [action.clone(), logp.clone()]
        else:
            twice(b, lambda: ops.policy_rows_fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["w3"], d["b3"], act, 1, 2, action,
                                                 w2_swz=d["swz"]), ("action",))
            outs.append(action.clone())
    return outs, v


@pytest.mark.parametrize("M,K0,H1,H2,A,act,swz,mode,mis", POLICY_ROWS)
def test_policy_rows_fwd(ops, M, K0, H1, H2, A, act, swz, mode, mis):
    (a0, lp0, a1), v = _run_policy_rows(ops, M, K0, H1, H2, A, act, swz, mode, mis)
    x64 = v["x"][0].double()
    h2 = _act64(_act64(x64 @ v["w1"].double().t() + v["b1"].double(), act) @ v["w2"].double().t() + v["b2"].double(), act)
    p64 = h2 @ v["w3"].double().t() + v["b3"].double()
    a64, lp64, u64 = _squashed64(p64[:, :A], p64[:, A:], v["eps"].double())
    # the bars of test_whole_policy_network_in_one_launch: actions 1e-5, log-probs 2e-4 (log(1 - a^2 + 1e-6) amplifies near saturation)
    assert rel_err(_cpu(a0), a64.numpy(), 1.0) < 1e-5
    assert rel_err(_cpu(lp0), _logp64_of_action(p64[:, :A], p64[:, A:], v["eps"].double(), a0).numpy(), 1.0) < 2e-4
    calm = (u64.abs().max(dim=1).values < 3).numpy()
    assert rel_err(_cpu(lp0)[calm], lp64.numpy()[calm], 1.0) < 2e-4
    assert rel_err(_cpu(a1), th.tanh(p64[:, :A]).numpy(), 1.0) < 1e-5
    if mis:
        (b0, blp, b1), _ = _run_policy_rows(ops, M, K0, H1, H2, A, act, swz, mode, None)
        assert th.equal(a0, b0) and th.equal(lp0, blp) and th.equal(a1, b1)


@pytest.mark.parametrize("what,code", [("w2", E_UNSUPPORTED), ("w3", E_UNSUPPORTED), ("w2_swz", E_BADARG), ("h1", E_UNSUPPORTED), ("h2", E_UNSUPPORTED)])
def test_policy_rows_fwd_refuses_unaligned_operands(ops, what, code):
    from core import _native as nv

    M, K0, A = 17, 4, 2
    H1, H2 = (34 if what == "h1" else 32), (34 if what == "h2" else 32)
    b = GuardedBufs()
    _, d = _policy_operands(b, ops, M, K0, H1, H2, A, what == "w2_swz", "contig", what, 2 * A)
    action, logp = b.new("action", M, A), b.new("logp", M)
    net = nv.PolicyMlp(K0, H1, H2, A, 1, 0, 0, 0, d["w1"].data_ptr(), d["b1"].data_ptr(), d["w2"].data_ptr(), d["b2"].data_ptr(), d["w3"].data_ptr(),
                       d["b3"].data_ptr(), None if d["swz"] is None else d["swz"].data_ptr())
    outputs = (action, logp) + ((d["swz"],) if d["swz"] is not None else ())
    refused(b, lambda: nv.lib().cstr_policy_rows_fwd_f32(C.byref(net), nv.ptr(d["x"]), C.c_int64(K0), nv.ptr(d["eps"]), None, nv.ptr(action), C.c_int64(A),
                                                         nv.ptr(logp), C.c_int64(M), nv.stream_ptr()), code, outputs)


# ---------------------------------------------------------------------------------------------------------- BUF = false bodies
# From 2^28 floats per operand the Linear kernels switch from buffer-descriptor loads (whose range check makes quads outside the matrix
# read as zeros) to plain global loads that do that bounds work themselves: load_k4<VEC>(row, k, K, valid) returns zeros without
# dereferencing for !valid (rows >= m, weight rows >= n) and for k >= K, its float4 form reads [k, k + 4) with k % 4 == 0 and K % 4 == 0;
# the weight gradient's loads stand behind (n_ok && m + e < M) / (k_ok && m + e < M); the input gradient's behind col_ok && n + e < N and
# m < M. The instantiations (every ACT of each) and the cases that launch them:
#   linear_act_fwd_kernel<ACT, VEC, WAVES, false>          test_buf_false_linear_fwd[K-extra-act]: (36, 0) = <true, 4>, (6, 1) = <false, 1>,
#                                                          (32, 0) = <true, 1>, (38, 2) = <false, 4>
#   linear_act_fwd_sets_kernel<ACT, VEC, WAVES, false>     test_buf_false_linear_fwd_sets, the same table
#   linear_bwd_weight_kernel<WAVES, false>                 test_buf_false_bwd_weight[33] = <4>, [17] = <1>
#   linear_bwd_weight_sets_kernel<WAVES, false>            test_buf_false_bwd_weight_sets[33] = <4>, [17] = <1>
#   linear_bwd_input_kernel<ACT, VEC, WAVES, false>        test_buf_false_bwd_input[N-K-act]: (260, 4) = <true, 4>, (257, 4) = <false, 4>,
#                                                          (4, 257) = <true, 1>, (3, 257) = <false, 1>
# x is a [M][ld] view into ONE uninitialised allocation of which only the K used columns of each row are written (and read). The
# reference launch takes a compact copy of the same values (BUF = true): same loads, same MFMA order, so the same bits.
def _strided_rows(M, K, ld, values):
    """[M][ld] float32 device view whose K leading columns hold `values`; the rest of each row is never written or read"""
    block = th.empty((M - 1) * ld + K, dtype=th.float32, device="cuda")
    x = block.as_strided((M, K), (ld, 1))
    x.copy_(values)
    return x


# K, ld - 2^24: (36, 0) vector loads + split-K, (6, 1) dword loads + one wave, (32, 0) vector loads + one wave, (38, 2) dword loads + split-K
BUF_FALSE_FWD = [(36, 0), (6, 1), (32, 0), (38, 2)]


@pytest.mark.parametrize("act", [1, 0, 2])
@pytest.mark.parametrize("K,extra", BUF_FALSE_FWD)
def test_buf_false_linear_fwd(ops, K, extra, act):
    M, N = 17, 17
    ld = 2 ** 24 + extra
    assert M * ld >= 2 ** 28
    g = _gen(M, N, K, 16)
    xv, w, bias = th.randn(1, M, K, generator=g), th.randn(1, N, K, generator=g) / K ** 0.5, th.randn(1, N, generator=g)
    b = GuardedBufs()
    d_w, d_b, xc = b.put_ro("w", w[0]), b.put_ro("bias", bias[0]), b.put_ro("x_compact", xv[0])
    y, y_ref = b.new("y", M, N), b.new("y_ref", M, N)
    x = _strided_rows(M, K, ld, xv[0])
    twice(b, lambda: ops.linear_act_fwd(x, d_w, d_b, act, out=y), ("y",))
    twice(b, lambda: ops.linear_act_fwd(xc, d_w, d_b, act, out=y_ref), ("y_ref",))
    assert th.equal(x, xc) and th.equal(y, y_ref)
    ref = _linear_ref(xv, w, bias, act)[0]
    assert rel_err(_cpu(y), ref.numpy(), max(1.0, float(ref.abs().max()))) < 2e-6


@pytest.mark.parametrize("act", [2, 0, 1])
@pytest.mark.parametrize("K,extra", BUF_FALSE_FWD)
def test_buf_false_linear_fwd_sets(ops, K, extra, act):
    M, N, ld = 17, 17, 2 ** 24 + extra
    g = _gen(M, N, K, 17)
    b = GuardedBufs()
    xv = [th.randn(1, M, K, generator=g) for _ in range(2)]
    wv, bv = [th.randn(1, N, K, generator=g) / K ** 0.5 for _ in range(2)], [th.randn(1, N, generator=g) for _ in range(2)]
    x_big = _strided_rows(M, K, ld, xv[1][0])  # one set beyond the threshold switches the whole launch
    sets, refs = [], []
    for i in range(2):
        d_w, d_b = b.put_ro(f"w{i}", wv[i][0]), b.put_ro(f"b{i}", bv[i][0])
        xc = b.put_ro(f"x{i}", xv[i][0])
        sets.append((x_big if i == 1 else xc, d_w, d_b, b.new_cols(f"y{i}", M, N + 5, 2, N)))
        refs.append((xc, d_w, d_b, b.new_cols(f"r{i}", M, N + 5, 2, N)))
    twice(b, lambda: ops.linear_act_fwd_sets(sets, act), ("y0", "y1"))
    twice(b, lambda: ops.linear_act_fwd_sets(refs, act), ("r0", "r1"))
    for i in range(2):
        ref = _linear_ref(xv[i], wv[i], bv[i], act)[0]
        assert th.equal(sets[i][3], refs[i][3])
        assert rel_err(_cpu(sets[i][3]), ref.numpy(), max(1.0, float(ref.abs().max()))) < 2e-6


@pytest.mark.parametrize("M", [33, 17])
def test_buf_false_bwd_weight(ops, M):
    N, K = 17, 36
    ld = 2 ** 23 if M == 33 else 2 ** 24
    assert M * ld >= 2 ** 28
    g = _gen(M, N, K, 18)
    dzv, xv = th.randn(M, N, generator=g), th.randn(M, K, generator=g)
    b = GuardedBufs()
    dz, xc = b.put_ro("dz", dzv), b.put_ro("x_compact", xv)
    dw, db, rw, rb = b.new("dw", N, K), b.new("db", N), b.new("dw_ref", N, K), b.new("db_ref", N)
    x = _strided_rows(M, K, ld, xv)
    twice(b, lambda: ops.linear_bwd_weight(dz, x, dw, db), ("dw", "db"))
    twice(b, lambda: ops.linear_bwd_weight(dz, xc, rw, rb), ("dw_ref", "db_ref"))
    assert th.equal(x, xc) and th.equal(dw, rw) and th.equal(db, rb)
    scale = float(M) ** 0.5
    assert rel_err(_cpu(dw), (dzv.double().t() @ xv.double()).numpy(), scale) < 2e-6
    assert rel_err(_cpu(db), dzv.double().sum(0).numpy(), scale) < 2e-6


@pytest.mark.parametrize("M", [33, 17])
def test_buf_false_bwd_weight_sets(ops, M):
    ld = 2 ** 23 if M == 33 else 2 ** 24
    g = _gen(M, 19)
    b = GuardedBufs()
    shapes = [(17, 36), (3, 6)]
    dzv, xv = [th.randn(M, n, generator=g) for n, _ in shapes], [th.randn(M, k, generator=g) for _, k in shapes]
    x_big = _strided_rows(M, shapes[0][1], ld, xv[0])
    sets, refs = [], []
    for i, (n, k) in enumerate(shapes):
        dz, xc = b.put_ro(f"dz{i}", dzv[i]), b.put_ro(f"x{i}", xv[i])
        sets.append((dz, x_big if i == 0 else xc, b.new(f"dw{i}", n, k), b.new(f"db{i}", n)))
        refs.append((dz, xc, b.new(f"rw{i}", n, k), b.new(f"rb{i}", n)))
    twice(b, lambda: ops.linear_bwd_weight_sets(sets), ("dw0", "db0", "dw1", "db1"))
    twice(b, lambda: ops.linear_bwd_weight_sets(refs), ("rw0", "rb0", "rw1", "rb1"))
    for i in range(2):
        assert th.equal(sets[i][2], refs[i][2]) and th.equal(sets[i][3], refs[i][3])
        assert rel_err(_cpu(sets[i][2]), (dzv[i].double().t() @ xv[i].double()).numpy(), float(M) ** 0.5) < 2e-6


@pytest.mark.parametrize("as_sets", [False, True])
def test_bwd_weight_rows_past_the_matrix_at_a_huge_row_stride(ops, as_sets):
    """BELOW the 2^28 threshold (33 rows, 5,000,000 floats apart: m * ldx = 1.65e8) the weight gradient reads its operands through buffer
    descriptors and visits rows up to m + 206, trusting the range check to return zeros there. 4 * row * ldx passes 2^32 from row 215 on
    and used to wrap back into the descriptor's range, i.e. to addresses BETWEEN the real rows: filled with NaN here, they turned every
    dW into NaN (0 * NaN). The dispatcher now sends such strides to the plain-load body."""
    M, N, K, ld = 33, 17, 36, 5_000_000
    assert M * ld < 2 ** 28 and 4 * 215 * ld >= 2 ** 32 and 4 * 215 * ld - 2 ** 32 < 4 * ((M - 1) * ld + K)
    g = _gen(M, N, K, 22)
    dzv, xv = th.randn(M, N, generator=g), th.randn(M, K, generator=g)
    b = GuardedBufs()
    dz, xc = b.put_ro("dz", dzv), b.put_ro("x_compact", xv)
    dw, db, rw, rb = b.new("dw", N, K), b.new("db", N), b.new("dw_ref", N, K), b.new("db_ref", N)
    block = th.full(((M - 1) * ld + K,), float("nan"), dtype=th.float32, device="cuda")
    x = block.as_strided((M, K), (ld, 1))
    x.copy_(xv)
    if as_sets:
        twice(b, lambda: ops.linear_bwd_weight_sets([(dz, x, dw, db)]), ("dw", "db"))
    else:
        twice(b, lambda: ops.linear_bwd_weight(dz, x, dw, db), ("dw", "db"))
    twice(b, lambda: ops.linear_bwd_weight(dz, xc, rw, rb), ("dw_ref", "db_ref"))
    assert bool(th.isfinite(dw).all()) and th.equal(dw, rw) and th.equal(db, rb)
    assert rel_err(_cpu(dw), (dzv.double().t() @ xv.double()).numpy(), float(M) ** 0.5) < 2e-6


# N, K, act: the issue's two cases first (m * n reaches the threshold), the other activations, and m * k reaching it with n <= 32
BUF_FALSE_BWD_INPUT = [(257, 4, 1), (260, 4, 1), (257, 4, 0), (260, 4, 2), (257, 4, 2), (260, 4, 0),
                       (4, 257, 1), (3, 257, 1), (4, 257, 0), (3, 257, 2), (4, 257, 2), (3, 257, 0)]


@pytest.mark.parametrize("N,K,act", BUF_FALSE_BWD_INPUT)
def test_buf_false_bwd_input(ops, N, K, act):
    """The input gradient's threshold is on the contiguous m * n (and m * k): the largest m the grid admits, n (or k) just above 2^28 / m;
    n % 4 == 0 takes the 16-byte loads of gz, otherwise the dword loads; n > 32 four waves. Bit for bit against BUF = true launches over
    slabs of 2^19 rows of the same gz; float64 on the first and last 64 rows and on 1024 rows drawn with a fixed seed."""
    M, slab = 1048560, 2 ** 19
    assert (M * N >= 2 ** 28 or M * K >= 2 ** 28) and slab * max(N, K) < 2 ** 28
    free, _ = th.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of free device memory, {free / 2 ** 30:.2f} GiB are free")
    g = th.Generator(device="cuda").manual_seed(1000 * N + K)
    gz = th.randn(M, N, device="cuda", generator=g)
    yv = th.randn(M, K, device="cuda", generator=g)
    yv = th.relu(yv) if act == 1 else (th.tanh(yv) if act == 2 else yv)
    w = th.randn(N, K, generator=_gen(N, K, 20)) / N ** 0.5
    b = GuardedBufs()
    d_w, dz, dz_ref = b.put_ro("w", w), b.new("dz", M, K), b.new("dz_ref", M, K)
    gz0, y0 = gz.clone(), yv.clone()
    twice(b, lambda: _bwd_input(gz, d_w, yv, act, dz, 1, False, M, N, K), ("dz",))
    for r0 in range(0, M, slab):
        r1 = min(M, r0 + slab)
        _bwd_input(gz[r0:r1], d_w, yv[r0:r1], act, dz_ref[r0:r1], 1, False, r1 - r0, N, K)
    b.check(("dz_ref",))
    assert th.equal(gz, gz0) and th.equal(yv, y0) and th.equal(dz, dz_ref)
    rows = th.cat([th.arange(64), th.arange(M - 64, M), th.randint(0, M, (1024,), generator=_gen(N, K, 21))]).cuda()
    ref = (gz[rows].double() @ w.double().cuda()) * _dact64(yv[rows], act)
    assert rel_err(_cpu(dz[rows]), _cpu(ref), max(1.0, float(ref.abs().max()))) < 2e-6
