"""GPU checks of the gSDE kernels (csrc/cstr_sde.hip) and of the BCQ kernels (csrc/cstr_bcq.hip), launch by launch, across shapes,
strides, optional operands and the in-kernel noise streams.

Every launch is compared with the fp64 statement of its own contract (tests/_rowkernel_reference.py) on the float32 inputs it reads:
a backward launch reads the forward launch's own stored outputs, the parameter-gradient launch the backward launch's own per-row
gradients. Reduced outputs and gradients are measured per element in units of 2**-24 * M, M from the statement's magnitude pass; the
bar of an output kind is four times the worst figure of the float32 ATen evaluation of the same statement over the cases of this
module (measured on the CPU, re-checked by tests/test_rowkernel_reference.py; no bar above 64 units). A `BAR ...` line is printed
before every assertion.

    kind         ATen     bar    kernel worst
    pre          5.202  20.81    1.225
    var         12.338  49.35    3.064
    g_pre        2.201   8.80    2.053
    g_x          3.405  13.62    4.108
    g_var        4.586  18.34    5.873
    dh           3.196  12.78    3.179
    dw           3.810  15.24    2.373
    db           1.630   6.52    0.886
    dlog_std     4.445  17.78    3.528
    bcq_z        1.850   7.40    1.896
    bcq_g_mean   1.000   4.00    1.000
    bcq_g_ls     2.681  10.72    2.625
    vae_loss     1.790   7.16    1.038
    vae_g_recon  1.717   6.87    2.075
    vae_g_mean   0.994   3.97    1.514
    vae_g_std    2.236   8.94    3.271
    perturb      1.355   5.42    1.355
    perturb_g    0.950   3.80    0.950
    target       1.702   6.81    1.702

Transcendental stages keep the tolerances tests/test_sde.py and tests/test_bcq.py apply to the same quantities: the gSDE action rtol
1e-4 / atol 2e-5, its log-prob 2e-4 of max(1, |reference|), std = exp(...) and the matrices rtol 2e-6. Drawn normals are compared with
the NumPy statement of the counter contract (normal_stream): the bar is four times the worst error of the float32 NumPy Box-Muller
over the drawn launches of this module, 9.78e-6 (float32 NumPy: 2.44e-6; not above 1e-5); the ~5e-4 of the elements whose uniform
float32 cannot hold get the bar plus the radius change of that representation error (normal_slack, see the reference module).
Kernel worst: 1.03e-6 outside those elements, 1.9e-9 beyond the slack inside them.

Input conditions, asserted before each launch: (a) no Hardtanh or clamp pre-activation of a sweep case within the bar of its bound,
except those placed exactly on a bound on purpose; (b) gSDE rows with |x| > 4 (atanh of a float32 tanh is ill-conditioned) are left out
of the log-prob and gradient comparison, at most B / 16 rows of a case and none for B < 16; such a row is still checked for its
action and for finite values.

Copies, clamps of given values and selections (state columns, clipped noise, indices, gathered actions, max_q, a gradient whose other
term is absent) are compared bit for bit. Every output buffer is filled with a sentinel and followed by 64 sentinel floats; every
launch runs twice and must repeat itself bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import _rowkernel_reference as R
from _sentinel_bufs import DEV, SENT, Bufs

pytestmark = pytest.mark.gpu
FIGS, NORMALS = {}, {"plain": 0.0, "slack": 0.0}
i64, cint, f32c = C.c_int64, C.c_int, C.c_float
F = np.float32


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def nv():
    from core import _native

    return _native


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def get(b, name, *shape):
    f, n = b.flat[name]
    return f[:n].view(*shape) if shape else f[:n]


def block(a, ld, col0):
    """a [rows, w] as the column block [col0, col0 + w) of a fresh sentinel-filled [rows, ld] device matrix (a row-strided view)"""
    a = np.asarray(a, F)
    t = th.full((a.shape[0], ld), SENT, dtype=th.float32, device=DEV)
    t[:, col0:col0 + a.shape[1]] = dev(a)
    return t[:, col0:col0 + a.shape[1]]


def twice(launch):
    b, b2 = launch(), launch()
    b2.same_as(b.snapshot())
    return b


def bits(a, b):
    a, b = (host(v) if isinstance(v, th.Tensor) else np.asarray(v) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bar(kind, got, want, mag, what, bad, rows=None):
    """the kernel's worst element of one output in units of 2**-24 * M: printed, recorded, judged against the kind's bar"""
    got, want, mag = (host(v) if isinstance(v, th.Tensor) else np.asarray(v) for v in (got, want, mag))
    if rows is not None:
        got, want, mag = got[rows], want[rows], mag[rows]
    if got.size == 0:
        return
    fig, _ = R.worst(got, want, mag)
    FIGS[kind] = max(FIGS.get(kind, 0.0), fig)
    print(f"BAR {what} {kind}: {fig:.3f} of {R.BARS[kind]:.2f} units")
    if not fig <= R.BARS[kind]:
        bad.append((what, kind, round(fig, 3)))


def normals(got, seed, base, n_total, tag, what, sl=slice(None)):
    """drawn values against the stream at the given offset: the bar outside the slack elements, bar + slack inside them"""
    got = (host(got) if isinstance(got, th.Tensor) else np.asarray(got)).astype(np.float64).reshape(-1)
    want, slack = R.normal_stream(seed, base, n_total, tag)[sl], R.normal_slack(seed, base, n_total, tag)[sl]
    assert got.shape == want.shape
    if not got.size:
        return
    err, plain = np.abs(got - want), slack == 0
    w = float(err[plain].max()) if plain.any() else 0.0
    ws = float((err - slack)[~plain].max()) if (~plain).any() else 0.0
    NORMALS["plain"], NORMALS["slack"] = max(NORMALS["plain"], w), max(NORMALS["slack"], ws)
    print(f"BAR {what} drawn normals: {w:.3g} (beyond the slack of {int((~plain).sum())} elements: {ws:.3g}) of {R.NORMAL_BAR:.3g}")
    assert w <= R.NORMAL_BAR and ws <= R.NORMAL_BAR and (~plain).mean() <= 1e-3, (what, w, ws)


def ctl_at(ops, seed, base):
    ctl = ops.new_rng_ctl(seed, DEV)
    ctl[1] = base
    return ctl


def ident(case):
    return "-".join(str(v) for v in case)


# ---- gSDE: draw (given z), head forward, head backward, parameter gradients -----------------------------------------------------------
def sde_draw_given(ops, inp, std_out=True):
    z = inp["z"]
    n, L, A = z.shape
    ls_t, z_t = dev(inp["log_std"]), dev(z)

    def launch():
        b = Bufs()
        mats, std = b.new("mats", n, L, A), (b.new("std", L, A) if std_out else None)
        ops.sde_draw(ls_t, A, inp["expln"], z_t, mats, std)
        b.check(written=["mats"] + (["std"] if std_out else []))
        assert bits(z_t, z)  # a given z is read, never written
        return b
    return twice(launch)


def sde_operands(inp, std_t, mats_t, strided):
    B, L = inp["h"].shape
    h = block(inp["h"], L + 3, 2) if strided else dev(inp["h"])
    m = None if inp["noise"] == "mode" else (mats_t if inp["noise"] == "per_row" else mats_t[0])
    return h, dev(inp["w"]), dev(inp["b"]), m, std_t


def sde_fwd(ops, inp, std_t, mats_t, strided, want=("logp", "aux")):
    B, L = inp["h"].shape
    A = inp["w"].shape[0]
    h, w, bias, m, std = sde_operands(inp, std_t, mats_t, strided)

    def launch():
        b = Bufs()
        wide = b.new("action", B, 3 + A) if strided else None
        action = wide[:, 3:] if strided else b.new("action", B, A)
        lp = b.new("logp", B) if "logp" in want else None
        aux = b.new("aux", B, 2 * A) if "aux" in want else None
        ops.sde_head_fwd(h, w, bias, inp["clip"], m, std, action, lp, aux)
        b.check(written=[k for k in want] + ([] if strided else ["action"]))
        if strided:  # the other columns of the [B, 3 + A] buffer keep their sentinel
            assert bool((wide[:, :3] == SENT).all()) and not bool((wide[:, 3:] == SENT).any())
        return b
    b = twice(launch)
    out = {k: host(get(b, k)).copy() for k in want}
    out["logp"] = out["logp"] if "logp" in out else None
    if "aux" in out:
        out["aux"] = out["aux"].reshape(B, 2 * A)
    out["action"] = host(get(b, "action", B, 3 + A)[:, 3:] if strided else get(b, "action", B, A)).copy()
    return out


def sde_bwd(ops, binp, std_t, mats_t, strided, want=("g_pre", "g_x", "g_var", "dh")):
    B, L = binp["h"].shape
    A = binp["w"].shape[0]
    h, w, _, m, std = sde_operands(binp, std_t, mats_t, strided)
    action = block(binp["action"], 3 + A, 3) if strided else dev(binp["action"])
    ga = None if binp.get("g_action") is None else (block(binp["g_action"], A + 2, 1) if strided else dev(binp["g_action"]))
    gl = None if binp.get("g_logp") is None else dev(binp["g_logp"])
    aux = dev(binp["aux"])

    def launch():
        b = Bufs()
        o = {k: (b.new(k, B, L if k == "dh" else A) if k in want else None) for k in ("g_pre", "g_x", "g_var", "dh")}
        ops.sde_head_bwd(ga, gl, action, aux, h, w, binp["clip"], m, std, binp["below"], o["g_pre"], o["g_x"], o["g_var"], o["dh"])
        b.check(written=list(want))
        return b
    b = twice(launch)
    return {k: host(get(b, k, B, L if k == "dh" else A)).copy() for k in want}


def sde_param(ops, pinp, std_t, strided, want=("dw", "db", "dlog_std")):
    B, L = pinp["h"].shape
    A = pinp["w"].shape[0]
    cols = pinp["log_std"].shape[1]
    h = block(pinp["h"], L + 3, 2) if strided else dev(pinp["h"])
    gp, gx, gv = (dev(pinp[k]) for k in ("g_pre", "g_x", "g_var"))
    z = None if pinp["z"] is None else dev(pinp["z"])
    ls = dev(pinp["log_std"])
    shapes = dict(dw=(A, L), db=(A,), dlog_std=(L, cols))

    def launch():
        b = Bufs()
        o = {k: (b.new(k, *shapes[k]) if k in want else None) for k in shapes}
        ops.sde_param_grad(h, gp, gx, gv, z, std_t, ls, pinp["expln"], o["dw"], o["db"], o["dlog_std"])
        b.check(written=list(want))
        return b
    b = twice(launch)
    return {k: host(get(b, k, *shapes[k])).copy() for k in want}


def sde_chain(ops, inp, what, bad, strided=False):
    """the four launches on one case, each twice, each against its statement; returns every output for the bit-for-bit comparisons"""
    B, L = inp["h"].shape
    A, noise, clip = inp["w"].shape[0], inp["noise"], inp["clip"]
    bd = sde_draw_given(ops, inp)
    std_t, mats_t = get(bd, "std", L, A), get(bd, "mats", *inp["z"].shape)
    std_g, mats_g = host(std_t).copy(), host(mats_t).copy()
    std64 = R.sde_std_stmt(inp["log_std"], inp["expln"], A).numpy()
    np.testing.assert_allclose(std_g, std64, rtol=2e-6, atol=0)
    np.testing.assert_allclose(mats_g, inp["z"].astype(np.float64) * std64, rtol=2e-6, atol=0)
    own = dict(inp, std=std_g, mats=None if noise == "mode" else (mats_g if noise == "per_row" else mats_g[0]))
    f, m = R.np64(R.sde_fwd_stmt(own)), R.np64(R.sde_fwd_stmt(own, mag=True))
    margin = R.hardtanh_margin(f["pre"], m["pre"], clip, R.BARS["pre"])  # condition (a)
    sat = R.sat_rows(f["x"])                                             # condition (b)
    print(f"BAR {what} Hardtanh margin: {margin:.3f} (>= 1); rows with |x| > 4: {int(sat.sum())} of {B}")
    assert margin >= 1.0 and sat.sum() <= (B // 16 if B >= 16 else 0), what
    keep = ~sat
    fw = sde_fwd(ops, own, std_t, mats_t, strided)
    bar("pre", fw["aux"][:, :A], f["pre"], m["pre"], what, bad)
    bar("var", fw["aux"][:, A:], f["var"], m["var"], what, bad)
    np.testing.assert_allclose(fw["action"], f["action"], rtol=1e-4, atol=2e-5)
    assert np.isfinite(fw["logp"]).all()
    if keep.any():
        err = np.abs(fw["logp"] - f["logp"]) / np.maximum(1.0, np.abs(f["logp"]))
        print(f"BAR {what} logp: {err[keep].max():.3g} of 2e-4")
        assert err[keep].max() < 2e-4, what
    binp = R.sde_bwd_inputs(own, fw["action"], fw["aux"])
    bw = sde_bwd(ops, binp, std_t, mats_t, strided)
    ref, mg = R.np64(R.sde_bwd_stmt(binp)), R.np64(R.sde_bwd_stmt(binp, mag=True))
    for k in ("g_pre", "g_x", "g_var", "dh"):
        assert np.isfinite(bw[k]).all(), (what, k)
        bar(k, bw[k], ref[k], mg[k], what, bad, rows=keep)
    if clip > 0 and B >= 3:  # a pre-clip mean exactly on the bound: hardtanh_backward gives zero AT the bound
        assert bw["g_pre"][1, 0] == 0.0 and bw["g_pre"][2, 0] == 0.0, what
    if noise == "mode":
        assert not bw["g_x"].any()
    out = dict(std=std_g, mats=mats_g, own=own, binp=binp, std_t=std_t, mats_t=mats_t, **fw, **bw)
    if noise != "per_row":
        pinp = dict(own, z=inp["z"][0] if noise == "shared" else None, **{k: bw[k] for k in ("g_pre", "g_x", "g_var")})
        pg = sde_param(ops, pinp, std_t, strided)
        ref, mg = R.np64(R.sde_param_stmt(pinp)), R.np64(R.sde_param_stmt(pinp, mag=True))
        for k in ("dw", "db", "dlog_std"):
            bar(k, pg[k], ref[k], mg[k], what, bad)
        out.update(pinp=pinp, **pg)
    return out


@pytest.mark.parametrize("noise", R.SDE_NOISE)
@pytest.mark.parametrize("si", range(len(R.SDE_SHAPES)), ids=lambda i: ident(R.SDE_SHAPES[i]))
def test_sde_launches_against_fp64(ops, si, noise):
    bad = []
    for vi, v in enumerate(R.sde_variants(si)):
        if v[2] == noise:
            sde_chain(ops, R.sde_case(si, vi), f"sde {ident(R.SDE_SHAPES[si])} full={v[0]} expln={v[1]} {noise} below={v[3]} clip={v[4]}", bad)
    assert not bad, bad


@pytest.mark.parametrize("noise", R.SDE_NOISE)
@pytest.mark.parametrize("si", R.SDE_STRIDED, ids=lambda i: ident(R.SDE_SHAPES[i]))
def test_sde_strides_and_optional_operands(ops, si, noise):
    """h a column block of [B, L + 3] rows, action a column block of a [B, 3 + A] buffer, g_action strided: the same bits as the
    contiguous launches. Each optional output left out in turn: the outputs that remain keep their bits. Each optional operand left
    out in turn: against the statement without it."""
    bad = []
    vi = next(i for i, v in enumerate(R.sde_variants(si)) if v[2] == noise and v[4] > 0)
    inp = R.sde_case(si, vi)
    what = f"sde strided {ident(R.SDE_SHAPES[si])} {noise}"
    c, s = sde_chain(ops, inp, what, bad), sde_chain(ops, inp, what + " strided", bad, strided=True)
    keys = ["std", "mats", "action", "logp", "aux", "g_pre", "g_x", "g_var", "dh"] + (["dw", "db", "dlog_std"] if noise != "per_row" else [])
    for k in keys:
        assert bits(c[k], s[k]), (what, k)
    own, binp, std_t, mats_t = c["own"], c["binp"], c["std_t"], c["mats_t"]
    B, L = inp["h"].shape
    assert bits(host(get(sde_draw_given(ops, inp, std_out=False), "mats", *inp["z"].shape)), c["mats"])
    for want in (("logp",), ("aux",), ()):
        o = sde_fwd(ops, own, std_t, mats_t, False, want=want)
        assert bits(o["action"], c["action"]) and all(bits(o[k], c[k]) for k in want), (what, want)
    full = ("g_pre", "g_x", "g_var", "dh")
    for drop in full:
        want = tuple(k for k in full if k != drop)
        o = sde_bwd(ops, binp, std_t, mats_t, False, want=want)
        assert all(bits(o[k], c[k]) for k in want), (what, drop)
    keep = ~R.sat_rows(R.np64(R.sde_fwd_stmt(own))["x"])
    for drop in ("g_action", "g_logp"):
        part = dict(binp, **{drop: None})
        o = sde_bwd(ops, part, std_t, mats_t, strided=drop == "g_logp")
        ref, mg = R.np64(R.sde_bwd_stmt(part)), R.np64(R.sde_bwd_stmt(part, mag=True))
        for k in full:
            bar(k, o[k], ref[k], mg[k], f"{what} without {drop}", bad, rows=keep)
        if drop == "g_logp":
            assert not o["g_var"].any()  # the variance enters the log-prob only
    if noise != "per_row":
        fullp = ("dw", "db", "dlog_std")
        for drop in fullp:
            want = tuple(k for k in fullp if k != drop)
            o = sde_param(ops, c["pinp"], std_t, False, want=want)
            assert all(bits(o[k], c[k]) for k in want), (what, drop)
    assert not bad, bad


@pytest.mark.parametrize("case", R.SDE_DRAWS, ids=ident)
def test_sde_draw_against_the_stream(ops, case):
    """z drawn in the kernel: the kept matrices' z against normal_stream, the z buffer beyond z_keep untouched, mats = draw * std, the
    offset advanced by the pairs drawn, a second launch on the same control block at base + pairs"""
    n, L, A, keep, seed, base = case
    per, total = L * A, n * L * A
    pairs = (total + 1) // 2
    ls = np.random.default_rng(n + L).normal(-1.0, 0.8, (L, A)).astype(F)
    ls_t = dev(ls)

    def launch(ctl):
        b = Bufs()
        z, mats, std = b.new("z", n, L, A), b.new("mats", n, L, A), b.new("std", L, A)
        ops.sde_draw(ls_t, A, False, z, mats, std, rng_ctl=ctl, z_keep=keep)
        b.check(written=["mats", "std"])
        return b

    def judge(b, offset, what):
        z, mats, std = host(get(b, "z")), host(get(b, "mats")), host(get(b, "std"))
        std_all = np.tile(std.astype(np.float64), n)
        assert (z[keep * per:] == F(SENT)).all(), "z beyond z_keep was written"
        normals(z[:keep * per], seed, offset, total, R.SDE_TAG, what, slice(0, keep * per))
        assert bits(mats[:keep * per], z[:keep * per] * np.tile(std, keep))  # the stored z is the z that was used
        draw = mats.astype(np.float64) / std_all  # mats = draw * std to rounding: one float32 product, 2**-24 of |draw|
        want, slack = R.normal_stream(seed, offset, total, R.SDE_TAG), R.normal_slack(seed, offset, total, R.SDE_TAG)
        err = np.abs(draw - want) - slack - 2.0 ** -23 * np.abs(want)
        assert err.max() <= R.NORMAL_BAR, (what, err.max())

    ctl = ctl_at(ops, seed, base)
    b1 = launch(ctl)
    assert int(ctl[0]) == seed and int(ctl[1]) == base + pairs and int(ctl[2]) == 0
    launch(ctl_at(ops, seed, base)).same_as(b1.snapshot())
    judge(b1, base, f"sde_draw {ident(case[:4])}")
    np.testing.assert_allclose(host(get(b1, "std", L, A)), np.exp(ls.astype(np.float64)), rtol=2e-6, atol=0)
    b2 = launch(ctl)
    assert int(ctl[1]) == base + 2 * pairs and int(ctl[2]) == 0
    judge(b2, base + pairs, f"sde_draw {ident(case[:4])} second launch")


# ---- BCQ: latent ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.BCQ_LATENT_SHAPES)), ids=lambda i: ident(R.BCQ_LATENT_SHAPES[i]))
def test_bcq_latent_against_fp64(ops, nv, i):
    B, D, L = R.BCQ_LATENT_SHAPES[i]
    what, bad, lib = f"bcq latent {B}-{D}-{L}", [], nv.lib()
    inp = R.bcq_latent_inputs(R.BCQ_SEED_BASE + i, B, D, L)
    params_t, obs_t, eps_t = dev(inp["params"]), block(inp["obs"], D + 2, 0), dev(inp["eps"])

    def launch():
        b = Bufs()
        xdec, std = b.new("xdec", B, D + L), b.new("std", B, L)
        ops.bcq_latent_fwd(params_t, obs_t, eps_t, None, xdec, std)
        b.check(written=["xdec", "std"])
        return b
    b = twice(launch)
    xdec_g, std_t = host(get(b, "xdec", B, D + L)), get(b, "std", B, L)
    std_g = host(std_t)
    assert bits(xdec_g[:, :D], inp["obs"])
    np.testing.assert_allclose(std_g, R.np64(R.bcq_latent_fwd_stmt(inp))["std"], rtol=2e-6, atol=0)
    ref, mg = R.np64(R.bcq_latent_fwd_stmt(inp, std=std_g)), R.np64(R.bcq_latent_fwd_stmt(inp, mag=True, std=std_g))
    bar("bcq_z", xdec_g[:, D:], ref["bcq_z"], mg["bcq_z"], what, bad)
    # ldp = 2 L + 2 and ldx = D + L + 1 through the C entry: the same bits, the gap column keeps its sentinel
    pw = block(inp["params"], 2 * L + 2, 0)

    def launch_wide():
        bw = Bufs()
        xw, std = bw.new("xw", B, D + L + 1), bw.new("std", B, L)
        ops.check(lib.cstr_bcq_latent_fwd_f32(ops.ptr(pw), i64(2 * L + 2), ops.ptr(obs_t), i64(D + 2), ops.ptr(eps_t), ops.ptr(None), ops.ptr(xw),
                                              i64(D + L + 1), ops.ptr(std), ops.ptr(None), i64(B), cint(D), cint(L), ops.stream_ptr()), "latent_fwd")
        bw.check(written=["std"])
        return bw
    bw = twice(launch_wide)
    xw = host(get(bw, "xw", B, D + L + 1))
    assert bits(xw[:, :D + L], xdec_g) and (xw[:, D + L] == F(SENT)).all() and bits(get(bw, "std", B, L), std_g)
    # backward: full, then each gradient source left out
    raw = inp["params"][:, L:]
    inside, on = (raw >= -4.0) & (raw <= 15.0), (raw == -4.0) | (raw == 15.0)
    assert on.any() and (B * L < 5 or (~inside).any())
    full = None
    for drop in (None, "g_z", "g_mean_kl", "g_std_kl"):
        binp = dict(inp, std=std_g)
        if drop:
            binp[drop] = None
        gz_t = None if drop == "g_z" else block(inp["g_z"], D + L, D)  # the latent columns of the decoder input's gradient
        gm_t, gs_t = (None if drop == k else dev(inp[k]) for k in ("g_mean_kl", "g_std_kl"))

        def launch_bwd(via_c=False):
            bb = Bufs()
            gp = bb.new("g_params", B, 2 * L)
            if via_c:
                ops.check(lib.cstr_bcq_latent_bwd_f32(ops.ptr(gz_t), i64(D + L), ops.ptr(gm_t), ops.ptr(gs_t), ops.ptr(pw), i64(2 * L + 2), ops.ptr(std_t),
                                                      ops.ptr(eps_t), ops.ptr(gp), i64(B), cint(L), ops.stream_ptr()), "latent_bwd")
            else:
                ops.bcq_latent_bwd(gz_t, gm_t, gs_t, params_t, std_t, eps_t, gp)
            bb.check(written=["g_params"])
            return bb
        got = host(get(twice(launch_bwd), "g_params", B, 2 * L))
        ref, mg = R.np64(R.bcq_latent_bwd_stmt(binp)), R.np64(R.bcq_latent_bwd_stmt(binp, mag=True))
        bar("bcq_g_mean", got[:, :L], ref["bcq_g_mean"], mg["bcq_g_mean"], f"{what} without {drop}", bad)
        bar("bcq_g_ls", got[:, L:], ref["bcq_g_ls"], mg["bcq_g_ls"], f"{what} without {drop}", bad)
        assert not got[:, L:][~inside].any()  # beyond the clamp: cut
        if drop is None:
            full = got
            assert (got[:, L:][on] != 0).all()  # exactly on a bound: the closed interval passes the gradient
            assert bits(host(get(launch_bwd(via_c=True), "g_params", B, 2 * L)), got)  # ldp = 2 L + 2
        if drop == "g_z":
            assert bits(got[:, :L], inp["g_mean_kl"])
        if drop == "g_mean_kl":
            assert bits(got[:, :L], inp["g_z"]) and bits(got[:, L:], full[:, L:])
    assert not bad, bad


@pytest.mark.parametrize("case", R.BCQ_LATENT_DRAWS, ids=ident)
def test_bcq_latent_draw_against_the_stream(ops, case):
    B, D, L, seed, base = case
    total = B * L
    pairs, what, bad = (total + 1) // 2, f"bcq latent draw {B}-{D}-{L}", []
    g = np.random.default_rng(B + L)
    params, obs = g.normal(0, 1.0, (B, 2 * L)).astype(F), g.uniform(-1, 1, (B, D)).astype(F)
    params_t, obs_t = dev(params), dev(obs)

    def launch(ctl):
        b = Bufs()
        xdec, std, eps = b.new("xdec", B, D + L), b.new("std", B, L), b.new("eps", B, L)
        ops.bcq_latent_fwd(params_t, obs_t, None, ctl, xdec, std, eps)
        b.check(written=["xdec", "std", "eps"])
        return b

    def judge(b, offset, what):
        xdec, std, eps = host(get(b, "xdec", B, D + L)), host(get(b, "std", B, L)), host(get(b, "eps", B, L))
        normals(eps, seed, offset, total, R.BCQ_TAG, what)
        assert bits(xdec[:, :D], obs)
        inp = dict(params=params, eps=eps)  # z = mean + std * eps on the launch's own std and eps
        ref, mg = R.np64(R.bcq_latent_fwd_stmt(inp, std=std)), R.np64(R.bcq_latent_fwd_stmt(inp, mag=True, std=std))
        bar("bcq_z", xdec[:, D:], ref["bcq_z"], mg["bcq_z"], what, bad)

    ctl = ctl_at(ops, seed, base)
    b1 = launch(ctl)
    assert int(ctl[1]) == base + pairs and int(ctl[2]) == 0
    launch(ctl_at(ops, seed, base)).same_as(b1.snapshot())
    judge(b1, base, what)
    b2 = launch(ctl)
    assert int(ctl[1]) == base + 2 * pairs and int(ctl[2]) == 0
    judge(b2, base + pairs, what + " second launch")
    assert not bad, bad


# ---- BCQ: VAE loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.BCQ_VAE_SHAPES)), ids=lambda i: ident(R.BCQ_VAE_SHAPES[i]))
def test_bcq_vae_loss_against_fp64(ops, i):
    B, A, L = R.BCQ_VAE_SHAPES[i]
    what, bad = f"bcq vae {B}-{A}-{L}", []
    inp = R.bcq_vae_inputs(R.BCQ_SEED_BASE + 100 + i, B, A, L)
    recon_t, act_t, params_t, std_t = dev(inp["recon"]), block(inp["act"], A + 4, 4), dev(inp["params"]), dev(inp["std"])
    shapes = dict(g_recon=(B, A), g_mean=(B, L), g_std=(B, L), loss_out=(1,), loss_sum=(1,))

    def run(want):
        def launch():
            b = Bufs()
            o = {k: ((b.put(k, np.full(1, 2.0, F)) if k == "loss_sum" else b.new(k, *shapes[k])) if k in want else None) for k in shapes}
            ops.bcq_vae_loss(recon_t, act_t, params_t, std_t, o["g_recon"], o["g_mean"], o["g_std"], o["loss_out"], o["loss_sum"])
            b.check(written=list(want))
            return b
        b = twice(launch)
        return {k: host(get(b, k, *shapes[k])).copy() for k in want}
    full = run(tuple(shapes))
    ref, mg = R.np64(R.bcq_vae_stmt(inp)), R.np64(R.bcq_vae_stmt(inp, mag=True))
    bar("vae_loss", full["loss_out"], ref["vae_loss"], mg["vae_loss"], what, bad)
    for k in ("g_recon", "g_mean", "g_std"):
        bar("vae_" + k, full[k], ref["vae_" + k], mg["vae_" + k], what, bad)
    assert bits(full["loss_sum"], F(2.0) + full["loss_out"])
    for want in (("loss_out",), ("loss_sum",), ("g_recon", "g_mean", "g_std"), ("g_recon",), ("g_mean",), ("g_std",)):
        o = run(want)
        assert all(bits(o[k], full[k]) for k in want), (what, want)
    b = Bufs()  # loss_sum accumulates over two launches
    total = b.put("loss_sum", np.full(1, 2.0, F))
    for _ in range(2):
        ops.bcq_vae_loss(recon_t, act_t, params_t, std_t, loss_sum=total)
    b.check()
    assert bits(total, (F(2.0) + full["loss_out"]) + full["loss_out"])
    assert not bad, bad


# ---- BCQ: expand ----------------------------------------------------------------------------------------------------------------------
def expand_buffers(b, rows, D, L, A, kind):
    xdec, xa = b.new("xdec", rows, D + L), b.new("xa", rows, D + A)
    if kind == "vec_a":  # xb 4 bytes off a 16-byte boundary: its rows are stored as scalars
        xb = b.new("xb", rows * (D + A) + 1)[1:].view(rows, D + A)
    else:
        xb = b.new("xb", rows, D + A)
    return xdec, xa, xb


def expand_state(state, D, A, kind):
    if kind == "scalar":
        return block(state, D + A, 0)
    if kind == "misaligned":
        flat = th.full((state.size + 1,), SENT, dtype=th.float32, device=DEV)
        flat[1:] = dev(state).reshape(-1)
        return flat[1:].view(*state.shape)
    return dev(state)


def expand_paths(state_t, xdec, xa, xb, D):
    """the host's choice of instantiation and store widths (cstr_bcq_expand_f32), restated: the case must run the path it is named for"""
    al = lambda t: t.data_ptr() % 16 == 0  # noqa: E731
    vec = D % 4 == 0 and al(state_t) and al(xdec) and state_t.stride(0) % 4 == 0 and xdec.stride(0) % 4 == 0
    return vec, al(xa) and xa.stride(0) % 4 == 0, al(xb) and xb.stride(0) % 4 == 0


EXPAND_PATHS = {"scalar": (False, None, None), "vec": (True, False, False), "vec_ab": (True, True, True), "vec_a": (True, True, False),
                "misaligned": (False, True, True)}


@pytest.mark.parametrize("case", R.BCQ_EXPAND_CASES, ids=ident)
def test_bcq_expand_bit_for_bit(ops, case):
    n, S, D, L, A, kind = case
    rows = n * S
    g = np.random.default_rng(rows + L)
    state, noise = g.uniform(-1, 1, (n, D)).astype(F), g.normal(0, 1, (rows, L)).astype(F)
    state_t, noise_t = expand_state(state, D, A, kind), dev(noise)
    rep, clipped = R.bcq_expand_stmt(state, noise, S, 0.5)

    def launch(with_ab=True):
        b = Bufs()
        xdec, xa, xb = expand_buffers(b, rows, D, L, A, kind)
        paths = expand_paths(state_t, xdec, xa, xb, D)
        assert all(w is None or w == p for w, p in zip(EXPAND_PATHS[kind], paths)), (kind, paths)
        ops.bcq_expand(state_t, S, noise_t, None, xdec, xa if with_ab else None, xb if with_ab else None)
        b.check(written=["xdec"])
        return b
    b = twice(launch)
    xdec, xa = host(get(b, "xdec", rows, D + L)), host(get(b, "xa", rows, D + A))
    xb = host(get(b, "xb")[1:] if kind == "vec_a" else get(b, "xb")).reshape(rows, D + A)
    assert bits(xdec[:, :D], rep) and bits(xdec[:, D:], clipped)
    for x in (xa, xb):  # the state columns are filled, the action columns behind them keep their sentinel
        assert bits(x[:, :D], rep) and (x[:, D:] == F(SENT)).all()
    if kind == "vec_a":
        assert float(get(b, "xb")[0]) == F(SENT)
    b0 = launch(with_ab=False)
    assert bits(get(b0, "xdec"), xdec.reshape(-1)) and bool((get(b0, "xa") == SENT).all()) and bool((get(b0, "xb") == SENT).all())


@pytest.mark.parametrize("case", R.BCQ_EXPAND_DRAWS, ids=ident)
def test_bcq_expand_draw_against_the_stream(ops, case):
    n, S, D, L, seed, base, clip = case
    rows = n * S
    total, A = rows * L, 4
    pairs = (total + 1) // 2
    state = np.random.default_rng(n).uniform(-1, 1, (n, D)).astype(F)
    state_t = dev(state)

    def launch(ctl):
        b = Bufs()
        xdec, xa = b.new("xdec", rows, D + L), b.new("xa", rows, D + A)
        ops.bcq_expand(state_t, S, None, ctl, xdec, xa, None, clip=clip)
        b.check(written=["xdec"])
        return b

    def judge(b, offset, what):
        xdec, xa = host(get(b, "xdec", rows, D + L)), host(get(b, "xa", rows, D + A))
        assert bits(xdec[:, :D], np.tile(state, (S, 1))) and bits(xa[:, :D], xdec[:, :D]) and (xa[:, D:] == F(SENT)).all()
        got = xdec[:, D:].astype(np.float64).reshape(-1)
        assert np.abs(got).max() <= clip
        want, slack = R.normal_stream(seed, offset, total, R.BCQ_TAG), R.normal_slack(seed, offset, total, R.BCQ_TAG)
        err = np.abs(got - np.clip(want, -clip, clip))  # the clamp is 1-Lipschitz: the normals' bar carries over
        plain = slack == 0
        w, ws = float(err[plain].max()), float((err - slack)[~plain].max()) if (~plain).any() else 0.0
        NORMALS["plain"], NORMALS["slack"] = max(NORMALS["plain"], w), max(NORMALS["slack"], ws)
        print(f"BAR {what} drawn normals (clip {clip}): {w:.3g} (beyond the slack: {ws:.3g}) of {R.NORMAL_BAR:.3g}")
        assert w <= R.NORMAL_BAR and ws <= R.NORMAL_BAR, what
        assert (np.abs(got) == clip).any() == bool((np.abs(want) > clip + 1e-4).any())

    what = f"bcq expand draw {ident(case[:4])}"
    ctl = ctl_at(ops, seed, base)
    b1 = launch(ctl)
    assert int(ctl[1]) == base + pairs and int(ctl[2]) == 0
    launch(ctl_at(ops, seed, base)).same_as(b1.snapshot())
    judge(b1, base, what)
    b2 = launch(ctl)
    assert int(ctl[1]) == base + 2 * pairs and int(ctl[2]) == 0
    judge(b2, base + pairs, what + " second launch")


# ---- BCQ: perturbation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", R.BCQ_PERTURB_ROWS)
def test_bcq_perturb_against_fp64(ops, rows):
    bad, D = [], 4
    for A in R.BCQ_PERTURB_ACT:
        what = f"bcq perturb {rows}-{A}"
        inp = R.bcq_perturb_inputs(R.BCQ_SEED_BASE + 1000 * rows + A, rows, A)
        ref, mg = R.np64(R.bcq_perturb_stmt(inp)), R.np64(R.bcq_perturb_stmt(inp, mag=True))
        margin = R.perturb_margin(ref["perturb_x"], mg["perturb_x"], R.BARS["perturb"])  # condition (a)
        print(f"BAR {what} clamp margin: {margin:.3f} (>= 1)")
        assert margin >= 1.0
        a_t, p_t, g_t = block(inp["a_vae"], D + A, D), block(inp["p"], A + 1, 0), block(inp["g"], D + A, D)

        def launch():
            b = Bufs()
            wide, g_p = b.new("out", rows, D + A), b.new("g_p", rows, A)
            ops.bcq_perturb_fwd(a_t, p_t, inp["mp"], wide[:, D:])
            ops.bcq_perturb_bwd(g_t, a_t, p_t, inp["mp"], g_p)
            b.check(written=["g_p"])
            assert bool((wide[:, :D] == SENT).all())
            return b
        b = twice(launch)
        out, g_p = host(get(b, "out", rows, D + A))[:, D:], host(get(b, "g_p", rows, A))
        bar("perturb", out, ref["perturb"], mg["perturb"], what, bad)
        bar("perturb_g", g_p, ref["perturb_g"], mg["perturb_g"], what, bad)
        x = ref["perturb_x"]
        assert bits(out[np.abs(x) >= 1.0], np.sign(x[np.abs(x) >= 1.0]).astype(F))  # on and beyond the bounds: exactly +-1
        assert not g_p[np.abs(x) > 1.0].any() and (g_p[np.abs(x) == 1.0] != 0).all()  # closed interval
        assert (np.abs(x) == 1.0).any() and (rows < 3 or (np.abs(x) > 1.0).any())
    assert not bad, bad


# ---- BCQ: target and selection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BCQ_TARGET_CASES, ids=ident)
def test_bcq_target_and_select(ops, nv, case):
    n, S, N = case
    rows, A, bad, lib = n * S, 3, [], nv.lib()
    what = f"bcq target {ident(case)}"
    inp = R.bcq_target_inputs(R.BCQ_SEED_BASE + 300 + R.BCQ_TARGET_CASES.index(case), n, S, N)
    q_t, rew_t, done_t = dev(inp["q"]), dev(inp["rew"]), dev(inp["done"])
    q_wide = block(inp["q"], rows + 5, 0)  # q_stride = rows + 5 through the C entry
    for grouping in (0, 1):
        ref, mg = R.np64(R.bcq_target_stmt(inp, grouping)), R.np64(R.bcq_target_stmt(inp, grouping, mag=True))

        def launch(want=("target", "max_q"), wide=False):
            b = Bufs()
            t, m = (b.new("target", n) if "target" in want else None), (b.new("max_q", n) if "max_q" in want else None)
            if wide:
                ops.check(lib.cstr_bcq_target_f32(ops.ptr(q_wide), i64(rows + 5), cint(N), i64(n), cint(S), cint(grouping), ops.ptr(rew_t), ops.ptr(done_t),
                                                  f32c(inp["gamma"]), ops.ptr(t), ops.ptr(m), ops.stream_ptr()), "target")
            else:
                ops.bcq_target(q_t, n, S, grouping == 0, rew_t if t is not None else None, done_t if t is not None else None, inp["gamma"], t, m)
            b.check(written=list(want))
            return b
        b = twice(launch)
        target, max_q = host(get(b, "target")), host(get(b, "max_q"))
        assert bits(max_q, ref["max_q"].astype(F))
        bar("target", target, ref["target"], mg["target"], f"{what} grouping {grouping}", bad)
        assert bits(get(launch(("target",)), "target"), target) and bits(get(launch(("max_q",)), "max_q"), max_q)
        bw = launch(wide=True)
        assert bits(get(bw, "target"), target) and bits(get(bw, "max_q"), max_q)
    cand = np.random.default_rng(rows).uniform(-1, 1, (rows, A)).astype(F)
    cand_t, q1_t = block(cand, 4 + A, 4), dev(inp["q"][0])
    idx_ref, act_ref = R.bcq_select_stmt(inp["q"][0], cand, n, S)
    if S >= 10 and n >= 64:  # ties at the maximum: the first one wins
        assert not np.array_equal(idx_ref, R.bcq_select_stmt(inp["q"][0], cand, n, S, mut="last_max")[0])

    def select(with_index=True):
        b = Bufs()
        act = b.new("act", n, A)
        idx = th.full((n + 8,), -7, dtype=th.int64, device=DEV) if with_index else None
        ops.bcq_select(q1_t, cand_t, n, S, None if idx is None else idx[:n], act)
        b.check(written=["act"])
        if with_index:
            assert bool((idx[n:] == -7).all())
        return host(get(b, "act", n, A)).copy(), None if idx is None else host(idx[:n]).copy()
    act, idx = select()
    act2, idx2 = select()
    assert bits(act, act2) and bits(idx, idx2) and bits(idx, idx_ref) and bits(act, act_ref)
    assert bits(select(with_index=False)[0], act_ref)
    assert not bad, bad


def test_zz_kernel_worst_figures():
    """a record, not a check: prints the worst figure per output kind that the tests of this run measured (it runs last; under -k or
    another order it prints what ran before it, possibly nothing). Every figure is asserted where it is measured"""
    for kind in sorted(FIGS):
        print(f"KERNEL {kind}: {FIGS[kind]:.3f} units, bar {R.BARS[kind]:.2f}")
    print(f"KERNEL drawn normals: {NORMALS['plain']:.3g} outside the slack elements, {NORMALS['slack']:.3g} beyond the slack inside them, bar {R.NORMAL_BAR:.3g}")
    assert all(FIGS[k] <= R.BARS[k] for k in FIGS)
