"""The lean Q forward kernel with a pending actor head against the generic one (cstr_q_chain_fwd_f32, csrc/cstr_chain.hip).

The lean kernel finalises the head in two halves: in front of its first barrier only the action, and only in the workgroups whose
network reads it; the log-prob half, the row sums and the stores of what later launches read (x_pi / x_next action columns, params,
logp_pi, logp_next) behind the barriers, in the workgroups that store them, on a wave the head stage leaves idle (tiles 1 and 2) or
behind the head stage (tiles 4). Both halves are the generic kernel's expressions, operand for operand, so every case runs the launch
twice from identical seeded inputs, once per setting of cstr_chain_lean, and compares every buffer the launch may write byte for byte:
q_part, h1, h2 of every network, x_pi, x_next, params, logp_pi, logp_next -- each filled with a sentinel first and followed by 64
sentinel floats, so that an element left unwritten or written beside its place shows as well.

Cases: one and three row groups (batch 16, 48), both layouts with lean instantiations ((4, 2) and (8, 2) at 256 x 256), the Q launch's
tiles 1, 2 and 4, the actor pass's column-group counts 8 (the 8-register bucket of the partial sums) and 16 (the 16-register bucket),
SAC's four roles as the learner launches them, a deterministic head with PI / NEXT_STORE, and next rows that do not start at `batch`.
The first and the last six rows of both row blocks carry the inputs that stress the moved arithmetic -- raw log-std at and beyond both
clamps (-20, 2), eps 0 and +-4, means of +-12 (1 - a^2 + 1e-6 = 1e-6), partial columns of -0.0 only -- chosen so that every logged
argument is positive and finite: sd = exp(clamp) >= exp(-20) > 0 and 1 - a^2 + 1e-6 >= 1e-6 because |tanh| <= 1 in f32.

The CPU test at the end checks the entry point's argument checks, which the change leaves as they were."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from _sentinel_bufs import DEV, SENT, Bufs

H = 256
HB = np.array([0.125, -0.25, 0.5, -0.375], np.float32)  # exactly representable, so that partial 0 = target - hb gives the target back
# (mean, raw log-std, eps) per (stress row, action): with every other partial zero the sums are exact
STRESS = [
    [(0.0, -20.0, 0.0), (0.0, 2.0, 0.0)],        # exactly at the clamps, no noise
    [(12.0, -20.0, 4.0), (-12.0, 2.0, -4.0)],    # |a| = 1: the tanh correction's argument is 1e-6
    [(12.0, -25.0, 0.0), (-12.0, 3.0, 0.0)],     # beyond the clamps
    [(0.5, -20.0, -4.0), (0.5, 2.0, 4.0)],
    [(12.0, 2.0, 4.0), (-12.0, -25.0, -4.0)],    # u = 12 + 4 e^2
    [(0.25, float(np.nextafter(np.float32(-20), np.float32(-21))), 4.0), (-0.75, float(np.nextafter(np.float32(2), np.float32(3))), -4.0)],
]


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


def net_weights(rng, W):
    w = dict(w1=rng.standard_normal((H, W)) * 0.4, b1=rng.standard_normal(H) * 0.1, w2=rng.standard_normal((H, H)) * 0.08,
             b2=rng.standard_normal(H) * 0.1, w3=rng.standard_normal(H) * 0.1, b3=np.array([rng.standard_normal()]))
    return {k: dev(v) for k, v in w.items()}


def layers(w):
    return ((w["w1"], w["b1"]), (w["w2"], w["b2"]), (w["w3"], w["b3"]))


def head_inputs(rng, B, A, n_parts, gauss, part_rows, next_offset):
    """head_part [n_parts][part_rows][HN], hb [HN], eps [part_rows][A] with the stress rows in the first and the last rows of both blocks"""
    hn = 2 * A if gauss else A
    part = (rng.standard_normal((n_parts, part_rows, hn)) * 0.3).astype(np.float32)
    eps = rng.standard_normal((part_rows, A)).astype(np.float32)
    hb = HB[:hn].copy()
    for base in (0, next_offset):
        for first in (0, B - len(STRESS)):
            for i, spec in enumerate(STRESS):
                row = base + first + i
                part[:, row, :] = 0.0
                for j, (mu, raw, e) in enumerate(spec):
                    part[0, row, j] = np.float32(mu) - hb[j]
                    if gauss:
                        part[0, row, A + j] = np.float32(raw) - hb[A + j]
                    eps[row, j] = e
        part[:, base + len(STRESS), 0] = -0.0  # columns of -0.0 only (the bucket's zero padding turns the sum into +0.0 in both kernels)
        part[:, base + B - len(STRESS) - 1, hn - 1] = -0.0
    if gauss:  # the inputs keep every logged argument positive and finite (f32, the kernel's expressions)
        mu, raw = part[..., :A].sum(0, dtype=np.float32) + hb[:A], part[..., A:].sum(0, dtype=np.float32) + hb[A:]
        sd = np.exp(np.clip(raw, -20, 2)).astype(np.float32)
        a = np.tanh((mu + sd * eps).astype(np.float32)).astype(np.float32)
        arg = (np.float32(1) - a * a + np.float32(1e-6)).astype(np.float32)
        assert np.isfinite(sd).all() and (sd > 0).all() and np.isfinite(arg).all() and (arg > 0).all()
        assert (arg <= np.float32(1.1e-6)).any() and (raw <= -20).any() and (raw >= 2).any()
    return part, hb, eps


def both(ops, launch):
    """launch(lean) -> {name: numpy array}; the switch is restored whatever happens"""
    out = []
    for lean in (0, 1):
        was = ops.chain_lean(lean)
        try:
            out.append(launch(lean))
            th.cuda.synchronize()
        finally:
            ops.chain_lean(was)
    assert out[0].keys() == out[1].keys()
    for name in out[0]:
        a, b = out[0][name], out[1][name]
        assert a.tobytes() == b.tobytes(), f"{name}: {int((a.view(np.int32) != b.view(np.int32)).sum())} of {a.size} words differ between the two kernels"


# (D, A, B, tiles of the Q launch, partial sums = column groups of the actor launch at its tiles 2 / 1, configuration)
CASES = [(D, 2, B, tiles, n_parts, "sac4") for D in (4, 8) for B in (16, 48) for tiles in (1, 2, 4) for n_parts in (8, 16)]
CASES += [(4, 2, 48, 2, 8, "det2"), (8, 2, 16, 1, 16, "det2"), (4, 2, 16, 4, 8, "det2")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward_with_pending_head(ops, nv, case):
    D, A, B, tiles, n_parts, cfg = case
    assert ops.chain_supported(H, H, B) and ops.chain_tiles_ok(H, tiles, forward=True)
    assert n_parts in (ops.chain_colgroups(H, 2), ops.chain_colgroups(H, 1))  # what an actor launch at 256 wide leaves
    rng = np.random.default_rng(1000 * D + 10 * B + tiles + n_parts + len(cfg))
    W, G = D + A, ops.chain_colgroups(H, tiles)
    P, S, NX, NS, PI = nv.CHAIN_ROLE_PLAIN, nv.CHAIN_ROLE_STORE_PI, nv.CHAIN_ROLE_NEXT, nv.CHAIN_ROLE_NEXT_STORE, nv.CHAIN_ROLE_PI
    gauss = cfg == "sac4"
    roles = [S, P, NS, NX] if gauss else [PI, NS]
    n = len(roles)
    part_rows, next_offset = 2 * B + 16, B + 16  # the next rows do not start where the pi rows end
    wts = [net_weights(rng, W) for _ in range(n)]
    x_obs = [rng.standard_normal((B, W)).astype(np.float32) for _ in range(n)]
    part, hb, eps = head_inputs(rng, B, A, n_parts, gauss, part_rows, next_offset)
    fin_in = [dev(part), dev(hb), dev(eps)]

    def launch(lean):
        b = Bufs()
        x_pi, x_next = b.new("x_pi", B, W), b.new("x_next", B, W)
        x_next[:, :D] = dev(x_obs[0][:, :D])
        if PI in roles:
            x_pi[:, :D] = dev(x_obs[1][:, :D])
        xs = [x_pi if r == PI else x_next if r in (NX, NS) else dev(x_obs[g]) for g, r in enumerate(roles)]
        stores = (None, None, None)
        if gauss:
            stores = tuple(t.data_ptr() for t in (b.new("params", B, 2 * A), b.new("logp_pi", B), b.new("logp_next", B)))
        fin = nv.SacHeadFin(fin_in[0].data_ptr(), fin_in[1].data_ptr(), fin_in[2].data_ptr(), n_parts, A, D,
                            nv.CHAIN_HEAD_GAUSSIAN if gauss else nv.CHAIN_HEAD_DETERMINISTIC, part_rows, next_offset, 0.2, 0.5,
                            x_pi.data_ptr(), x_next.data_ptr(), *stores)
        nets = [ops.chain_net(layers(wts[g]), xs[g], b.new(f"h1_{g}", B, H), b.new(f"h2_{g}", B, H), b.new(f"q_part_{g}", G, B), roles[g]) for g in range(n)]
        ops.q_chain_fwd(nets, W, D, H, H, B, tiles, fin)
        written = [f"{k}_{g}" for g in range(n) for k in ("h1", "h2", "q_part")] + (["params", "logp_pi", "logp_next"] if gauss else [])
        b.check(written=written)
        out = {name: f.cpu().numpy().copy() for name, (f, _) in b.flat.items()}
        for nm in ("x_pi", "x_next"):  # the action columns are written, every one; the observation columns are not the launch's
            m = out[nm][:B * W].reshape(B, W)
            assert (m[:, D:] != np.float32(SENT)).all(), (nm, lean)
            assert (np.abs(m[:, D:]) <= 1).all(), (nm, lean)
        assert (out["x_pi"][:B * W].reshape(B, W)[:, :D] == (x_obs[1][:, :D] if PI in roles else np.float32(SENT))).all(), lean
        assert (out["x_next"][:B * W].reshape(B, W)[:, :D] == x_obs[0][:, :D]).all(), lean
        if gauss:
            assert np.isfinite(out["logp_pi"][:B]).all() and np.isfinite(out["logp_next"][:B]).all(), lean
            assert (out["params"][:B * 2 * A].reshape(B, 2 * A)[0] == np.float32([0.0, 0.0, -20.0, 2.0])).all(), lean  # the exact stress sums
        return out

    both(ops, launch)


def test_argument_checks_are_unchanged(nv):
    """return codes of cstr_q_chain_fwd_f32's argument checks: none of them reaches a launch"""
    lib = nv.lib()
    BAD, UNSUP = -1, -2
    p = 0x1000  # never dereferenced: the checks fail first
    null = C.c_void_p(None)

    def call(nets, w_in=6, obs_dim=4, h1=H, h2=H, batch=16, fin=None, tiles=2):
        arr = (nv.ChainNet * len(nets))(*nets)
        return lib.cstr_q_chain_fwd_f32(arr, C.c_int(len(nets)), C.c_int(w_in), C.c_int(obs_dim), C.c_int(h1), C.c_int(h2), C.c_int64(batch),
                                        None if fin is None else C.byref(fin), C.c_int(tiles), null)

    def net(role=0, **kw):
        f = dict(w1=p, b1=p, w2=p, b2=p, w3=p, b3=p, x=p, h1=p, h2=p, q_part=p)
        f.update(kw)
        return nv.ChainNet(f["w1"], f["b1"], f["w2"], f["b2"], f["w3"], f["b3"], f["x"], f["h1"], f["h2"], f["q_part"], role, 0)

    def fin(**kw):
        f = dict(head_part=p, hb=p, eps=p, n_parts=8, act_dim=2, obs_dim=4, kind=nv.CHAIN_HEAD_GAUSSIAN, part_rows=32, next_offset=16, sigma=0.2,
                 clip=0.5, x_pi=p, x_next=p, params=p, logp_pi=p, logp_next=p)
        f.update(kw)
        return nv.SacHeadFin(*[f[k] for k in ("head_part", "hb", "eps", "n_parts", "act_dim", "obs_dim", "kind", "part_rows", "next_offset", "sigma",
                                              "clip", "x_pi", "x_next", "params", "logp_pi", "logp_next")])

    assert lib.cstr_q_chain_fwd_f32(null, C.c_int(1), C.c_int(6), C.c_int(4), C.c_int(H), C.c_int(H), C.c_int64(16), None, C.c_int(2), null) == BAD
    assert call([net()] * 17) == BAD and call([net()], w_in=13) == BAD and call([net()], obs_dim=6) == BAD and call([net()], obs_dim=0) == BAD
    assert call([net()], batch=24) == UNSUP and call([net()], h1=258) == UNSUP and call([net()], tiles=3) == UNSUP
    assert call([net(x=None)]) == BAD and call([net(q_part=None)]) == BAD and call([net(w2=p + 4)]) == BAD
    assert call([net(role=5)]) == BAD and call([net(role=-1)]) == BAD
    assert call([net(role=nv.CHAIN_ROLE_NEXT)]) == BAD  # a role without a pending head
    roles = [net(role=r) for r in (nv.CHAIN_ROLE_STORE_PI, nv.CHAIN_ROLE_PLAIN, nv.CHAIN_ROLE_NEXT_STORE, nv.CHAIN_ROLE_NEXT)]
    for kw in (dict(head_part=None), dict(hb=None), dict(n_parts=0), dict(act_dim=0), dict(act_dim=5), dict(obs_dim=3), dict(act_dim=3), dict(kind=2),
               dict(part_rows=15), dict(next_offset=-1), dict(next_offset=17), dict(eps=None), dict(x_pi=None), dict(x_next=None), dict(params=None),
               dict(logp_pi=None), dict(logp_next=None)):
        assert call(roles, fin=fin(**kw)) == BAD, kw
    det = dict(kind=nv.CHAIN_HEAD_DETERMINISTIC, eps=None, params=None, logp_pi=None, logp_next=None)
    assert call([net(role=nv.CHAIN_ROLE_NEXT_STORE)], fin=fin(x_next=None, **det)) == BAD
    assert call([net(role=nv.CHAIN_ROLE_PI)], fin=fin(x_pi=None, **det)) == BAD and call([net(role=nv.CHAIN_ROLE_STORE_PI)], fin=fin(x_pi=None, **det)) == BAD
    assert call(roles, w_in=5, obs_dim=3, fin=fin(obs_dim=3)) == UNSUP  # (3, 2) is not a layout
