"""GPU checks of the TRPO launches (csrc/cstr_trpo.hip) against the fp64 statements of tests/_trpo_reference.py on the same float32 inputs.
Every output sits behind GuardedBufs sentinels, a relaunch gives the same bits, every case prints its worst error over its bar
before asserting.

Bars. The float32 MFMA kinds (tangent layer, head metric, whole Fisher-vector product into the gradient layout) are judged per element
in units of 2**-24 * M at four times the worst float32 ATen figure over this module's cases, measured on the CPU
(tests/test_trpo_reference.py re-measures them): ATen tangent 4.155, head 9.627, fvp 1.220 units -> bars 16.62, 38.51, 4.88. No element
is excluded. Input conditions, asserted before each launch: no ReLU pre-activation within the bar of zero (mask_margin at the 64-unit
cap), tanh outputs below 1 - 2**-12; both found by seed search on the CPU.
The launches that compute in float64 and store float32 (objective, KL, accepted flag, CG step, apply step, value loss) take the
project's kernel-against-fp64 bar |got - want| <= 2e-6 |want| + 1e-7 max |want|.
Measured on MI355X (2026-10-21): tangent layer 4.743 units over the 324 cases, head metric 10.457, whole product 0.149; the worst of the
548 fp64-bar checks 0.096 of its bar; the x0 stream 8.8e-07 from the fp64 counter contract (bar 1.01e-05)."""
import numpy as np
import pytest
import torch as th

import _rowkernel_reference as RK
import _trpo_reference as R
from _sentinel_bufs import GuardedBufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = th.float64


@pytest.fixture(scope="module")
def ops():
    from core import _native as nv
    from core.common import hip_ops

    nv.lib()
    th.cuda.set_device(0)
    return hip_ops, nv


def head_id(head):
    kind, k = head
    return {"gauss": (0, k, 0), "cat": (1, k, 0)}[kind] if kind != "mcat" else (2, k[0], k[1])


def report(what, fig, bar):
    print(f"TRPO {what}: worst {fig:.3f} of a bar of {bar:.2f}")
    assert fig <= bar, (what, fig, bar)


def report64(what, got, want):
    w, ok = R.close64(got.detach().cpu().numpy() if isinstance(got, th.Tensor) else got, want.detach().cpu().numpy() if isinstance(want, th.Tensor) else want)
    print(f"TRPO {what}: worst {w:.3f} of the fp64 bar")
    assert ok, (what, w)


# ---- the tangent layer ------------------------------------------------------------------------------------------------------------------
def test_tangent_layer(ops):
    hip_ops, _ = ops
    worst_fig = 0.0
    for case in R.tangent_cases():
        rows, k, n, act, with_xdot = case
        c = R.tangent_case(*case)
        R.assert_conditions(c)
        gb = GuardedBufs()
        x, w, wd, bd, y = (gb.put_ro(nm, c[nm]) for nm in ("x", "w", "w_dot", "b_dot", "y"))
        xd = gb.put_ro("x_dot", c["x_dot"]) if with_xdot else None
        z = gb.new("z_dot", rows, n)
        hip_ops.linear_tangent_fwd(x, xd, w, wd, bd, y, R.ACT_ID[act], out=z)
        gb.check(written=("z_dot",))
        snap = gb.snapshot()
        hip_ops.linear_tangent_fwd(x, xd, w, wd, bd, y, R.ACT_ID[act], out=z)
        gb.check()
        gb.same_as(snap)
        fig = R.worst(z.cpu().numpy(), R.tangent_eval(c), R.tangent_eval(c, mag=True))
        worst_fig = max(worst_fig, fig)
        assert fig <= R.BARS["tangent"], (case, fig)
    report("tangent layer over %d cases" % len(list(R.tangent_cases())), worst_fig, R.BARS["tangent"])


def test_tangent_layer_strided_rows_and_scalar_path(ops):
    """x and x_dot as column blocks of wider matrices (row stride 72: vector loads; 67: the scalar path), K = 6 (no multiple of 4)"""
    hip_ops, _ = ops
    for ld, k in ((72, 64), (67, 64), (6, 6), (9, 6)):
        c = R.tangent_case(37, k, 20, "tanh", True)
        gb = GuardedBufs()
        x, xd = gb.put_ro_cols("x", c["x"], ld, 0), gb.put_ro_cols("x_dot", c["x_dot"], ld, 0)
        w, wd, bd, y = (gb.put_ro(nm, c[nm]) for nm in ("w", "w_dot", "b_dot", "y"))
        z = gb.new("z_dot", 37, 20)
        hip_ops.linear_tangent_fwd(x, xd, w, wd, bd, y, 2, out=z)
        gb.check(written=("z_dot",))
        report(f"tangent layer ld {ld} k {k}", R.worst(z.cpu().numpy(), R.tangent_eval(c), R.tangent_eval(c, mag=True)), R.BARS["tangent"])


# ---- the head metric --------------------------------------------------------------------------------------------------------------------
def test_fisher_head(ops):
    hip_ops, _ = ops
    worst_fig = 0.0
    for head in R.HEADS + (("gauss", 4), ("cat", 64), ("mcat", (32, 32)), ("cat", 2), ("mcat", (2, 2))):
        for rows in (1, 3, 65, 257) + ((16384 + 77,) if head in (("cat", 9), ("mcat", (3, 5))) else ()):  # the last: beyond one grid pass
            c = R.head_case(head, rows)
            gb = GuardedBufs()
            dd = gb.put_ro("dist_dot", c["dist_dot"])
            gauss = head[0] == "gauss"
            dist = None if gauss else gb.put_ro("dist", c["dist"])
            ls, vls = (gb.put_ro("log_std", c["log_std"]), gb.put_ro("v_log_std", c["v_log_std"])) if gauss else (None, None)
            up = gb.new("up", rows, R.head_width(head))
            gls = gb.new("g_log_std", R.head_width(head)) if gauss else None
            hip_ops.trpo_fisher_head(*head_id(head), dd, dist, ls, vls, up, gls)
            gb.check(written=("up", "g_log_std") if gauss else ("up",))
            snap = gb.snapshot()
            hip_ops.trpo_fisher_head(*head_id(head), dd, dist, ls, vls, up, gls)
            gb.same_as(snap)
            fig = R.worst(up.cpu().numpy(), R.head_eval(c), R.head_eval(c, mag=True))
            worst_fig = max(worst_fig, fig)
            assert fig <= R.BARS["head"], (head, rows, fig)
            if gauss:
                assert np.array_equal(gls.cpu().numpy(), 2.0 * c["v_log_std"])  # exact in float32
    report("head metric", worst_fig, R.BARS["head"])


# ---- the whole Fisher-vector product ------------------------------------------------------------------------------------------------------
def kernel_fvp(hip_ops, c, gb=None):
    """J^T M J v / R through the launches train() uses, into separate gradient buffers -> the flat product WITHOUT the damping term"""
    actor, acts = c["actor"], [th.as_tensor(a).to(DEV) for a in c["acts"]]
    dev = lambda a: th.as_tensor(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    v_ls, vs = R.split(actor, th.as_tensor(c["v"]))
    ws = [(dev(w), dev(b)) for w, b in actor["ws"]]
    n_layers = len(ws)
    aid = R.ACT_ID[actor["act"]]
    x_dot = None
    for i, ((w, _), (wd, bd)) in enumerate(zip(ws, vs)):
        x_dot = hip_ops.linear_tangent_fwd(acts[i], x_dot, w, dev(wd.numpy()), dev(bd.numpy()), acts[i + 1], aid if i < n_layers - 1 else 0)
    head = actor["head"]
    gauss = head[0] == "gauss"
    gb = GuardedBufs() if gb is None else gb
    up = gb.new("up", acts[0].shape[0], R.head_width(head))
    gls = gb.new("g_log_std", head[1]) if gauss else None
    hip_ops.trpo_fisher_head(*head_id(head), x_dot, None if gauss else acts[-1], dev(actor["log_std"]) if gauss else None,
                             dev(v_ls.numpy()) if gauss else None, up, gls)
    grads = [(gb.new(f"dw{i}", *w.shape), gb.new(f"db{i}", *b.shape)) for i, (w, b) in enumerate(ws)]
    gz, sets = up, []
    for i in range(n_layers - 1, -1, -1):
        sets.append((gz, acts[i], grads[i][0], grads[i][1]))
        if i > 0:
            gz = hip_ops.linear_bwd_input(gz, ws[i][0], acts[i], aid)
    hip_ops.linear_bwd_weight_sets(sets)
    gb.check(written=["up"] + (["g_log_std"] if gauss else []) + [f"d{k}{i}" for i in range(n_layers) for k in "wb"])
    flat = ([gls.reshape(-1)] if gauss else []) + [t.reshape(-1) for g in grads for t in g]
    return th.cat(flat).cpu().numpy().astype(np.float64)


def test_whole_fisher_vector_product(ops):
    hip_ops, _ = ops
    worst_fig = 0.0
    for case in R.FVP_CASES:
        c = R.fvp_case(*case)
        got = kernel_fvp(hip_ops, c) + c["damping"] * c["v"].astype(np.float64)
        assert np.array_equal(got, kernel_fvp(hip_ops, c) + c["damping"] * c["v"].astype(np.float64))  # a relaunch gives the same bits
        fig = R.worst(got, R.fvp_eval(c), R.fvp_eval(c, mag=True))
        print(f"TRPO fvp {case}: {fig:.3f} units")
        worst_fig = max(worst_fig, fig)
    report("whole Fisher-vector product", worst_fig, R.BARS["fvp"])


# ---- the objective launch -----------------------------------------------------------------------------------------------------------------
def objective_case(head, rows, seed=0, shift=0.05):
    """distribution parameters at the current point and at theta0 (they differ: the KL has a scale), actions, old log-probs, advantages"""
    rng = np.random.default_rng(911 * seed + rows + 17 * R.head_width(head))
    n = R.head_width(head)
    old_dist = rng.standard_normal((rows, n)).astype(np.float32)
    dist = (old_dist + shift * rng.standard_normal((rows, n))).astype(np.float32)
    gauss = head[0] == "gauss"
    old_ls = (0.3 * rng.standard_normal(n)).astype(np.float32) if gauss else None
    ls = (old_ls + 0.02 * rng.standard_normal(n)).astype(np.float32) if gauss else None
    if gauss:
        actions = (dist + np.exp(ls) * rng.standard_normal((rows, n))).astype(np.float32)
    else:
        actions = np.stack([rng.integers(0, k, rows) for k in R._blocks(head)], 1).astype(np.float32)
    t64 = lambda a: None if a is None else th.as_tensor(a).to(F64)  # noqa: E731
    logp, _ = R.logp_kl(head, t64(dist), t64(ls), t64(old_dist), t64(old_ls), actions)
    old_log_prob = (logp.numpy() + 0.1 * rng.standard_normal(rows)).astype(np.float32)
    adv = (0.7 + 1.3 * rng.standard_normal(rows)).astype(np.float32)
    return dict(head=head, dist=dist, log_std=ls, old_dist=old_dist, old_log_std=old_ls, actions=actions, old_log_prob=old_log_prob, adv=adv)


def objective_stmt(c, normalize=True, dist=None):
    """fp64: objective, kl and d objective / d (dist, log_std)"""
    t64 = lambda a: None if a is None else th.as_tensor(a).to(F64)  # noqa: E731
    d = t64(c["dist"] if dist is None else dist).requires_grad_(True)
    ls = None if c["log_std"] is None else t64(c["log_std"]).requires_grad_(True)
    logp, kl = R.logp_kl(c["head"], d, ls, t64(c["old_dist"]), t64(c["old_log_std"]), c["actions"])
    adv = R.normalize(c["adv"]) if normalize else t64(c["adv"])
    obj = (adv * th.exp(logp - t64(c["old_log_prob"]))).mean()
    grads = th.autograd.grad(obj, [d] + ([] if ls is None else [ls]))
    return float(obj.detach()), float(kl.mean().detach()), grads[0].numpy(), (None if ls is None else grads[1].numpy())


def put_objective(gb, hip_ops, nv, c):
    gauss = c["head"][0] == "gauss"
    t = dict(dist=gb.put_ro("dist", c["dist"]), old_dist=gb.put_ro("old_dist", c["old_dist"]), actions=gb.put_ro("actions", c["actions"]),
             old_log_prob=gb.put_ro("old_log_prob", c["old_log_prob"]), adv=gb.put_ro("adv", c["adv"]))
    t["log_std"] = gb.put_ro("log_std", c["log_std"]) if gauss else None
    t["old_log_std"] = gb.put_ro("old_log_std", c["old_log_std"]) if gauss else None
    t["ctl"] = gb.put("ctl", np.zeros(nv.TRPO_CTL_WORDS), dtype=th.float64)
    t["ws"] = gb.put("ws", np.zeros(nv.PPO_WS_WORDS, np.int64), dtype="uint64")
    t["scalars"] = gb.new("scalars", 2)
    return t


@pytest.mark.parametrize("head", R.HEADS + (("gauss", 4), ("cat", 64), ("mcat", (32, 2))), ids=str)
def test_objective_gradient_mode(ops, head):
    hip_ops, nv = ops
    gauss = head[0] == "gauss"
    for rows in R.FLAT_ROWS:
        for normalize in ((True, False) if rows == 65 else (True,)):
            c = objective_case(head, rows)
            gb = GuardedBufs()
            t = put_objective(gb, hip_ops, nv, c)
            g_dist = gb.new("g_dist", rows, R.head_width(head))
            g_ls = gb.new("g_log_std", head[1]) if gauss else None
            launch = lambda: hip_ops.trpo_objective(*head_id(head), t["dist"], t["log_std"], t["old_dist"], t["old_log_std"], t["actions"],  # noqa: E731
                                                    t["old_log_prob"], t["adv"], normalize, t["ctl"], t["ws"], g_dist=g_dist, g_log_std=g_ls,
                                                    scalars_out=t["scalars"])
            launch()
            gb.check(written=("g_dist", "scalars") + (("g_log_std",) if gauss else ()))
            snap = gb.snapshot()
            launch()
            gb.check()
            gb.same_as(snap)
            obj, kl, gd, gl = objective_stmt(c, normalize)
            tag = f"{head} rows {rows} normalize {normalize}"
            ctl = t["ctl"].cpu().numpy()
            report64(f"objective {tag}", t["scalars"][:1], [obj])
            report64(f"kl {tag}", t["scalars"][1:], [kl])
            report64(f"g_dist {tag}", g_dist, gd)
            if gauss:
                report64(f"g_log_std {tag}", g_ls, gl)
            assert abs(ctl[nv.TRPO_CTL["objective"]] - obj) <= 1e-10 * abs(obj) and abs(ctl[nv.TRPO_CTL["kl"]] - kl) <= 1e-10 * kl  # the float64 words
            assert ctl[nv.TRPO_CTL["coeff"]] == 1.0 and int(t["ws"][0]) == 0  # the ticket reset itself
    # at theta0 the two distributions are the same buffers: the KL is exactly zero
    c = objective_case(head, 65)
    c["dist"], c["log_std"] = c["old_dist"], c["old_log_std"]
    gb = GuardedBufs()
    t = put_objective(gb, hip_ops, nv, c)
    hip_ops.trpo_objective(*head_id(head), t["old_dist"], t["old_log_std"], t["old_dist"], t["old_log_std"], t["actions"], t["old_log_prob"],
                           t["adv"], True, t["ctl"], t["ws"], g_dist=gb.new("g_dist", 65, R.head_width(head)),
                           g_log_std=gb.new("g_log_std", head[1]) if gauss else None, scalars_out=t["scalars"])
    gb.check()
    assert float(t["scalars"][1]) == 0.0


def _ls_sequence(c, delta, coeffs):
    return [(c["old_dist"].astype(np.float64) + k * delta).astype(np.float32) for k in coeffs]


@pytest.mark.parametrize("head", R.HEADS, ids=str)
def test_objective_line_search_mode(ops, head):
    """the decision, the shrinking coefficient and the logged scalars over sequences of launches whose distributions move along
    +- the objective's gradient: accepted at iteration 1, at iteration 3, never (rejected by the KL alone), rejected by the objective alone"""
    hip_ops, nv = ops
    shrink, rows = 0.8, 257
    c = objective_case(head, rows, seed=3, shift=0.0)
    c["log_std"] = c["old_log_std"]
    obj0, kl0, gd, _ = objective_stmt(c, dist=c["old_dist"])
    assert kl0 == 0.0
    delta = 0.3 * gd / np.abs(gd).max()  # ascent direction in distribution-parameter space
    _, kl_at_1, _, _ = objective_stmt(c, dist=_ls_sequence(c, delta, [1.0])[0])
    plans = {"first": (delta, 2.0 * kl_at_1, [True]), "third": (delta, 0.5 * kl_at_1, [False, False, True]),
             "never_kl": (delta, kl_at_1 * shrink ** 12, [False] * 5), "objective_only": (-delta, 100.0 * kl_at_1, [False] * 4)}
    for name, (dl, target_kl, want_flags) in plans.items():
        gb = GuardedBufs()
        t = put_objective(gb, hip_ops, nv, c)
        acc = gb.new("accepted", 1, dtype=th.int32)
        ctl0 = np.zeros(nv.TRPO_CTL_WORDS)
        ctl0[nv.TRPO_CTL["objective"]], ctl0[nv.TRPO_CTL["coeff"]] = obj0, 1.0
        t["ctl"].copy_(th.as_tensor(ctl0))
        coeff = 1.0
        for it, want_ok in enumerate(want_flags):
            dist_h = _ls_sequence(c, dl, [coeff])[0]
            obj, kl, _, _ = objective_stmt(c, dist=dist_h)
            margin = R.ls_margins([(coeff, obj, kl, want_ok)], obj0, target_kl)[0]
            assert margin >= 100.0, (name, it, margin)  # the fp64 decision is 100 bars clear of both thresholds
            assert (kl < target_kl and obj > obj0) == want_ok, (name, it)
            if name == "never_kl":
                assert obj > obj0 and not kl < target_kl
            if name == "objective_only":
                assert kl < target_kl and not obj > obj0
            dist = th.as_tensor(dist_h).to(DEV)
            hip_ops.trpo_objective(*head_id(head), dist, t["log_std"], t["old_dist"], t["old_log_std"], t["actions"], t["old_log_prob"], t["adv"],
                                   True, t["ctl"], t["ws"], scalars_out=t["scalars"], accepted=acc, target_kl=target_kl, shrink=shrink)
            gb.check(written=("accepted", "scalars"))
            ctl = t["ctl"].cpu().numpy()
            assert int(acc[0]) == int(want_ok), (name, it)
            coeff = coeff if want_ok else coeff * shrink
            assert ctl[nv.TRPO_CTL["coeff"]] == pytest.approx(coeff, rel=1e-15) and ctl[nv.TRPO_CTL["objective"]] == obj0
            report64(f"line search {head} {name} iteration {it + 1} objective'", t["scalars"][:1], [obj])
            report64(f"line search {head} {name} iteration {it + 1} kl'", t["scalars"][1:], [kl])
            assert abs(ctl[nv.TRPO_CTL["ls_kl"]] - kl) <= 1e-10 * kl


# ---- conjugate gradient -------------------------------------------------------------------------------------------------------------------
class Spd:
    """an explicit symmetric positive definite matrix diag(d) + U U^T in fp64 (n up to the default actor's 4612 without n^2 storage)"""

    def __init__(self, n, seed, rank=6):
        rng = np.random.default_rng(seed)
        self.d = rng.uniform(0.5, 2.0, n)
        self.u = rng.standard_normal((n, min(rank, n))) / np.sqrt(n)

    def __call__(self, v):
        v = np.asarray(v, np.float64)
        return self.d * v + self.u @ (self.u.T @ v)


def cg_bufs(gb, nv, n, x0, g):
    t = dict(x=gb.put("x", x0), r=gb.new("r", n), p=gb.new("p", n), g=gb.put_ro("g", g), ap=gb.put("ap", np.zeros(n, np.float32)),
             ctl=gb.put("ctl", np.zeros(nv.TRPO_CTL_WORDS), dtype=th.float64))
    return t


def host(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("n", R.CG_LENGTHS)
def test_cg_launch_by_launch(ops, n):
    hip_ops, nv = ops
    damping, tol, K = 0.1, 1e-10, nv.TRPO_CTL
    a = Spd(n, n)
    rng = np.random.default_rng(n + 1)
    g = rng.standard_normal(n).astype(np.float32)
    x0 = (1e-4 * rng.standard_normal(n)).astype(np.float32)
    for max_steps in (1, 3, 15):
        gb = GuardedBufs()
        t = cg_bufs(gb, nv, n, x0, g)
        t["ap"].copy_(th.as_tensor(a(x0).astype(np.float32)))
        ap0 = host(t["ap"])
        hip_ops.trpo_cg_step(nv.TRPO_CG_INIT, t["x"], t["r"], t["p"], t["ap"], t["g"], damping, tol, t["ctl"])
        gb.check(written=("r", "p"))
        r_want = g.astype(np.float64) - (ap0 + damping * x0.astype(np.float64))
        report64(f"cg init n {n} r", t["r"], r_want)
        assert th.equal(t["r"], t["p"]) and th.equal(t["x"].cpu(), th.as_tensor(x0))
        ctl = host(t["ctl"])
        r32 = host(t["r"])
        assert abs(ctl[K["rr"]] - r32 @ r32) <= 1e-12 * (r32 @ r32) and ctl[K["done"]] == 0.0 and ctl[K["iters"]] == 0.0
        for i in range(max_steps):
            last = i == max_steps - 1
            x, r, p, rr = host(t["x"]), host(t["r"]), host(t["p"]), host(t["ctl"])[K["rr"]]
            done_before = host(t["ctl"])[K["done"]]
            t["ap"].copy_(th.as_tensor(a(p).astype(np.float32)))
            ap = host(t["ap"])
            before = gb.snapshot()
            hip_ops.trpo_cg_step(nv.TRPO_CG_STEP, t["x"], t["r"], t["p"], t["ap"], None, damping, tol, t["ctl"], last=last)
            gb.check()
            if done_before:  # an earlier residual_tol exit: the launch is a no-op
                gb.same_as(before)
                continue
            st = R.cg_step_stmt(x, r, p, ap, rr, damping, last, tol)
            ctl = host(t["ctl"])
            tag = f"cg n {n} max {max_steps} step {i}"
            report64(f"{tag} x", t["x"], st["x"])
            assert abs(ctl[K["alpha"]] - st["alpha"]) <= 1e-11 * abs(st["alpha"])
            assert ctl[K["done"]] == float(st["done"])
            if st["done"]:  # the last iteration (or the tolerance) returns before r / p / rr move on... r moves only on the tolerance exit
                assert ctl[K["rr"]] == rr and th.equal(t["p"], before["p"][gb.span["p"][0]:gb.span["p"][1]])
                if last:
                    assert th.equal(t["r"], before["r"][gb.span["r"][0]:gb.span["r"][1]])
            else:
                report64(f"{tag} r", t["r"], st["r"])
                report64(f"{tag} p", t["p"], st["p"])
                assert abs(ctl[K["rr"]] - st["rr"]) <= 1e-6 * st["rr"] and abs(ctl[K["beta"]] - st["beta"]) <= 1e-6 * st["beta"]
        assert host(t["ctl"])[K["done"]] == 1.0
        # the finishing form
        s = host(t["x"])
        t["ap"].copy_(th.as_tensor(a(s).astype(np.float32)))
        ap = host(t["ap"])
        snap = gb.snapshot()
        hip_ops.trpo_cg_step(nv.TRPO_CG_FINISH, t["x"], None, None, t["ap"], None, damping, tol, t["ctl"], target_kl=0.01)
        gb.check()
        gb.same_as(snap, skip=("ctl",))
        sfs = s @ (ap + damping * s)
        ctl = host(t["ctl"])
        report64(f"cg finish n {n} max {max_steps} sFs / step", np.array([ctl[K["sfs"]], ctl[K["step"]]]), np.array([sfs, np.sqrt(2 * 0.01 / sfs)]))
        assert ctl[K["coeff"]] == 1.0


def test_cg_early_exits(ops):
    hip_ops, nv = ops
    K, n = nv.TRPO_CTL, 65
    # (a) r = g - F x0 = 0: done at the init launch, every later step launch is a no-op
    gb = GuardedBufs()
    x0 = np.random.default_rng(0).standard_normal(n).astype(np.float32)
    t = cg_bufs(gb, nv, n, x0, 2.0 * x0)
    t["ap"].copy_(th.as_tensor(2.0 * x0))
    hip_ops.trpo_cg_step(nv.TRPO_CG_INIT, t["x"], t["r"], t["p"], t["ap"], t["g"], 0.0, 1e-10, t["ctl"])
    assert host(t["ctl"])[K["rr"]] == 0.0 and host(t["ctl"])[K["done"]] == 1.0
    snap = gb.snapshot()
    for last in (False, True):
        hip_ops.trpo_cg_step(nv.TRPO_CG_STEP, t["x"], t["r"], t["p"], t["ap"], None, 0.0, 1e-10, t["ctl"], last=last)
    gb.check()
    gb.same_as(snap)
    # (b) F = 2 I: the first iteration solves the system, new_rr < tol: done, x moved, p and rr as they were; then no-ops
    gb = GuardedBufs()
    g = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    t = cg_bufs(gb, nv, n, np.zeros(n, np.float32), g)
    hip_ops.trpo_cg_step(nv.TRPO_CG_INIT, t["x"], t["r"], t["p"], t["ap"], t["g"], 0.0, 1e-10, t["ctl"])
    rr0 = host(t["ctl"])[K["rr"]]
    t["ap"].copy_(2.0 * t["p"])
    hip_ops.trpo_cg_step(nv.TRPO_CG_STEP, t["x"], t["r"], t["p"], t["ap"], None, 0.0, 1e-10, t["ctl"], last=False)
    ctl = host(t["ctl"])
    assert ctl[K["done"]] == 1.0 and ctl[K["rr"]] == rr0 and ctl[K["iters"]] == 1.0 and ctl[K["alpha"]] == pytest.approx(0.5, rel=1e-12)
    report64("cg tolerance exit x", t["x"], 0.5 * g.astype(np.float64))
    assert th.equal(t["p"].cpu(), th.as_tensor(g)) and float(t["r"].abs().max()) <= 1e-6
    snap = gb.snapshot()
    hip_ops.trpo_cg_step(nv.TRPO_CG_STEP, t["x"], t["r"], t["p"], t["ap"], None, 0.0, 1e-10, t["ctl"], last=False)
    gb.check()
    gb.same_as(snap)


# ---- apply step, value loss, the start vector -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CG_LENGTHS + (262144 + 77,))  # the last: beyond one pass of the grid (1024 x 256 lanes)
def test_apply_step(ops, n):
    hip_ops, nv = ops
    rng = np.random.default_rng(n)
    theta0, s = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    mask = (rng.uniform(size=n) < 0.6).astype(np.float32)
    before = rng.standard_normal(n).astype(np.float32)
    gb = GuardedBufs()
    theta = gb.put("theta", before)
    t0, sv, mk = gb.put_ro("theta0", theta0), gb.put_ro("s", s), gb.put_ro("mask", mask)
    ctl_h = np.zeros(nv.TRPO_CTL_WORDS)
    ctl_h[nv.TRPO_CTL["coeff"]], ctl_h[nv.TRPO_CTL["step"]] = 0.8 ** 3, 0.37
    ctl = gb.put_ro("ctl", ctl_h, dtype=th.float64)
    hip_ops.trpo_apply_step(theta, t0, sv, mk, ctl)
    gb.check()
    snap = gb.snapshot()
    hip_ops.trpo_apply_step(theta, t0, sv, mk, ctl)
    gb.same_as(snap)
    got = theta.cpu().numpy()
    on = mask != 0
    assert np.array_equal(got[~on], before[~on])  # untouched outside the actor's tensors, bit for bit
    if on.any():
        report64(f"apply step n {n}", got[on], theta0[on].astype(np.float64) + (0.8 ** 3 * 0.37) * s[on].astype(np.float64))


def test_value_loss(ops):
    hip_ops, _ = ops
    for rows in R.FLAT_ROWS:
        rng = np.random.default_rng(rows)
        v, ret = rng.standard_normal(rows).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
        gb = GuardedBufs()
        vd, rd = gb.put_ro("values", v), gb.put_ro("returns", ret)
        g, loss, total = gb.new("g", rows), gb.new("loss", 1), gb.put("sum", np.float32([1.5]))
        hip_ops.trpo_value_loss(vd, rd, g, loss, total)
        gb.check(written=("g", "loss"))
        d = v.astype(np.float64) - ret.astype(np.float64)
        report64(f"value loss rows {rows} g", g, 2.0 * d / rows)
        report64(f"value loss rows {rows} loss", loss, [np.mean(d * d)])
        assert float(total[0]) == np.float32(1.5) + loss.cpu().numpy()[0]
        first = g.clone()
        hip_ops.trpo_value_loss(vd, rd, g, loss, None)
        assert th.equal(g, first)


def test_x0_stream(ops):
    """the start vector against the counter contract in fp64 (tests/_rowkernel_reference.normal_stream): element i = 1e-4 * z_(i % 2) of
    pair i // 2 at the stream's offset, zero outside the mask; the second launch continues where the first ended"""
    hip_ops, nv = ops
    scale = 1e-4
    for n, seed, base in ((1, 5, 0), (4612, 7, 0), (9217, (0xABCDE << 32) | 17, 2 ** 32 - 3)):
        gb = GuardedBufs()
        x = gb.new("x", n)
        ones = gb.put_ro("mask", np.ones(n, np.float32))
        rng_ctl = hip_ops.new_rng_ctl(seed, DEV)
        rng_ctl[1] = base
        for launch in range(2):
            off = base + launch * ((n + 1) // 2)
            hip_ops.trpo_x0(x, ones, scale, rng_ctl)
            gb.check(written=("x",))
            assert int(rng_ctl[1]) == off + (n + 1) // 2 and int(rng_ctl[2]) == 0
            w, ws, share = RK.normal_worst(x.cpu().numpy().astype(np.float64) / float(np.float32(scale)), seed, off, n, nv.TRPO_TAG)
            bar = RK.NORMAL_BAR + 6 * 2.0 ** -24  # + the one float32 rounding of scale * z: |z| <= sqrt(-2 ln 2**-25) = 5.89
            print(f"TRPO x0 n {n} launch {launch}: worst {w:.3g} / {ws:.3g} beyond the slack, bar {bar:.3g}")
            assert w <= bar and ws <= bar and share <= 1e-3
    full = x.clone()
    mask_h = (np.arange(n) % 3 != 0).astype(np.float32)
    rng_ctl[1] = off
    hip_ops.trpo_x0(x, gb.put_ro("mask3", mask_h), scale, rng_ctl)
    gb.check()
    got, on = x.cpu().numpy(), mask_h != 0
    assert np.array_equal(got[on], full.cpu().numpy()[on]) and not got[~on].any()
