"""CPU checks of tests/_trpo_reference.py and of TRPO's host side. No GPU.

The ties: the Fisher-form product (tangent layers, head metric, per-layer backward: what the kernels compute) equals the published double
backward through autograd on the mean KL at rtol 1e-10, on all three heads; the CG loop reproduces np.linalg.solve on the damped Fisher
matrix of a tiny actor assembled column by column; a zero right-hand side, the early `residual_tol` exit and the last-iteration rule
behave as specified; the line search accepts or restores on hand-built cases.

The bars: per kind (tangent layer, head metric, whole product) the float32 ATen evaluation is re-measured over the GPU module's cases in
units of 2**-24 * M; it must pass its bar, the bar must be four times that figure (ATen builds differ a little: within a factor of two
either way) and no bar may exceed 64 units -- the rule of tests/test_rowkernel_reference.py.

The host side: the refusals that need no device, and the new entry points' argument checks (nothing is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import _trpo_reference as R
from core import TRPO, _native as nv  # noqa: F401  (the product under test: without it nothing here runs)
from core.trpo import MlpPolicy  # noqa: F401

assert {"cstr_linear_tangent_fwd_f32", "cstr_trpo_objective_f32", "cstr_trpo_fisher_head_f32", "cstr_trpo_cg_step_f32", "cstr_trpo_apply_step_f32",
        "cstr_trpo_value_loss_f32", "cstr_trpo_x0_f32"} <= set(nv.SYMBOLS)  # the entry points the statements below describe

F64 = th.float64


@pytest.mark.parametrize("head", R.HEADS + (("gauss", 4),))
@pytest.mark.parametrize("rows", [2, 17])
def test_fisher_form_equals_double_backward(head, rows):
    for act in ("tanh", "relu"):
        actor = R.make_actor(11 + rows, head, hidden=(7, 5), act=act)
        theta0 = th.as_tensor(R.flat_of(actor)).to(F64)
        obs = np.random.default_rng(rows).uniform(-1, 1, (rows, 4)).astype(np.float32)
        acts = [a.numpy() for a in R.forward(actor, theta0, obs)]
        for seed in range(4):
            v = th.as_tensor(np.random.default_rng(100 + seed).standard_normal(theta0.numel())).to(F64)
            want = R.fvp_double_backward(actor, theta0, obs, v, 0.1)
            got = R.fvp_fisher(actor, theta0.numpy(), acts, v.numpy(), 0.1)
            assert th.allclose(got, want, rtol=1e-10, atol=1e-10 * float(want.abs().max())), (head, rows, act, seed)


def _fisher_matrix(actor, theta0, obs, damping):
    acts = [a.numpy() for a in R.forward(actor, theta0, obs)]
    n = theta0.numel()
    cols = [R.fvp_fisher(actor, theta0.numpy(), acts, np.eye(n)[:, j], damping) for j in range(n)]
    return th.stack(cols, 1), acts


@pytest.mark.parametrize("head", R.HEADS)
def test_cg_reproduces_the_linear_solve(head):
    actor = R.make_actor(5, head, hidden=(4,))  # net_arch [4]
    theta0 = th.as_tensor(R.flat_of(actor)).to(F64)
    obs = np.random.default_rng(0).uniform(-1, 1, (64, 4)).astype(np.float32)
    fm, acts = _fisher_matrix(actor, theta0, obs, 0.1)
    assert th.allclose(fm, fm.T, rtol=1e-9, atol=1e-12)  # symmetric positive definite
    g = th.as_tensor(np.random.default_rng(1).standard_normal(theta0.numel())).to(F64)
    x0 = 1e-4 * th.as_tensor(np.random.default_rng(2).standard_normal(theta0.numel())).to(F64)
    fvp = lambda v: R.fvp_fisher(actor, theta0.numpy(), acts, v.numpy(), 0.1)  # noqa: E731
    x, hist, iters = R.cg_solve(fvp, g, x0, max_iter=4 * theta0.numel(), tol=1e-22)
    want = th.as_tensor(np.linalg.solve(fm.numpy(), g.numpy()))
    assert float((x - want).abs().max()) <= 1e-8 * float(want.abs().max()), (iters, hist[-1])
    assert all(b < a * 1e3 for a, b in zip(hist, hist[1:]))  # the residual history is recorded per completed iteration


def test_cg_exits_and_last_iteration_rule():
    a = th.diag(th.tensor([1.0, 2.0, 4.0], dtype=F64))
    fvp = lambda v: a @ v  # noqa: E731
    zero = th.zeros(3, dtype=F64)
    # a zero right-hand side from a zero start: rr = 0 < tol, x is returned as it is, no product beyond the first
    x, hist, iters = R.cg_solve(fvp, zero, zero.clone(), 15)
    assert iters == 0 and hist == [0.0] and th.equal(x, zero)
    # three distinct eigenvalues: exact after three iterations, the residual_tol exit fires there (before max_iter)
    g = th.tensor([1.0, 1.0, 1.0], dtype=F64)
    x, hist, iters = R.cg_solve(fvp, g, zero.clone(), 15)
    assert iters == 3 and th.allclose(x, th.tensor([1.0, 0.5, 0.25], dtype=F64), rtol=1e-12)
    # max_iter = 1: x moves once and r, rr are not updated (the last iteration returns before them)
    x, hist, iters = R.cg_solve(fvp, g, zero.clone(), 1)
    assert iters == 1 and len(hist) == 1 and th.allclose(x, g * (3.0 / 7.0))
    # launch by launch: cg_step_stmt walks the same iterates as cg_solve
    x, r, p, rr = zero.clone(), g.clone(), g.clone(), float(g @ g)
    for i in range(3):
        st = R.cg_step_stmt(x, r, p, a @ p, rr, 0.0, last=False)
        x, r, p, rr = st["x"], st["r"], st["p"], st["rr"]
    assert st["done"] and th.allclose(x, th.tensor([1.0, 0.5, 0.25], dtype=F64), rtol=1e-12)


def test_line_search_accepts_or_restores():
    theta0, s = th.tensor([1.0, -2.0], dtype=F64), th.tensor([1.0, 1.0], dtype=F64)
    # objective' = the first coordinate's move, kl' = its square: accepted once coeff * step < sqrt(target_kl)
    ev = lambda t: (5.0 + (t[0] - theta0[0]), (t[0] - theta0[0]) ** 2)  # noqa: E731
    theta, coeff, recs = R.line_search(ev, theta0, s, 1.0, 5.0, 0.5, 0.8, 10)
    assert [r[3] for r in recs] == [False, False, True] and coeff == pytest.approx(0.64) and th.allclose(theta, theta0 + 0.64 * s)
    theta, coeff, recs = R.line_search(ev, theta0, s, 0.1, 5.0, 0.5, 0.8, 10)
    assert coeff == 1.0 and len(recs) == 1
    # rejected by the objective alone (kl fine), by the KL alone (objective fine), never accepted: theta0 comes back bit for bit
    theta, coeff, recs = R.line_search(lambda t: (4.0, 0.0), theta0, s, 1.0, 5.0, 0.5, 0.8, 10)
    assert coeff is None and len(recs) == 10 and th.equal(theta, theta0) and recs[-1][0] == pytest.approx(0.8 ** 9)
    theta, coeff, recs = R.line_search(lambda t: (6.0, 0.5), theta0, s, 1.0, 5.0, 0.5, 0.8, 3)  # kl' == target_kl is no acceptance
    assert coeff is None and len(recs) == 3 and th.equal(theta, theta0)
    m = R.ls_margins([(1.0, 6.0, 0.1, True)], 5.0, 0.5)
    assert m[0] > 100


def test_objective_gradient_and_critic_statements():
    for head in R.HEADS:
        actor = R.make_actor(2, head, hidden=(6, 6))
        batch = R.make_batch(3, actor, 33)
        theta0 = th.as_tensor(R.flat_of(actor)).to(F64)
        obj, kl, g = R.objective_grad(actor, theta0, batch)
        assert abs(float(kl)) < 1e-15 and g.shape == theta0.shape and float(g.abs().max()) > 0
        eps = 1e-6 * g / g.norm()
        old = R.old_of(actor, theta0, batch["obs"])
        up, _ = R.objective_kl(actor, theta0 + eps, batch, *old)
        dn, _ = R.objective_kl(actor, theta0 - eps, batch, *old)
        assert float(up - dn) / 2e-6 == pytest.approx(float(g.norm()), rel=1e-5)
    rng = np.random.default_rng(0)
    vws = [(rng.standard_normal((5, 4)).astype(np.float32), np.zeros(5, np.float32)), (rng.standard_normal((1, 5)).astype(np.float32), np.zeros(1, np.float32))]
    mbs = [(rng.standard_normal((8, 4)).astype(np.float32), rng.standard_normal(8).astype(np.float32)) for _ in range(3)]
    new, losses = R.critic_pass(vws, "tanh", mbs, 1e-3)
    ps = [th.as_tensor(a).to(F64).requires_grad_(True) for wb in vws for a in wb]
    opt = th.optim.Adam(ps, lr=1e-3, eps=1e-5)
    for obs, ret in mbs:
        loss = th.nn.functional.mse_loss(th.as_tensor(ret).to(F64), R.mlp_value([(ps[0], ps[1]), (ps[2], ps[3])], th.as_tensor(obs).to(F64), "tanh"))
        opt.zero_grad()
        loss.backward()
        opt.step()
    for (w, b), pw, pb in zip(new, ps[0::2], ps[1::2]):
        assert th.allclose(w, pw.detach(), rtol=1e-12, atol=1e-15) and th.allclose(b, pb.detach(), rtol=1e-12, atol=1e-15)


# ---- the bars ---------------------------------------------------------------------------------------------------------------------------
def test_float32_aten_sets_the_bars():
    fig = R.measure_aten()
    assert set(fig) == set(R.BARS)
    for kind, f in sorted(fig.items()):
        print(f"ATEN {kind}: {f:.3f} units, bar {R.BARS[kind]:.2f}")
        assert f <= R.BARS[kind] <= R.CAP, (kind, f)
        assert 2.0 * f <= R.BARS[kind] <= 8.0 * f, (kind, f, R.BARS[kind])  # 4 x the figure, within ATen's build-to-build factor of two


def test_cases_meet_the_input_conditions():
    n = 0
    for case in R.tangent_cases():
        R.assert_conditions(R.tangent_case(*case))
        n += 1
    assert n == len(R.TANGENT_ROWS) * len(R.TANGENT_KN) * 6
    for case in R.FVP_CASES:
        c = R.fvp_case(*case)
        if case[2] == "tanh":
            assert max(np.abs(a).max() for a in c["acts"][1:-1]) < R.TANH_MAX
    w, ok = R.close64(np.float32([1.0, 2.0]), [1.0 + 1e-6, 2.0])
    assert ok and 0 < w < 1 and not R.close64([1.0 + 1e-5, 2.0], [1.0, 2.0])[1]


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_no_device():
    import core
    from core import TRPO
    from core.common.on_policy_algorithm import OnPolicyAlgorithm
    from core.common.policies import ActorCriticPolicy
    from core.trpo import TRPO as T2, MlpPolicy

    assert TRPO is T2 and TRPO is core.TRPO and "TRPO" in core.__all__ and issubclass(TRPO, OnPolicyAlgorithm)
    assert MlpPolicy is ActorCriticPolicy and TRPO.policy_aliases.keys() == {"MlpPolicy"} and TRPO.goal_face_support is False
    for kw, word in ((dict(cg_max_steps=0), "cg_max_steps"), (dict(line_search_max_iter=0), "line_search_max_iter"),
                     (dict(line_search_shrinking_factor=1.0), "line_search_shrinking_factor"), (dict(line_search_shrinking_factor=0.0), "shrinking"),
                     (dict(target_kl=0.0), "target_kl"), (dict(target_kl=-1.0), "target_kl"), (dict(sub_sampling_factor=0), "sub_sampling_factor"),
                     (dict(n_critic_updates=-1), "n_critic_updates"), (dict(use_sde=True), "gSDE")):
        with pytest.raises(ValueError, match=word):
            TRPO("MlpPolicy", None, **kw)
    keys = TRPO._ctor_keys()
    import inspect

    params = inspect.signature(TRPO.__init__).parameters
    assert all(k in params for k in keys)  # every key is a constructor argument
    for k in ("cg_max_steps", "cg_damping", "line_search_shrinking_factor", "line_search_max_iter", "n_critic_updates", "target_kl",
              "sub_sampling_factor", "normalize_advantage", "gae_lambda", "n_steps", "batch_size"):
        assert k in keys
    assert params["learning_rate"].default == 1e-3 and params["batch_size"].default == 128 and params["cg_max_steps"].default == 15
    assert params["target_kl"].default == 0.01 and params["n_critic_updates"].default == 10 and params["cg_damping"].default == 0.1


def test_entry_points_reject_bad_arguments_on_the_host():
    from core import _native as nv

    lib = nv.lib()
    null, fake, odd, other = C.c_void_p(None), C.c_void_p(0x10000), C.c_void_p(0x10002), C.c_void_p(0x9000000)
    i64, f64 = C.c_int64, C.c_double

    def tangent(x=fake, xd=null, w=C.c_void_p(0x200000), wd=C.c_void_p(0x300000), bd=C.c_void_p(0x400000), y=C.c_void_p(0x500000), act=2,
                z=other, m=8, n=8, k=4, ldx=4):
        return lib.cstr_linear_tangent_fwd_f32(x, i64(ldx), xd, i64(ldx), w, wd, bd, y, act, z, i64(m), i64(n), i64(k), null)

    assert tangent(x=null) == -1 and tangent(wd=null) == -1 and tangent(z=null) == -1 and tangent(y=null) == -1  # tanh needs y
    assert tangent(x=odd) == -1 and tangent(ldx=3) == -1 and tangent(m=0) == -1 and tangent(act=3) == -2 and tangent(m=1 << 24) == -2
    assert tangent(z=fake) == -1  # z_dot over x
    assert tangent(ldx=1 << 31) == -2  # the kernel carries the row strides as int

    def objective(**kw):
        base = dict(dist=0x10000, ld=2, log_std=0x20000, old_dist=0x10000, old_ld=2, old_log_std=0x20000, actions=0x30000, old_log_prob=0x40000,
                    adv=0x50000, batch=16, head=0, k0=2, k1=0, normalize_advantage=1, line_search=0, reserved=0, target_kl=0.01, shrink=0.8,
                    g_dist=0x60000, g_log_std=0x70000, scalars_out=0x80000, ctl=0x90000, accepted=None)
        base.update(kw)
        p = nv.TrpoObjective(*[base[f[0]] for f in nv.TrpoObjective._fields_])
        return lib.cstr_trpo_objective_f32(C.byref(p), C.c_void_p(0xA0000), null)

    assert lib.cstr_trpo_objective_f32(null, fake, null) == -1
    assert objective(dist=None) == -1 and objective(ctl=None) == -1 and objective(batch=0) == -1 and objective(g_dist=None) == -1
    assert objective(line_search=1) == -1  # no `accepted`
    assert objective(line_search=1, accepted=0xB0000, shrink=1.0) == -1 and objective(line_search=1, accepted=0xB0000, target_kl=0.0) == -1
    assert objective(k0=3) == -2 and objective(head=7) == -2 and objective(head=1, k0=65) == -2 and objective(head=2, k0=3, k1=33) == -2
    assert objective(ld=1) == -1 and objective(dist=0x10004) == -1 and objective(g_dist=0x10000) == -1 and objective(ctl=0x90004) == -1
    assert objective(adv=0x50002) == -1 and objective(scalars_out=0x90008) == -1  # misaligned; scalars over the control block

    def head(h=0, k0=2, k1=0, dd=fake, dist=null, ls=C.c_void_p(0x20000), vls=C.c_void_p(0x30000), up=other, gls=C.c_void_p(0x40000), b=8):
        return lib.cstr_trpo_fisher_head_f32(h, k0, k1, dd, i64(max(k0 + k1, 2)), dist, i64(max(k0 + k1, 2)), ls, vls, i64(b), up, gls, null)

    assert head(dd=null) == -1 and head(up=null) == -1 and head(ls=null) == -1 and head(h=1, k0=9) == -1  # a discrete head needs the logits
    assert head(k0=3) == -2 and head(h=1, k0=1, dist=fake) == -2 and head(up=fake) == -1 and head(b=0) == -1 and head(dd=C.c_void_p(0x10004)) == -1

    def cg(mode=1, x=fake, r=C.c_void_p(0x200000), p=C.c_void_p(0x300000), ap=C.c_void_p(0x400000), g=C.c_void_p(0x500000), n=64, damping=0.1,
           tol=1e-10, kl=0.01, ctl=other):
        return lib.cstr_trpo_cg_step_f32(mode, x, r, p, ap, g, i64(n), f64(damping), f64(tol), f64(kl), 0, ctl, null)

    assert cg(mode=5) == -1 and cg(x=null) == -1 and cg(r=null) == -1 and cg(mode=0, g=null) == -1 and cg(ctl=null) == -1 and cg(n=0) == -1
    assert cg(damping=-1.0) == -1 and cg(damping=float("nan")) == -1 and cg(mode=2, kl=0.0) == -1 and cg(n=(1 << 24) + 1) == -2
    assert cg(x=odd) == -1 and cg(p=fake) == -1 and cg(ap=fake) == -1 and cg(ctl=C.c_void_p(0x9000004)) == -1  # misaligned / overlapping
    assert lib.cstr_trpo_apply_step_f32(null, fake, fake, fake, i64(8), other, null) == -1
    assert lib.cstr_trpo_apply_step_f32(fake, fake, C.c_void_p(0x200000), C.c_void_p(0x300000), i64(8), other, null) == -1  # theta over theta0
    assert lib.cstr_trpo_apply_step_f32(fake, C.c_void_p(0x200000), C.c_void_p(0x300000), C.c_void_p(0x400000), i64(0), other, null) == -1
    assert lib.cstr_trpo_value_loss_f32(fake, null, i64(8), other, null, null, null) == -1
    assert lib.cstr_trpo_value_loss_f32(fake, C.c_void_p(0x200000), i64(8), fake, null, null, null) == -1  # g_value over values
    assert lib.cstr_trpo_x0_f32(fake, null, i64(8), C.c_float(1e-4), other, null) == -1
    assert lib.cstr_trpo_x0_f32(fake, C.c_void_p(0x200000), i64(8), C.c_float(1e-4), C.c_void_p(0x9000004), null) == -1
