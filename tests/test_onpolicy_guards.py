"""The on-policy and DQN kernels (csrc/cstr_ppo.hip, csrc/cstr_a2c.hip, csrc/cstr_dqn.hip, the core in csrc/cstr_onpolicy_device.h) past
their grid caps, under guard (tests/_sentinel_bufs.py: GuardedBufs) and on NaN inputs. Their values at small shapes are compared in
tests/test_ppo.py, test_a2c.py, test_dqn.py and test_rmsprop_tf.py; the references, the bars and the float32 model that shows the bars'
room are in tests/_onpolicy_reference.py (checked on the CPU by tests/test_onpolicy_reference.py).

A. Past the caps. The loss launches at 16383 ... 32769 rows (64 workgroups, up to a third pass of the stride loop, all 64 partials)
   against fp64 autograd; dqn_loss at the same caps with strided q / g_q; the sum-of-squares pass behind grad_clip / rmsprop /
   rmsprop_tf at 16384 ... 32771 elements (bit for bit the NumPy statements) and the step kernels one pass beyond 4096 x 512 float4;
   the lane-per-env launches at 4096 x 64 + 1 rows, the gather at 2048 x 256 + 1.
B. Guards at small shapes: sentinel bands on both sides of every buffer, outputs fully written, inputs bit-unchanged, a second launch
   from the same state gives the same bits, the workspace ticket back at 0; every optional output dropped in turn; strided `mean`;
   a full and a broken rollout position; the closed ends of both clips against fp64 autograd.
C. NaN: a NaN value (value clip on / off), mean or advantage in any one row, PPO and A2C: NaN exactly where the fp64 torch statement
   has one, the other rows within their bars; once each through the Categorical and MultiCategorical launches.
Every figure is printed in units of its bar (BAR ...) before it is asserted."""
import contextlib

import numpy as np
import pytest
import torch as th

import _mcat_helpers as mh
import _onpolicy_reference as R
import test_categorical as tcat
import test_multicategorical as tmcat
from _sentinel_bufs import GuardedBufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SMALL_B = (1, 255, 256, 257)   # one row, one short of a workgroup, a workgroup, its first row of the next
SMALL_N = (1, 63, 64, 65)      # the same around one wave of the lane-per-env launches
I64 = th.int64


def bits(t):
    return t.view({4: th.int32, 8: th.int64}[t.element_size()]) if t.is_floating_point() else t


class BitBufs(GuardedBufs):
    """GuardedBufs whose input and relaunch comparisons are on bit patterns, so that a NaN equals itself (the NaN cases)"""

    def check(self, written=()):
        frozen = {name: ro for name, (_, _, ro) in self.bufs.items() if ro is not None}
        for name in frozen:
            self.bufs[name] = self.bufs[name][:2] + (None,)
        try:
            super().check(written)
        finally:
            for name, ro in frozen.items():
                self.bufs[name] = self.bufs[name][:2] + (ro,)
        for name, ro in frozen.items():
            assert th.equal(bits(self.bufs[name][0]), bits(ro)), f"{name}: a read-only input was changed"

    def same_as(self, snap, skip=()):
        for name, (f, _, _) in self.bufs.items():
            if name not in skip:
                assert th.equal(bits(f), bits(snap[name])), f"{name}: the second launch differs from the first"


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    assert th.cuda.is_available()
    from core import _native as nv
    from core.common import hip_ops

    nv.lib()
    return hip_ops


def report(tag, fig):
    for k, v in fig.items():
        print(f"BAR {tag} {k}: {v:.3f}")
    assert max(fig.values()) <= 1.0, (tag, {k: v for k, v in fig.items() if not v <= 1.0})


def units(got, want, what):
    """max |got - want| / (2e-6 |want| + 1e-7), printed, then asserted"""
    got, want = np.asarray(host(got) if isinstance(got, th.Tensor) else got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    u = float((np.abs(got - want) / R.bar(want)).max())
    print(f"BAR {what}: {u:.3f}")
    assert u <= 1.0, (what, u)


def twice(b, launch, written, restore=(), skip=()):
    """launch, check the guards, restore the in-place operands, launch again: the same bits"""
    saved = [(t, t.clone()) for t in restore]
    launch()
    b.check(written)
    snap = b.snapshot()
    for t, v in saved:
        t.copy_(v)
    launch()
    b.check(written)
    b.same_as(snap, skip=skip)


# ==== the loss launches ===================================================================================================================
LOSS_OUT = ("g_mean", "g_value", "g_log_std", "scalars", "sums", "log_prob")


def loss_launch(ops, ppo, case, vf, norm, clip_range=R.CLIP_RANGE, drop=(), ldm=None, guarded=True, old_logp=None):
    """one loss launch on guarded buffers (guarded=False: plain tensors, for the large cases) -> (bufs, launch, the tensors by name)"""
    mean, log_std, actions, values, old_values, old_lp, adv, returns = R.unpack(case, ppo)
    B, A = actions.shape
    ns = 6 if ppo else 4
    b = BitBufs()
    ro = (lambda name, a: b.put_ro(name, a)) if guarded else (lambda name, a: dev(a))
    new = (lambda name, *s: b.new(name, *s)) if guarded else (lambda name, *s: th.full(s, 77.0, device=DEV))
    t = dict(log_std=ro("log_std", log_std), actions=ro("actions", actions), values=ro("values", values), adv=ro("adv", adv),
             returns=ro("returns", returns))
    t["mean"] = b.put_ro_cols("mean", mean, ldm, ldm - A) if ldm else ro("mean", mean)  # the LAST A columns of a wider matrix
    if ppo:
        t["old_values"] = ro("old_values", old_values)
        t["old_lp"] = ro("old_lp", old_lp) if old_logp is None else old_logp
    for name, shape in (("g_mean", (B, A)), ("g_value", (B,)), ("g_log_std", (A,)), ("scalars", (ns,)), ("log_prob", (B,))):
        t[name] = new(name, *shape)
    t["sums"] = b.put("sums", np.arange(ns, dtype=np.float32)) if guarded else dev(np.arange(ns, dtype=np.float32))
    t["ws"] = b.put("ws", th.zeros(ops.new_ppo_workspace(DEV).shape, dtype=I64), dtype=I64) if guarded else ops.new_ppo_workspace(DEV)
    opt = {k: (None if k in drop else t[k]) for k in ("scalars", "sums", "log_prob")}

    def launch():
        if ppo:
            ops.ppo_loss(t["mean"], t["log_std"], t["actions"], t["values"], t["old_values"], t["old_lp"], t["adv"], t["returns"], clip_range, vf,
                         norm, R.ENT_COEF, R.VF_COEF, t["g_mean"], t["g_value"], t["g_log_std"], t["ws"], scalars_out=opt["scalars"],
                         scalars_sum=opt["sums"], log_prob_out=opt["log_prob"])
        else:
            ops.a2c_loss(t["mean"], t["log_std"], t["actions"], t["values"], t["adv"], t["returns"], norm, R.ENT_COEF, R.VF_COEF, t["g_mean"],
                         t["g_value"], t["g_log_std"], t["ws"], scalars_out=opt["scalars"], log_prob_out=opt["log_prob"])

    return b, launch, t


def loss_outputs(t):
    th.cuda.synchronize()
    return dict(scalars=host(t["scalars"]), g_mean=host(t["g_mean"]), g_value=host(t["g_value"]), g_log_std=host(t["g_log_std"]),
                log_prob=host(t["log_prob"]))


ALGOS = [("ppo", vf, norm) for vf, norm in R.PPO_VARIANTS] + [("a2c", None, True), ("a2c", None, False)]


# ---- A.1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,vf,norm", ALGOS)
@pytest.mark.parametrize("B,A", R.CAP_SIZES)
def test_loss_past_the_cap(ops, B, A, algo, vf, norm):
    ppo = algo == "ppo"
    case = R.loss_inputs(ppo, B, A)
    ref = R.loss_reference(case, ppo, vf, norm)
    if ppo:
        assert np.min(np.abs(np.abs(ref["ratio"] - 1) - R.CLIP_RANGE)) > 1e-3  # no row sits on a clip bound: clip_fraction compares exactly
        assert 0 < ref["scalars"][5] < 1
    _, launch, t = loss_launch(ops, ppo, case, vf, norm, guarded=False)
    launch()
    got = loss_outputs(t)
    assert int(t["ws"][0]) == 0  # the ticket reset itself
    report(f"{algo} loss B={B} A={A} vf={vf} norm={norm}", R.loss_figures(got, ref))
    first = {k: v.copy() for k, v in got.items()}
    launch()
    again = loss_outputs(t)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)


# ---- B: guards, optional outputs, strided mean ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["ppo", "a2c"])
@pytest.mark.parametrize("B", SMALL_B)
def test_loss_guarded(ops, B, algo):
    ppo, A = algo == "ppo", 2 if B % 2 else 4
    vf, norm = (0.2 if ppo else None), B > 1  # A2C normalises a single row to NaN (tests/test_a2c.py has that case)
    case = R.loss_inputs(ppo, B, A)
    written = tuple(k for k in LOSS_OUT if ppo or k != "sums")
    b, launch, t = loss_launch(ops, ppo, case, vf, norm)
    twice(b, launch, written, restore=(t["sums"], t["ws"]))
    full = loss_outputs(t)
    assert int(t["ws"][0]) == 0
    if ppo:
        np.testing.assert_array_equal(host(t["sums"]), np.arange(6, dtype=np.float32) + full["scalars"])  # scalars_sum accumulates
    report(f"{algo} guarded loss B={B} A={A}", R.loss_figures(full, R.loss_reference(case, ppo, vf, norm)))
    for drop in ("scalars", "sums", "log_prob") if ppo else ("scalars", "log_prob"):  # each optional output left out in turn
        bd, launch_d, td = loss_launch(ops, ppo, case, vf, norm, drop=(drop,))
        twice(bd, launch_d, tuple(k for k in written if k != drop), restore=(td["sums"], td["ws"]))
        assert all(th.equal(td[k], t[k]) for k in written if k != drop), drop  # the remaining outputs: the bits of the full launch
        if drop == "sums":
            np.testing.assert_array_equal(host(td["sums"]), np.arange(6, dtype=np.float32))  # untouched
    # `mean` as the last A columns of a [B, 2 A] matrix (ldm = 4 / 8): the same bits, the other columns untouched
    bs, launch_s, ts = loss_launch(ops, ppo, case, vf, norm, ldm=2 * A)
    twice(bs, launch_s, written, restore=(ts["sums"], ts["ws"]))
    assert all(th.equal(ts[k], t[k]) for k in ("g_mean", "g_value", "g_log_std", "scalars", "log_prob"))


def test_ppo_clip_range_zero_keeps_the_gradient_at_ratio_one(ops):
    """every rollout's first minibatch, taken at the boundary: old_log_prob = the launch's own log_prob_out, ratio == 1 sits on the
    closed interval [1, 1] and the gradient is the unclipped one"""
    B, A = 257, 2
    case = list(R.loss_inputs(True, B, A))
    b0, launch0, t0 = loss_launch(ops, True, tuple(case), None, True, clip_range=0.0)
    launch0()
    b0.check(LOSS_OUT)
    b, launch, t = loss_launch(ops, True, tuple(case), None, True, clip_range=0.0, old_logp=t0["log_prob"].clone())
    twice(b, launch, LOSS_OUT, restore=(t["sums"], t["ws"]))
    got = loss_outputs(t)
    lp64 = R.loss_reference(tuple(case), True, None, True)["log_prob"]
    case[5] = lp64  # old = log_prob.detach(), in fp64
    ref = R.loss_reference(tuple(case), True, None, True, clip_range=0.0)
    open_ref = R.loss_reference(tuple(case), True, None, True, clip_range=10.0)
    assert np.array_equal(ref["g_mean"], open_ref["g_mean"]) and np.abs(ref["g_mean"]).min() > 0  # the statement passes it whole
    assert ref["scalars"][4] == 0.0 and ref["scalars"][5] == 0.0
    assert got["scalars"][4] == 0.0 and got["scalars"][5] == 0.0  # approx_kl and clip_fraction: exactly 0
    report("ppo clip_range=0", R.loss_figures(got, ref))


def test_ppo_value_clip_passes_the_gradient_on_its_bounds(ops):
    """value steps of exactly +cv and -cv (cv = 0.25, old_values = -20): torch's clamp passes the gradient on the closed interval"""
    case = R.on_the_value_clip_bound(R.loss_inputs(True, 12, 2))
    assert set(np.abs(case[3][:8] - case[4][:8]).tolist()) == {0.25}
    ref = R.loss_reference(case, True, 0.25, False)
    b, launch, t = loss_launch(ops, True, case, 0.25, False)
    twice(b, launch, LOSS_OUT, restore=(t["sums"], t["ws"]))
    got = loss_outputs(t)
    assert (ref["g_value"][:8] != 0).all() and (got["g_value"][:8] != 0).all()
    assert (ref["g_value"] == 0).any() and np.array_equal(ref["g_value"] == 0, got["g_value"] == 0)  # the clamped rows of the case pass none
    report("ppo value step on +-clip_range_vf", R.loss_figures(got, ref))


# ---- C: NaN ----------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def nan_arguments():
    """the fp64 statements build a torch Normal, which by default refuses a NaN mean before computing anything"""
    before = th.distributions.Distribution._validate_args
    th.distributions.Distribution.set_default_validate_args(False)
    try:
        yield
    finally:
        th.distributions.Distribution.set_default_validate_args(before)


def with_nan(case, ppo, what, row):
    c = [x.copy() for x in case]
    if what in ("values_clip", "values"):
        c[3][row] = np.nan
    elif what == "mean":
        c[0][row, 1] = np.nan
    else:
        c[6 if ppo else 4][row] = np.nan
    return tuple(c)


NAN_CASES = [("ppo", w) for w in ("values_clip", "values", "mean", "adv")] + [("a2c", w) for w in ("values", "mean", "adv")]  # A2C has no value clip


@pytest.mark.parametrize("algo,what", NAN_CASES)
def test_loss_propagates_a_nan_as_the_fp64_statement_does(ops, algo, what):
    """B = 12, normalisation off, the NaN in each row in turn (the rows' ratios lie inside and on both sides of the clip range)"""
    ppo = algo == "ppo"
    vf = 0.2 if what == "values_clip" else None
    clean = R.loss_inputs(ppo, 12, 2)
    worst, seen = {}, set()
    for row in range(12):
        case = with_nan(clean, ppo, what, row)
        with nan_arguments(), np.errstate(all="ignore"):
            ref = R.loss_reference(case, ppo, vf, False)
        b, launch, t = loss_launch(ops, ppo, case, vf, False)
        written = tuple(k for k in LOSS_OUT if ppo or k != "sums")
        twice(b, launch, written, restore=(t["sums"], t["ws"]))
        got = loss_outputs(t)
        for k, v in R.nan_figures(got, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
        seen.add((tuple(np.isnan(ref["scalars"]).tolist()), bool(np.isnan(ref["g_value"][row])), bool(np.isnan(ref["g_mean"][row]).all())))
        others = np.arange(12) != row
        assert np.isfinite(got["g_mean"][others]).all() and np.isfinite(got["g_value"][others]).all()
    print(f"NAN {algo} {what}: the statement's (NaN scalars, NaN g_value[row], NaN g_mean[row]) = {sorted(seen)}")
    assert len(seen) == 1  # the same verdict whichever row carries the NaN
    report(f"{algo} NaN in {what}, finite outputs", worst)


@pytest.mark.parametrize("head", ["categorical", "multicategorical"])
def test_discrete_loss_launches_share_the_nan_contract(ops, head):
    """policy_term / value_term serve all four loss launches: a NaN value under the value clip and a NaN old log-prob, once each"""
    B = 12
    if head == "categorical":
        clean = tcat.loss_case(B, 9, 4242)
        stmt = lambda c, crv: tcat.loss_torch(c, 0, th.float64, False, 0.01, 0.5, clip_range_vf=crv)  # noqa: E731
        run = lambda c, crv: tcat.run_loss(ops, c, 3, 3, 0, False, 0.01, 0.5, clip_range_vf=crv)  # noqa: E731
    else:
        clean = mh.loss_case(B, (3, 5), 4242)
        stmt = lambda c, crv: mh.loss_torch(c, (3, 5), 0, th.float64, False, 0.01, 0.5, clip_range_vf=crv)  # noqa: E731
        run = lambda c, crv: tmcat.run_loss(ops, c, (3, 5), 3, 0, False, 0.01, 0.5, clip_range_vf=crv)  # noqa: E731
    for key, crv, row in (("values", 0.1, 5), ("old_lp", None, 7)):
        c = {k: v.copy() for k, v in clean.items()}
        c[key][row] = np.nan
        with np.errstate(all="ignore"):
            want = stmt(c, crv)
        got = run(c, crv)  # sentinels, accumulation and the second launch are checked in there
        assert np.isnan(want[0]).any()
        for i, name in enumerate(("scalars", "g_logits", "g_value")):
            assert np.array_equal(np.isnan(got[i]), np.isnan(want[i])), (head, key, name, np.argwhere(np.isnan(got[i])).tolist(), np.argwhere(np.isnan(want[i])).tolist())
        # what stays finite: the gradients at the bar tests/test_categorical.py holds them to, a scalar at the same bar relative to
        # the magnitude behind it (the mean of its absolute terms, loss_torch's `mags`; clip_fraction, the sixth, is exact)
        for i, name in ((1, "g_logits"), (2, "g_value")):
            ok = ~np.isnan(want[i])
            np.testing.assert_allclose(got[i][ok], want[i][ok], rtol=tcat.RTOL, atol=tcat.ATOL, err_msg=f"{head} {key} {name}")
        for k in range(5):
            if not np.isnan(want[0][k]):
                assert abs(got[0][k] - want[0][k]) <= tcat.RTOL * max(abs(want[0][k]), want[4][k]) + tcat.ATOL, (head, key, k, got[0][k], want[0][k])
        assert abs(got[0][5] - want[0][5]) <= np.nan_to_num(want[4][5]) + 1e-7  # test_categorical.check_scalars' rule


# ==== dqn_loss ============================================================================================================================
def dqn_loss_launch(ops, case, K, drop=()):
    q, nq, index, rew, done = case
    B, M = q.shape
    b = BitBufs()
    t = dict(q=b.put_ro_cols("q", q, M + 3, 0), next_q=b.put_ro_cols("next_q", nq, M + 4, 0), valve=b.put_ro("valve", R.pair_np(index, K)),
             reward=b.put_ro("reward", rew), done=b.put_ro("done", done), g_q=b.new_cols("g_q", B, M + 3, 0, M), loss=b.new("loss", 1),
             loss_sum=b.put("loss_sum", np.array([3.0], np.float32)), cur=b.new("cur", B), tgt=b.new("tgt", B),
             ws=b.put("ws", th.zeros(ops.new_ppo_workspace(DEV).shape, dtype=I64), dtype=I64))
    opt = {k: (None if k in drop else t[k]) for k in ("loss_sum", "cur", "tgt")}
    launch = lambda: ops.dqn_loss(t["q"], t["next_q"], t["valve"], t["reward"], t["done"], 0.99, K, t["g_q"], t["loss"], t["ws"],  # noqa: E731
                                  loss_sum=opt["loss_sum"], cur_q_out=opt["cur"], target_out=opt["tgt"])
    return b, launch, t


def check_dqn_loss(t, case, tag):
    q, nq, index, rew, done = case
    B = q.shape[0]
    wc, wt, wl, wg = R.dqn_loss_f64(q, nq, index, rew, done, 0.99)
    g, cur, tgt, loss = host(t["g_q"]), host(t["cur"]), host(t["tgt"]), float(t["loss"])
    u_t, u_c, u_g = R.ulps(tgt, wt).max(), R.ulps(cur, wc).max(), R.ulps(g, wg).max()
    fig = abs(loss - wl) / float(R.bar(wl))
    print(f"BAR {tag}: target {u_t:.2f} ulp, current {u_c:.2f} ulp, gradient {u_g:.2f} ulp (bar 2); loss {fig:.3f}")
    assert u_t <= 2 and u_c <= 2 and u_g <= 2 and fig <= 1.0
    assert np.count_nonzero(g) == B and np.array_equal(np.nonzero(g)[1], index)  # one entry per row, at the taken index
    assert int(t["ws"][0]) == 0 and float(t["loss_sum"]) == np.float32(3.0) + np.float32(loss)


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("B", [16384, 16385, 32769])
def test_dqn_loss_past_the_cap(ops, B, K):
    """row stride M + 3 for q and g_q (M + 4 for next_q): every gap column of g_q keeps its sentinel"""
    case = R.dqn_cap_case(B, K)
    b, launch, t = dqn_loss_launch(ops, case, K)
    twice(b, launch, ("g_q", "loss", "cur", "tgt"), restore=(t["loss_sum"], t["ws"]))
    check_dqn_loss(t, case, f"dqn loss B={B} K={K}")


@pytest.mark.parametrize("B", SMALL_B)
def test_dqn_loss_guarded(ops, B):
    K = 3
    case = R.dqn_loss_case(B, K, 77 * K + B)
    b, launch, t = dqn_loss_launch(ops, case, K)
    twice(b, launch, ("g_q", "loss", "cur", "tgt"), restore=(t["loss_sum"], t["ws"]))
    check_dqn_loss(t, case, f"dqn guarded loss B={B}")
    for drop in ("loss_sum", "cur", "tgt"):
        bd, launch_d, td = dqn_loss_launch(ops, case, K, drop=(drop,))
        twice(bd, launch_d, tuple(k for k in ("g_q", "loss", "cur", "tgt") if k != drop), restore=(td["loss_sum"], td["ws"]))
        assert all(th.equal(td[k], t[k]) for k in ("g_q", "loss", "cur", "tgt") if k != drop), drop
        assert float(td["loss_sum"]) == (3.0 if drop == "loss_sum" else float(t["loss_sum"]))


# ==== grad_clip, rmsprop, rmsprop_tf ======================================================================================================
CAP_N = (16384, 16385, 32771)  # the sum-of-squares pass: exactly 64 workgroups, the first element of a second pass, a third pass + a float4 tail
TF_FULL = dict(weight_decay=1e-2, centered=True, momentum=0.9)  # rmsprop_tf_kernel<true, true, true>: every arena


def modes(norm, k):
    return {"engaged": 0.25 * float(norm), "not_engaged": 4.0 * float(norm) + 1.0, "off": 0.0 if k else None}


@pytest.mark.parametrize("n", CAP_N)
def test_grad_clip_past_the_cap(ops, n):
    g = np.random.default_rng(n).normal(size=n).astype(np.float32)
    norm = R.device_norm(g)
    units(np.array([norm]), [np.sqrt((g.astype(np.float64) ** 2).sum())], f"grad_clip n={n} chunked norm model vs fp64")
    for mode in ("engaged", "not_engaged"):
        max_norm = modes(norm, 0)[mode]
        b = BitBufs()
        grad, out = b.put("grad", g), b.new("norm", 1)
        ws = b.put("ws", th.zeros(ops.new_ppo_workspace(DEV).shape, dtype=I64), dtype=I64)
        ops.grad_clip(grad, max_norm, ws, out)
        b.check(("norm",))
        coef = R.clip_coef(norm, max_norm)
        assert (coef < 1) == (mode == "engaged")
        assert float(out) == float(norm)  # the bits of the chunked order
        np.testing.assert_array_equal(host(grad), g * coef)


def tf_launch(ops, kw, st, grad, lr_dev, max_norm=None, ws=None, out=None):
    ops.rmsprop_tf(st["param"], grad, st["square_avg"], lr_dev, kw.get("alpha", 0.99), kw.get("eps", 1e-8), kw.get("weight_decay", 0.0),
                   kw.get("momentum", 0.0), st.get("momentum_buffer"), st.get("grad_avg"), max_norm, ws, out)


STATE = ("param", "square_avg", "momentum_buffer", "grad_avg")


@pytest.mark.parametrize("mode", ["engaged", "not_engaged", "off"])
@pytest.mark.parametrize("form", ["rmsprop", "tf_plain", "tf_full"])
@pytest.mark.parametrize("n", CAP_N)
def test_optimiser_steps_past_the_sumsq_cap(ops, n, form, mode):
    """three consecutive steps, bit for bit the NumPy float32 statements with the coefficient from the chunked norm"""
    lr, alpha, eps = 7e-4, 0.99, 1e-5
    kw = dict(eps=eps, **(TF_FULL if form == "tf_full" else {}))
    w, grads = R.rmsprop_case(n, seed=n)
    hs = (w, np.zeros(n, np.float32), None, None) if form == "rmsprop" else (w,) + R.new_state(n, kw)
    b = BitBufs()
    st = {name: b.put(name, a) for name, a in zip(STATE, hs) if a is not None}
    lr_dev = b.put_ro("lr", np.array([lr]), dtype=th.float64)
    ws = b.put("ws", th.zeros(ops.new_ppo_workspace(DEV).shape, dtype=I64), dtype=I64)
    out, grad = b.put("norm", np.array([-1.0], np.float32)), b.put("grad", grads[0])
    for k, g in enumerate(grads):
        norm = R.device_norm(g)
        max_norm = modes(norm, k)[mode]
        coef = F(1.0) if mode == "off" else R.clip_coef(norm, max_norm)
        assert (coef < 1) == (mode == "engaged")
        grad.copy_(dev(g))
        args = (max_norm,) if mode == "off" else (max_norm, ws, out)
        if form == "rmsprop":
            ops.rmsprop(st["param"], grad, st["square_avg"], lr_dev, alpha, eps, *args)
            p, gc, sq = R.rmsprop_numpy(hs[0], g, hs[1], lr, alpha, eps, coef)
            hs = (p, sq, None, None)
        else:
            tf_launch(ops, kw, st, grad, lr_dev, *args)
            p, gc, sq, buf, ga = R.rmsprop_tf_numpy(hs[0], g, *hs[1:], lr, coef=coef, **kw)
            hs = (p, sq, buf, ga)
        b.check()
        assert float(out) == (-1.0 if mode == "off" else float(norm)), (k, float(out), float(norm))
        for name, a in zip(STATE, hs):
            if a is not None:
                np.testing.assert_array_equal(host(st[name]), a, err_msg=f"{name}, step {k}")
        np.testing.assert_array_equal(host(grad), gc, err_msg=f"grad, step {k}")  # written back clipped; untouched when off
    assert not np.array_equal(hs[0], w) and np.isfinite(hs[0]).all()


@pytest.mark.parametrize("form", ["rmsprop", "tf_full"])
def test_optimiser_step_past_the_step_kernels_cap(ops, form):
    """n = 4096 x 512 x 4 + 5: the step kernel's stride loop takes a second pass of one float4, then the scalar tail; clip engaged"""
    n = R.STEP_CAP + 5
    lr, alpha, eps = 7e-4, 0.99, 1e-5
    kw = dict(eps=eps, **TF_FULL)
    rng = np.random.default_rng(5)
    w = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    g = rng.standard_normal(n, dtype=np.float32) * F(0.01)
    g[-6:] = F(0.5)  # the second pass and the tail carry weight of their own
    norm = R.device_norm(g)
    max_norm = 0.25 * float(norm)
    coef = R.clip_coef(norm, max_norm)
    hs = (w, np.zeros(n, np.float32), None, None) if form == "rmsprop" else (w,) + R.new_state(n, kw)
    b = BitBufs()
    st = {name: b.put(name, a) for name, a in zip(STATE, hs) if a is not None}
    grad, out = b.put("grad", g), b.new("norm", 1)
    lr_dev = b.put_ro("lr", np.array([lr]), dtype=th.float64)
    ws = b.put("ws", th.zeros(ops.new_ppo_workspace(DEV).shape, dtype=I64), dtype=I64)
    if form == "rmsprop":
        ops.rmsprop(st["param"], grad, st["square_avg"], lr_dev, alpha, eps, max_norm, ws, out)
        p, gc, sq = R.rmsprop_numpy(w, g, hs[1], lr, alpha, eps, coef)
        hs = (p, sq, None, None)
    else:
        tf_launch(ops, kw, st, grad, lr_dev, max_norm, ws, out)
        p, gc, sq, buf, ga = R.rmsprop_tf_numpy(w, g, *hs[1:], lr, coef=coef, **kw)
        hs = (p, sq, buf, ga)
    b.check(("norm",))
    assert float(out) == float(norm) and coef < 1
    for name, a in zip(STATE, hs):
        if a is not None:
            assert th.equal(st[name], dev(a)), name
    assert th.equal(grad, dev(gc))
    assert not np.array_equal(hs[0][-9:], w[-9:])  # the last float4 and the tail moved


@pytest.mark.parametrize("n", [5, 1030])
def test_clip_and_steps_guarded_with_and_without_norm_out(ops, n):
    w, grads = R.rmsprop_case(n, seed=n)
    g = grads[0]
    max_norm = 0.25 * float(R.device_norm(g))
    results = {}
    for entry in ("grad_clip", "rmsprop", "tf_full"):
        for with_norm in (True, False):
            kw = dict(eps=1e-5, **TF_FULL)
            hs = (w,) + R.new_state(n, kw) if entry == "tf_full" else (w, np.zeros(n, np.float32), None, None)
            b = BitBufs()
            st = {name: b.put(name, a) for name, a in zip(STATE, hs) if a is not None}
            grad, out = b.put("grad", g), b.new("norm", 1)
            lr_dev = b.put_ro("lr", np.array([7e-4]), dtype=th.float64)
            ws = b.put("ws", th.zeros(ops.new_ppo_workspace(DEV).shape, dtype=I64), dtype=I64)
            o = out if with_norm else None
            if entry == "grad_clip":
                launch = lambda: ops.grad_clip(grad, max_norm, ws, o)  # noqa: E731
            elif entry == "rmsprop":
                launch = lambda: ops.rmsprop(st["param"], grad, st["square_avg"], lr_dev, 0.99, 1e-5, max_norm, ws, o)  # noqa: E731
            else:
                launch = lambda: tf_launch(ops, kw, st, grad, lr_dev, max_norm, ws, o)  # noqa: E731
            twice(b, launch, ("norm",) if with_norm else (), restore=[grad, ws] + list(st.values()))
            if entry == "grad_clip":  # the state arenas are bystanders of this launch
                assert all(np.array_equal(host(st[k]), a) for k, a in zip(STATE, hs) if a is not None)
            results[(entry, with_norm)] = {k: v.clone() for k, v in dict(st, grad=grad).items()}
        a, c = results[(entry, True)], results[(entry, False)]
        assert all(th.equal(a[k], c[k]) for k in a), entry  # norm_out left out: the same bits everywhere else


# ==== the lane-per-env launches ===========================================================================================================
def head_launch(ops, n, A, seed, draw=False, drop=(), deterministic=False):
    mean, log_std, eps, low, high = R.head_inputs(n, A, seed)
    b = BitBufs()
    t = dict(mean=b.put_ro("mean", mean), log_std=b.put_ro("log_std", log_std), low=b.put_ro("low", low), high=b.put_ro("high", high),
             action=b.new("action", n, A), env_action=b.new("env_action", n, A), log_prob=b.new("log_prob", n), eps_out=b.new("eps_out", n, A))
    t["eps"] = None if draw or deterministic else b.put_ro("eps", eps)
    t["ctl"] = b.put("ctl", ops.new_rng_ctl(1234, DEV).cpu(), dtype=I64) if draw else None
    opt = {k: (None if k in drop else t[k]) for k in ("env_action", "log_prob", "eps_out")}
    launch = lambda: ops.diag_gaussian_act(t["mean"], t["log_std"], t["eps"], t["ctl"], t["low"], t["high"], deterministic, t["action"],  # noqa: E731
                                           opt["env_action"], opt["log_prob"], opt["eps_out"])
    return b, launch, t, (mean, log_std, eps, low, high)


HEAD_OUT = ("action", "env_action", "log_prob", "eps_out")


def check_head(t, inputs, tag, large=False):
    """large: a quarter of a million rows, where some actions cancel and the bars are relative to the outputs' condition
    (_onpolicy_reference.head_bars); the small shapes keep tests/test_ppo.py's bar(want)"""
    mean, log_std, eps, low, high = inputs
    if large:
        fa, fl = R.head_figures(host(t["action"]), host(t["log_prob"]), mean, log_std, eps, low, high)
        report(tag, {"action": fa, "log_prob": fl})
    else:
        a64, _, lp64 = R.head_f64(mean, log_std, eps, low, high)
        units(t["action"], a64, tag + " action"), units(t["log_prob"], lp64, tag + " log_prob")
    np.testing.assert_array_equal(host(t["env_action"]), np.clip(host(t["action"]), low, high))  # exact on the stored f32 action
    np.testing.assert_array_equal(host(t["eps_out"]), eps)


@pytest.mark.parametrize("A", [2, 4])
def test_head_past_the_lane_cap(ops, A):
    n = R.LANE_CAP + 1
    b, launch, t, inputs = head_launch(ops, n, A, seed=n + A)
    twice(b, launch, HEAD_OUT)
    check_head(t, inputs, f"head n={n} A={A}", large=True)


def test_head_draws_from_philox_past_the_lane_cap(ops):
    """eps_out = the Philox + Box-Muller restatement at counters base + row (the restatement's float32 Box-Muller is not bit-faithful to
    the device's sincospif form, so the bar is the one tests/test_rowkernel_reference.py sets for drawn normals)"""
    n, A = R.LANE_CAP + 1, 2
    b, launch, t, (mean, log_std, _, low, high) = head_launch(ops, n, A, seed=3, draw=True)
    twice(b, launch, HEAD_OUT, restore=(t["ctl"],))
    assert int(t["ctl"][1]) == n and int(t["ctl"][2]) == 0 and int(t["ctl"][0]) == 1234  # offset += rows, the ticket reset itself
    eps = host(t["eps_out"])
    w, ws, share = R.normal_worst(eps, 1234, 0, n * A, R.PPO_STREAM_TAG)
    print(f"BAR head drawn normals n={n}: {w / R.NORMAL_BAR:.3f} (beyond the slack {ws / R.NORMAL_BAR:.3f}, slack share {share:.2g})")
    assert w <= R.NORMAL_BAR and ws <= R.NORMAL_BAR and share <= 1e-3
    check_head(t, (mean, log_std, eps, low, high), f"head drawn n={n}", large=True)  # the action and log-prob of the stored draw
    launch()  # the second call on the advanced stream: the next n counters
    th.cuda.synchronize()
    assert int(t["ctl"][1]) == 2 * n
    w2, ws2, _ = R.normal_worst(host(t["eps_out"]), 1234, n, n * A, R.PPO_STREAM_TAG)
    assert w2 <= R.NORMAL_BAR and ws2 <= R.NORMAL_BAR


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("n", SMALL_N)
def test_head_guarded(ops, n, A):
    b, launch, t, inputs = head_launch(ops, n, A, seed=n + A)
    twice(b, launch, HEAD_OUT)
    check_head(t, inputs, f"head guarded n={n} A={A}")
    for drop in ("env_action", "log_prob", "eps_out"):
        bd, launch_d, td, _ = head_launch(ops, n, A, seed=n + A, drop=(drop,))
        twice(bd, launch_d, tuple(k for k in HEAD_OUT if k != drop))
        assert all(th.equal(td[k], t[k]) for k in HEAD_OUT if k != drop), drop
    bw, launch_w, tw, _ = head_launch(ops, n, A, seed=n + A, draw=True)
    twice(bw, launch_w, HEAD_OUT, restore=(tw["ctl"],))
    assert int(tw["ctl"][1]) == n and int(tw["ctl"][2]) == 0
    bm, launch_m, tm, (mean, *_) = head_launch(ops, n, A, seed=n + A, deterministic=True)
    twice(bm, launch_m, HEAD_OUT)
    np.testing.assert_array_equal(host(tm["action"]), mean)
    assert float(tm["eps_out"].abs().max()) == 0.0


def dqn_act_case(n, K, seed):
    """test_dqn.py's act_case without its per-row Python loop: every third row has its maximum twice (the first one wins)"""
    rng = np.random.default_rng(seed)
    M = K * K
    q = rng.normal(size=(n, M)).astype(np.float32)
    rows = np.arange(0, n, 3)
    c1 = rng.integers(0, M, rows.size)
    c2 = (c1 + rng.integers(1, M, rows.size)) % M
    top = q[rows].max(1) + F(1)
    q[rows, c1], q[rows, c2] = top, top
    eps = 0.375
    u = rng.uniform(size=(n, 2)).astype(np.float32)
    u[::4, 0] = F(eps)                              # exactly at the rate: greedy
    u[1::4, 0] = np.nextafter(F(eps), F(0))         # just below: explores
    u[::5, 1] = np.nextafter(F(1), F(0))            # just below 1: the last index, never M
    u[2::7, 1] = 0.0
    return q, u, eps


def dqn_act_launch(ops, q, u, eps, K, mode, flag=0, draw=False, drop=()):
    n, M = q.shape
    b = BitBufs()
    t = dict(q=b.put_ro_cols("q", q, M + 3, 0), valve=b.new("valve", n, 2), index=b.new("index", n, dtype=I64))
    kw = {}
    if mode == 1:
        kw["flag"] = b.put_ro("flag", np.array([flag]), dtype=th.int32)
    if mode == 2:
        kw["eps"] = b.put_ro("eps", np.array([eps]), dtype=th.float64)
    if mode and draw:
        kw["rng_ctl"] = t["ctl"] = b.put("ctl", ops.new_rng_ctl(99, DEV).cpu(), dtype=I64)
    elif mode:
        kw["u"] = b.put_ro("u", u)
    launch = lambda: ops.dqn_act(t["q"], K, mode, t["valve"], None if "index" in drop else t["index"], **kw)  # noqa: E731
    return b, launch, t


def check_dqn_act(t, want, K):
    index = host(t["index"])
    assert np.array_equal(index, want) and host(t["valve"]).tobytes() == R.pair_np(index, K).tobytes()


def dqn_act_all_modes(ops, n, K, drops):
    q, u, eps = dqn_act_case(n, K, 1000 * K + n)
    for mode, flag in ((0, 0), (1, 0), (1, 1), (2, 0)):
        b, launch, t = dqn_act_launch(ops, q, u, eps, K, mode, flag)
        twice(b, launch, ("valve", "index"))
        check_dqn_act(t, R.act_np(q, K, mode, eps=eps, flag=flag, u=u), K)
        for drop in drops:
            bd, launch_d, td = dqn_act_launch(ops, q, u, eps, K, mode, flag, drop=(drop,))
            twice(bd, launch_d, ("valve",))
            assert th.equal(td["valve"], t["valve"])
    b, launch, t = dqn_act_launch(ops, q, u, eps, K, 2, draw=True)  # uniforms from the Philox stream
    twice(b, launch, ("valve", "index"), restore=(t["ctl"],))
    assert int(t["ctl"][1]) == n and int(t["ctl"][2]) == 0
    check_dqn_act(t, R.act_np(q, K, 2, eps=eps, u=R.dqn_uniforms(99, 0, n)), K)


def test_dqn_act_past_the_lane_cap(ops):
    dqn_act_all_modes(ops, R.LANE_CAP + 1, 3, drops=())


@pytest.mark.parametrize("n", SMALL_N)
def test_dqn_act_guarded(ops, n):
    dqn_act_all_modes(ops, n, 5, drops=("index",))


# ---- the rollout buffer: add, GAE, gather -------------------------------------------------------------------------------------------------
FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def guarded_rollout(ops, b, T, N, D, A, goal, rng, read_only=False):
    """a DeviceRollout whose eight field arrays and control words live in GuardedBufs, filled with known values"""
    from core import _native as nv

    rb = ops.DeviceRollout(T, N, D, A, DEV, goal=goal)
    hostv = {}
    for f in FIELDS:
        shape = tuple(getattr(rb, f).shape)
        hostv[f] = rng.normal(size=shape).astype(np.float32)
        setattr(rb, f, (b.put_ro if read_only else b.put)("rb_" + f, hostv[f]))
    rb.ctl = b.put("rb_ctl", np.zeros(rb.ctl.numel(), np.int64), dtype=I64)
    rb.c = nv.Rollout(*(getattr(rb, f).data_ptr() for f in FIELDS), T, N, D, A)
    return rb, hostv


def add_launch(ops, T, N, D, A, goal, pos, seed):
    rng = np.random.default_rng(seed)
    b = BitBufs()
    rb, before = guarded_rollout(ops, b, T, N, D, A, goal, rng)
    rb.ctl[0] = pos
    done = (rng.uniform(size=N) < 0.5).astype(np.float32)
    h = dict(obs=rng.normal(size=(N, D)), act=rng.normal(size=(N, A)), rew=rng.normal(size=N), val=rng.normal(size=N), logp=rng.normal(size=N),
             tv=rng.normal(size=N), start=(rng.uniform(size=N) < 0.3), done=done, timeout=(rng.uniform(size=N) < 0.5) & (done > 0))
    h = {k: np.asarray(v, np.float32) for k, v in h.items()}
    t = {k: b.put_ro(k, v) for k, v in h.items() if k != "start"}
    t["start"] = b.put("start", h["start"])
    t["ep_ret"], t["ep_len"] = b.put("ep_ret", np.ones(N, np.float32)), b.put("ep_len", np.full(N, 3), dtype=th.int32)
    t["stats"] = b.put("stats", np.zeros(4), dtype=th.float64)
    add = ops.goal_rollout_add if goal else ops.rollout_add
    launch = lambda: add(rb, t["obs"], t["act"], t["rew"], t["start"], t["val"], t["logp"], t["timeout"], t["tv"], 0.99, t["done"],  # noqa: E731
                         t["ep_ret"], t["ep_len"], t["stats"])
    inplace = [rb.ctl, t["start"], t["ep_ret"], t["ep_len"], t["stats"]] + [getattr(rb, f) for f in FIELDS]
    return b, launch, rb, t, h, before, inplace


def check_add(rb, t, h, before, pos, T):
    boot = np.where(h["timeout"] != 0, h["rew"] + F(0.99) * h["tv"], h["rew"]).astype(np.float32)
    want = dict(observations=h["obs"], actions=h["act"], rewards=boot, episode_starts=h["start"], values=h["val"], log_probs=h["logp"],
                advantages=np.zeros_like(h["rew"]), returns=np.zeros_like(h["rew"]))
    for f in FIELDS:
        got = host(getattr(rb, f))
        np.testing.assert_array_equal(got[pos], want[f], err_msg=f)
        rest = np.arange(T) != pos
        np.testing.assert_array_equal(got[rest], before[f][rest], err_msg=f + ": a row other than the position was written")
    np.testing.assert_array_equal(host(t["start"]), h["done"])  # episode_start <- done for the next step
    assert host(rb.ctl).tolist() == [pos + 1, int(pos + 1 == T), 0, 1]
    d = h["done"] > 0
    stats = host(t["stats"])
    assert stats[0] == d.sum() and stats[2] == 4 * d.sum() and abs(stats[1] - (1.0 + h["rew"].astype(np.float64))[d].sum()) < 1e-4
    np.testing.assert_array_equal(host(t["ep_len"]), np.where(d, 0, 4))


@pytest.mark.parametrize("D,A", [(4, 2), (8, 4)])
def test_rollout_add_past_the_lane_cap(ops, D, A):
    N = R.LANE_CAP + 1
    b, launch, rb, t, h, before, inplace = add_launch(ops, 1, N, D, A, False, 0, seed=D)
    twice(b, launch, (), restore=inplace, skip=("stats",))  # the return sum is an f64 atomicAdd: not order-deterministic
    check_add(rb, t, h, before, 0, 1)


@pytest.mark.parametrize("D,A,goal", [(4, 2, False), (8, 4, False), (4, 1, False), (6, 2, True)])  # the goal face's row: three float2
@pytest.mark.parametrize("N", SMALL_N)
def test_rollout_add_guarded(ops, N, D, A, goal):
    T = 3
    for pos in (0, 1, 2):
        b, launch, rb, t, h, before, inplace = add_launch(ops, T, N, D, A, goal, pos, seed=10 * N + D + pos)
        twice(b, launch, (), restore=inplace, skip=("stats",))
        check_add(rb, t, h, before, pos, T)
    for pos in (T, -1):  # a full buffer and a broken position: every ring byte, ctl and the env-side words stay as they are
        b, launch, rb, t, h, before, _ = add_launch(ops, T, N, D, A, goal, pos, seed=N + D)
        snap = b.snapshot()
        launch()
        b.check()
        b.same_as(snap)
        assert host(rb.ctl).tolist() == [pos, 0, 0, 0]


def gae_launch(ops, T, N, seed):
    rng = np.random.default_rng(seed)
    b = BitBufs()
    rb, h = guarded_rollout(ops, b, T, N, 4, 2, False, rng)
    starts = (rng.uniform(size=(T, N)) < 0.25).astype(np.float32)
    starts[0, :], starts[T - 1, ::2] = 1.0, 1.0
    rb.episode_starts.copy_(dev(starts))
    h["episode_starts"] = starts
    for f in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs"):
        b.freeze("rb_" + f)
    b.freeze("rb_ctl")
    last, dones = rng.normal(-20, 10, N).astype(np.float32), (rng.uniform(size=N) < 0.5).astype(np.float32)
    lv, dn = b.put_ro("last_values", last), b.put_ro("dones", dones)
    rb.advantages.fill_(12345.678), rb.returns.fill_(12345.678)  # the sentinel: every cell must be written
    launch = lambda: ops.gae(rb, lv, dn, 0.99, 0.95)  # noqa: E731
    want = R.gae_numpy(h["rewards"], h["values"], starts, last, dones, 0.99, 0.95)
    return b, launch, rb, want


@pytest.mark.parametrize("T,N", [(2, R.LANE_CAP + 1), (2048, 3)] + [(3, n) for n in SMALL_N])  # past the cap, PPO's default n_steps, one wave's edges
def test_gae_guarded_and_past_the_lane_cap(ops, T, N):
    b, launch, rb, (adv, ret) = gae_launch(ops, T, N, seed=100 * T + N)
    twice(b, launch, ("rb_advantages", "rb_returns"))
    np.testing.assert_array_equal(host(rb.advantages), adv)
    np.testing.assert_array_equal(host(rb.returns), ret)


def gather_launch(ops, T, N, D, A, goal, idx, seed):
    rng = np.random.default_rng(seed)
    b = BitBufs()
    rb, h = guarded_rollout(ops, b, T, N, D, A, goal, rng, read_only=True)
    b.freeze("rb_ctl")
    B = len(idx)
    out = (b.new("obs", B, D), b.new("act", B, A), b.new("old_value", B), b.new("old_log_prob", B), b.new("adv", B), b.new("ret", B))
    di = b.put_ro("idx", idx, dtype=I64)
    gather = ops.goal_ppo_gather if goal else ops.ppo_gather
    launch = lambda: gather(rb, di, *out)  # noqa: E731
    flat = {f: h[f].swapaxes(0, 1).reshape(T * N, -1) for f in FIELDS}
    return b, launch, out, flat


GATHER_OUT = ("obs", "act", "old_value", "old_log_prob", "adv", "ret")
GATHER_FIELDS = ("observations", "actions", "values", "log_probs", "advantages", "returns")


def check_gather(out, flat, idx, total):
    rows = np.clip(idx, 0, total - 1)  # out-of-range indices are the caller's bug: clamped, never a fault
    for t, f in zip(out, GATHER_FIELDS):
        np.testing.assert_array_equal(host(t).reshape(len(idx), -1), flat[f][rows], err_msg=f)


def test_gather_past_its_lane_cap(ops):
    """B = 2048 x 256 + 1 from a 5 x 7 buffer: every index many times over. The last pass holds ONE row, so the two out-of-range indices
    sit on it in two launches (-5, then T N + 9); the last row of the first pass carries one as well"""
    T, N = 5, 7
    B = R.GATHER_CAP + 1
    idx = np.random.default_rng(B).integers(0, T * N, B)
    idx[-1], idx[-2] = -5, T * N + 9
    b, launch, out, flat = gather_launch(ops, T, N, 4, 2, False, idx, seed=1)
    twice(b, launch, GATHER_OUT)
    check_gather(out, flat, idx, T * N)
    idx[-1], idx[-2] = T * N + 9, -5
    b, launch, out, flat = gather_launch(ops, T, N, 4, 2, False, idx, seed=1)
    launch()
    b.check(GATHER_OUT)
    check_gather(out, flat, idx, T * N)


@pytest.mark.parametrize("D,A,goal", [(4, 2, False), (8, 4, False), (6, 2, True)])
@pytest.mark.parametrize("B", SMALL_B)
def test_gather_guarded(ops, B, D, A, goal):
    T, N = 5, 7
    idx = np.random.default_rng(B + D).integers(0, T * N, B)
    idx[0] = T * N - 1
    if B > 2:
        idx[1], idx[2] = -3, T * N
    b, launch, out, flat = gather_launch(ops, T, N, D, A, goal, idx, seed=B)
    twice(b, launch, GATHER_OUT)
    check_gather(out, flat, idx, T * N)
