"""What the kernel-level tests of the on-policy family share (csrc/cstr_ppo.hip, csrc/cstr_a2c.hip, csrc/cstr_dqn.hip and the core in
csrc/cstr_onpolicy_device.h): tests/test_onpolicy_reference.py on the CPU, tests/test_onpolicy_guards.py on the GPU.

The fp64 statements, the NumPy float32 statements of the optimiser steps and of GAE, the chunked norm and the Philox restatement are
IMPORTED from where they live (tests/test_ppo.py, test_a2c.py, test_a2c_abi.py, test_ppo_abi.py, test_rmsprop_tf_abi.py,
_dqn_helpers.py, _rowkernel_reference.py). Added here:

  loss_reference  the fp64 autograd statement of a loss launch plus the absolute terms behind its cancelling sums (policy_loss, loss,
                  d/d log_std), restated in fp64 NumPy from the statement's own log-probs and ratios and tied back to its results
  loss_figures    the comparator: every output of a loss launch in units of its bar
  loss_model_f32  a float32 NumPy model of diag_gaussian_loss_kernel's arithmetic and of its reduction (grid min(ceil(B / 256), 64),
                  grid-stride rows, f64 per-thread sums, the halving tree, the partials in workgroup order), with the mistakes of
                  MISTAKES on request. It is a model, not a reference: it shows that a correct float32 kernel has room under the
                  bars and that a wrong one has not.

THE BARS, with bar(x) = 2e-6 |x| + 1e-7 (the project's):
  log_prob_out, value_loss, entropy_loss, approx_kl   bar(want)
  policy_loss, loss                                  2e-6 * (sum of |term|) / B + 1e-7: sums of f32 terms of either sign, so the bar
                                                     is relative to the sum's condition. One row dropped or doubled moves them by
                                                     1 / B = 6e-5 of a term at the grid cap, 30 bars.
  d/d log_std                                        2e-6 * (sum of |term|) + 1e-7, the same reasoning on a sum instead of a mean
  A2C g_mean, g_value of both                        bar(B * want) on B * g: at the raw 1 / B scale the 1e-7 floor would be 1e-3 of
                                                     the value at 16384 rows and would hide a wrong row
  PPO g_mean                                         (2e-6 + bar(logp_b)) |B * want| + 1e-7 on B * g: the row's log-prob error goes
                                                     through exp into the ratio, so the gradient's relative error is the log-prob's
                                                     ABSOLUTE error; under the plain bar a correct float32 evaluation reaches 1.9
  clip_fraction                                      exact (no ratio of the cases lies within 1e-3 of a clip bound)
  dqn loss                                           bar(want): a mean of non-negative f32 Huber terms summed in f64; loss_case's
                                                     rows have no cancellation (|cur| and |target| add), so a term carries the 2 ulp
                                                     of its target twice through the square: <= 5e-7 relative, a quarter of the bar
"""
import numpy as np

from _dqn_helpers import act_np, dqn_uniforms, loss_f32 as dqn_loss_f32, loss_f64 as dqn_loss_f64, pair_np, ulps  # noqa: F401
from _rowkernel_reference import NORMAL_BAR, normal_stream, normal_worst  # noqa: F401  (the Philox + Box-Muller restatement)
from test_a2c import a2c_loss_f64, clip_coef, device_norm, rmsprop_case  # noqa: F401
from test_a2c import loss_case as a2c_loss_case
from test_a2c_abi import rmsprop_numpy  # noqa: F401
from test_dqn import loss_case as dqn_loss_case  # noqa: F401
from test_ppo import head_f64, ppo_loss_f64  # noqa: F401
from test_ppo import loss_case as ppo_loss_case
from test_ppo_abi import gae_numpy  # noqa: F401
from test_rmsprop_tf_abi import new_state, rmsprop_tf_numpy  # noqa: F401

F = np.float32
RTOL, ATOL = 2e-6, 1e-7
PPO_STREAM_TAG = 0x990A11C7  # csrc/cstr_ppo.hip
MAX_BLOCKS, BLOCK = 64, 256  # CSTR_PPO_MAX_BLOCKS workgroups of 256 rows: the cap of the loss launches and of the sum-of-squares pass
LANE_CAP = 4096 * 64         # lanes of the lane-per-env launches (act, add, GAE, dqn_act)
GATHER_CAP = 2048 * 256      # lanes of the minibatch gather
STEP_CAP = 4096 * 512 * 4    # floats one pass of the RMSprop step kernels covers
# (B, A): one row short of the cap, the cap, the first row of the second pass, A2C's default 4096 x 5, the first row of a third pass
CAP_SIZES = ((16383, 2), (16384, 4), (16385, 2), (20480, 2), (20480, 4), (32769, 4))
PPO_VARIANTS = tuple((vf, norm) for vf in (None, 0.2) for norm in (True, False))  # (clip_range_vf, normalize_advantage)
CLIP_RANGE, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5
LOG_SQRT_2PI = F(0.918938533204672742)
HALF_LOG_2PI_E = F(1.418938533204672742)
MISTAKES = ("skip_second_pass", "63_partials", "row_twice", "inv_b_grid", "vclip_open")


def bar(x):
    return RTOL * np.abs(np.asarray(x, np.float64)) + ATOL


def loss_inputs(ppo, B, A):
    """the existing generators at the seed every cap case uses"""
    return (ppo_loss_case if ppo else a2c_loss_case)(B, A, seed=17 * B + A)


def unpack(case, ppo):
    if ppo:
        return case
    mean, log_std, actions, values, adv, returns = case
    return mean, log_std, actions, values, None, None, adv, returns


# ---- the fp64 statement and the terms behind its sums ------------------------------------------------------------------------------------
def loss_reference(case, ppo, clip_range_vf=None, normalize=True, clip_range=CLIP_RANGE, ent_coef=ENT_COEF, vf_coef=VF_COEF):
    """dict(scalars, g_mean, g_value, g_log_std, log_prob, ratio, policy_abs, loss_abs, log_std_abs): the fp64 autograd statement of
    tests/test_ppo.py / tests/test_a2c.py, and sum |term| behind policy_loss (already / B), loss and d/d log_std [A]. The terms are
    restated here from the statement's log-probs; their signed sums must give the statement's own results back (asserted)."""
    mean, log_std, actions, values, old_values, old_logp, adv, returns = unpack(case, ppo)
    if ppo:
        scal, gm, gv, gl, lp, ratio = ppo_loss_f64(*case, clip_range, clip_range_vf, normalize, ent_coef, vf_coef)
    else:
        scal, gm, gv, gl, lp = a2c_loss_f64(*case, normalize, ent_coef, vf_coef)
        ratio = None
    B = actions.shape[0]
    a = adv.astype(np.float64)
    with np.errstate(all="ignore"):
        if normalize and (B > 1 or not ppo):
            a = (a - a.mean()) / (a.std(ddof=1) + 1e-8)
        if ppo:
            pl1, pl2 = a * ratio, a * np.clip(ratio, 1 - clip_range, 1 + clip_range)
            term = np.minimum(pl1, pl2)
            inside = (ratio >= 1 - clip_range) & (ratio <= 1 + clip_range)
            g_logp = -np.where(inside | (pl1 < pl2), a, 0.0) * ratio / B
        else:
            term = a * lp
            g_logp = -a / B
        d = actions.astype(np.float64) - mean.astype(np.float64)
        ls_terms = g_logp[:, None] * (d * d / np.exp(2.0 * log_std.astype(np.float64)) - 1.0)
    ref = dict(scalars=np.asarray(scal, np.float64), g_mean=gm, g_value=gv, g_log_std=gl, log_prob=lp, ratio=ratio, B=B, ppo=ppo)
    ref["policy_abs"] = np.nansum(np.abs(term)) / B  # a NaN term: the sum is NaN and is compared as a NaN, not against this bar
    ref["loss_abs"] = ref["policy_abs"] + ent_coef * abs(scal[2]) + vf_coef * np.nan_to_num(abs(scal[1]))
    ref["log_std_abs"] = np.nansum(np.abs(ls_terms), 0) + ent_coef
    if np.isfinite(term).all() and np.isfinite(ls_terms).all():  # the tie (the NaN cases of the GPU module have no finite sums)
        assert abs(-term.mean() - scal[0]) <= 1e-12 * max(ref["policy_abs"], 1.0), (-term.mean(), scal[0])
        assert np.all(np.abs(ls_terms.sum(0) - ent_coef - gl) <= 1e-12 * np.maximum(ref["log_std_abs"], 1.0)), (ls_terms.sum(0) - ent_coef, gl)
    return ref


def loss_figures(got, ref):
    """{output: worst |got - want| / bar}. got: dict(scalars [6 | 4], g_mean [B, A], g_value [B], g_log_std [A], log_prob [B]) of
    NumPy arrays of any float type."""
    g = {k: np.asarray(v, np.float64) for k, v in got.items()}
    B, scal = ref["B"], ref["scalars"]
    fig = {}
    fig["log_prob"] = float((np.abs(g["log_prob"] - ref["log_prob"]) / bar(ref["log_prob"])).max())
    fig["value_loss"] = float(abs(g["scalars"][1] - scal[1]) / bar(scal[1]))
    fig["entropy_loss"] = float(abs(g["scalars"][2] - scal[2]) / bar(scal[2]))
    fig["policy_loss"] = float(abs(g["scalars"][0] - scal[0]) / (RTOL * ref["policy_abs"] + ATOL))
    fig["loss"] = float(abs(g["scalars"][3] - scal[3]) / (RTOL * ref["loss_abs"] + ATOL))
    fig["g_log_std"] = float((np.abs(g["g_log_std"] - ref["g_log_std"]) / (RTOL * ref["log_std_abs"] + ATOL)).max())
    fig["g_value"] = float((np.abs(B * g["g_value"] - B * ref["g_value"]) / bar(B * ref["g_value"])).max())
    want_gm = B * ref["g_mean"]
    if ref["ppo"]:
        fig["approx_kl"] = float(abs(g["scalars"][4] - scal[4]) / bar(scal[4]))
        fig["clip_fraction"] = 0.0 if F(g["scalars"][5]) == F(scal[5]) else float("inf")
        gm_bar = (RTOL + bar(ref["log_prob"]))[:, None] * np.abs(want_gm) + ATOL
    else:
        gm_bar = bar(want_gm)
    fig["g_mean"] = float((np.abs(B * g["g_mean"] - want_gm) / gm_bar).max())
    return fig


OUTPUTS = ("scalars", "g_mean", "g_value", "g_log_std", "log_prob")


def nan_figures(got, ref):
    """loss_figures where the statement has NaNs: every output must be NaN exactly where the statement's is (asserted, element by
    element); what the statement leaves finite is held to its bar"""
    g, r = {k: np.array(got[k], np.float64) for k in OUTPUTS}, dict(ref)
    for k in OUTPUTS:
        want = np.array(ref[k], np.float64)
        assert np.array_equal(np.isnan(g[k]), np.isnan(want)), (k, "NaN at", np.argwhere(np.isnan(g[k])).tolist(), "want", np.argwhere(np.isnan(want)).tolist())
        g[k], r[k] = np.nan_to_num(g[k], nan=0.0), np.nan_to_num(want, nan=0.0)
    return loss_figures(g, r)


# ---- the float32 model of the loss launch ------------------------------------------------------------------------------------------------
def _tree(acc):
    """block_sum_f64: the halving tree over the last axis (256 wide); the sum lands in element 0"""
    acc = acc.copy()
    o = acc.shape[-1] // 2
    while o > 0:
        acc[..., :o] = acc[..., :o] + acc[..., o:2 * o]
        o >>= 1
    return acc[..., 0]


def _batch_sum(terms, grid, mistake=None, twice=None):
    """reduce_partials over f32 terms [B] widened to f64: thread t of workgroup w adds rows w * 256 + t + pass * grid * 256 in pass
    order, the tree per workgroup, the partials in workgroup order"""
    B, stride = terms.shape[0], grid * BLOCK
    sq = np.zeros(-(-B // stride) * stride, np.float64)
    sq[:B] = terms
    chunks = sq.reshape(-1, grid, BLOCK)
    if mistake == "skip_second_pass":
        chunks = chunks[:1]
    acc = np.zeros((grid, BLOCK), np.float64)
    for chunk in chunks:
        acc = acc + chunk
    if mistake == "row_twice":
        acc[(twice // BLOCK) % grid, twice % BLOCK] += np.float64(terms[twice])
    part = _tree(acc)
    s = 0.0
    for w in range(min(grid, 63) if mistake == "63_partials" else grid):
        s = s + part[w]
    return s


def _advantage_stats(adv):
    """advantage_stats: one workgroup's 256 threads stride over the whole batch, twice"""
    B = adv.shape[0]

    def total(x):
        pad = np.zeros(-(-B // BLOCK) * BLOCK, np.float64)
        pad[:B] = x
        acc = np.zeros(BLOCK, np.float64)
        for chunk in pad.reshape(-1, BLOCK):
            acc = acc + chunk
        return _tree(acc)

    with np.errstate(all="ignore"):
        a_mean = F(total(adv) / np.float64(B))
        d = adv - a_mean
        a_den = F(np.sqrt(total(d * d) / np.float64(B - 1))) + F(1e-8)
    return a_mean, a_den


def loss_model_f32(case, ppo, clip_range_vf=None, normalize=True, clip_range=CLIP_RANGE, ent_coef=ENT_COEF, vf_coef=VF_COEF, sig_ulp=0,
                   mistake=None):
    """diag_gaussian_loss_kernel<A, ppo> in float32 NumPy, operation by operation; sig_ulp moves exp(log_std) by that many ulp (NumPy's
    exp and the device's expf may differ in the last place). -> dict(scalars, g_mean, g_value, g_log_std, log_prob), all float32"""
    mean, log_std, actions, values, old_values, old_logp, adv, returns = unpack(case, ppo)
    assert all(x is None or x.dtype == np.float32 for x in (mean, log_std, actions, values, old_values, old_logp, adv, returns))
    B, A = actions.shape
    grid = min(-(-B // BLOCK), MAX_BLOCKS)
    one, two = F(1), F(2)
    a_mean, a_den = F(0), F(1)
    norm = normalize and (not ppo or B > 1)
    if norm:
        a_mean, a_den = _advantage_stats(adv)
    sig = np.exp(log_std)
    for _ in range(abs(sig_ulp)):
        sig = np.nextafter(sig, F(np.inf if sig_ulp > 0 else -np.inf))
    var = sig * sig
    lo, hi, cr = F(1.0 - clip_range), F(1.0 + clip_range), F(clip_range)
    vclip = ppo and clip_range_vf is not None and clip_range_vf > 0
    inv_b = one / F(grid * BLOCK if mistake == "inv_b_grid" else B)
    ent_coef, vf_coef = F(ent_coef), F(vf_coef)
    sums = lambda t: _batch_sum(t, grid, mistake, twice=B // 2)  # noqa: E731
    with np.errstate(all="ignore"):
        d = actions - mean
        logp = np.zeros(B, np.float32)
        for k in range(A):
            logp = logp + ((-(d[:, k] * d[:, k]) / (two * (sig[k] * sig[k])) - np.log(sig[k])) - LOG_SQRT_2PI)
        advn = (adv - a_mean) / a_den if norm else adv
        tot = {}
        if ppo:
            lr = logp - old_logp
            ratio = np.exp(lr)
            pl1, pl2 = advn * ratio, advn * np.minimum(np.maximum(ratio, lo), hi)
            tot["policy"] = sums(np.minimum(pl1, pl2))
            tot["kl"] = sums((ratio - one) - lr)
            tot["clipped"] = sums((np.abs(ratio - one) > cr).astype(np.float32))
            dmin = np.where(((ratio >= lo) & (ratio <= hi)) | (pl1 < pl2), advn, F(0))
            g_logp = -(inv_b * dmin) * ratio
        else:
            tot["policy"] = sums(advn * logp)
            g_logp = -(inv_b * advn)
        g_mean = np.stack([g_logp * (d[:, k] / var[k]) for k in range(A)], 1)
        ls = [sums(g_logp * ((d[:, k] * d[:, k]) / var[k] - one)) for k in range(A)]
        vp, passes = values, np.ones(B, bool)
        if vclip:
            cv = F(clip_range_vf)
            dv = values - old_values
            vp = old_values + np.minimum(np.maximum(dv, -cv), cv)
            passes = ((dv > -cv) & (dv < cv)) if mistake == "vclip_open" else ((dv >= -cv) & (dv <= cv))
        dr = returns - vp
        tot["value"] = sums(dr * dr)
        g_value = np.where(passes, vf_coef * ((two * inv_b) * (vp - returns)), F(0))
        ent = F(0)
        for k in range(A):
            ent = ent + (HALF_LOG_2PI_E + np.log(sig[k]))
        out = np.zeros(6 if ppo else 4, np.float32)
        out[0] = -F(tot["policy"] / np.float64(B))
        out[1] = F(tot["value"] / np.float64(B))
        out[2] = -ent
        out[3] = (out[0] + ent_coef * out[2]) + vf_coef * out[1]
        if ppo:
            out[4], out[5] = F(tot["kl"] / np.float64(B)), F(tot["clipped"] / np.float64(B))
        g_log_std = np.array([F(s) - ent_coef for s in ls], np.float32)
    for x in (logp, g_mean, g_value, g_log_std):
        assert x.dtype == np.float32
    return dict(scalars=out, g_mean=g_mean, g_value=g_value, g_log_std=g_log_std, log_prob=logp)


# ---- the rollout head at a quarter of a million rows -------------------------------------------------------------------------------------
def head_inputs(n, A, seed):
    """tests/test_ppo.py::test_head_with_given_eps's inputs"""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1.2, 1.2, (n, A)).astype(np.float32)
    log_std = rng.uniform(-1.5, 0.3, A).astype(np.float32)
    eps = rng.normal(size=(n, A)).astype(np.float32)
    return mean, log_std, eps, -np.ones(A, np.float32), np.ones(A, np.float32)


def head_bars(mean, log_std, eps):
    """(bar of the action [n, A], bar of the log-prob [n]) against head_f64: the project's 2e-6 / 1e-7, relative to each output's
    CONDITION instead of its value. tests/test_ppo.py holds 130 rows to bar(want); among a million elements some actions cancel
    (mean = -sigma eps to three digits) and some log-probs are taken at a d = action - mean that is small beside its operands, and
    there a correct float32 evaluation passes bar(want): the NumPy model below reaches 2.1 (action) and 4.1 (log-prob) of it on the
    inputs of tests/test_onpolicy_guards.py, and 0.12 / 0.06 of these bars, which a sigma off by 1e-5 still misses by a factor 2.6. With u = 2**-24:
      action = mean + sigma eps: sigma carries expf's 2 u, the product and the sum one rounding each: <= 3 u |sigma eps| + u |action|,
               so the bar is 2e-6 (|mean| + |sigma eps|) + 1e-7 (33 u against 4 u);
      log_prob = sum_k -(d_k^2) / (2 var_k) - log sigma_k - c with d_k = f32(action_k) - mean_k: the stored action is off by up to
               u |action_k|, so the quadratic term moves by u (|action_k| + |mean_k|) |d_k| / var_k on top of its own size; the bar is
               2e-6 * sum_k [(|action_k| + |mean_k|) |d_k| / var_k + d_k^2 / (2 var_k) + |log sigma_k| + c] + 1e-7."""
    mean, eps, ls = mean.astype(np.float64), eps.astype(np.float64), log_std.astype(np.float64)
    sig = np.exp(ls)
    d = sig * eps
    act = mean + d
    a_bar = RTOL * (np.abs(mean) + np.abs(d)) + ATOL
    cond = (np.abs(act) + np.abs(mean)) * np.abs(d) / sig ** 2 + d * d / (2 * sig ** 2) + np.abs(ls) + float(LOG_SQRT_2PI)
    return a_bar, RTOL * cond.sum(1) + ATOL


def head_model_f32(mean, log_std, eps, sig_ulp=0):
    """diag_gaussian_act_kernel's action and log-prob in float32 NumPy"""
    sig = np.exp(log_std)
    for _ in range(abs(sig_ulp)):
        sig = np.nextafter(sig, F(np.inf if sig_ulp > 0 else -np.inf))
    act = mean + sig * eps
    lp = np.zeros(mean.shape[0], np.float32)
    for k in range(mean.shape[1]):
        d = act[:, k] - mean[:, k]
        lp = lp + ((-(d * d) / (F(2) * (sig[k] * sig[k])) - np.log(sig[k])) - LOG_SQRT_2PI)
    assert act.dtype == lp.dtype == np.float32
    return act, lp


def head_figures(action, log_prob, mean, log_std, eps, low, high):
    """(worst action error, worst log-prob error) in units of head_bars, against tests/test_ppo.py::head_f64"""
    a64, _, lp64 = head_f64(mean, log_std, eps, low, high)
    a_bar, lp_bar = head_bars(mean, log_std, eps)
    return (float((np.abs(np.asarray(action, np.float64) - a64) / a_bar).max()),
            float((np.abs(np.asarray(log_prob, np.float64) - lp64) / lp_bar).max()))


def on_the_value_clip_bound(case, cv=0.25):
    """a PPO case whose value steps include exactly +cv and -cv (old_values = -20, values = -19.75 / -20.25): the closed interval's ends"""
    mean, log_std, actions, values, old_values, old_logp, adv, returns = case
    values, old_values = values.copy(), old_values.copy()
    old_values[:8], values[:8:2], values[1:8:2] = -20.0, F(-20.0 + cv), F(-20.0 - cv)
    return mean, log_std, actions, values, old_values, old_logp, adv, returns


def device_norm_first_chunk(g):
    """device_norm with the stride loop's second and later passes dropped"""
    n = g.size
    return device_norm(g[:min(n, min(-(-n // BLOCK), MAX_BLOCKS) * BLOCK)])


def dqn_cap_case(B, K):
    """test_dqn.py's loss_case with a heavy last row (reward 40 on a terminal step: target 40 against a taken Q <= 0, still no
    cancellation). The last row is the first of a new pass at 16385 and 32769; its Huber term is some 15 times the mean, so the mean
    moves by 4e-4 relative without it, where a row with an average term could hide below the bar."""
    q, nq, index, rew, done = dqn_loss_case(B, K, 77 * K + B)
    rew[-1], done[-1] = 40.0, 1.0
    return q, nq, index, rew, done


def dqn_loss_model_f32(q, nq, index, rew, done, gamma):
    """dqn_loss_kernel's scalar: the f32 Huber terms of _dqn_helpers.loss_f32's d, summed in f64 (the order cannot matter at this bar)"""
    cur, target, _ = dqn_loss_f32(q, nq, index, rew, done, gamma)
    d = cur - target
    z = np.abs(d)
    per = np.where(z < F(1), (F(0.5) * z) * z, z - F(0.5))
    assert per.dtype == np.float32
    return F(per.astype(np.float64).sum() / np.float64(len(per)))
