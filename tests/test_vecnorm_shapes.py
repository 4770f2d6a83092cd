"""cstr_vecnorm_step_f64 / cstr_vecnorm_apply_f32 (csrc/cstr_vecnorm.hip) at the shapes its one golden run never launches: the step is
ONE 1024-lane workgroup with strided row loops, a shuffle + LDS tree and a two-pass variance, so N = 1, N below / above a wave,
N at and just above the workgroup size and several strides per lane, with D = 1, 3, 4, 8, are all different trips through it.

Reference: numpy.float64, written here from the kernel's documented formulas (two-pass batch mean and variance,
RunningMeanStd.update_from_moments, clip after normalising) -- not oracle/vecnorm_np.py, which reduces in float32 like the
reference implementation does. Kernel and reference then differ in the ORDER of an f64 sum of N terms only (the merge and the
discounted returns are the same IEEE operations in the same order: the library is built with -ffp-contract=off), which bounds

    |got - want| <= 4 * N * 2**-52 * sum|terms|        per statistic,

with terms = x_i / N for a batch mean and (x_i - mean)**2 / N for a batch variance; a running moment after k updates is a convex
combination of the batch moments, so it gets the sum of the k updates' bounds. Observations are offset to a mean of 300, like the raw
temperature column: a one-pass variance (E[x^2] - E[x]^2) would lose 300^2 * 2**-24 = 5e-3 to the float32 inputs' spacing alone.
Every buffer is guarded on both sides (tests/_sentinel_bufs.py)."""
import numpy as np
import pytest
import torch as th

from conftest import rel_err
from _sentinel_bufs import GuardedBufs

pytestmark = pytest.mark.gpu

NS, DS = [1, 2, 63, 65, 1024, 1025, 4097], [1, 3, 4, 8]
U = 2.0 ** -52
CLIP_OBS, CLIP_REW, GAMMA, EPS = 2.5, 1.5, 0.9, 1e-8  # clips that bind on part of the batch


def _cfg(nv, d, training):
    return nv.VecNormCfg(int(training), 1, 1, d, CLIP_OBS, CLIP_REW, GAMMA, EPS)


class Moments:
    """RunningMeanStd (running_mean_std.py:34-55) in float64, with the summation-order bound of every statistic beside it"""

    def __init__(self, d):
        self.mean, self.var, self.count = np.zeros(d), np.ones(d), 1e-4
        self.tol_mean, self.tol_var = np.zeros(d), np.zeros(d)

    def update(self, x):  # x [N, d] float64
        n = x.shape[0]
        b_mean = x.sum(0) / n
        dev = x - b_mean
        b_var = (dev * dev).sum(0) / n
        self.tol_mean += 4 * n * U * np.abs(x).sum(0) / n
        self.tol_var += 4 * n * U * (dev * dev).sum(0) / n
        delta, tot = b_mean - self.mean, self.count + n
        new_mean = self.mean + delta * n / tot
        m2 = self.var * self.count + b_var * n + delta * delta * self.count * n / (self.count + n)
        self.mean, self.var, self.count = new_mean, m2 / (self.count + n), n + self.count
        return b_var


def _norm_obs(m, x):
    return np.clip((x.astype(np.float64) - m.mean) / np.sqrt(m.var + EPS), -CLIP_OBS, CLIP_OBS).astype(np.float32)


def _norm_rew(m, r):
    return np.clip(r.astype(np.float64) / np.sqrt(m.var[0] + EPS), -CLIP_REW, CLIP_REW).astype(np.float32)


def _check_state(st, D, obs_m, ret_m):
    s = st.cpu().numpy()
    assert np.all(np.abs(s[0:D] - obs_m.mean) <= obs_m.tol_mean), (s[0:D] - obs_m.mean, obs_m.tol_mean)
    assert np.all(np.abs(s[8:8 + D] - obs_m.var) <= obs_m.tol_var), (s[8:8 + D] - obs_m.var, obs_m.tol_var)
    assert s[16] == obs_m.count and s[19] == ret_m.count  # 1e-4 + k * N: the same additions
    assert abs(s[17] - ret_m.mean[0]) <= ret_m.tol_mean[0] and abs(s[18] - ret_m.var[0]) <= ret_m.tol_var[0], (s[17:19], ret_m.mean, ret_m.var)
    assert np.all(s[D:8] == 0.0) and np.all(s[8 + D:16] == 1.0)  # the words of columns this D does not have: still cstr_vecnorm_init_f64's


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_vecnorm_step_and_apply_at_ragged_sizes(N, D):
    from core import _native as nv
    from core.common import hip_ops as ops

    rng = np.random.default_rng(1000 * N + D)
    col_mean, col_std = 300.0 + 10.0 * np.arange(D), 1.0 + 0.5 * np.arange(D)
    raw_obs = (col_mean + col_std * rng.standard_normal((4, N, D))).astype(np.float32)
    raw_rew = (-3.0 + 2.0 * rng.standard_normal((3, N))).astype(np.float32)
    raw_obs[3, 0], raw_rew[2, 0] = col_mean + 10.0 * col_std, -40.0  # outliers in the step that only applies the statistics
    done = np.zeros((3, N), np.float32)
    done[:, N // 2] = 1.0  # one env finishes its episode in every step

    b = GuardedBufs()
    st = b.new("state", nv.VECNORM_STATE_WORDS, dtype=th.float64)
    ret = b.put("returns", np.ones(N), dtype=th.float64)  # the reset form must zero it
    ops.vecnorm_init(st)
    b.check(written=("state",))
    obs_m, ret_m, returns = Moments(D), Moments(1), np.zeros(N)

    # reset form (reward = None): observation moments, normalised observations, returns = 0
    o_in, o_out = b.put_ro("obs0", raw_obs[0]), b.new("nobs0", N, D)
    ops.vecnorm_step(_cfg(nv, D, True), st, ret, o_in, None, None, o_out, None)
    b.check(written=("nobs0", "returns"))
    b_var = obs_m.update(raw_obs[0].astype(np.float64))
    if N == 1:
        assert np.all(b_var == 0.0)
    _check_state(st, D, obs_m, ret_m)
    assert float(ret.abs().max()) == 0.0
    assert rel_err(o_out.cpu().numpy(), _norm_obs(obs_m, raw_obs[0]), 1.0) < 2e-6

    for k in range(3):
        training = k < 2  # the third step only applies the statistics
        o_in, r_in, d_in = b.put_ro(f"obs{k + 1}", raw_obs[k + 1]), b.put_ro(f"rew{k}", raw_rew[k]), b.put_ro(f"done{k}", done[k])
        o_out, r_out = b.new(f"nobs{k + 1}", N, D), b.new(f"nrew{k}", N)
        st_before, ret_before = st.clone(), ret.clone()
        ops.vecnorm_step(_cfg(nv, D, training), st, ret, o_in, r_in, d_in, o_out, r_out)
        b.check(written=(f"nobs{k + 1}", f"nrew{k}"))
        ret_terms = np.zeros(N)
        if training:
            b_var = obs_m.update(raw_obs[k + 1].astype(np.float64))
            ret_terms = np.abs(returns * GAMMA) + np.abs(raw_rew[k].astype(np.float64))
            returns = returns * GAMMA + raw_rew[k].astype(np.float64)
            b_ret_var = ret_m.update(returns[:, None])
            if N == 1:  # a batch of one has variance exactly 0.0: with it the merge is bit for bit the reference's
                assert np.all(b_var == 0.0) and np.all(b_ret_var == 0.0)
                s = st.cpu().numpy()
                assert np.array_equal(s[8:8 + D], obs_m.var) and s[18] == ret_m.var[0]
        else:
            assert th.equal(st, st_before)
        _check_state(st, D, obs_m, ret_m)
        # discounted returns (a sum of two terms per element, untouched when not training), then the done mask
        want_ret = returns.copy()
        want_ret[done[k] != 0] = 0.0
        got_ret = ret.cpu().numpy()
        assert np.all(np.abs(got_ret - want_ret) <= 4 * 2 * U * ret_terms), np.abs(got_ret - want_ret).max()
        assert got_ret[N // 2] == 0.0
        returns = want_ret
        assert rel_err(o_out.cpu().numpy(), _norm_obs(obs_m, raw_obs[k + 1]), 1.0) < 2e-6, k
        assert rel_err(r_out.cpu().numpy(), _norm_rew(ret_m, raw_rew[k]), 1.0) < 2e-6, k
        # the same launch from the same state: the same bits
        snap = b.snapshot()
        st.copy_(st_before)
        ret.copy_(ret_before)
        ops.vecnorm_step(_cfg(nv, D, training), st, ret, o_in, r_in, d_in, o_out, r_out)
        b.check(written=(f"nobs{k + 1}", f"nrew{k}"))
        b.same_as(snap)
    assert float(o_out.abs().max()) == CLIP_OBS and float(r_out.abs().max()) == CLIP_REW  # the outliers of the last step: both clips bind

    # a sampled batch, in place, with the current statistics; all three operands, then each alone
    held_o, held_o2, held_r = raw_obs[0], raw_obs[1][::-1].copy(), raw_rew[0]
    a = GuardedBufs()
    st_ro = a.put_ro("state", st, dtype=th.float64)
    o, o2, r = a.put("obs", held_o), a.put("next_obs", held_o2), a.put("rew", held_r[:, None])
    ops.vecnorm_apply(_cfg(nv, D, False), st_ro, o, o2, r)
    a.check()
    assert rel_err(o.cpu().numpy(), _norm_obs(obs_m, held_o), 1.0) < 2e-6
    assert rel_err(o2.cpu().numpy(), _norm_obs(obs_m, held_o2), 1.0) < 2e-6
    assert rel_err(r.cpu().numpy()[:, 0], _norm_rew(ret_m, held_r), 1.0) < 2e-6
    snap = a.snapshot()
    o.copy_(th.as_tensor(held_o)), o2.copy_(th.as_tensor(held_o2)), r.copy_(th.as_tensor(held_r[:, None]))
    ops.vecnorm_apply(_cfg(nv, D, False), st_ro, o, o2, r)
    a.check()
    a.same_as(snap)
    o3, o4, r2 = a.put("obs_alone", held_o), a.put("next_alone", held_o2), a.put("rew_alone", held_r)
    ops.vecnorm_apply(_cfg(nv, D, False), st_ro, o3, None, None)
    ops.vecnorm_apply(_cfg(nv, D, False), st_ro, None, o4, None)
    ops.vecnorm_apply(_cfg(nv, D, False), st_ro, None, None, r2)
    a.check()
    assert th.equal(o3, o) and th.equal(o4, o2) and th.equal(r2, r[:, 0])
