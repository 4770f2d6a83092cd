"""GPU checks of the MultiCategorical head of PPO / A2C on the MultiDiscrete valve face (csrc/cstr_multicategorical.hip).

Head (cstr_multicategorical_act_f32) against fp64 of logp = sum over the valves of z_a - logsumexp(z): within 4 x the error of the
float32 ATen evaluation (torch.log_softmax per split on the CPU, then summed) of the same inputs, per element in units of 2**-24 * M
with M the sum over the valves of |z_a| + |logsumexp z| (test_categorical.logp_units on the pair), the ATen figure measured here over
all the cases and all pairs; the deterministic pair exact (ties: the first; a NaN: the greatest); forced and clamped pairs; exact
uniforms per valve; the inverse CDF exact outside a 2e-5 band round the fp64 cumulative boundaries of each valve; the drawn uniforms
against the Philox counter contract (words 0 and 1 of one block); valve pairs; sentinels; repeat launches.

Loss (cstr_multicategorical_loss_f32) against fp64 autograd of the reference's statements (core/ppo/ppo.py:213-264,
core/a2c/a2c.py:150-171 on one torch Categorical per th.split, _mcat_helpers.loss_torch) with test_categorical's VARIANTS, RTOL / ATOL
and check_scalars rule; the scalar bars are 4 x the float32 ATen autograd's figures measured here.

Shapes: nvec (2, 2) (the least face; four logits like Discrete(4)), (3, 5), (16, 16), (31, 32) (a prime beside the bound) and (32, 2)
(a full half beside the least one); ldz = K0 + K1 and + 3; rows 1, 3, 5 (one wave, a partial workgroup, two workgroups) and 1030 (more
than one pass of the loss launch's 64 x 4 rows, and of the head's 256 x 4).

Then the classes: teacher-forced rollouts and train() of PPO and A2C against the fixtures the unmodified reference wrote on a
MultiDiscrete([K0, K1]) face (tools/refharness/gen_golden.py gen_ppo_multidiscrete / gen_a2c_multidiscrete; the reference's sampled
pairs are queued) on the fused, rocBLAS and torch-statement paths with the bars of tests/test_categorical.py; predict;
evaluate_policy and EvalCallback; save / load; the refusals; fused_learner switched mid-run; a learning run."""
import warnings

import numpy as np
import pytest
import torch as th

import _mcat_helpers as mh
from _mcat_helpers import NVECS, ROWS, U24
from _parity_helpers import check_init, check_weights, q_err, rel_err
from _sentinel_bufs import SENT, Bufs
from test_categorical import (ATOL, PATHS, ROLLOUT_FIELDS, RTOL, VARIANTS, check_ppo_train, check_scalars, dev, same_bits, scalar_units,
                              scale_err, set_path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = (0.01, 1.0, 4.0)


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


def run_head(ops, z, nvec, pad=0, want=("valve", "log_prob"), **kw):
    """-> dict of numpy outputs; the logits sit in a [n, K0 + K1 + pad] matrix whose tail columns hold 100 (never read)"""
    n, M = z.shape
    wide = np.full((n, M + pad), 100.0, np.float32)
    wide[:, :M] = z
    b = Bufs()
    act_f = b.new("action_f32", n, 2)
    valve = b.new("valve", n, 2) if "valve" in want else None
    logp = b.new("log_prob", n) if "log_prob" in want else None
    u_out = b.new("u_out", n, 2) if "u_out" in want else None
    pairs = th.full((n + 4, 2), -7, dtype=th.int64, device=DEV)
    args = dict(action_out=pairs[:n], valve_out=valve, log_prob=logp, u_out=u_out, **kw)
    ops.multicategorical_act(dev(wide)[:, :M], nvec, act_f, **args)
    b.check(written=list(b.flat))
    snap, first = b.snapshot(), pairs.clone()
    if kw.get("rng_ctl") is None:  # a drawing launch moves its stream: its repeat is checked where the stream is
        ops.multicategorical_act(dev(wide)[:, :M], nvec, act_f, **args)
        th.cuda.synchronize()
        same_bits(b, snap)
        assert th.equal(pairs, first)
    assert bool((pairs[n:] == -7).all())
    out = dict(pairs=pairs[:n].cpu().numpy(), action_f32=act_f.cpu().numpy())
    assert np.array_equal(out["action_f32"], out["pairs"].astype(np.float32))
    assert (out["pairs"] >= 0).all() and (out["pairs"] < np.array(nvec)).all()
    if valve is not None:
        out["valve"] = valve.cpu().numpy()
        assert out["valve"].tobytes() == mh.valves_np(out["pairs"], nvec).tobytes()  # decode_valve_levels' statement
    if logp is not None:
        out["log_prob"] = logp.cpu().numpy()
    if u_out is not None:
        out["u_out"] = u_out.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def aten_logp_bar():
    """4 x the worst float32 ATen figure (CPU log_softmax per split, the two summed in float32) over every head case of this module,
    all pairs of levels"""
    worst = 0.0
    for nvec in NVECS:
        for n in ROWS:
            for scale in SCALES:
                z = mh.head_case(n, nvec, 7000 + 100 * nvec[0] + nvec[1] + n, scale)
                z0, z1 = mh.split(z, nvec)
                got = (th.log_softmax(th.as_tensor(z0), dim=1)[:, :, None] + th.log_softmax(th.as_tensor(z1), dim=1)[:, None, :]).numpy()
                (lp0, lse0), (lp1, lse1) = mh.logp64(z0), mh.logp64(z1)
                want = lp0[:, :, None] + lp1[:, None, :]
                mag = (np.abs(z0.astype(np.float64)) + np.abs(lse0))[:, :, None] + (np.abs(z1.astype(np.float64)) + np.abs(lse1))[:, None, :]
                worst = max(worst, float((np.abs(got.astype(np.float64) - want) / (U24 * mag)).max()))
    print(f"float32 ATen log_softmax per split, summed, against fp64: worst {worst:.3f} units; bar {4 * worst:.3f}")
    return 4.0 * worst


def argmax_pairs(z, nvec):
    """NumPy's argmax per valve: the first maximum, a NaN is the maximum"""
    return np.stack([s.astype(np.float64).argmax(axis=1) for s in mh.split(z, nvec)], axis=1)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("nvec", NVECS)
def test_head_log_prob_and_deterministic_pair(ops, aten_logp_bar, nvec, pad):
    K0, K1 = nvec
    for n in ROWS:
        for scale in SCALES:
            z = mh.head_case(n, nvec, 7000 + 100 * K0 + K1 + n, scale)
            top = z[0].max() + np.float32(0.5)
            z[0, [0, K0 - 1]] = top              # valve 0: tied maxima at both ends, the first wins
            z[0, [K0 + 1, K0 + K1 - 1]] = top    # valve 1: tied at 1 and the last level
            if n > 1:
                z[1, K0 - 1] = np.nan            # a NaN counts as the greatest value (valve 0's last level)
                z[1, [K0, K0 + K1 - 1]] = np.nan  # ... the first one (valve 1)
            if n > 2:
                z[2, :] = np.float32(0.25)       # every logit tied: the pair (0, 0)
            out = run_head(ops, z, nvec, pad, deterministic=True)
            want = argmax_pairs(z, nvec)
            assert np.array_equal(out["pairs"], want), (n, scale)
            assert out["pairs"][0].tolist() == [0, 1] and (n < 2 or out["pairs"][1].tolist() == [K0 - 1, 0])
            assert n < 3 or out["pairs"][2].tolist() == [0, 0]
            ok = np.ones(n, bool)
            if n > 1:
                ok[1] = False
                assert np.isnan(out["log_prob"][1])
            fig = mh.logp_units(out["log_prob"][ok], z[ok], nvec, out["pairs"][ok]).max()
            print(f"nvec={nvec} pad={pad} n={n} scale={scale}: log_prob {fig:.3f} units (bar {aten_logp_bar:.3f})")
            assert fig <= aten_logp_bar, (n, scale, fig)


@pytest.mark.parametrize("nvec", NVECS)
def test_head_forced_pairs_are_clamped_per_valve(ops, aten_logp_bar, nvec):
    K0, K1 = nvec
    for n in ROWS:
        z = mh.head_case(n, nvec, 8000 + 100 * K0 + K1 + n)
        rng = np.random.default_rng(K0 * K1 * n)
        a = np.stack([rng.integers(0, K0, n), rng.integers(0, K1, n)], axis=1)
        a[0] = (K0 - 1, K1 - 1)
        if n > 2:
            a[1], a[2] = (-5, K1 + 3), (K0, -1)  # the caller's bug: clamped into the face, each valve by its own count
        out = run_head(ops, z, nvec, 3, action_in=dev(a, th.int64))
        want = np.clip(a, 0, np.array(nvec) - 1)
        assert np.array_equal(out["pairs"], want)
        assert mh.logp_units(out["log_prob"], z, nvec, want).max() <= aten_logp_bar


@pytest.mark.parametrize("nvec", NVECS)
def test_head_exact_uniform_cases(ops, nvec):
    K0, K1 = nvec
    n = 5
    z = mh.head_case(n, nvec, 8100 + 100 * K0 + K1)
    z[1, : K0 // 2] = -np.inf            # valve 0: p = 0 up to K0 / 2, u = 0 gives the first level with p > 0
    z[2, K0: K0 + K1 // 2] = -np.inf     # valve 1 likewise
    z[3, 0] = -200.0                     # valve 0: p underflows to 0 in f32
    z[4, K0] = -200.0                    # valve 1
    out = run_head(ops, z, nvec, 0, u=dev(np.zeros((n, 2), np.float32)), want=("valve",))
    assert out["pairs"].tolist() == [[0, 0], [K0 // 2, 0], [0, K1 // 2], [1, 0], [0, 1]]
    eq = np.full((n, K0 + K1), 0.75, np.float32)
    last = np.float32(1.0 - 2.0 ** -24)
    out = run_head(ops, eq, nvec, 3, u=dev(np.full((n, 2), last, np.float32)), want=())
    assert (out["pairs"] == np.array([K0 - 1, K1 - 1])).all()
    mixed = np.tile(np.array([[0.0, last]], np.float32), (n, 1))  # the two valves read their own uniform
    out = run_head(ops, eq, nvec, 3, u=dev(mixed), want=())
    assert (out["pairs"] == np.array([0, K1 - 1])).all()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nvec", NVECS)
def test_head_inverse_cdf(ops, nvec, scale):
    n = 4096
    z = mh.head_case(n, nvec, 8200 + 100 * nvec[0] + nvec[1], scale)
    u = np.random.default_rng(nvec[0] * 64 + nvec[1]).uniform(size=(n, 2)).astype(np.float32)
    out = run_head(ops, z, nvec, 3, u=dev(u), want=("valve", "log_prob", "u_out"))
    assert np.array_equal(out["u_out"], u)
    near_all, swapped = [], 0
    for g, zg in enumerate(mh.split(z, nvec)):
        K = nvec[g]
        lp, _ = mh.logp64(zg)
        cum = np.cumsum(np.exp(lp), axis=1)
        u64 = u[:, g].astype(np.float64)[:, None]
        near = (np.abs(cum - u64) <= 2e-5).any(axis=1)  # u within 2e-5 of a boundary: either neighbour
        want = np.minimum((cum <= u64).sum(axis=1), K - 1)
        lo = np.minimum((cum <= u64 - 2e-5).sum(axis=1), K - 1)
        hi = np.minimum((cum <= u64 + 2e-5).sum(axis=1), K - 1)
        got = out["pairs"][:, g]
        assert np.array_equal(got[~near], want[~near]), (g, int((got[~near] != want[~near]).sum()))
        assert ((got >= lo) & (got <= hi)).all(), g
        near_all.append(near)
        swapped += int((got != want).sum())
    share = float(np.concatenate(near_all).mean())
    print(f"nvec={nvec} scale={scale}: {share:.4f} of the draws near a boundary, {swapped} of them took the neighbour")
    assert share <= 0.03, share


def test_head_draws_its_uniforms_from_philox(ops):
    nvec, n = (3, 5), 1030
    hi_seed = (0xABCDE << 32) | 17
    z = mh.head_case(n, nvec, 8300)
    for seed, base in ((99, 0), (hi_seed, 2 ** 32 - 3)):  # the second: a 64-bit key and a counter that carries into word 1
        ctl = ops.new_rng_ctl(seed, DEV)
        ctl[1] = base
        for call in range(2):
            u = mh.mcat_uniforms(seed, base + call * n, n)
            out = run_head(ops, z, nvec, 0, rng_ctl=ctl, want=("valve", "log_prob", "u_out"))
            assert np.array_equal(out["u_out"][:, 0], u[:, 0]) and np.array_equal(out["u_out"][:, 1], u[:, 1])  # words 0 and 1, element by element
            same = run_head(ops, z, nvec, 0, u=dev(u))
            assert np.array_equal(out["pairs"], same["pairs"]) and np.array_equal(out["log_prob"], same["log_prob"])
            assert int(ctl[1]) == base + (call + 1) * n and int(ctl[2]) == 0  # advanced by the row count; the ticket reset itself
        assert abs(float(u.mean()) - 0.5) < 0.05 and not np.array_equal(u[:, 0], u[:, 1])
    act_f = th.zeros(n, 2, device=DEV)
    with pytest.raises(Exception, match="code -1"):
        ops.multicategorical_act(dev(z), nvec, act_f)  # no source
    with pytest.raises(Exception, match="code -1"):
        ops.multicategorical_act(dev(z), nvec, act_f, deterministic=True, rng_ctl=ctl)  # two sources
    with pytest.raises(Exception, match="code -2"):
        ops.multicategorical_act(dev(np.zeros((4, 38), np.float32)), (33, 5), th.zeros(4, 2, device=DEV), deterministic=True)
    with pytest.raises(ValueError, match="do not fit"):
        ops.multicategorical_act(dev(z), (4, 5), act_f, deterministic=True)


# ---- cstr_multicategorical_loss_f32 --------------------------------------------------------------------------------------------------
def run_loss(ops, c, nvec, pad, objective, norm, ent_coef, vf_coef, clip_range=0.2, clip_range_vf=None):
    B, M = c["z"].shape
    wide = np.full((B, M + pad), 100.0, np.float32)
    wide[:, :M] = c["z"]
    ns = 6 if objective == 0 else 4
    b = Bufs()
    g_wide = b.new("g_logits", B, M + pad)
    g_value, scalars, logp = b.new("g_value", B), b.new("scalars", ns), b.new("log_prob", B)
    sums = b.put("sums", np.arange(ns, dtype=np.float32))
    ws = ops.new_ppo_workspace(DEV)
    call = lambda: ops.multicategorical_loss(  # noqa: E731
        objective, dev(wide)[:, :M], nvec, dev(c["a"].astype(np.float32)), dev(c["values"]), dev(c["adv"]), dev(c["returns"]), norm,
        ent_coef, vf_coef, g_wide[:, :M], g_value, ws, old_values=dev(c["old_values"]), old_log_prob=dev(c["old_lp"]), clip_range=clip_range,
        clip_range_vf=clip_range_vf, scalars_out=scalars, scalars_sum=sums, log_prob_out=logp)
    call()
    b.check(written=("g_value", "scalars", "log_prob"))
    assert bool((g_wide[:, M:] == SENT).all()) and not bool((g_wide[:, :M] == SENT).any())  # the tail columns keep their sentinel
    s1 = scalars.cpu().numpy().copy()
    np.testing.assert_array_equal(sums.cpu().numpy(), np.arange(ns, dtype=np.float32) + s1)  # scalars_sum accumulates
    snap = b.snapshot()
    call()
    th.cuda.synchronize()
    same_bits(b, snap, skip=("sums",))
    np.testing.assert_array_equal(sums.cpu().numpy(), (np.arange(ns, dtype=np.float32) + s1) + s1)  # NaN == NaN here
    assert int(ws[0]) == 0  # the ticket reset itself
    return s1.astype(np.float64), g_wide[:, :M].cpu().numpy().astype(np.float64), g_value.cpu().numpy().astype(np.float64), logp.cpu().numpy()


LOSS_ROWS = (1, 5, 1030)


@pytest.fixture(scope="module")
def loss_refs():
    """Every loss case once: (inputs, fp64 autograd, float32 ATen autograd) per (nvec, B, variant), shared by the tests; and 4 x the
    worst float32 ATen figure per scalar over all of them, in the units of test_categorical.scalar_units"""
    refs, worst = {}, np.zeros(5)
    for nvec in NVECS:
        for B in LOSS_ROWS:
            c = mh.loss_case(B, nvec, 9000 + 100 * nvec[0] + nvec[1] + B)
            for v in VARIANTS:
                objective, norm, ent_coef, crv = v
                kw = dict(clip_range_vf=crv) if objective == 0 else {}
                with np.errstate(all="ignore"):
                    want = mh.loss_torch(c, nvec, objective, th.float64, norm, ent_coef, 0.5, **kw)
                    aten = mh.loss_torch(c, nvec, objective, th.float32, norm, ent_coef, 0.5, **kw)
                refs[(nvec, B, v)] = (c, want, aten)
                if not (objective == 1 and norm and B == 1):
                    u = scalar_units(aten[0], want)
                    worst[:len(u)] = np.maximum(worst[:len(u)], u)
    print(f"float32 ATen scalars against fp64, worst units of 2**-24 M: {np.round(worst, 3).tolist()}; bars {np.round(4 * worst, 3).tolist()}")
    return refs, 4.0 * worst


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("nvec", NVECS)
def test_loss_against_fp64_autograd(ops, loss_refs, nvec, pad):
    refs, bars = loss_refs
    for B in LOSS_ROWS:
        for objective, norm, ent_coef, crv in VARIANTS:
            kw = dict(clip_range_vf=crv) if objective == 0 else {}
            c, want, aten = refs[(nvec, B, (objective, norm, ent_coef, crv))]
            got = run_loss(ops, c, nvec, pad, objective, norm, ent_coef, 0.5, **kw)
            tag = (nvec, pad, B, objective, norm, ent_coef, crv)
            if objective == 1 and norm and B == 1:  # torch.std of one element: NaN, no guard in the reference
                assert np.isnan(want[0][0]) and np.isnan(got[0][0]) and np.isnan(got[1]).all() and np.isfinite(got[2]).all(), tag
                continue
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all(), tag
            check_scalars(got[0], want, tag, bars)
            np.testing.assert_allclose(got[2], want[2], rtol=RTOL, atol=ATOL, err_msg=f"g_value {tag}")
            err = np.abs(got[1] - want[1])
            worst = float((err / (ATOL + RTOL * np.abs(want[1]))).max())
            print(f"{tag}: g_logits worst err / (atol + rtol |want|) = {worst:.3f}; ATen worst abs err {np.abs(aten[1] - want[1]).max():.3e}, "
                  f"kernel {err.max():.3e}")
            assert worst <= 1.0, (tag, worst)
            np.testing.assert_allclose(got[3], want[3], rtol=RTOL, atol=ATOL, err_msg=f"log_prob {tag}")


@pytest.mark.parametrize("objective", [0, 1])
def test_entropy_gradient_uses_each_valves_own_entropy(ops, objective):
    """H_0 near 0 (valve 0 saturated on one level), H_1 = log 5 (valve 1 uniform), ent_coef 0.5: d(-ent_coef mean H) / dz of valve g is
    (ent_coef / B) p_j (logp_j + H_g). With the row's H = H_0 + H_1 in place of H_g every column of valve 1 moves by about
    (ent_coef / B) * p_j * H_0 and of valve 0 by p_j * H_1: far outside the bar, which this test asserts of its own reference first."""
    nvec, B, ent_coef = (3, 5), 5, 0.5
    c = mh.loss_case(B, nvec, 4242)
    c["z"][:, :3] = np.array([9.0, 0.0, -1.0], np.float32) + c["z"][:, :3] * np.float32(0.1)  # H_0 ~ 1e-3
    c["z"][:, 3:] = np.float32(0.3)                                                            # H_1 = log 5
    c["z"][1, 1] = np.float32(8.5)                                                             # row 1: two live levels, H_0 ~ 0.66
    # the old log-probs belong to these logits, as loss_case makes them: ratios on both sides of the clip range, none astronomical
    c["old_lp"] = (mh.pair_logp64(c["z"], nvec, c["a"])[0] + np.random.default_rng(4243).normal(size=B) * 0.25).astype(np.float32)
    want =mh.loss_torch(c, nvec, objective, th.float64, False, ent_coef, 0.5)
    (lp0, _), (lp1, _) = mh.logp64(c["z"][:, :3]), mh.logp64(c["z"][:, 3:])
    H0, H1 = -(np.exp(lp0) * lp0).sum(axis=1), -(np.exp(lp1) * lp1).sum(axis=1)
    assert (np.abs(H1 - np.log(5)) < 1e-6).all() and (H0 < 0.7).all() and H0[0] < 0.01
    wrong = want[1].copy()  # what a kernel that used the row's H would write
    wrong[:, :3] += (ent_coef / B) * np.exp(lp0) * H1[:, None]
    wrong[:, 3:] += (ent_coef / B) * np.exp(lp1) * H0[:, None]
    assert (np.abs(wrong - want[1]) / (ATOL + RTOL * np.abs(want[1]))).max() > 1e3
    got = run_loss(ops, c, nvec, 3, objective, False, ent_coef, 0.5)
    assert float((np.abs(got[1] - want[1]) / (ATOL + RTOL * np.abs(want[1]))).max()) <= 1.0
    assert abs(got[0][2] - want[0][2]) <= ATOL + RTOL * abs(want[0][2])  # entropy_loss = -mean(H_0 + H_1)


def test_loss_value_clip_engages(ops, loss_refs):
    """rows inside and outside the value clip range: the gradient passes on the closed interval only"""
    nvec, B = (3, 5), 12
    c = mh.loss_case(B, nvec, 77)
    c["values"] = (c["old_values"] + np.linspace(-0.3, 0.3, B).astype(np.float32)).astype(np.float32)
    want = mh.loss_torch(c, nvec, 0, th.float64, True, 0.0, 0.5, clip_range_vf=0.1)
    got = run_loss(ops, c, nvec, 0, 0, True, 0.0, 0.5, clip_range_vf=0.1)
    np.testing.assert_allclose(got[2], want[2], rtol=RTOL, atol=ATOL)
    assert (got[2] == 0).sum() >= 4 and (got[2] != 0).sum() >= 2
    check_scalars(got[0], want, "value clip", loss_refs[1])


# ---- the classes against the reference's fixtures (tools/refharness/gen_golden.py gen_ppo_multidiscrete / gen_a2c_multidiscrete) ------
def face_env(n, nvec):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n, multi_discrete_actions=tuple(int(k) for k in nvec), device=DEV)


def make_model(cls, g, prefix="before", **kw):
    extra = dict(batch_size=int(g["batch_size"]), n_epochs=int(g["n_epochs"])) if "batch_size" in g else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the truncated-minibatch warning (checked in test_ppo_abi.py)
        model = cls("MlpPolicy", face_env(int(g["n_envs"]), g["nvec"]), seed=int(g["seed"]), n_steps=int(g["n_steps"]),
                    learning_rate=float(g["learning_rate"]), ent_coef=float(g["ent_coef"]),
                    policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]]), device=DEV, **extra, **kw)
    if f"{prefix}/policy/action_net.weight" in g:  # the class-default fixture keeps digests: its seeded initial weights are checked instead
        with th.no_grad():
            for k, v in model.policy.state_dict().items():
                v.copy_(th.as_tensor(g[f"{prefix}/policy/{k}"]))
    else:
        check_init(model, g, ["policy"])
    assert model._fast is not None and model._fast.multi_discrete and not model._fast.discrete
    return model


def check_rollout(model, g, pre=""):
    rb = model.rollout_buffer
    want_a = g[f"{pre}rollout/actions"]
    assert tuple(rb.actions.shape) == want_a.shape == (int(g["n_steps"]), int(g["n_envs"]), 2) and rb.actions.dtype == th.float32
    np.testing.assert_array_equal(rb.actions.cpu().numpy(), want_a)  # the reference's shape and values: the level pair as floats
    np.testing.assert_array_equal(rb.episode_starts.cpu().numpy(), g[f"{pre}rollout/episode_starts"])
    for f in ("observations", "values", "log_probs", "rewards", "advantages", "returns"):
        assert scale_err(getattr(rb, f), g[f"{pre}rollout/{f}"]) < 1e-5, f


def queue_actions(model, actions, path):
    q = [th.as_tensor(a.reshape(-1, 2).astype(np.int64)) for a in actions]
    if path == "torch":
        model.policy.action_dist.action_queue = q
    else:
        model._fast.action_queue = q
    return q


@pytest.mark.parametrize("path", PATHS)
def test_ppo_rollout_teacher_forced(golden, path, monkeypatch):
    """collect_rollouts against the reference's rollout: the `before/` weights, the initial observations and step counters injected
    after _setup_learn's reset, the reference's sampled pairs queued. The kernel paths roll out on the device."""
    from core.ppo import PPO

    g = golden("ppo_mcat_train_kat_small.npz")
    model = make_model(PPO, g)
    set_path(model, path, monkeypatch)
    assert model._device_rollout() == (path != "torch")
    _, cb = model._setup_learn(int(g["n_envs"] * g["n_steps"]), None)
    model.env.set_state(g["init_obs"], g["init_steps"])
    if path == "torch":
        model._last_obs = model.env.obs.cpu().numpy().copy()
    q = queue_actions(model, g["rollout/actions"], path)
    assert model.collect_rollouts(model.env, cb, model.rollout_buffer, int(g["n_steps"]))
    assert model.rollout_buffer.full and not q and g["timeouts"].sum() >= 2
    check_rollout(model, g)
    assert scale_err(th.as_tensor(np.asarray(model._last_obs.cpu() if isinstance(model._last_obs, th.Tensor) else model._last_obs)), g["last_obs"]) < 1e-5


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["small", "default"])
def test_ppo_train_teacher_forced(golden, name, path, monkeypatch):
    from core.common.buffers import RolloutBuffer
    from core.ppo import PPO

    g = golden(f"ppo_mcat_train_kat_{name}.npz")
    model = make_model(PPO, g)
    set_path(model, path, monkeypatch)
    model.rollout_buffer = RolloutBuffer.from_arrays(model.observation_space, model.action_space, DEV, gamma=model.gamma,
                                                     gae_lambda=model.gae_lambda, **{f: g[f"rollout/{f}"] for f in ROLLOUT_FIELDS})
    assert tuple(model.rollout_buffer.actions.shape) == g["rollout/actions"].shape
    model.rollout_buffer.forced_permutations = [p for p in g["permutations"]]
    model.debug_capture = True
    model.train()
    assert name == "default" or any(float(g[f"mb{k}/scalars"][5]) > 0 for k in range(int(g["n_minibatches"])))
    check_ppo_train(model, g, path)


@pytest.mark.parametrize("path", PATHS)
def test_a2c_two_iterations_teacher_forced(golden, path, monkeypatch):
    """rollout (pairs queued) and train(), twice, against a2c_mcat_train_kat_small.npz with the bars of tests/test_categorical.py"""
    from core.a2c import A2C

    g = golden("a2c_mcat_train_kat_small.npz")
    label = {"fused": "a2c_fused", "rocblas": "a2c_rocblas", "torch": "a2c_aten"}[path]
    model = make_model(A2C, g)
    set_path(model, path, monkeypatch)
    n, T, iters = int(g["n_envs"]), int(g["n_steps"]), int(g["iterations"])
    _, cb = model._setup_learn(iters * n * T, None)
    model.env.set_state(g["init_obs"], g["init_steps"])
    if path == "torch":
        model._last_obs = model.env.obs.cpu().numpy().copy()
    model.debug_capture = True
    for it in range(iters):
        pre = f"it{it}/"
        q = queue_actions(model, g[pre + "rollout/actions"], path)
        assert model.collect_rollouts(model.env, cb, model.rollout_buffer, T) and not q
        check_rollout(model, g, pre)
        model.rollout_buffer.forced_permutations = [g[pre + "permutation"]]
        model._update_current_progress_remaining((it + 1) * n * T, iters * n * T)
        model.train()
        cap = model.last_train_capture
        perm = g[pre + "permutation"]
        order = (perm % T) * n + perm // T  # the fixture's rows are in get(None)'s order: back into storage order
        want_v, want_lp = np.empty(T * n, np.float32), np.empty(T * n, np.float32)
        want_v[order], want_lp[order] = g[pre + "values"].reshape(-1), g[pre + "log_prob"]
        assert rel_err(cap["values"].cpu().numpy(), want_v, float(np.abs(want_v).mean())) < 1e-5, (it, "values")
        assert q_err(cap["log_prob"].cpu().numpy(), want_lp, label) < 1e-5, (it, "log_prob")
        got, want_s = cap["scalars"].cpu().numpy().astype(np.float64), g[pre + "scalars"].astype(np.float64)
        for i in range(4):
            assert abs(got[i] - want_s[i]) <= 1e-5 * max(abs(want_s[i]), 1.0), (it, i, got[i], want_s[i])
        assert rel_err(cap["grad_norm"].cpu().numpy(), g[pre + "grad_norm"]) < 5e-5, (it, "grad_norm")
        assert model._n_updates == int(g[pre + "n_updates"]) and model.policy.optimizer.step_count == int(g[pre + "optimizer_steps"])
        check_weights(model, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre + "after/")}, "after", ["policy"])
        logged = model.logger.resolved()
        want = dict(zip([str(k) for k in g[pre + "logged_keys"]], g[pre + "logged_values"]))
        assert set(want) == {"train/n_updates", "train/explained_variance", "train/entropy_loss", "train/policy_loss", "train/value_loss",
                             "train/learning_rate"} and "train/std" not in logged
        for key, w in want.items():
            assert abs(float(logged[key]) - w) <= 1e-5 * max(abs(w), 1.0), (key, logged[key], w)


def test_predict_matches_the_reference(golden):
    from core.ppo import PPO

    g, small = golden("ppo_mcat_predict_kat.npz"), golden("ppo_mcat_train_kat_small.npz")
    model = make_model(PPO, {**{k: small[k] for k in small.files}, **{f"before/policy/{k[7:]}": g[k] for k in g.files if k.startswith("policy/")}})
    act, state = model.predict(g["obs"], deterministic=True)
    assert state is None and act.shape == (16, 2) and act.dtype == np.int64
    np.testing.assert_array_equal(act, g["deterministic"])  # every row: the generator kept the logit gaps wide
    one, _ = model.predict(g["obs"][3], deterministic=True)
    assert one.shape == (2,) and one.dtype == np.int64 and np.array_equal(one, g["deterministic"][3])
    with th.no_grad():
        logits = model._fast.logits(dev(g["obs"]))
        values = model.policy.predict_values(dev(g["obs"]))
        a, v, lp = model.policy(dev(g["obs"]), deterministic=True)
    assert scale_err(logits, g["logits"]) < 1e-5 and values.shape == (16, 1) and q_err(values.cpu().numpy(), g["values"], "ppo_fused") < 1e-5
    assert a.dtype == th.int64 and tuple(a.shape) == (16, 2) and tuple(v.shape) == (16, 1) and tuple(lp.shape) == (16,)
    a1 = np.stack([model.predict(g["obs"], deterministic=False)[0] for _ in range(8)])  # unforced: the Philox stream
    assert a1.dtype == np.int64 and a1.shape == (8, 16, 2) and a1.min() >= 0 and a1[..., 0].max() < 3 and a1[..., 1].max() < 5
    assert len(np.unique(a1.reshape(8, -1), axis=0)) > 1
    model.fused_learner = False  # the torch statements: argmax(probs) per split
    np.testing.assert_array_equal(model.predict(g["obs"], deterministic=True)[0], g["deterministic"])


def test_env_face_steps_with_integer_pairs():
    env = face_env(4, (2, 32))
    assert env.multi_discrete_actions == (2, 32) and env.discrete_actions is None and env.act_dim == 2
    assert env.action_space.nvec.tolist() == [2, 32] and env.action_space.shape == (2,) and env.valve_space.shape == (2,)
    env.seed(0)
    env.reset()
    pairs = np.array([[0, 0], [1, 31], [0, 17], [1, 5]], np.int64)
    env.step_async(pairs)
    assert env._pending_actions.cpu().numpy().tobytes() == mh.valves_np(pairs, (2, 32)).tobytes()
    obs, rew, done, infos = env.step_wait()
    assert obs.shape == (4, 4) and rew.shape == (4,) and len(infos) == 4
    env.step(th.as_tensor(pairs))  # an integer tensor is taken too
    for bad in (pairs.astype(np.float32), pairs[:, 0], pairs[:3], np.array([[2, 0]] * 4), np.array([[0, 32]] * 4), np.array([[-1, 0]] * 4)):
        with pytest.raises(ValueError, match="multi-discrete actions"):
            env.step_async(bad)
    out = env.step_device(th.zeros(4, 2, device=DEV))  # the kernels keep seeing the valve pair
    assert tuple(out[0].shape) == (4, 4)


def test_evaluation_callbacks_save_load_and_refusals(golden, tmp_path):
    from core.a2c import A2C
    from core.common import evaluation
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv, VecNormalize
    from core.dqn import DQN
    from core.ppo import PPO

    env = face_env(8, (3, 5))
    model = PPO("MlpPolicy", env, n_steps=8, batch_size=32, n_epochs=2, seed=3, device=DEV)
    assert model.fused_learner and model._device_rollout() and model._fast.multi_discrete and model._fast.nvec == (3, 5)
    ev_env = face_env(2, (3, 5))
    assert not evaluation.supported(model, ev_env)
    with pytest.raises(ValueError, match="MultiDiscrete"):
        evaluation.evaluate_policy_fused(model, ev_env, n_eval_episodes=2)
    forced = EvalCallback(ev_env, n_eval_episodes=2, eval_freq=8, verbose=0, warn=False, fused=True)
    forced.init_callback(model)
    with pytest.raises(ValueError, match="MultiDiscrete"):
        forced._evaluate()
    ev = EvalCallback(ev_env, n_eval_episodes=2, eval_freq=8, verbose=0, warn=False)  # fused=None: falls back to the loop
    model.learn(8 * 8 * 2, callback=ev)
    assert ev.n_calls == 16 and np.isfinite(ev.last_mean_reward) and model._n_updates == 4
    mean, std = evaluate_policy(model, ev_env, n_eval_episodes=2, deterministic=True)
    assert np.isfinite(mean) and mean < 0
    keys = set(model.logger.last_dump) | set(model.logger.resolved())
    assert "train/std" not in keys and {"train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss"} <= keys
    assert tuple(model.rollout_buffer.actions.shape) == (8, 8, 2)
    # save / load continue identically
    path = str(tmp_path / "ppo_mcat.zip")
    model.save(path)
    loaded = PPO.load(path, env=face_env(8, (3, 5)), device=DEV)
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count > 0 and loaded._fast.multi_discrete
    obs = np.random.default_rng(0).uniform(-1, 1, (5, 4)).astype(np.float32)
    after = loaded.predict(obs, deterministic=True)[0]
    assert after.dtype == np.int64 and after.shape == (5, 2)
    np.testing.assert_array_equal(model.predict(obs, deterministic=True)[0], after)
    for other in (face_env(8, (5, 3)), face_env(8, (3, 4)), CSTRVecEnv(8, device=DEV), CSTRVecEnv(8, discrete_actions=3, device=DEV)):
        with pytest.raises(ValueError, match=r"the archive was written for MultiDiscrete\(\[3, 5\]\)"):
            PPO.load(path, env=other, device=DEV)
    box_path = str(tmp_path / "ppo_box.zip")
    PPO("MlpPolicy", CSTRVecEnv(8, device=DEV), n_steps=8, batch_size=32, device=DEV).save(box_path)
    with pytest.raises(ValueError, match="the archive was written for a Box action space"):
        PPO.load(box_path, env=face_env(8, (3, 5)), device=DEV)
    # the refusals stay
    with pytest.raises(NotImplementedError, match="hipGraph"):
        model.enable_graph_capture(True)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        PPO("MlpPolicy", VecNormalize(face_env(4, (3, 5))), device=DEV)
    for cls in (PPO, A2C):
        with pytest.raises(ValueError, match="does not support gSDE"):
            cls("MlpPolicy", env, use_sde=True, device=DEV)
    from core.common import distributed as dist_util

    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            PPO("MlpPolicy", env, device=DEV)
    finally:
        dist_util.rank_world = orig
    from core.sac import SAC
    from core.td3 import TD3

    for cls in (SAC, TD3, DQN):  # everyone else refuses the face with the reference's assertion
        with pytest.raises(AssertionError, match=r"only supports .* but MultiDiscrete\(\[3 5\]\) was provided"):
            cls("MlpPolicy", face_env(2, (3, 5)), device=DEV)


@pytest.mark.parametrize("cls_name", ["PPO", "A2C"])
def test_fused_learner_switches_mid_run(cls_name):
    from core.a2c import A2C
    from core.ppo import PPO

    cls = {"PPO": PPO, "A2C": A2C}[cls_name]
    kw = dict(n_steps=8, batch_size=32, n_epochs=1) if cls is PPO else dict(n_steps=8)
    model = cls("MlpPolicy", face_env(8, (5, 7)), seed=1, device=DEV, **kw)
    model.learn(64)
    model.fused_learner = False
    model.learn(64, reset_num_timesteps=False)
    assert not model._device_rollout() and tuple(model.rollout_buffer.actions.shape) == (8, 8, 2)
    a = model.rollout_buffer.actions.cpu().numpy()
    assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a[..., 0].max() < 5 and a[..., 1].max() < 7
    model.fused_learner = True
    model.learn(64, reset_num_timesteps=False)
    assert model._device_rollout() and model.num_timesteps == 192 and model._n_updates == 3
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())


def test_ppo_learns_on_the_multi_discrete_face():
    """The env count, step count and seed of test_categorical.test_ppo_learns_on_the_discrete_face on MultiDiscrete([5, 5]): the mean
    episode return of the rollouts improves over its first-iteration value (direction only). First run on an MI355X:
    rollout/ep_rew_mean -315.5 after the first iteration, -187.4 after the twentieth."""
    from core.ppo import PPO

    model = PPO("MlpPolicy", face_env(32, (5, 5)), n_steps=64, batch_size=512, n_epochs=4, seed=0, device=DEV)
    seen = []
    dump = model._dump_logs
    model._dump_logs = lambda it: (dump(it), seen.append(model.logger.last_dump.get("rollout/ep_rew_mean")))[0]
    model.learn(32 * 64 * 20)
    seen = [s for s in seen if s is not None]
    print(f"PPO on MultiDiscrete([5, 5]): rollout/ep_rew_mean first {seen[0]:.1f}, last {seen[-1]:.1f}")
    assert len(seen) >= 2 and np.isfinite(seen[-1]) and seen[-1] > seen[0]
