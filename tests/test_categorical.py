"""GPU checks of the Categorical head of PPO / A2C on the discrete valve face (csrc/cstr_categorical.hip).

Head (cstr_categorical_act_f32) against fp64 of logp = z - logsumexp(z): the log-prob within 4 x the error of the float32 ATen
evaluation (torch.log_softmax on the CPU) of the same inputs, per element in units of 2**-24 * M with M = |z_a| + |logsumexp z| (the
two additive terms; the unit of tests/_rowkernel_reference.py), the ATen figure measured here over all the cases; the deterministic
index exact (ties: the first; a NaN: the greatest); forced and clamped indices; the inverse CDF exact outside a 2e-5 band round the
fp64 cumulative boundaries; the drawn uniforms against the Philox counter contract; valve pairs; sentinels; repeat launches.

Loss (cstr_categorical_loss_f32) against fp64 autograd of the reference's statements (core/ppo/ppo.py:213-264, core/a2c/a2c.py:150-171
on torch's Categorical). Bar: the rtol 2e-6 / atol 1e-7 convention of tests/test_ppo.py for g_logits, g_value and the log-prob (the softmax did not make it
too tight: the worst g_logits figure over all the cases below is 0.39 of that bar, the float32 ATen autograd's figures are printed
next to the kernel's) and for the scalars; a scalar whose terms cancel (the policy loss over normalised advantages, approx_kl) and that misses it is
held to 4 x the float32 ATen autograd's figure instead, measured here over all the loss cases in units of 2**-24 M, M the magnitude
behind the scalar (check_scalars prints every such case).

Shapes: n_actions over the faces below, at and above one, two and three 64-lane chunks; ldz = n_actions and n_actions + 3; rows 1,
3, 4, 5 (one wave, a partial workgroup), 257 and 1030 (more than one pass of the loss launch's 64 x 4 rows, and of the head's 256 x 4).
The face admits squares only (n_actions = levels^2), so 65 is refused as unsupported (asserted) and 81 stands for 'just above one
chunk'.

Then the classes: teacher-forced rollouts and train() of PPO and A2C against the fixtures the unmodified reference wrote on the
Discrete(K * K) face (tools/refharness/gen_golden.py gen_ppo_discrete / gen_a2c_discrete; the reference's sampled indices are queued)
on the fused, rocBLAS and torch-statement paths with the bars of tests/test_ppo.py / tests/test_a2c.py; predict; evaluate_policy and
EvalCallback; save / load; the refusals; fused_learner switched mid-run; a learning run."""
import warnings

import numpy as np
import pytest
import torch as th

from _dqn_helpers import pair_np, philox4x32_10
from _parity_helpers import check_init, check_weights, q_err, rel_err
from _sentinel_bufs import SENT, Bufs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = (2, 3, 5, 8, 9, 10, 12, 14, 15, 16)  # M = 4, 9, 25, 64 | 81, 100 | 144 | 196, 225, 256
ROWS = (1, 3, 4, 5, 257, 1030)
CAT_STREAM_TAG = 0xCA7A11C7  # csrc/cstr_categorical.hip
U24 = 2.0 ** -24


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


def same_bits(b, snap, skip=()):
    """Bufs.same_as on the bit patterns: a NaN output (a NaN logit, A2C's one-row normalisation) must repeat as well"""
    for name, (f, _) in b.flat.items():
        if name not in skip:
            assert th.equal(f.view(th.int32), snap[name].view(th.int32)), f"{name}: the second launch differs from the first"


def logp64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    return z - lse, lse


def head_case(n, M, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, M)) * scale).astype(np.float32)


def cat_uniforms(seed, base, n):
    """u [n] as cstr_categorical_act_f32 draws them: counter (base + row, 0, tag), key = seed; word 0 >> 8 times 2^-24"""
    ctr = np.uint64(base) + np.arange(n, dtype=np.uint64)
    c = np.zeros((n, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 3] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32), CAT_STREAM_TAG
    x = philox4x32_10(c, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    return ((x[:, 0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def run_head(ops, z, K, pad=0, want=("index", "valve", "log_prob"), **kw):
    """-> dict of numpy outputs; the logits sit in a [n, M + pad] matrix whose tail columns hold 100 (never read)"""
    n, M = z.shape
    wide = np.full((n, M + pad), 100.0, np.float32)
    wide[:, :M] = z
    b = Bufs()
    idx_f = b.new("index_f32", n)
    valve = b.new("valve", n, 2) if "valve" in want else None
    logp = b.new("log_prob", n) if "log_prob" in want else None
    u_out = b.new("u_out", n) if "u_out" in want else None
    index = th.full((n + 8,), -7, dtype=th.int64, device=DEV)
    args = dict(index_out=index[:n], valve_out=valve, log_prob=logp, u_out=u_out, **kw)
    ops.categorical_act(dev(wide)[:, :M], K, idx_f, **args)
    b.check(written=list(b.flat))
    snap, first = b.snapshot(), index.clone()
    if kw.get("rng_ctl") is None:  # a drawing launch moves its stream: its repeat is checked where the stream is
        ops.categorical_act(dev(wide)[:, :M], K, idx_f, **args)
        th.cuda.synchronize()
        same_bits(b, snap)
        assert th.equal(index, first)
    assert bool((index[n:] == -7).all())
    out = dict(index=index[:n].cpu().numpy(), index_f32=idx_f.cpu().numpy())
    assert np.array_equal(out["index_f32"], out["index"].astype(np.float32))
    if valve is not None:
        out["valve"] = valve.cpu().numpy()
        assert out["valve"].tobytes() == pair_np(out["index"], K).tobytes()  # decode_valve_index's statement
    if logp is not None:
        out["log_prob"] = logp.cpu().numpy()
    if u_out is not None:
        out["u_out"] = u_out.cpu().numpy()
    return out


def logp_units(got, z, a):
    lp, lse = logp64(z)
    r = np.arange(len(a))
    mag = np.abs(np.asarray(z, np.float64)[r, a]) + np.abs(lse[:, 0])
    return np.abs(np.asarray(got, np.float64) - lp[r, a]) / (U24 * mag)


@pytest.fixture(scope="module")
def aten_logp_bar():
    """4 x the worst float32 ATen (CPU log_softmax) figure over every head case of this module, all columns"""
    worst = 0.0
    for K in LEVELS:
        for n in ROWS:
            for scale in (0.01, 1.0, 4.0):
                z = head_case(n, K * K, 7000 + 100 * K + n, scale)
                got = th.log_softmax(th.as_tensor(z), dim=1).numpy().astype(np.float64)
                lp, lse = logp64(z)
                worst = max(worst, float((np.abs(got - lp) / (U24 * (np.abs(z.astype(np.float64)) + np.abs(lse)))).max()))
    print(f"float32 ATen log_softmax against fp64: worst {worst:.3f} units; bar {4 * worst:.3f}")
    return 4.0 * worst


def test_the_face_admits_squares_only(ops):
    z = dev(np.zeros((4, 65), np.float32))
    with pytest.raises(Exception, match="code -2"):
        ops.categorical_act(z, 8, th.zeros(4, device=DEV), deterministic=True)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("K", LEVELS)
def test_head_log_prob_and_deterministic_index(ops, aten_logp_bar, K, pad):
    M = K * K
    for n in ROWS:
        for scale in (0.01, 1.0, 4.0):
            z = head_case(n, M, 7000 + 100 * K + n, scale)
            z[0, [1, M - 1]] = z[0].max() + np.float32(0.5)  # tied maxima: the first wins
            if n > 1:
                z[1, M // 2] = np.nan                            # a NaN counts as the greatest value
                z[1, M - 1] = np.nan                             # ... the first one
            if n > 2:
                z[2, :] = np.float32(0.25)                       # every logit tied: index 0
            out = run_head(ops, z, K, pad, deterministic=True)
            want = z.astype(np.float64).argmax(axis=1)           # NumPy's argmax: first maximum, a NaN is the maximum
            assert np.array_equal(out["index"], want), (n, scale)
            assert out["index"][0] == 1 and (n < 2 or out["index"][1] == M // 2) and (n < 3 or out["index"][2] == 0)
            ok = np.ones(n, bool)
            if n > 1:
                ok[1] = False
                assert np.isnan(out["log_prob"][1])
            fig = logp_units(out["log_prob"][ok], z[ok], out["index"][ok]).max()
            print(f"K={K} pad={pad} n={n} scale={scale}: log_prob {fig:.3f} units (bar {aten_logp_bar:.3f})")
            assert fig <= aten_logp_bar, (n, scale, fig)


@pytest.mark.parametrize("K", LEVELS)
def test_head_forced_indices_are_clamped(ops, aten_logp_bar, K):
    M = K * K
    for n in ROWS:
        z = head_case(n, M, 8000 + K + n)
        rng = np.random.default_rng(K * n)
        a = rng.integers(0, M, n)
        a[0] = M - 1
        if n > 2:
            a[1], a[2] = -5, M + 3  # the caller's bug: clamped into the face
        out = run_head(ops, z, K, 3, action_in=dev(a, th.int64))
        want = np.clip(a, 0, M - 1)
        assert np.array_equal(out["index"], want)
        assert logp_units(out["log_prob"], z, want).max() <= aten_logp_bar


@pytest.mark.parametrize("K", LEVELS)
def test_head_exact_uniform_cases(ops, K):
    M = K * K
    n = 5
    z = head_case(n, M, 8100 + K)
    z[1, : M // 2] = -np.inf   # p = 0 up to M / 2: u = 0 gives the first index with p > 0
    z[2, 0] = -200.0           # p underflows to 0 in f32
    out = run_head(ops, z, K, 0, u=dev(np.zeros(n, np.float32)), want=("index", "valve"))
    assert out["index"].tolist() == [0, M // 2, 1, 0, 0]
    eq = np.full((n, M), 0.75, np.float32)
    out = run_head(ops, eq, K, 3, u=dev(np.full(n, 1.0 - 2.0 ** -24, np.float32)), want=("index",))
    assert (out["index"] == M - 1).all()


@pytest.mark.parametrize("scale", [0.01, 1.0, 4.0])
@pytest.mark.parametrize("K", LEVELS)
def test_head_inverse_cdf(ops, K, scale):
    M, n = K * K, 4096
    z = head_case(n, M, 8200 + K, scale)
    u = np.random.default_rng(K).uniform(size=n).astype(np.float32)
    lp, _ = logp64(z)
    cum = np.cumsum(np.exp(lp), axis=1)
    u64 = u.astype(np.float64)[:, None]
    near = (np.abs(cum - u64) <= 2e-5).any(axis=1)  # u within 2e-5 of a boundary: either neighbour
    assert near.mean() <= 0.03, near.mean()
    want = np.minimum((cum <= u64).sum(axis=1), M - 1)
    lo = np.minimum((cum <= u64 - 2e-5).sum(axis=1), M - 1)
    hi = np.minimum((cum <= u64 + 2e-5).sum(axis=1), M - 1)
    out = run_head(ops, z, K, 3, u=dev(u), want=("index", "valve", "log_prob", "u_out"))
    got = out["index"]
    assert np.array_equal(out["u_out"], u)
    assert np.array_equal(got[~near], want[~near]), int((got[~near] != want[~near]).sum())
    assert ((got >= lo) & (got <= hi)).all()
    print(f"K={K} scale={scale}: {near.mean():.4f} of the rows near a boundary, {int((got != want).sum())} of them took the neighbour")


def test_head_draws_its_uniforms_from_philox(ops):
    K, n = 5, 1030
    M = K * K
    hi_seed = (0xABCDE << 32) | 17
    for seed, base in ((99, 0), (hi_seed, 2 ** 32 - 3)):  # the second: a 64-bit key and a counter that carries into word 1
        ctl = ops.new_rng_ctl(seed, DEV)
        ctl[1] = base
        z = head_case(n, M, 8300)
        for call in range(2):
            u = cat_uniforms(seed, base + call * n, n)
            out = run_head(ops, z, K, 0, rng_ctl=ctl, want=("index", "valve", "log_prob", "u_out"))
            assert np.array_equal(out["u_out"], u)  # element by element
            same = run_head(ops, z, K, 0, u=dev(u))
            assert np.array_equal(out["index"], same["index"]) and np.array_equal(out["log_prob"], same["log_prob"])
            assert int(ctl[1]) == base + (call + 1) * n and int(ctl[2]) == 0  # advanced by the row count; the ticket reset itself
        assert abs(float(u.mean()) - 0.5) < 0.05
    with pytest.raises(Exception, match="code -1"):
        ops.categorical_act(dev(z), K, th.zeros(n, device=DEV))  # no source
    with pytest.raises(Exception, match="code -1"):
        ops.categorical_act(dev(z), K, th.zeros(n, device=DEV), deterministic=True, rng_ctl=ctl)  # two sources


# ---- cstr_categorical_loss_f32 ------------------------------------------------------------------------------------------------------
def loss_case(B, M, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(B, M)).astype(np.float32)
    a = rng.integers(0, M, B)
    a[0] = 0
    a[-1] = M - 1
    if B > 2:
        z[1, a[1]] = 30.0  # a saturated softmax on the taken action
        z[2, (a[2] + 1) % M] = 30.0  # ... and on another one
    lp, _ = logp64(z)
    old_lp = (lp[np.arange(B), a] + rng.normal(size=B) * 0.25).astype(np.float32)  # ratios on both sides of the clip range
    f = lambda: rng.normal(size=B).astype(np.float32)  # noqa: E731
    return dict(z=z, a=a, old_lp=old_lp, values=f(), old_values=f(), adv=f(), returns=f())


def loss_torch(c, objective, dtype, norm, ent_coef, vf_coef, clip_range=0.2, clip_range_vf=None):
    """the reference's statements (ppo.py:213-264 / a2c.py:150-171) with autograd -> (scalars, g_logits, g_value, log_prob, mags).
    mags: per scalar the magnitude M behind it (the mean of the absolute additive terms, each weighted by the conditioning of its
    float32 operands: the normalised advantage (|adv| + |mean|) / den, the log-prob |z_a| + |logsumexp z|, the ratio's exponent)."""
    t = lambda x: th.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    z, values = t(c["z"]).requires_grad_(True), t(c["values"]).requires_grad_(True)
    actions = t(c["a"].astype(np.float32))
    dist = th.distributions.Categorical(logits=z)
    log_prob, entropy = dist.log_prob(actions.long().flatten()), dist.entropy()
    adv, returns = t(c["adv"]), t(c["returns"])
    with th.no_grad():
        normed = norm and len(adv) > 1
        amag = (adv.abs() + adv.mean().abs()) / (adv.std() + 1e-8) if normed else adv.abs()
        lmag = z.detach().gather(1, actions.long().reshape(-1, 1)).reshape(-1).abs() + th.logsumexp(z.detach(), dim=1).abs()
    if objective == 0:
        if norm and len(adv) > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = th.exp(log_prob - t(c["old_lp"]))
        pl1, pl2 = adv * ratio, adv * th.clamp(ratio, 1 - clip_range, 1 + clip_range)
        policy_loss = -th.min(pl1, pl2).mean()
        clip_fraction = th.mean((th.abs(ratio - 1) > clip_range).to(dtype))
        vp = values if clip_range_vf is None else t(c["old_values"]) + th.clamp(values - t(c["old_values"]), -clip_range_vf, clip_range_vf)
        value_loss = th.nn.functional.mse_loss(returns, vp)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
        lr = (log_prob - t(c["old_lp"])).detach()
        scalars = [policy_loss, value_loss, entropy_loss, loss, th.mean((th.exp(lr) - 1) - lr), clip_fraction]
        with th.no_grad():
            r = ratio.detach()
            cond = 1 + lmag + t(c["old_lp"]).abs()  # the exponent logp - old_logp carries 2**-24 of each operand into the ratio
            dr = (returns - vp).abs()
            m0 = (amag * th.maximum(r, th.clamp(r, 1 - clip_range, 1 + clip_range)) * cond).mean()
            m1 = value_loss + 2 * (dr * (returns.abs() + vp.abs())).mean()
            m4 = ((r - 1).abs() + lr.abs() + (r - 1).abs() * cond).mean()
            near = ((r - 1).abs() - clip_range).abs() < 1e-4  # a ratio on a clip bound may count either way
            mags = [m0, m1, entropy_loss.abs(), m0 + ent_coef * entropy_loss.abs() + vf_coef * m1, m4, near.to(dtype).mean()]
    else:
        if norm:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # torch.std of one element warns and gives NaN: the case under test
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        policy_loss = -(adv * log_prob).mean()
        value_loss = th.nn.functional.mse_loss(returns, values)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
        scalars = [policy_loss, value_loss, entropy_loss, loss]
        with th.no_grad():
            m0 = (amag * lmag).mean()
            m1 = value_loss + 2 * ((returns - values).abs() * (returns.abs() + values.abs())).mean()
            mags = [m0, m1, entropy_loss.abs(), m0 + ent_coef * entropy_loss.abs() + vf_coef * m1]
    loss.backward()
    return (np.array([float(s.detach()) for s in scalars]), z.grad.numpy().astype(np.float64), values.grad.numpy().astype(np.float64),
            log_prob.detach().numpy().astype(np.float64), np.array([float(m) for m in mags]))


def run_loss(ops, c, K, pad, objective, norm, ent_coef, vf_coef, clip_range=0.2, clip_range_vf=None):
    B, M = c["z"].shape
    wide = np.full((B, M + pad), 100.0, np.float32)
    wide[:, :M] = c["z"]
    ns = 6 if objective == 0 else 4
    b = Bufs()
    g_wide = b.new("g_logits", B, M + pad)
    g_value, scalars, logp = b.new("g_value", B), b.new("scalars", ns), b.new("log_prob", B)
    sums = b.put("sums", np.arange(ns, dtype=np.float32))
    ws = ops.new_ppo_workspace(DEV)
    call = lambda: ops.categorical_loss(  # noqa: E731
        objective, dev(wide)[:, :M], K, dev(c["a"].astype(np.float32)).reshape(B, 1), dev(c["values"]), dev(c["adv"]), dev(c["returns"]), norm,
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


RTOL, ATOL = 2e-6, 1e-7


def scalar_units(got, want):
    """per scalar |got - want| / (2**-24 * M), M the magnitude behind it (loss_torch), at least |want|"""
    scal, mags = want[0], want[4]
    k = min(len(scal), 5)
    return np.abs(np.asarray(got, np.float64)[:k] - scal[:k]) / (U24 * np.maximum(mags[:k], np.abs(scal[:k])))


@pytest.fixture(scope="module")
def loss_refs():
    """Every loss case once: (inputs, fp64 autograd, float32 ATen autograd) per (K, B, variant), shared by the tests; and 4 x the worst
    float32 ATen figure per scalar over all of them, in the units of scalar_units"""
    refs, worst = {}, np.zeros(5)
    for K in LEVELS:
        for B in ROWS:
            c = loss_case(B, K * K, 9000 + 10 * K + B)
            for v in VARIANTS:
                objective, norm, ent_coef, crv = v
                kw = dict(clip_range_vf=crv) if objective == 0 else {}
                with np.errstate(all="ignore"):
                    want = loss_torch(c, objective, th.float64, norm, ent_coef, 0.5, **kw)
                    aten = loss_torch(c, objective, th.float32, norm, ent_coef, 0.5, **kw)
                refs[(K, B, v)] = (c, want, aten)
                if not (objective == 1 and norm and B == 1):
                    u = scalar_units(aten[0], want)
                    worst[:len(u)] = np.maximum(worst[:len(u)], u)
    print(f"float32 ATen scalars against fp64, worst units of 2**-24 M: {np.round(worst, 3).tolist()}; bars {np.round(4 * worst, 3).tolist()}")
    return refs, 4.0 * worst


def check_scalars(got, want, tag, bars):
    """Per scalar: the project's convention |got - want| <= atol + rtol |want|, or, where a cancelling sum makes that too tight (the
    policy loss over normalised advantages, approx_kl), 4 x the float32 ATen figure in units of 2**-24 M. Which one held is printed.
    clip_fraction: exact, up to the rows whose ratio sits within 1e-4 of a clip bound."""
    scal, mags = want[0], want[4]
    units = scalar_units(got, want)
    for k in range(len(units)):
        plain = abs(got[k] - scal[k]) <= ATOL + RTOL * abs(scal[k])
        if not plain:
            print(f"{tag} scalar {k}: outside rtol / atol of |want|, {units[k]:.3f} units of 2**-24 M (bar {bars[k]:.3f})")
        assert plain or units[k] <= bars[k], (tag, k, got[k], scal[k], units[k], bars[k])
    if len(scal) > 5:
        assert abs(got[5] - scal[5]) <= mags[5] + 1e-7, (tag, got[5], scal[5])
VARIANTS = [  # (objective, normalize, ent_coef, clip_range_vf)
    (0, True, 0.0, None), (0, False, 0.01, 0.1), (0, True, 0.01, 0.1), (1, True, 0.0, None), (1, False, 0.01, None), (1, True, 0.01, None),
]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("K", LEVELS)
def test_loss_against_fp64_autograd(ops, loss_refs, K, pad):
    refs, bars = loss_refs
    for B in ROWS:
        for objective, norm, ent_coef, crv in VARIANTS:
            kw = dict(clip_range_vf=crv) if objective == 0 else {}
            c, want, aten = refs[(K, B, (objective, norm, ent_coef, crv))]
            got = run_loss(ops, c, K, pad, objective, norm, ent_coef, 0.5, **kw)
            tag = (K, pad, B, objective, norm, ent_coef, crv)
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


def test_loss_value_clip_engages(ops, loss_refs):
    """rows inside and outside the value clip range: the gradient passes on the closed interval only"""
    K, B = 3, 12
    c = loss_case(B, K * K, 77)
    c["values"] = (c["old_values"] + np.linspace(-0.3, 0.3, B).astype(np.float32)).astype(np.float32)
    want = loss_torch(c, 0, th.float64, True, 0.0, 0.5, clip_range_vf=0.1)
    got = run_loss(ops, c, K, 0, 0, True, 0.0, 0.5, clip_range_vf=0.1)
    np.testing.assert_allclose(got[2], want[2], rtol=RTOL, atol=ATOL)
    assert (got[2] == 0).sum() >= 4 and (got[2] != 0).sum() >= 2
    check_scalars(got[0], want, "value clip", loss_refs[1])


# ---- the classes against the reference's fixtures (tools/refharness/gen_golden.py gen_ppo_discrete / gen_a2c_discrete) ----------------
ROLLOUT_FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")
PATHS = ("fused", "rocblas", "torch")


def make_model(cls, g, prefix="before", **kw):
    from core.common.vec_env import CSTRVecEnv

    extra = dict(batch_size=int(g["batch_size"]), n_epochs=int(g["n_epochs"])) if "batch_size" in g else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the truncated-minibatch warning (checked in test_ppo_abi.py)
        model = cls("MlpPolicy", CSTRVecEnv(int(g["n_envs"]), discrete_actions=int(g["levels"]), device=DEV), seed=int(g["seed"]),
                    n_steps=int(g["n_steps"]), learning_rate=float(g["learning_rate"]), ent_coef=float(g["ent_coef"]),
                    policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]]), device=DEV, **extra, **kw)
    if f"{prefix}/policy/action_net.weight" in g:  # the class-default fixture keeps digests: its seeded initial weights are checked instead
        with th.no_grad():
            for k, v in model.policy.state_dict().items():
                v.copy_(th.as_tensor(g[f"{prefix}/policy/{k}"]))
    else:
        check_init(model, g, ["policy"])
    return model


def set_path(model, path, monkeypatch):
    from core.common import fused

    if path == "rocblas":  # the kernel path with every GEMM left to PyTorch-ROCm / rocBLAS (CSTR_FUSED_LINEAR=0)
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    if path == "torch":
        model.fused_learner = False
    assert model.fused_learner == (path != "torch") and not hasattr(model.policy, "log_std")


def scale_err(got, want):
    want = np.asarray(want, np.float64)
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, th.Tensor) else np.asarray(got, np.float64)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


def check_rollout(model, g, pre=""):
    rb = model.rollout_buffer
    want_a = g[f"{pre}rollout/actions"]
    assert tuple(rb.actions.shape) == want_a.shape == (int(g["n_steps"]), int(g["n_envs"]), 1) and rb.actions.dtype == th.float32
    np.testing.assert_array_equal(rb.actions.cpu().numpy(), want_a)  # the reference's shape and values: the index as a float
    np.testing.assert_array_equal(rb.episode_starts.cpu().numpy(), g[f"{pre}rollout/episode_starts"])
    for f in ("observations", "values", "log_probs", "rewards", "advantages", "returns"):
        assert scale_err(getattr(rb, f), g[f"{pre}rollout/{f}"]) < 1e-5, f


def queue_actions(model, actions, path):
    q = [th.as_tensor(a.reshape(-1).astype(np.int64)) for a in actions]
    if path == "torch":
        model.policy.action_dist.action_queue = q
    else:
        model._fast.action_queue = q
    return q


@pytest.mark.parametrize("path", PATHS)
def test_ppo_rollout_teacher_forced(golden, path, monkeypatch):
    """collect_rollouts against the reference's rollout: the `before/` weights, the initial observations and step counters injected
    after _setup_learn's reset, the reference's sampled indices queued. The kernel paths roll out on the device."""
    from core.ppo import PPO

    g = golden("ppo_cat_train_kat_small.npz")
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


def check_ppo_train(model, g, path):
    """the bars of tests/test_ppo.py::check_train"""
    label = {"fused": "ppo_fused", "rocblas": "ppo_rocblas", "torch": "ppo_aten"}[path]
    assert len(model.last_train_minibatches) == int(g["n_minibatches"])
    for k, cap in enumerate(model.last_train_minibatches):
        want_v, want_lp, want_s = g[f"mb{k}/values"], g[f"mb{k}/log_prob"], g[f"mb{k}/scalars"].astype(np.float64)
        assert cap["values"].shape[0] == want_v.shape[0]
        assert rel_err(cap["values"].cpu().numpy(), want_v, float(np.abs(want_v).mean())) < 1e-5, (k, "values")
        assert q_err(cap["log_prob"].cpu().numpy(), want_lp, label) < 1e-5, (k, "log_prob")
        got = cap["scalars"].cpu().numpy().astype(np.float64)
        floors = (1.0, max(want_s[1], 1.0), max(abs(want_s[2]), 1.0), max(abs(want_s[3]), 1.0))
        for i, fl in enumerate(floors):
            assert abs(got[i] - want_s[i]) <= 1e-5 * max(abs(want_s[i]), fl), (k, i, got[i], want_s[i])
        assert abs(got[4] - want_s[4]) <= 1e-5 * abs(want_s[4]) + 2.4e-7, (k, got[4], want_s[4])
        assert got[5] == want_s[5], (k, "clip_fraction")
        assert rel_err(cap["grad_norm"].cpu().numpy(), g[f"mb{k}/grad_norm"]) < 5e-5, (k, "grad_norm")
    assert model._n_updates == int(g["n_updates"]) and model.policy.optimizer.step_count == int(g["optimizer_steps"])
    check_weights(model, g, "after", ["policy"])
    logged = model.logger.resolved()
    want = dict(zip([str(k) for k in g["logged_keys"]], g["logged_values"]))
    assert "train/std" not in want and "train/std" not in logged  # no log_std, as in the reference
    for key in ("train/entropy_loss", "train/policy_gradient_loss", "train/value_loss", "train/clip_fraction", "train/loss",
                "train/explained_variance", "train/n_updates", "train/clip_range", "train/learning_rate"):
        assert abs(float(logged[key]) - want[key]) <= 1e-5 * max(abs(want[key]), 1.0), (key, logged[key], want[key])
    assert abs(float(logged["train/approx_kl"]) - want["train/approx_kl"]) <= 1e-5 * abs(want["train/approx_kl"]) + 2.4e-7
    assert set(want) <= set(logged), set(want) - set(logged)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["small", "default"])
def test_ppo_train_teacher_forced(golden, name, path, monkeypatch):
    from core.common.buffers import RolloutBuffer
    from core.ppo import PPO

    g = golden(f"ppo_cat_train_kat_{name}.npz")
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
    """rollout (indices queued) and train(), twice, against a2c_cat_train_kat_small.npz with the bars of tests/test_a2c.py"""
    from core.a2c import A2C

    g = golden("a2c_cat_train_kat_small.npz")
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

    g, small = golden("ppo_cat_predict_kat.npz"), golden("ppo_cat_train_kat_small.npz")
    model = make_model(PPO, {**{k: small[k] for k in small.files}, **{f"before/policy/{k[7:]}": g[k] for k in g.files if k.startswith("policy/")}})
    act, state = model.predict(g["obs"], deterministic=True)
    assert state is None and act.shape == (16,) and act.dtype == np.int64
    np.testing.assert_array_equal(act, g["deterministic"])
    one, _ = model.predict(g["obs"][3], deterministic=True)
    assert one.shape == () and int(one) == int(g["deterministic"][3])
    with th.no_grad():
        logits = model._fast.logits(dev(g["obs"]))
        values = model.policy.predict_values(dev(g["obs"]))
        a, v, lp = model.policy(dev(g["obs"]), deterministic=True)
    assert scale_err(logits, g["logits"]) < 1e-5 and values.shape == (16, 1) and q_err(values.cpu().numpy(), g["values"], "ppo_fused") < 1e-5
    assert a.dtype == th.int64 and tuple(a.shape) == (16,) and tuple(v.shape) == (16, 1) and tuple(lp.shape) == (16,)
    a1 = np.stack([model.predict(g["obs"], deterministic=False)[0] for _ in range(8)])  # unforced: the Philox stream
    assert a1.dtype == np.int64 and a1.min() >= 0 and a1.max() < 9 and len(np.unique(a1, axis=0)) > 1
    model.fused_learner = False  # the torch statements: argmax(probs)
    np.testing.assert_array_equal(model.predict(g["obs"], deterministic=True)[0], g["deterministic"])


def test_evaluation_callbacks_save_load_and_refusals(golden, tmp_path):
    from core.a2c import A2C
    from core.common import evaluation
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv, VecNormalize
    from core.ppo import PPO

    env = CSTRVecEnv(8, discrete_actions=3, device=DEV)
    model = PPO("MlpPolicy", env, n_steps=8, batch_size=32, n_epochs=2, seed=3, device=DEV)
    assert model.fused_learner and model._device_rollout() and model._fast.discrete and model._fast.levels == 3
    ev_env = CSTRVecEnv(2, discrete_actions=3, device=DEV)
    assert not evaluation.supported(model, ev_env)
    with pytest.raises(Exception):
        evaluation.evaluate_policy_fused(model, ev_env, n_eval_episodes=2)
    ev = EvalCallback(ev_env, n_eval_episodes=2, eval_freq=8, verbose=0, warn=False)  # fused=None: falls back to the loop
    model.learn(8 * 8 * 2, callback=ev)
    assert ev.n_calls == 16 and np.isfinite(ev.last_mean_reward) and model._n_updates == 4
    mean, std = evaluate_policy(model, ev_env, n_eval_episodes=2, deterministic=True)
    assert np.isfinite(mean) and mean < 0
    keys = set(model.logger.last_dump) | set(model.logger.resolved())
    assert "train/std" not in keys and {"train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss"} <= keys
    # save / load continue identically
    path = str(tmp_path / "ppo_cat.zip")
    model.save(path)
    loaded = PPO.load(path, env=CSTRVecEnv(8, discrete_actions=3, device=DEV), device=DEV)
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count > 0 and loaded._fast.discrete
    obs = np.random.default_rng(0).uniform(-1, 1, (5, 4)).astype(np.float32)
    np.testing.assert_array_equal(model.predict(obs, deterministic=True)[0], loaded.predict(obs, deterministic=True)[0])
    with pytest.raises(ValueError, match="discrete_actions"):
        PPO.load(path, env=CSTRVecEnv(8, discrete_actions=4, device=DEV), device=DEV)
    with pytest.raises(ValueError, match="discrete_actions"):
        PPO.load(path, env=CSTRVecEnv(8, device=DEV), device=DEV)
    # the refusals stay
    with pytest.raises(NotImplementedError, match="hipGraph"):
        model.enable_graph_capture(True)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        PPO("MlpPolicy", VecNormalize(CSTRVecEnv(4, discrete_actions=3, device=DEV)), device=DEV)
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

    for cls in (SAC, TD3):  # the continuous-action classes keep refusing the discrete face
        with pytest.raises(AssertionError, match="only supports"):
            cls("MlpPolicy", CSTRVecEnv(2, discrete_actions=3, device=DEV), device=DEV)


@pytest.mark.parametrize("cls_name", ["PPO", "A2C"])
def test_fused_learner_switches_mid_run(cls_name):
    from core.a2c import A2C
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    cls = {"PPO": PPO, "A2C": A2C}[cls_name]
    kw = dict(n_steps=8, batch_size=32, n_epochs=1) if cls is PPO else dict(n_steps=8)
    model = cls("MlpPolicy", CSTRVecEnv(8, discrete_actions=5, device=DEV), seed=1, device=DEV, **kw)
    model.learn(64)
    model.fused_learner = False
    model.learn(64, reset_num_timesteps=False)
    assert not model._device_rollout() and tuple(model.rollout_buffer.actions.shape) == (8, 8, 1)
    a = model.rollout_buffer.actions.cpu().numpy()
    assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() < 25
    model.fused_learner = True
    model.learn(64, reset_num_timesteps=False)
    assert model._device_rollout() and model.num_timesteps == 192 and model._n_updates == 3
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())


def test_ppo_learns_on_the_discrete_face():
    """The env, step count and seed of tests/test_ppo.py::test_it_learns on the Discrete(25) face: the mean episode return of the
    rollouts improves over its first-iteration value (direction only). First run on an MI355X: rollout/ep_rew_mean -312.9 after the
    first iteration, -294.2 after the twentieth."""
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    model = PPO("MlpPolicy", CSTRVecEnv(32, discrete_actions=5, device=DEV), n_steps=64, batch_size=512, n_epochs=4, seed=0, device=DEV)
    seen = []
    dump = model._dump_logs
    model._dump_logs = lambda it: (dump(it), seen.append(model.logger.last_dump.get("rollout/ep_rew_mean")))[0]
    model.learn(32 * 64 * 20)
    seen = [s for s in seen if s is not None]
    print(f"PPO on Discrete(25): rollout/ep_rew_mean first {seen[0]:.1f}, last {seen[-1]:.1f}")
    assert len(seen) >= 2 and np.isfinite(seen[-1]) and seen[-1] > seen[0]
