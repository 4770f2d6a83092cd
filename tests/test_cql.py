"""CQL on the HIP learner (core/cql, csrc/cstr_cql.hip) against the fp64 statements of tests/_cql_reference.py.

The candidate launch with given noise: actions and log-probs bit-equal to the SAC head launch (cstr_gaussian_head_fwd_f32) on the same
(mean, raw, eps), uniform rows bit-equal to u, observation columns bit-equal; drawn noise element by element against the counter contract
(uniforms exact; normals through tanh at sd = 0.25 within 0.25 x (the Box-Muller bar of tests/_rowkernel_reference.py + the element's
float32 u1 slack) + 2^-22).
The loss launch against fp64: target bit-equal to the twin TD head; every element of gq and every scalar within
max(4 x the distance of the float32 torch statement (CPU ATen, the same inputs) from fp64 FOR THAT ELEMENT, 2 float32 ulp + the element's
conditioning). The conditioning (tests/_cql_reference.py gq_floor, derived there rounding by rounding) is what float32 arithmetic can move
the element by whatever evaluates it -- exp(z - m) turns the roundings of z = (q - corr) / T and of z - m into relative error, and a data
row's q - t cancels: a single element's ATen distance can be zero by luck, and no float32 evaluation can promise 4 x zero there.
Teacher-forced learning: Q values and targets through `q_err`, scalars through `rel_err`, weights within 2e-5 of the tensor's scale + 1e-4
relative (tests/_parity_helpers.py); candidate actions (tanh outputs) within 2e-5, log-probs at the Q bar plus the float32 conditioning
of the tanh correction (printed as a share of that bar).

Measured on MI355X: over the 48 cases of the loss tests the worst element-wise error / bar is 0.33 (without the conditioning term it
would be 12.9, at elements whose ATen distance happens to be next to nothing); the worst element in ulps is printed beside ATen's (both
up to 2050 ulp of the smallest softmax shares at B 256 / N 21 / T 0.5); the scalars within 2.4 ulp. Teacher-forced: Q values and targets within 1.3e-7 of their scale on every path, candidate actions within 1.5e-7, log-probs
at most 0.16 of their bar, weights at most 0.22 of theirs after the two steps. mean(lse - Q(s,a)) 3.973 after w = 0 and -0.222 after
w = 5; behaviour cloning error 0.024 after learn(1000) from 0.409. Launches and times: profiles/cql_probe.txt (tools/cql_probe.py)."""
import numpy as np
import pytest
import torch as th

import _cql_reference as ref
from _parity_helpers import q_err, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]

DEV = "cuda"
SENT = float(np.float32(12345.678))
PAD = 64
MODS = ["actor", "critic", "critic_target"]


def _env(n=1, **kw):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n, **kw)


def _spaces():
    from core.common.spaces import Box

    return Box(-1, 1, (4,)), Box(-1, 1, (2,))


def _out(*shape):
    """a sentinel-filled output with 64 sentinel floats in front of it and behind it -> (whole buffer, the output view)"""
    n = int(np.prod(shape))
    f = th.full((n + 2 * PAD,), SENT, dtype=th.float32, device=DEV)
    return f, f[PAD:PAD + n].view(*shape)


def _pads_clean(f) -> bool:
    return bool((f[:PAD] == SENT).all()) and bool((f[-PAD:] == SENT).all())


def _strided(a: np.ndarray, ld: int):
    """[R, W] values as the first W columns of rows ld floats wide (the rest sentinels)"""
    R, W = a.shape
    t = th.full((R, ld), SENT, dtype=th.float32, device=DEV)
    t[:, :W] = th.as_tensor(a)
    return t, t[:, :W]


def _d(a):
    return th.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(th.int32)


# ------------------------------------------------------------------------------------ the candidate launch
CAND_SHAPES = [(1, 1, 1, 0, 0), (3, 2, 2, 0, 3), (65, 10, 2, 2, 0), (256, 21, 4, 1, 5), (256, 10, 2, 0, 0), (3, 21, 1, 4, 1), (65, 1, 4, 0, 2)]


def _cand_inputs(B, N, A, seed, D=4):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    pc = np.concatenate([rng.normal(0, 0.8, (B, A)), rng.normal(-1, 1.0, (B, A))], 1).astype(np.float32)
    pn = np.concatenate([rng.normal(0, 0.8, (B, A)), rng.normal(-1, 1.0, (B, A))], 1).astype(np.float32)
    if B >= 3:  # raw log_std beyond both clamp bounds
        pc[0, A:], pc[1, A:], pn[2, A:] = 5.0, -30.0, 2.5
    u = (rng.integers(0, 1 << 24, (B, N, A)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0))
    eps = rng.normal(0, 1, (B, 2 * N, A)).astype(np.float32)
    return obs, pc, pn, u, eps


@pytest.mark.parametrize("B,N,A,xpad,ppad", CAND_SHAPES)
def test_candidates_given_noise_bit_for_bit(B, N, A, xpad, ppad):
    from core.common import hip_ops

    D = 4
    obs, pc, pn, u, eps = _cand_inputs(B, N, A, seed=B + N + A)
    if B >= 3:
        eps[1] = 0.0  # eps = 0: the mode
    _, obs_d = _strided(obs, D + 2)
    pfull, pc_d = _strided(pc, 2 * A + ppad)
    _, pn_d = _strided(pn, 2 * A + ppad)
    rows = B * 3 * N
    xfull = th.full((rows * (D + A + xpad) + 2 * PAD,), SENT, dtype=th.float32, device=DEV)
    x = xfull[PAD:PAD + rows * (D + A + xpad)].view(rows, D + A + xpad)[:, :D + A]
    fc, corr = _out(B, 3 * N)
    hip_ops.cql_candidates(obs_d, pc_d, pn_d, N, x, corr, u=_d(u), eps=_d(eps))
    th.cuda.synchronize()
    xr = x.reshape(B, 3 * N, D + A) if xpad == 0 else x.contiguous().reshape(B, 3 * N, D + A)
    assert th.equal(_bits(xr[:, :, :D]), _bits(_d(obs)[:, None, :].expand(B, 3 * N, D)))  # every row carries the CURRENT observation
    assert th.equal(_bits(xr[:, :N, D:]), _bits(_d(u)))
    assert th.equal(corr[:, :N], th.full((B, N), hip_ops.cql_log_unif(A), device=DEV))
    assert hip_ops.cql_log_unif(A) == float(np.float32(A) * np.log(np.float32(0.5)))
    # the SAC head launch on the same (mean, raw, eps), one row per (state, sample)
    for kind, p in ((0, pc), (1, pn)):
        par = _d(np.repeat(p[:, None, :], N, axis=1).reshape(B * N, 2 * A))
        e = _d(eps[:, kind * N:(kind + 1) * N].reshape(B * N, A))
        act, lp = th.empty(B * N, A, device=DEV), th.empty(B * N, device=DEV)
        hip_ops.gaussian_head_fwd_(par, None, e, None, act, lp)
        sl = slice((1 + kind) * N, (2 + kind) * N)
        assert th.equal(_bits(xr[:, sl, D:]), _bits(act.view(B, N, A))), kind
        assert th.equal(_bits(corr[:, sl]), _bits(lp.view(B, N))), kind
    if B >= 3:  # the mode, and finite log-probs at the clamp bounds
        np.testing.assert_allclose(xr[1, N:2 * N, D:].cpu().numpy(), np.repeat(np.tanh(pc[1:2, :A].astype(np.float64)), N, 0), atol=2e-7)
        assert bool(th.isfinite(corr).all())
    # against fp64 (layout, signs)
    xw, cw = ref.candidates(obs, pc, pn, u, eps)
    assert np.abs(xr.cpu().numpy().reshape(rows, -1) - xw).max() < 2e-6
    # log-probs against fp64 where float32 can state them: not at a saturated tanh (log(1 - a^2 + 1e-6)) and not in the states whose raw
    # log_std sits beyond a clamp bound (sd = exp(-20): u - mean is one float32 ulp of the mean or nothing)
    ok = np.abs(xw[:, D:]).max(axis=1).reshape(B, 3 * N) < 0.999
    ok[:3] = ok[:3] & (B < 3)
    if ok.any():
        assert np.abs(corr.cpu().numpy() - cw)[ok].max() < 2e-4 * max(1.0, np.abs(cw[ok]).max())
    # nothing outside the outputs, the row padding included; relaunch bit-identical
    assert _pads_clean(fc) and _pads_clean(xfull)
    if xpad:
        assert bool((xfull[PAD:PAD + rows * (D + A + xpad)].view(rows, -1)[:, D + A:] == SENT).all())
    assert bool((pfull[:, 2 * A:] == SENT).all())
    snap = (xfull.clone(), fc.clone())
    hip_ops.cql_candidates(obs_d, pc_d, pn_d, N, x, corr, u=_d(u), eps=_d(eps))
    th.cuda.synchronize()
    assert th.equal(_bits(xfull), _bits(snap[0])) and th.equal(_bits(fc), _bits(snap[1]))
    # corr = NULL
    x2full = xfull.clone().fill_(SENT)
    x2 = x2full[PAD:PAD + rows * (D + A + xpad)].view(rows, D + A + xpad)[:, :D + A]
    hip_ops.cql_candidates(obs_d, pc_d, pn_d, N, x2, None, u=_d(u), eps=_d(eps))
    th.cuda.synchronize()
    assert th.equal(_bits(x2full), _bits(xfull))


@pytest.mark.parametrize("B,N,A,seed,base", [(3, 2, 2, 41, 0), (65, 10, 2, ref.CQL_TAG, 2 ** 32 - 3), (7, 21, 3, (0xABCDE << 32) | 17, 5),
                                             (256, 4, 4, 7, 2 ** 32 - 200), (5, 1, 1, 3, 1)])
def test_candidates_drawn_noise_follows_the_counter_contract(B, N, A, seed, base):
    """mean 0, raw log 0.25: action = tanh(0.25 eps), |0.25 eps| < 1.5, so the draw shows through the action. A counter that carries
    into word 1 inside the launch, a seed above 2^32, and a second launch that continues the stream."""
    import _rowkernel_reference as rk
    from core.common import hip_ops

    D, sd = 4, 0.25
    obs = np.random.default_rng(0).uniform(-1, 1, (B, D)).astype(np.float32)
    p = np.concatenate([np.zeros((B, A)), np.full((B, A), np.log(sd))], 1).astype(np.float32)
    ctl = hip_ops.new_rng_ctl(seed, DEV)
    ctl[1] = base
    seed_used = int(ctl[0])
    assert seed_used == seed & 0x7FFFFFFFFFFFFFFF
    sd32 = float(np.exp(np.float32(np.log(sd))))
    for launch in range(2):
        start = base + launch * B * N
        fx, x = _out(B * 3 * N, D + A)
        fc, corr = _out(B, 3 * N)
        hip_ops.cql_candidates(_d(obs), _d(p), _d(p), N, x, corr, rng_ctl=ctl)
        th.cuda.synchronize()
        assert int(ctl[1]) == start + B * N and int(ctl[2]) == 0 and int(ctl[0]) == seed_used  # the ticket resets itself
        xr = x.view(B, 3 * N, D + A).cpu().numpy()
        assert np.array_equal(xr[:, :N, D:].view(np.uint32), ref.cql_uniforms(seed_used, start, B, N, A).view(np.uint32))
        eps, slack = ref.cql_normals(seed_used, start, B, N, A), ref.cql_normal_slack(seed_used, start, B, N, A)
        err = np.abs(xr[:, N:, D:].astype(np.float64) - np.tanh(sd32 * eps))
        bar = sd32 * (rk.NORMAL_BAR + slack) + 2.0 ** -22
        assert (err <= bar).all(), (launch, float((err / bar).max()))
        _, lp = ref.squashed_sample(0.0, np.log(sd32), eps)
        assert np.abs(corr.cpu().numpy()[:, N:] - lp).max() < 1e-3 + 8 * slack.max()
        assert _pads_clean(fx) and _pads_clean(fc)
    # the same control words again: the same bits
    ctl2 = hip_ops.new_rng_ctl(seed, DEV)
    ctl2[1] = base + B * N
    _, x2 = _out(B * 3 * N, D + A)
    hip_ops.cql_candidates(_d(obs), _d(p), _d(p), N, x2, None, rng_ctl=ctl2)
    th.cuda.synchronize()
    assert th.equal(_bits(x2), _bits(x))


# ------------------------------------------------------------------------------------ the loss launch
def _loss_inputs(B, N, seed, mode="plain", T=1.0):
    rng = np.random.default_rng(seed)
    M = (1 + 3 * N) * B
    q = rng.normal(-3, 1.5, (2, M)).astype(np.float32)
    corr = np.concatenate([np.full((B, N), 2 * np.log(0.5)), rng.normal(1.0, 1.5, (B, 2 * N))], 1).astype(np.float32)
    if mode == "overflow":  # exp(c / T) overflows float32 without the maximum subtraction
        q[:, B:] = rng.normal(300, 60, (2, M - B)).astype(np.float32)
    if mode == "equal":
        q[:, B:] = np.float32(-1.25)
        corr[:] = np.float32(0.5)
    if mode == "nan":
        q[0, B + (3 * N) * (B // 2) + N // 2] = np.nan
    f = lambda lo, hi: rng.uniform(lo, hi, B).astype(np.float32)  # noqa: E731
    return dict(q=q, corr=corr, q1_t=f(-6, 0), q2_t=f(-6, 0), next_logp=f(-3, 2), rew=f(-8, 0), done=(rng.uniform(size=B) < 0.2).astype(np.float32),
                ent_coef=np.float32(0.37), gamma=0.99)


def _run_loss(inp, importance, backup, w, T, pads=False):
    from core.common import hip_ops

    B = inp["rew"].shape[0]
    M = inp["q"].shape[1]
    bufs = {k: _out(*s) for k, s in dict(target=(B, 1), gq=(2, M, 1), loss=(1,), lsum=(1,), aux=(4,)).items()}
    bufs["lsum"][1].fill_(1.5)
    hip_ops.cql_q_loss(_d(inp["q"]).view(2, M, 1), _d(inp["corr"]) if importance else None, not importance, _d(inp["q1_t"]), _d(inp["q2_t"]),
                       _d(inp["next_logp"]) if backup else None, _d(inp["rew"]), _d(inp["done"]), _d([inp["ent_coef"]]), inp["gamma"], w, T,
                       bufs["target"][1], bufs["gq"][1], bufs["loss"][1], bufs["lsum"][1], bufs["aux"][1])
    th.cuda.synchronize()
    assert all(_pads_clean(f) for f, _ in bufs.values())
    return {k: v.clone() for k, (_, v) in bufs.items()}


def _ref_args(inp, importance, backup, w, T):
    return (inp["q"], inp["corr"] if importance else None, not importance, inp["q1_t"], inp["q2_t"], inp["next_logp"] if backup else None,
            inp["rew"], inp["done"], inp["ent_coef"], inp["gamma"], w, T)


def _check_loss(got, inp, importance, backup, w, T, label):
    args = _ref_args(inp, importance, backup, w, T)
    want, aten = ref.q_loss_f64(*args), ref.q_loss_torch(*args, dtype=th.float32)
    M = inp["q"].shape[1]
    floor = ref.gq_floor(*args)
    outs = dict(gq=(got["gq"].cpu().numpy().reshape(2, M), want["gq"], aten["gq"]), aux=(got["aux"].cpu().numpy(), want["aux"], aten["aux"]),
                loss=(got["loss"].cpu().numpy(), np.array([want["loss"]]), np.array([aten["loss"]])))
    line = []
    for k, (g, w_, a) in outs.items():
        if k == "aux":  # four scalars: each its own bar
            figs = [(ref.worst_ulps(g[i], w_[i]), ref.worst_ulps(a[i], w_[i])) for i in range(4)]
            assert all(fg <= max(4 * fa, 2.0) for fg, fa in figs), (label, k, figs)
            line.append("aux " + "/".join(f"{fg:.1f}({fa:.1f})" for fg, fa in figs))
            continue
        fg, fa = ref.worst_ulps(g, w_), ref.worst_ulps(a, w_)
        ratio = ref.close(g, w_, a, floor=floor if k == "gq" else None)  # element by element; the loss: 4 x ATen, floor 2 ulp
        line.append(f"{k} worst element-wise error / bar {ratio:.2f} (worst element {fg:.1f} ulp, ATen's {fa:.1f})")
        assert ratio <= 1.0, (label, k, ratio, fg, fa)
    print(f"{label}: " + "; ".join(line))
    assert abs(float(got["lsum"]) - (1.5 + float(got["loss"]))) <= 2 * np.spacing(np.float32(abs(1.5 + float(got["loss"])))) or np.isnan(want["loss"])
    return want


@pytest.mark.parametrize("importance", [True, False])
@pytest.mark.parametrize("B,N", [(1, 1), (3, 2), (65, 10), (256, 21), (256, 10), (3, 21), (65, 1)])
def test_q_loss_against_fp64(B, N, importance):
    from core.common import hip_ops

    for backup, T, w in ((False, 1.0, 5.0), (True, 0.5, 5.0), (False, 10.0, 0.7)):
        inp = _loss_inputs(B, N, seed=B * 31 + N)
        got = _run_loss(inp, importance, backup, w, T)
        _check_loss(got, inp, importance, backup, w, T, f"B{B} N{N} imp={importance} backup={backup} T={T} w={w}")
        # the TD target: the twin TD head's bits on the same inputs
        tq, g1, g2 = (th.empty(B, 1, device=DEV) for _ in range(3))
        hip_ops.td_twin_q_loss(_d(inp["q1_t"]), _d(inp["q2_t"]), _d(inp["next_logp"]) if backup else None, _d(inp["rew"]), _d(inp["done"]),
                               _d([inp["ent_coef"]]), inp["gamma"], _d(inp["q"][0, :B]), _d(inp["q"][1, :B]), 0.5, tq, g1, g2)
        assert th.equal(_bits(got["target"]), _bits(tq))
        # relaunch: the same bits
        again = _run_loss(inp, importance, backup, w, T)
        assert all(th.equal(_bits(got[k]), _bits(again[k])) for k in got)
    # w = 0: exact zeros on the candidate rows, the twin TD head's gradient bits on the data rows
    got0 = _run_loss(inp, importance, False, 0.0, 1.0)
    tq, g1, g2 = (th.empty(B, 1, device=DEV) for _ in range(3))
    hip_ops.td_twin_q_loss(_d(inp["q1_t"]), _d(inp["q2_t"]), None, _d(inp["rew"]), _d(inp["done"]), None, inp["gamma"], _d(inp["q"][0, :B]),
                           _d(inp["q"][1, :B]), 0.5, tq, g1, g2)
    assert bool((got0["gq"][:, B:] == 0).all()) and th.equal(_bits(got0["gq"][0, :B]), _bits(g1)) and th.equal(_bits(got0["gq"][1, :B]), _bits(g2))
    assert th.equal(_bits(got0["target"]), _bits(tq)) and float(got0["aux"][1]) == 0.0


@pytest.mark.parametrize("importance", [True, False])
@pytest.mark.parametrize("mode", ["overflow", "equal", "nan"])
def test_q_loss_edge_values(mode, importance):
    B, N, w, T = 65, 10, 5.0, 0.5 if mode == "overflow" else 1.0
    inp = _loss_inputs(B, N, seed=11, mode=mode, T=T)
    got = _run_loss(inp, importance, False, w, T)
    want = _check_loss(got, inp, importance, False, w, T, f"{mode} imp={importance}")
    gq = got["gq"].cpu().numpy().reshape(2, -1)
    if mode == "overflow":
        assert np.isfinite(gq).all() and np.isfinite(float(got["loss"])) and float(got["aux"][2]) > 88.0 * T
    if mode == "equal" and importance:  # softmax exactly 1 / (3N) up to rounding
        share = gq[:, B:].astype(np.float64) / float(np.float32(0.5 * w) / np.float32(B))  # the launch's float32 (0.5 w) / B
        assert np.abs(share - 1.0 / (3 * N)).max() <= 2 * np.spacing(np.float32(1.0 / (3 * N)))
    if mode == "nan":
        b = B // 2
        rows = slice(B + 3 * N * b, B + 3 * N * (b + 1))
        assert np.isnan(gq[0, rows]).all() and np.isnan(float(got["loss"])) and np.isnan(want["loss"])
        other = np.ones(gq.shape[1], bool)
        other[rows] = False
        other[b] = importance  # the data row takes a share of the softmax only with the appended entry
        assert np.isfinite(gq[0, other]).all() and np.isfinite(gq[1]).all()


# ------------------------------------------------------------------------------------ datasets and models
def _raw_dataset(rows=2048, seed=3):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (rows, 4)).astype(np.float32)
    nobs = np.clip(obs + rng.normal(0, 0.05, obs.shape), -1, 1).astype(np.float32)
    act = rng.uniform(-1, 1, (rows, 2)).astype(np.float32)
    rew = rng.uniform(-8, 0, rows).astype(np.float32)
    done = (rng.uniform(size=rows) < 0.1).astype(np.float32)
    return dict(observations=obs, next_observations=nobs, actions=act, rewards=rew, dones=done)


def _buffer(raw, sampler_seed=5):
    from core.common.buffers import ReplayBuffer

    rows = raw["rewards"].shape[0]
    rb = ReplayBuffer(rows, *_spaces(), device=DEV, n_envs=1)
    rb.observations.copy_(th.as_tensor(raw["observations"]).reshape(rows, 1, 4))
    rb.next_observations.copy_(th.as_tensor(raw["next_observations"]).reshape(rows, 1, 4))
    rb.actions.copy_(th.as_tensor(raw["actions"]).reshape(rows, 1, 2))
    rb.rewards.copy_(th.as_tensor(raw["rewards"]).reshape(rows, 1))
    rb.dones.copy_(th.as_tensor(raw["dones"]).reshape(rows, 1))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    if sampler_seed is not None:
        rb.seed_sampler(sampler_seed)
    return rb


def _fields(rb):
    return [getattr(rb, k).clone() for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")] + [rb.ring.ctl.clone()]


def _model(raw=None, arch=(64, 64), B=64, seed=0, **kw):
    from core.cql import CQL

    raw = _raw_dataset() if raw is None else raw
    pk = dict(kw.pop("policy_kwargs", {}))
    if arch is not None:
        pk.setdefault("net_arch", list(arch))
    model = CQL("MlpPolicy", _env(), dataset=_buffer(raw), seed=seed, batch_size=B, policy_kwargs=pk, **kw)
    model.replay_buffer.seed_sampler(5)
    return model


def _select_path(monkeypatch, model, path):
    from core.common import fused

    assert model.fused_learner
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    if path == "aten":
        model.fused_learner = False


def _ref_policy(model, arch):
    from core.sac.policies import SACPolicy

    pk = {} if arch is None else dict(net_arch=list(arch))
    p = SACPolicy(*_spaces(), lambda _: 3e-4, **pk)
    p.load_state_dict({k: v.detach().cpu() for k, v in model.policy.state_dict().items()})
    return p.double()


@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("tag", ["small", "default"])
def test_cql_teacher_forced(tag, path, monkeypatch):
    """Two steps against the fp64 reference, from the seeded initial weights with ONE change made to the model and the reference alike:
    the output biases of the critics and their targets start at the dataset's mean reward (about -4) instead of 0. The bars of
    tests/_parity_helpers.py are relative, per element: |dq| <= 5e-5 max(|q|, 1e-3). An untrained critic gives Q = 0 +- 0.1 as a sum of
    256 terms of that size, so an element with |q| < 1e-3 asks for 5e-8 where float32 resolves 1e-7: the float32 torch statement itself
    (torch.optim.Adam, CPU ATen, tests/_cql_reference.py RefCQL in float32 against float64, class defaults, three seeds) is at 1.1e-4
    and 1.3e-4 of that bar at the second step whenever the batch holds such an element, and at 2.7e-5 when it does not. With Q at the
    scale of the rewards the same evaluation is at 7e-8, and the bar measures the step instead of the distance of a Q value from zero.
    Weights, losses and the four scalars do not depend on that choice. Measured on MI355X: the printed lines."""
    arch, B, N = ((64, 64), 64, 2) if tag == "small" else (None, 256, 10)
    raw = _raw_dataset()
    model = _model(raw, arch=arch, B=B, cql_n_actions=N)
    with th.no_grad():
        for critic in (model.critic, model.critic_target):
            for qnet in critic.q_networks:
                qnet[-1].bias.fill_(float(raw["rewards"].mean()))
    _select_path(monkeypatch, model, path)
    assert (model.conservative_weight, model.cql_temp, model.tau, model.gamma, model.lr_schedule(1)) == (5.0, 1.0, 0.005, 0.99, 3e-4)
    assert model.target_entropy == -2.0 and float(model.log_ent_coef.detach()) == 0.0
    refm = ref.RefCQL(_ref_policy(model, arch), 3e-4, model.gamma, model.tau, 5.0, N, 1.0, target_entropy=-2.0)
    index = {a.tobytes(): i for i, a in enumerate(raw["actions"])}
    model.debug_capture = True
    gen = th.Generator().manual_seed(11)
    lab = f"cql_{tag}_{path}"
    rs = np.random.RandomState(5)  # the sampler's stream (seed_sampler(5)): every path draws NumPy's indices, so the same batches
    for k in range(2):
        eps_pi, eps_next = th.randn(B, 2, generator=gen), th.randn(B, 2, generator=gen)
        u, eps = th.rand(B, N, 2, generator=gen) * 2 - 1, th.randn(B, 2 * N, 2, generator=gen)
        model.actor.action_dist.eps_queue = [eps_pi.clone(), eps_next.clone()]
        model.cql_noise_queue = [(u.clone(), eps.clone())]
        model.train(gradient_steps=1, batch_size=B)
        assert not model.cql_noise_queue and not model.actor.action_dist.eps_queue
        b = model._static_batch
        acts = b.actions.cpu().numpy()
        idx = np.array([index[r.tobytes()] for r in acts])
        batch = [getattr(b, n).cpu().numpy().copy() for n in ("observations", "actions", "next_observations", "rewards", "dones")]
        # bit-equal across paths: each path's batch is the dataset's rows at the indices NumPy's stream gives, bit for bit
        want_idx = rs.randint(0, raw["rewards"].shape[0], size=B)
        rs.randint(0, 1, size=B)
        np.testing.assert_array_equal(idx, want_idx)
        for got_f, name in zip(batch, ("observations", "actions", "next_observations", "rewards", "dones")):
            np.testing.assert_array_equal(got_f.reshape(B, -1), raw[name][idx].reshape(B, -1), err_msg=f"{lab} step {k} {name}")
        want = refm.step(raw["observations"][idx], raw["actions"][idx], raw["next_observations"][idx], raw["rewards"][idx], raw["dones"][idx],
                         eps_pi.numpy(), eps_next.numpy(), u.numpy(), eps.numpy())
        t = model.last_train_tensors
        xc = t["x_cand"].cpu().numpy()
        assert np.array_equal(xc[:, :4], np.repeat(batch[0], 3 * N, axis=0)) and np.array_equal(xc.reshape(B, 3 * N, 6)[:, :N, 4:], u.numpy())
        strict = lambda g, w_: float((np.abs(np.asarray(g, np.float64) - w_) / np.maximum(np.abs(w_), 1e-3)).max())  # noqa: E731
        print(f"{lab} step {k}: per-element |dq| / max(|q|, 1e-3): target {strict(t['target_q'].cpu().numpy(), want['target_q']):.2e} "
              f"q1 {strict(t['current_q'][0].cpu().numpy(), want['current_q'][0]):.2e} q2 {strict(t['current_q'][1].cpu().numpy(), want['current_q'][1]):.2e}"
              f" (|q| from {np.abs(want['current_q'][0]).min():.2e} to {np.abs(want['current_q'][0]).max():.2e})")
        e_a = float(np.abs(xc[:, 4:] - want["x_cand"][:, 4:]).max())
        # log-probs: the Q bar of tests/_parity_helpers.py (1e-5 of max(|v|, mean|v|)) plus what float32 can do to the tanh correction
        # log(1 - a^2 + 1e-6) of a nearly saturated action: a and a^2 carry 2^-23 between them, divided by (1 - a^2 + 1e-6); 4 x that
        a_ref = want["x_cand"][:, 4:].reshape(B, 3 * N, 2)
        cbar = 1e-5 * np.maximum(np.abs(want["corr"]), np.abs(want["corr"]).mean()) + 4 * 2.0 ** -23 * (1.0 / (1 - a_ref ** 2 + 1e-6)).sum(axis=2)
        e_c = float((np.abs(t["corr"].cpu().numpy() - want["corr"]) / cbar).max())
        e_t = q_err(t["target_q"].cpu().numpy(), want["target_q"], lab)
        e_q = [q_err(t["current_q"][i].cpu().numpy(), want["current_q"][i], lab) for i in range(2)]
        e_all = rel_err(t["q_all"].cpu().numpy().reshape(2, -1), want["q_all"], float(np.abs(want["q_all"]).mean()))
        e_l = rel_err(float(t["critic_loss"]), want["critic_loss"], 1e-3)
        e_al = rel_err(float(t["actor_loss"]), want["actor_loss"], 1e-3)
        aux = t["aux"].cpu().numpy()
        e_aux = [rel_err(float(aux[i]), want["aux"][i], 1e-3) for i in range(4)]
        lv = model.logger.name_to_value
        logged = [float(lv[f"train/{n}"]) for n in ("bellman_loss", "cql_loss", "cql_lse", "q_data")]
        assert all(abs(a - g) <= 2 * np.spacing(np.float32(abs(g))) for a, g in zip(logged, aux)), (logged, aux)
        assert rel_err(float(lv["train/critic_loss"]), want["critic_loss"], 1e-3) < 1e-5
        assert rel_err(float(lv["train/ent_coef"]), want["ent_coef"], 1e-3) < 1e-5
        line = (f"{lab} step {k}: cand {e_a:.2e} corr {e_c:.2e} target_q {e_t:.2e} q {e_q[0]:.2e} {e_q[1]:.2e} q_all {e_all:.2e} "
                f"critic_loss {e_l:.2e} actor_loss {e_al:.2e} aux " + " ".join(f"{e:.2e}" for e in e_aux))
        print(line)
        assert e_a < 2e-5 and e_c < 1.0 and e_t < 1e-5 and max(e_q) < 1e-5 and e_all < 1e-5 and e_l < 1e-5 and e_al < 1e-5, line
        assert max(e_aux) < 1e-5, line
    assert model._n_updates == 2 and model.actor.optimizer.step_count == 2 and model.critic.optimizer.step_count == 2
    worst = 0.0
    for nm in MODS:
        wsd = getattr(refm.p, nm).state_dict()
        for k, v in getattr(model.policy, nm).state_dict().items():
            got, w = v.detach().cpu().numpy().astype(np.float64), wsd[k].numpy()
            scale = max(float(np.abs(w).max()), 1e-3)
            worst = max(worst, float((np.abs(got - w) / (2e-5 * scale + 1e-4 * np.abs(w))).max()))
    e_ent = abs(float(model.log_ent_coef.detach()) - float(refm.log_ent_coef.detach())) / (2e-5 * 1e-3 + 1e-4 * abs(float(refm.log_ent_coef.detach())))
    print(f"{lab}: weights after 2 steps, worst err / (2e-5 scale + 1e-4 |w|) = {worst:.3f}; log_ent_coef {e_ent:.3f}")
    assert worst < 1.0 and e_ent < 1.0, (worst, e_ent)


# ------------------------------------------------------------------------------------ graph replay, allocations, paths
def _digest(model):
    pol = model.policy
    parts = [pol.actor_arena.flat, pol.critic_arena.flat, pol.critic_target_arena.flat, model.log_ent_coef]
    for o in (model.actor.optimizer, model.critic.optimizer, model.ent_coef_optimizer):
        parts += [o.exp_avg, o.exp_avg_sq, o.ctl[:1].float()]
    parts += [model.replay_buffer.sampler_stream.float(), model._loss_sum_buf, model._fast_actor.rng_ctl[:2].float(), model._rng_ctl[:2].float(),
              model._x_wide]
    return [p.detach().clone() for p in parts]


@pytest.mark.parametrize("unroll", [1, 4])
def test_graph_replay_equals_eager(unroll):
    outs = []
    warm, n = 16, 9
    for graph in (False, True):
        model = _model(B=64, seed=3, cql_n_actions=3)
        if graph:
            model.enable_graph_capture(True, unroll=unroll)
        model.learn(warm)
        th.cuda.synchronize()
        before = model.graph_status()["replays"]
        start = _digest(model)
        model.learn(n)
        th.cuda.synchronize()
        st = model.graph_status()
        assert model._n_updates == warm + n and model.num_timesteps == n
        if graph:
            assert st["active"] and st["replays"] - before >= (8 if unroll == 1 else 2) and st["error"] is None, st
        else:
            assert st["replays"] == 0
        outs.append((start, _digest(model)))
    for a, b in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]):
        assert th.equal(a, b)
    assert not all(th.equal(a, b) for a, b in zip(outs[0][0], outs[0][1]))  # the nine iterations did change the state
    model.cql_noise_queue = [(th.zeros(64, 3, 2), th.zeros(64, 6, 2))]  # a queued draw keeps the iteration eager
    assert not model._graph_eligible(model._noop_callback())
    model.cql_noise_queue = []
    assert model._graph_eligible(model._noop_callback())


def test_nothing_is_allocated_after_the_first_steps():
    """the fused-Linear path (2B-row actor pass, stacked critic output): every buffer of the step persists from the second step on"""
    model = _model(B=64, cql_n_actions=5)
    model.train(1, 64)
    model.train(1, 64)
    th.cuda.synchronize()
    blk = model._critic_block
    ptrs = lambda: [t.data_ptr() for t in (model._x_wide, model._cql_corr, model._cql_params, blk.gq_wide, blk.gq, blk.g_logp, model._packed.x_data)]  # noqa: E731
    before, mem = ptrs(), th.cuda.memory_allocated()
    assert model._packed.x_data.data_ptr() == model._x_wide.data_ptr() and blk.gq_wide.shape == (2, 16 * 64, 1) and blk.gq.shape[1] == 64
    model.train(1, 64)
    th.cuda.synchronize()
    assert ptrs() == before and th.cuda.memory_allocated() == mem


def test_path_selection(monkeypatch):
    from core.common import hip_ops

    calls = {}
    for name in ("cql_candidates", "cql_q_loss", "td_twin_q_loss"):
        orig = getattr(hip_ops, name)

        def wrapped(*a, _o=orig, _n=name, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _o(*a, **k)

        monkeypatch.setattr(hip_ops, name, wrapped)
    model = _model(B=32, arch=(32, 32))
    assert model.fused_learner and model._chain_for(32) is None and type(model).chain_type is None
    model.train(gradient_steps=2, batch_size=32)
    assert calls == dict(cql_candidates=2, cql_q_loss=2), calls
    calls.clear()
    model.fused_learner = False
    model.train(gradient_steps=2, batch_size=32)
    assert not calls
    for extra in (dict(policy_kwargs=dict(net_arch=[32, 32], n_critics=3)), dict(cql_n_actions=22),
                  dict(policy_kwargs=dict(net_arch=[32, 32], optimizer_class=th.optim.AdamW))):
        calls.clear()
        m = _model(B=32, arch=(32, 32), **extra)
        assert not m.fused_learner, extra
        m.debug_capture = True
        m.train(gradient_steps=2, batch_size=32)
        t = m.last_train_tensors
        n_c = 3 if "n_critics" in str(extra) else 2
        assert len(t["current_q"]) == n_c and t["q_all"].shape == (n_c, 32 * (1 + 3 * m.cql_n_actions), 1) and not calls
        assert all(bool(th.isfinite(v).all()) for v in (t["critic_loss"], t["actor_loss"], t["target_q"], t["aux"])) and m._n_updates == 2
    # both importance modes and the entropy backup on the kernels
    for kw in (dict(cql_importance_sample=False), dict(backup_entropy=True), dict(ent_coef=0.2), dict(gradient_steps=3)):
        m = _model(B=32, arch=(32, 32), **kw)
        m.debug_capture = True
        calls.clear()
        m.train(gradient_steps=m.gradient_steps, batch_size=32)
        assert m.fused_learner and calls == dict(cql_candidates=m.gradient_steps, cql_q_loss=m.gradient_steps), (kw, calls)
        t = m.last_train_tensors
        assert (t["corr"] is None) == (kw.get("cql_importance_sample") is False) and bool(th.isfinite(t["aux"]).all())
        sums = m._loss_sum_buf.cpu().numpy()
        assert np.isfinite(sums).all() and abs(sums[1] - (sums[4] + sums[5])) <= 1e-5 * max(abs(sums[1]), 1.0)  # critic = bellman + cql


# ------------------------------------------------------------------------------------ dataset forms, predict
def test_dataset_forms_and_the_callers_buffer(tmp_path):
    from core.common.save_util import save_to_pkl
    from core.cql import CQL

    raw = _raw_dataset(rows=300)
    src = _buffer(raw)
    before = _fields(src)
    pkl, npz = str(tmp_path / "data.pkl"), str(tmp_path / "data.npz")
    save_to_pkl(pkl, src)
    np.savez(npz, **{k: getattr(src, k).cpu().numpy() for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")})
    pk = dict(net_arch=[32, 32])
    models = []
    for dataset in (src, pkl, npz):
        m = CQL("MlpPolicy", _env(), dataset=dataset, seed=0, batch_size=32, policy_kwargs=pk, cql_n_actions=3)
        rb = m.replay_buffer
        assert rb.size() == 300 and rb.n_envs == 1 and m.n_envs == 1
        assert all(th.equal(getattr(rb, k), getattr(src, k)) for k in ("observations", "next_observations", "actions", "rewards", "dones"))
        m.replay_buffer.seed_sampler(5)  # (for `src` this is the caller's object: its sampler stream is not one of its data fields)
        m.learn(3)
        assert m._n_updates == 3 and m.fused_learner
        models.append(m)
    for m in models[1:]:  # the three forms train identically from the same sampler stream
        assert all(th.equal(a, b) for a, b in zip(m.policy.parameters(), models[0].policy.parameters()))
    assert all(th.equal(a, b) for a, b in zip(before, _fields(src)))  # the caller's buffer: bit-identical after construction and learning


def test_predict_is_sacs():
    model = _model(B=32, arch=(32, 32))
    model.learn(4)
    obs = np.random.default_rng(0).uniform(-1, 1, (7, 4)).astype(np.float32)
    act, state = model.predict(obs, deterministic=True)
    assert state is None and act.shape == (7, 2)
    with th.no_grad():
        want = model.policy.unscale_action(model.actor(th.as_tensor(obs, device=DEV), deterministic=True).cpu().numpy())
    np.testing.assert_array_equal(act, np.clip(want, model.action_space.low, model.action_space.high))
    a1, a2 = model.predict(obs)[0], model.predict(obs)[0]
    assert a1.shape == (7, 2) and not np.array_equal(a1, a2)  # stochastic by default, as SAC


# ------------------------------------------------------------------------------------ learn(), checkpoints
class _Dumps:
    def __init__(self):
        self.rows = []

    def write(self, vals, excluded, step):
        self.rows.append((step, dict(vals)))


def test_learn_counters_and_logger_keys():
    from core.common.callbacks import BaseCallback
    from core.common.logger import Logger

    model = _model(B=32, arch=(32, 32))
    dumps = _Dumps()
    model.set_logger(Logger(output_formats=[dumps]))
    assert model.learn(8, log_interval=4) is model
    assert model.num_timesteps == 8 and model._n_updates == 8 and [s for s, _ in dumps.rows] == [4, 8]
    want = {"time/fps", "time/time_elapsed", "time/total_timesteps", "dataset/size", "training/bc_warmup_steps", "training/conservative_weight",
            "train/n_updates", "train/ent_coef", "train/actor_loss", "train/critic_loss", "train/ent_coef_loss", "train/cql_loss",
            "train/bellman_loss", "train/cql_lse", "train/q_data", "train/learning_rate"}
    for step, row in dumps.rows:
        assert set(row) == want, (step, sorted(set(row) ^ want))
        assert row["dataset/size"] == 2048 and row["training/conservative_weight"] == 5.0 and row["train/n_updates"] == step
        assert all(np.isfinite(float(row[k])) for k in want if k.startswith("train/"))
        assert float(row["train/critic_loss"]) == pytest.approx(float(row["train/bellman_loss"]) + float(row["train/cql_loss"]), rel=1e-5)
    with pytest.warns(UserWarning, match="do not collect rollouts"):
        assert model.collect_rollouts(model.env, None, None, model.replay_buffer) is None

    class Stop(BaseCallback):
        def _on_step(self):
            return self.n_calls < 3

    stopped = _model(B=32, arch=(32, 32))
    stopped.learn(8, callback=Stop())
    assert stopped.num_timesteps == 3 and stopped._n_updates == 3
    multi = _model(B=32, arch=(32, 32), gradient_steps=4)  # the logged values are means over the call's steps
    multi.debug_capture = True
    multi.learn(1)
    assert multi._n_updates == 4 and multi.critic.optimizer.step_count == 4
    lv, sums = multi.logger.name_to_value, multi._loss_sum_buf.cpu().numpy().astype(np.float64)
    assert float(lv["train/cql_lse"]) == pytest.approx(sums[6] / 4, rel=1e-6) and float(lv["train/q_data"]) == pytest.approx(sums[7] / 4, rel=1e-6)
    assert float(multi.last_train_tensors["aux"][2]) != pytest.approx(sums[6] / 4, rel=1e-7)


def test_checkpoint_round_trip_continues_identically(tmp_path):
    import json
    import zipfile

    from core.cql import CQL

    raw = _raw_dataset()
    model = _model(raw, B=32, arch=(32, 32), conservative_weight=3.5, cql_n_actions=4, cql_temp=0.8, cql_importance_sample=False, backup_entropy=True)
    model.learn(5)
    path = str(tmp_path / "cql_ckpt")
    model.save(path)
    with zipfile.ZipFile(path + ".zip") as z:
        assert {"data", "policy.pth", "actor.optimizer.pth", "critic.optimizer.pth", "ent_coef_optimizer.pth"} <= set(z.namelist())
        data = json.loads(z.read("data"))
    assert (data["conservative_weight"], data["cql_n_actions"], data["cql_temp"], data["cql_importance_sample"], data["backup_entropy"]) == (
        3.5, 4, 0.8, False, True) and "dataset" not in data
    clone = CQL.load(path, env=_env(), dataset=_buffer(raw))
    assert clone._n_updates == 5 and clone.num_timesteps == 5 and clone.fused_learner
    assert (clone.conservative_weight, clone.cql_n_actions, clone.cql_temp, clone.cql_importance_sample, clone.backup_entropy) == (3.5, 4, 0.8, False, True)
    for a, b in zip(model.policy.state_dict().values(), clone.policy.state_dict().values()):
        assert th.equal(a, b)
    assert th.equal(model.log_ent_coef, clone.log_ent_coef)
    for o, c in ((model.actor.optimizer, clone.actor.optimizer), (model.critic.optimizer, clone.critic.optimizer),
                 (model.ent_coef_optimizer, clone.ent_coef_optimizer)):
        assert o.step_count == c.step_count and th.equal(o.exp_avg, c.exp_avg) and th.equal(o.exp_avg_sq, c.exp_avg_sq)
    obs = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(model.predict(obs, deterministic=True)[0], clone.predict(obs, deterministic=True)[0])
    outs = []
    for m in (model, clone):
        m.set_random_seed(7)
        m.replay_buffer.seed_sampler(99)
        m.train(gradient_steps=3, batch_size=32)
        outs.append([p.detach().clone() for p in m.policy.parameters()] + [m.log_ent_coef.detach().clone()])
    for a, b in zip(*outs):
        assert th.equal(a, b)
    # a dataset path travels in the archive: load() without dataset= reads it again
    from core.common.save_util import save_to_pkl

    pkl = str(tmp_path / "data.pkl")
    save_to_pkl(pkl, _buffer(raw))
    by_path = CQL("MlpPolicy", _env(), dataset=pkl, seed=0, batch_size=32, policy_kwargs=dict(net_arch=[32, 32]))
    by_path.save(path + "_p")
    again = CQL.load(path + "_p", env=_env())
    assert again.dataset == pkl and again.replay_buffer.size() == 2048 and again.conservative_weight == 5.0


def test_every_refusal():
    from core.common.vec_env import VecNormalize
    from core.cql import CQL

    ds = _buffer(_raw_dataset(rows=64))
    with pytest.raises(ValueError, match="VecNormalize"):
        CQL("MlpPolicy", VecNormalize(_env()), dataset=ds)
    with pytest.raises(ValueError, match="does not support a Dict observation space"):
        CQL("MlpPolicy", _env(goal_conditioned=True, goal_range=(0.10, 0.40)), dataset=ds)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        CQL("MlpPolicy", _env(discrete_actions=3), dataset=ds)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        CQL("MlpPolicy", _env(multi_discrete_actions=(3, 5)), dataset=ds)
    with pytest.raises(ValueError, match="does not support gSDE"):
        CQL("MlpPolicy", _env(), dataset=ds, policy_kwargs=dict(use_sde=True))
    with pytest.raises(ValueError, match="the model does not support multiple envs"):
        CQL("MlpPolicy", _env(8), dataset=ds)
    from core.common import distributed as dist_util

    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            CQL("MlpPolicy", _env(), dataset=ds)
    finally:
        dist_util.rank_world = orig
    with pytest.raises(ValueError, match="Policy MultiInputPolicy unknown|MultiInputPolicy"):
        CQL("MultiInputPolicy", _env(), dataset=ds)
    import inspect

    assert "replay_buffer_class" not in inspect.signature(CQL.__init__).parameters  # HER: the goal face is refused above, and no buffer class is taken
    for kw, msg in ((dict(conservative_weight=-1.0), "conservative_weight"), (dict(conservative_weight=float("nan")), "conservative_weight"),
                    (dict(cql_temp=0.0), "cql_temp"), (dict(cql_temp=float("nan")), "cql_temp"), (dict(cql_n_actions=0), "cql_n_actions")):
        with pytest.raises(ValueError, match=msg):
            CQL("MlpPolicy", _env(), dataset=ds, **kw)
    with pytest.raises(ValueError, match="needs `env`"):
        CQL("MlpPolicy", None, dataset=ds)
    from core.common.buffers import ReplayBuffer

    with pytest.raises(ValueError, match="Loaded dataset is empty"):
        CQL("MlpPolicy", _env(), dataset=ReplayBuffer(64, *_spaces(), device=DEV, n_envs=1))
    m = CQL("MlpPolicy", _env(), dataset=ds, policy_kwargs=dict(net_arch=[32, 32]), behavior_cloning_warmup=3)
    assert m.conservative_weight == 5.0 and m.behavior_cloning_warmup == 3 and m.n_eval_episodes == 10
    m.learn(2)  # behavior_cloning_warmup is accepted, without effect
    assert m._n_updates == 2


# ------------------------------------------------------------------------------------ evaluation, collection
def _short_env(n, seed):
    from core.common.vec_env import CSTRVecEnv

    class Short(CSTRVecEnv):
        max_steps = 20

    e = Short(n)
    e.seed(seed)
    return e


def _both_ways(model, n_envs=4, episodes=8):
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused

    loop = evaluate_policy(model, _short_env(n_envs, 21), n_eval_episodes=episodes, return_episode_rewards=True, warn=False)
    fused = evaluate_policy_fused(model, _short_env(n_envs, 21), n_eval_episodes=episodes, return_episode_rewards=True, warn=False)
    assert len(loop[0]) == len(fused[0]) == episodes and loop[1] == fused[1] and all(n == 20 for n in fused[1])
    return np.asarray(loop[0], np.float64), np.asarray(fused[0], np.float64)


def test_fused_evaluation_and_collection_cover_a_cql_model():
    """evaluate_policy_fused against evaluate_policy, order and lengths equal, returns within 4 x d0: d0 = the worst |fused - loop| episode
    return of a plain SAC model of the same shape and seed (two float32 implementations of one network, propagated through the episodes),
    floor one float32 ulp of a step reward per step."""
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy_fused, evaluate_trajectories, supported
    from core.common.offline_dataset import collect_offline_dataset
    from core.bcq import BCQ
    from core.cql import CQL
    from core.sac import SAC
    from core.td3bc import TD3BC

    sac = SAC("MlpPolicy", _env(1), seed=0, policy_kwargs=dict(net_arch=[32, 32]))
    loop, fused = _both_ways(sac)
    floor = 20 * float(np.spacing(np.float32(np.abs(loop).max() / 20)))
    d0 = max(float(np.abs(loop - fused).max()), floor)
    model = _model(arch=(32, 32), B=32)
    model.learn(4)
    assert supported(model, _short_env(4, 21))
    loop, fused = _both_ways(model)
    print(f"CQL (32, 32): worst |fused - loop| return {float(np.abs(loop - fused).max()):.3e}, bar {4 * d0:.3e}")
    assert float(np.abs(loop - fused).max()) <= 4 * d0
    ev = EvalCallback(_short_env(4, 7), n_eval_episodes=4, eval_freq=5, verbose=0, warn=False)
    model.learn(10, callback=ev)
    assert ev.n_calls == 10 and np.isfinite(ev.last_mean_reward)
    tr = evaluate_trajectories(model, _short_env(4, 3), n_eval_episodes=4)
    rets, lens = evaluate_policy_fused(model, _short_env(4, 3), n_eval_episodes=4, return_episode_rewards=True, warn=False)
    assert tr["states"].shape == (4, 20, 4) and list(tr["episode_lengths"]) == lens
    np.testing.assert_allclose(tr["episode_rewards"], rets, rtol=1e-6)
    rb, stats = collect_offline_dataset(model, _short_env(8, 5), num_episodes=16, random_action_prob=0.2, seed=1)
    assert rb.size() == 40 and rb.n_envs == 8 and stats["num_episodes"] >= 16
    # the three offline algorithms beside each other on that one buffer; the caller's buffer stays bit-identical
    before = _fields(rb)
    pk = dict(net_arch=[32, 32])
    cql = CQL("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=pk, cql_n_actions=4)
    bcq = BCQ("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=dict(critic_net_arch=[32, 32]))
    tbc = TD3BC("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=pk)
    for m in (cql, bcq, tbc):
        m.learn(20)
    th.cuda.synchronize()
    assert cql._n_updates == 20 and cql.fused_learner and all(bool(th.isfinite(p).all()) for m in (cql, bcq, tbc) for p in m.policy.parameters())
    assert all(th.equal(a, b) for a, b in zip(before, _fields(rb)))
    from twoseriescstr import evaluate_model

    ep_rewards, ep_states = evaluate_model(cql, _short_env(4, 3), num_episodes=4, plot=False)
    assert len(ep_rewards) == 4 and np.asarray(ep_states).shape == (4, 20, 4) and np.isfinite(ep_rewards).all()


# ------------------------------------------------------------------------------------ what the conservative term does, and a learning run
def _synthetic_buffer(data):
    from core.common.buffers import ReplayBuffer

    rows = data["rewards"].shape[0]
    rb = ReplayBuffer(rows, *_spaces(), device=DEV, n_envs=1)
    f = lambda a, *sh: th.as_tensor(a).reshape(*sh)  # noqa: E731
    rb.observations.copy_(f(data["observations"], rows, 1, 4)), rb.next_observations.copy_(f(data["next_observations"], rows, 1, 4))
    rb.actions.copy_(f(data["actions"], rows, 1, 2)), rb.rewards.copy_(f(data["rewards"], rows, 1)), rb.dones.copy_(f(data["dones"], rows, 1))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    return rb


def test_conservative_weight_lowers_lse_minus_q():
    """BCQ's synthetic dataset, seed 0, K = 200 steps at (32, 32) / batch 64 / N = 4 / lr 3e-3 (tests/_cql_reference.py GAP_ARGS): the
    dataset mean of lse - Q(s, a) over both critics after w = 5 is below that after w = 0. The reference alone: 3.985 after w = 0, -0.173
    after w = 5 (asserted in tests/test_cql_abi.py). Here only the inequality."""
    from core.cql import CQL
    GAP_ARGS = ref.GAP_ARGS
    data = ref.synthetic_dataset()
    gaps = {}
    for w in (0.0, 5.0):
        m = CQL("MlpPolicy", _env(), dataset=_synthetic_buffer(data), seed=GAP_ARGS["seed"], batch_size=GAP_ARGS["B"], learning_rate=GAP_ARGS["lr"],
                cql_n_actions=GAP_ARGS["N"], cql_temp=GAP_ARGS["T"], conservative_weight=w, policy_kwargs=dict(net_arch=list(GAP_ARGS["arch"])))
        assert m.fused_learner
        m.learn(GAP_ARGS["steps"])
        gaps[w] = ref.dataset_gap(_ref_policy(m, GAP_ARGS["arch"]), data, GAP_ARGS["N"], GAP_ARGS["T"], rows=512)
    print(f"kernels: mean(lse - Q(s,a)) after w=0: {gaps[0.0]:.3f}, after w=5: {gaps[5.0]:.3f}")
    assert gaps[5.0] < gaps[0.0], gaps


def test_cql_learns_the_behaviour_policy():
    """test_bcq_learns_the_behaviour_policy's dataset: actions = clip(tanh(obs K) + N(0, 0.05)), 20 000 rows, default_rng(0); after
    learn(1000) at the class defaults the deterministic predict() is within 0.2 (mean absolute error) of tanh(obs K). The fp64 reference
    on the CPU (tests/_cql_reference.py train_reference at (256, 256) / 256 / N = 10, seed 0) reaches 0.030 after 500 steps and 0.024
    after 1000, from 0.41."""
    from core.cql import CQL

    data = ref.synthetic_dataset()
    K = data["K"]
    test_obs = np.random.default_rng(99).uniform(-1, 1, (200, 4)).astype(np.float32)
    model = CQL("MlpPolicy", _env(), dataset=_synthetic_buffer(data), seed=0)
    assert model.fused_learner and model.batch_size == 256 and model.cql_n_actions == 10 and model.conservative_weight == 5.0

    def score():
        pred = model.policy.scale_action(model.predict(test_obs, deterministic=True)[0])
        return float(np.abs(pred - np.tanh(test_obs @ K)).mean())

    before = score()
    model.learn(1000)
    after = score()
    print(f"behaviour cloning error: untrained {before:.3f}, after learn(1000) {after:.3f}; "
          f"cql_lse {float(model._loss_sums['lse']):.3f}, q_data {float(model._loss_sums['q_data']):.3f}")
    assert model._n_updates == 1000
    assert after < 0.2, f"mean |predict - tanh(obs K)| = {after:.3f} after learn(1000) (untrained {before:.3f})"
