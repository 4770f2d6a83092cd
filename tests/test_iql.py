"""IQL on the HIP learner (core/iql, csrc/cstr_iql.hip) against the fp64 statements of tests/_iql_reference.py.

The loss launch against fp64: every element of u, g_v, y, gq1, gq2, w, logp, g_params and every scalar of the loss and aux rows within
max(4 x the distance of the float32 torch statement (CPU ATen, the same inputs) from fp64 FOR THAT ELEMENT, 2 float32 ulp + the
element's conditioning). The conditioning (tests/_iql_reference.py `floors`, derived there rounding by rounding) is what float32 arithmetic
can move the element by whatever evaluates it: exp(beta u) turns the roundings of beta u into relative error, (g - mean)^2 / sd^2 - 1
cancels, and log(1 - a^2 + 1e-6) near |a| = 1 divides 2^-24 by 1e-6. The clipped share and the log-std mask are exact (the inputs keep
a margin from the clip bound; the mask is a comparison of inputs). The critic part is bit-equal to cstr_td_twin_q_loss_f32.
Teacher-forced learning: Q values, V and targets through `q_err`, u / w / logp at the bars derived from it (see the test), scalars
through `rel_err`, weights within 2e-5 of the tensor's scale + 1e-4 relative (tests/_parity_helpers.py).

Measured on MI355X: over the 39 cases of the loss tests the worst element-wise error / bar is 0.57 (a raw log-std gradient at B 255 /
A 4 / beta 10); most outputs sit at 0.25, the float32 torch statement's own distance. Teacher-forced: Q values, V and targets within
9.1e-8 of their scale on every path, u and w at most 0.006 of their bars, logp at most 0.046, the losses within 2.1e-6, the weights of
the four networks at most 0.036 of their bar after the two steps. A gradient step at the class defaults makes 27 ABI calls. mean V
-3.173 after expectile 0.5 and -2.489 after 0.9; behaviour cloning error 0.009 after learn(1000) from 0.409. Launches and times:
profiles/iql_probe.txt (tools/iql_probe.py)."""
import numpy as np
import pytest
import torch as th

import _iql_reference as ref
from _parity_helpers import q_err, rel_err
from _sentinel_bufs import Bufs

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]

DEV = "cuda"
SENT = float(np.float32(12345.678))
MODS = ["actor", "critic", "critic_target", "value_net"]
VEC_KEYS = ("u", "g_v", "y", "gq1", "gq2", "logp", "g_params")


def _env(n=1, **kw):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n, **kw)


def _spaces():
    from core.common.spaces import Box

    return Box(-1, 1, (4,)), Box(-1, 1, (2,))


def _d(a):
    return th.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(th.int32)


def _strided(a: np.ndarray, ld: int):
    """[R, W] values as the first W columns of rows ld floats wide (the rest sentinels) -> the view"""
    R, W = a.shape
    t = th.full((R, ld), SENT, dtype=th.float32, device=DEV)
    t[:, :W] = th.as_tensor(a)
    return t[:, :W]


# ------------------------------------------------------------------------------------ the loss launch
def _loss_inputs(B, A, seed, mode="mixed", beta=3.0, M=100.0):
    """float32 inputs. mode: the sign pattern of u = min(qt) - v ("mixed", "neg", "pos", "zero": exactly 0, "clip": about half of the
    rows with exp(beta u) > M, "overflow": exp(beta u) = inf in float32, "nan": a NaN q1, "beyond": one action beyond 1). From 8 rows on the
    first rows hold the edge actions (0, next to +-1, exactly +-1) and the edge log-stds (below -20, above 2, exactly on both bounds)."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    qt1, qt2 = f(rng.normal(-3, 1.5, B)), f(rng.normal(-3, 1.5, B))
    qt = np.minimum(qt1, qt2)
    du = dict(mixed=rng.normal(0, 0.6, B), neg=-np.abs(rng.normal(0.5, 0.5, B)) - 0.01, pos=np.abs(rng.normal(0.5, 0.5, B)) + 0.01,
              zero=np.zeros(B), clip=rng.normal(np.log(M) / max(beta, 1e-3), 1.0, B), overflow=rng.normal(40.0, 2.0, B)).get(mode)
    du = rng.normal(0, 0.6, B) if du is None else du
    v = f(qt.astype(np.float64) - du)
    if mode == "zero":
        v = qt.copy()
    # keep beta u away from log M: the clipped share is then the same in every arithmetic
    u = qt.astype(np.float64) - v.astype(np.float64)
    near = np.abs(beta * u - np.log(M)) < 1e-3
    v[near] -= np.float32(0.01)
    params = f(np.concatenate([rng.normal(0, 0.5, (B, A)), rng.normal(-1, 0.7, (B, A))], axis=1))
    act = f(np.tanh(rng.normal(0, 1, (B, A))))
    if B >= 8:
        edge_a = [0.0, 1.0 - 2.0 ** -20, -1.0 + 2.0 ** -22, 1.0, -1.0]
        edge_l = [-25.0, 3.0, -20.0, 2.0]
        for i, e in enumerate(edge_a):
            act[i, :] = np.float32(e)
        for i, e in enumerate(edge_l):
            r = 4 + i
            params[r, A:] = np.float32(e)
            if e <= -20.0:  # sd = exp(-20): the mean sits next to atanh(a), or the row's logp is -1e17 and the batch sums with it
                x = np.clip(act[r].astype(np.float64), -1 + ref.EPS32, 1 - ref.EPS32)
                params[r, :A] = f(0.5 * (np.log1p(x) - np.log1p(-x)))
    inp = dict(qt1=qt1, qt2=qt2, v=v, v_next=f(rng.normal(-3, 1.5, B)), q1=f(rng.normal(-3, 1.5, B)), q2=f(rng.normal(-3, 1.5, B)), params=params,
               act=act, rew=f(rng.uniform(-8, 0, B)), done=f(rng.uniform(size=B) < 0.2), gamma=0.99)
    if mode == "nan":
        inp["q1"][B // 2] = np.nan
    if mode == "beyond":
        inp["act"][B // 2, A - 1] = np.float32(1.0 + 2.0 ** -10)
    return inp


def _args(inp, expectile, beta, M):
    return tuple(inp[k] for k in ("qt1", "qt2", "v", "v_next", "q1", "q2", "params", "act", "rew", "done")) + (inp["gamma"], expectile, beta, M)


OUT_SHAPES = lambda B, A: dict(g_v=(B,), gq1=(B, 1), gq2=(B, 1), g_params=(B, 2 * A), loss_out=(3,), loss_sum=(3,), aux=(6,),  # noqa: E731
                               target_out=(B, 1), adv_out=(B,), logp_out=(B,))


def _run_loss(inp, expectile, beta, M, ppad=0, apad=0, leave_out=(), halves=False):
    """one launch into sentinel-padded outputs -> {name: clone}. halves: v and v_next as the two halves of one [2B] tensor"""
    from core.common import hip_ops

    B, A = inp["act"].shape
    bufs = Bufs()
    outs = {k: (None if k in leave_out else bufs.new(k, *s)) for k, s in OUT_SHAPES(B, A).items()}
    if outs["loss_sum"] is not None:
        outs["loss_sum"].copy_(th.tensor([1.5, -2.5, 0.25], device=DEV))
    params = _strided(inp["params"], 2 * A + ppad) if ppad else _d(inp["params"])
    act = _strided(inp["act"], A + apad) if apad else _d(inp["act"])
    v2 = th.cat([_d(inp["v"]), _d(inp["v_next"])])
    v, v_next = (v2[:B], v2[B:]) if halves else (_d(inp["v"]), _d(inp["v_next"]))
    hip_ops.iql_loss(_d(inp["qt1"]), _d(inp["qt2"]), v, v_next, _d(inp["q1"]), _d(inp["q2"]), params, act, _d(inp["rew"]), _d(inp["done"]),
                     inp["gamma"], expectile, beta, M, **outs)
    bufs.check(written=[k for k in outs if outs[k] is not None and k != "loss_sum"])
    return {k: v.clone() for k, v in outs.items() if v is not None}


def _as_ref(got):
    """the launch's outputs under the reference's names, as float64 NumPy"""
    n = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    B = got["adv_out"].shape[0]
    return dict(u=n(got["adv_out"]), g_v=n(got["g_v"]), y=n(got["target_out"]).reshape(B), gq1=n(got["gq1"]).reshape(B), gq2=n(got["gq2"]).reshape(B),
                logp=n(got["logp_out"]), g_params=n(got["g_params"]), losses=n(got["loss_out"]), aux=n(got["aux"]))


def _check_loss(got, inp, expectile, beta, M, label):
    args = _args(inp, expectile, beta, M)
    want, aten, fl = ref.loss_f64(*args), ref.loss_torch(*args, dtype=th.float32), ref.floors(*args)
    g = _as_ref(got)
    ratios = {}
    for k in VEC_KEYS + ("losses", "aux"):
        # the scalars one by one: each has its own bar
        parts = [(g[k][i:i + 1], want[k][i:i + 1], aten[k][i:i + 1], fl[k][i:i + 1]) for i in range(len(want[k]))] if k in ("losses", "aux") \
            else [(g[k], want[k], aten[k], fl[k])]
        ratios[k] = max(ref.close(a, b, c, floor=d) for a, b, c, d in parts)
    # w is not an output of the launch: aux[1] is its mean and aux[2] the clipped share, exact
    clip_share = float(np.float32(want["clipped"].mean()))
    line = f"{label}: worst element-wise error / bar " + " ".join(f"{k} {r:.2f}" for k, r in ratios.items())
    print(line)
    assert all(r <= 1.0 for r in ratios.values()), line
    assert float(got["aux"][2]) == clip_share or np.isnan(want["u"]).any(), (label, float(got["aux"][2]), clip_share)
    # the log-std mask: exact zeros outside the closed interval, and only there (a row whose w / B is 0 aside)
    A = inp["act"].shape[1]
    raw = inp["params"][:, A:]
    outside = (raw < -20.0) | (raw > 2.0)
    gl = g["g_params"][:, A:]
    assert (gl[outside] == 0).all() and (want["g_params"][:, A:][outside] == 0).all()
    s = 1.5 + float(got["loss_out"][0]), -2.5 + float(got["loss_out"][1]), 0.25 + float(got["loss_out"][2])
    for i in range(3):  # loss_sum accumulates
        assert abs(float(got["loss_sum"][i]) - s[i]) <= 2 * np.spacing(np.float32(abs(s[i]))) or np.isnan(s[i]), (label, i)
    return want, g


def _twin_td(inp):
    """cstr_td_twin_q_loss_f32 fed v_next as both target Q's, no next_logp, scale 0.5"""
    from core.common import hip_ops

    B = inp["rew"].shape[0]
    tq, g1, g2 = (th.empty(B, 1, device=DEV) for _ in range(3))
    loss = th.empty(1, device=DEV)
    hip_ops.td_twin_q_loss(_d(inp["v_next"]), _d(inp["v_next"]), None, _d(inp["rew"]), _d(inp["done"]), None, inp["gamma"], _d(inp["q1"]),
                           _d(inp["q2"]), 0.5, tq, g1, g2, loss)
    return tq, g1, g2, loss


COMBOS = [(1, 0.5, 0.0, 0, 0), (2, 0.7, 3.0, 2, 4), (4, 0.9, 10.0, 3, 1), (2, 0.9, 3.0, 0, 4)]  # A, expectile, beta, ppad, apad


@pytest.mark.parametrize("B", [1, 3, 65, 255, 256, 257, 1030, 16384])
def test_loss_against_fp64(B):
    for A, tau_e, beta, ppad, apad in COMBOS:
        inp = _loss_inputs(B, A, seed=B * 31 + A, beta=beta)
        got = _run_loss(inp, tau_e, beta, 100.0, ppad, apad)
        want, g = _check_loss(got, inp, tau_e, beta, 100.0, f"B{B} A{A} tau_e={tau_e} beta={beta} ld+{ppad}/{apad}")
        # the critic part: the twin TD head's bits
        tq, g1, g2, loss = _twin_td(inp)
        assert th.equal(_bits(got["target_out"]), _bits(tq)) and th.equal(_bits(got["gq1"]), _bits(g1)) and th.equal(_bits(got["gq2"]), _bits(g2))
        assert th.equal(_bits(got["loss_out"][1:2]), _bits(loss))
        if beta == 0.0:  # w = 1 exactly: mean w = 1, nothing clipped, the actor loss is -mean(logp)
            assert float(got["aux"][1]) == 1.0 and float(got["aux"][2]) == 0.0
            assert abs(float(got["loss_out"][2]) + float(got["aux"][3])) <= 2 * np.spacing(np.float32(abs(float(got["aux"][3]))))
        # relaunch, row strides at the widths, v | v_next as the halves of one tensor: the same bits
        again = _run_loss(inp, tau_e, beta, 100.0, 0, 0, halves=True)
        assert all(th.equal(_bits(got[k]), _bits(again[k])) for k in got), [k for k in got if not th.equal(_bits(got[k]), _bits(again[k]))]


@pytest.mark.parametrize("mode", ["neg", "pos", "zero", "clip", "overflow", "nan", "beyond"])
def test_loss_sign_patterns_and_edge_values(mode):
    B, A, tau_e, beta, M = 257, 2, 0.7, 3.0, 100.0
    inp = _loss_inputs(B, A, seed=11, mode=mode, beta=beta, M=M)
    got = _run_loss(inp, tau_e, beta, M)
    want, g = _check_loss(got, inp, tau_e, beta, M, mode)
    gp = g["g_params"]
    if mode == "neg":
        assert (want["u"] < 0).all() and (g["u"] < 0).all()
    if mode == "pos":
        assert (want["u"] > 0).all() and (g["u"] > 0).all()
    if mode == "zero":  # u = 0 takes weight tau_e, contributes nothing, and w = exp(0) = 1
        assert (g["u"] == 0).all() and (g["g_v"] == 0).all() and float(got["loss_out"][0]) == 0.0 and float(got["aux"][1]) == 1.0
    if mode == "clip":  # on the fp64 reference alone: at least a quarter of the rows clipped, at least a quarter not
        share = want["clipped"].mean()
        assert 0.25 <= share <= 0.75, share
        assert float(got["aux"][2]) == float(np.float32(share))
    if mode == "overflow":  # exp(beta u) = inf in float32: clipped to M, every gradient finite
        assert np.isinf(np.exp(np.float32(beta) * g["u"].astype(np.float32))).all() and want["clipped"].all()
        assert float(got["aux"][1]) == M and float(got["aux"][2]) == 1.0 and np.isfinite(gp).all() and np.isfinite(g["losses"]).all()
    if mode == "nan":  # a NaN q1: its own gradient and the critic loss, nothing else
        b = B // 2
        assert np.isnan(g["gq1"][b]) and np.isnan(g["losses"][1]) and np.isfinite(np.delete(g["gq1"], b)).all()
        assert all(np.isfinite(g[k]).all() for k in ("u", "g_v", "y", "gq2", "logp", "g_params", "aux")) and np.isfinite(g["losses"][[0, 2]]).all()
    if mode == "beyond":  # |a| > 1: torch's NaN (the log of a negative number) in that row's logp and in the sums over logp, nowhere else
        b = B // 2
        assert np.isnan(g["logp"][b]) and np.isnan(want["logp"][b]) and np.isfinite(np.delete(g["logp"], b)).all()
        assert np.isnan(g["losses"][2]) and np.isnan(g["aux"][3]) and np.isfinite(g["losses"][:2]).all() and np.isfinite(g["aux"][[0, 1, 2, 4, 5]]).all()
        assert all(np.isfinite(g[k]).all() for k in ("u", "g_v", "y", "gq1", "gq2", "g_params"))


def test_optional_outputs_left_out_in_turn_and_bad_shapes():
    from core.common import hip_ops

    B, A = 65, 2
    inp = _loss_inputs(B, A, seed=5)
    full = _run_loss(inp, 0.7, 3.0, 100.0)
    for group in (("g_v",), ("gq1", "gq2"), ("g_params",), ("loss_out",), ("loss_sum",), ("aux",), ("target_out",), ("adv_out",), ("logp_out",),
                  ("g_v", "gq1", "gq2", "g_params"), tuple(OUT_SHAPES(B, A))):
        part = _run_loss(inp, 0.7, 3.0, 100.0, leave_out=group)
        assert set(part) == set(full) - set(group)
        assert all(th.equal(_bits(part[k]), _bits(full[k])) for k in part), group
    z = lambda *s: th.zeros(*s, device=DEV)  # noqa: E731
    ok = lambda: [z(8), z(8), z(8), z(8), z(8), z(8), z(8, 4), z(8, 2), z(8), z(8)]  # noqa: E731
    for i, bad, msg in ((7, z(7, 2), "act"), (6, z(8, 5), "params"), (0, z(9), "qt1"), (3, z(8, 2)[:, 0], "v_next"), (6, z(8, 4).double(), "params")):
        args = ok()
        args[i] = bad
        with pytest.raises(ValueError, match=msg):
            hip_ops.iql_loss(*args, 0.99, 0.7, 3.0, 100.0)
    with pytest.raises(ValueError, match="both or neither"):
        hip_ops.iql_loss(*ok(), 0.99, 0.7, 3.0, 100.0, gq1=z(8))
    with pytest.raises(ValueError, match="g_params"):
        hip_ops.iql_loss(*ok(), 0.99, 0.7, 3.0, 100.0, g_params=z(8, 2))


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
    f = lambda a, *sh: th.as_tensor(np.asarray(a, np.float32)).reshape(*sh)  # noqa: E731
    rb.observations.copy_(f(raw["observations"], rows, 1, 4)), rb.next_observations.copy_(f(raw["next_observations"], rows, 1, 4))
    rb.actions.copy_(f(raw["actions"], rows, 1, 2)), rb.rewards.copy_(f(raw["rewards"], rows, 1)), rb.dones.copy_(f(raw["dones"], rows, 1))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    if sampler_seed is not None:
        rb.seed_sampler(sampler_seed)
    return rb


def _fields(rb):
    return [getattr(rb, k).clone() for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")] + [rb.ring.ctl.clone()]


def _model(raw=None, arch=(64, 64), B=64, seed=0, **kw):
    from core.iql import IQL

    raw = _raw_dataset() if raw is None else raw
    pk = dict(kw.pop("policy_kwargs", {}))
    if arch is not None:
        pk.setdefault("net_arch", list(arch))
    model = IQL("MlpPolicy", _env(), dataset=_buffer(raw), seed=seed, batch_size=B, policy_kwargs=pk, **kw)
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
    from core.iql.policies import IQLPolicy

    pk = {} if arch is None else dict(net_arch=list(arch))
    p = IQLPolicy(*_spaces(), lambda _: 3e-4, **pk)
    p.load_state_dict({k: v.detach().cpu() for k, v in model.policy.state_dict().items()})
    return p.double()


@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("tag", ["small", "default"])
def test_iql_teacher_forced(tag, path, monkeypatch):
    """Two steps against the fp64 reference (RefIQL), from the seeded initial weights with ONE change made to the model and the reference
    alike: the output biases of the critics, their targets and V start at the dataset's mean reward (about -4) instead of 0, as CQL's
    teacher-forced runs do and for the reason measured there and, for IQL, in tests/test_iql_abi.py
    (test_float32_torch_statement_at_an_untrained_critic): `q_err`'s per-element bar |dq| <= 5e-5 max(|q|, 1e-3) asks 5e-8 of an
    untrained output of 0 +- 0.1, which the float32 torch statement itself does not give.
    Bars: Q values, V and the targets y through `q_err`. u = qt - v inherits both operands' bars: 1e-5 (max(|qt|, mean|qt|) + max(|v|,
    mean|v|)) per element. w = min(exp(beta u), M): relative beta x that + 1e-5. logp: 1e-5 max(|logp|, mean|logp|) plus what float32 can
    do to log(1 - a^2 + 1e-6) of a nearly saturated dataset action (4 x 2^-23 / (1 - a^2 + 1e-6) per component, as CQL's log-prob bar).
    The three losses within 1e-5 relative, the weights of all four networks by check_weights' formula. Every path draws the same batches,
    bit for bit. The printed lines say what was measured."""
    arch, B = ((64, 64), 64) if tag == "small" else (None, 256)
    raw = _raw_dataset()
    model = _model(raw, arch=arch, B=B)
    bias = float(raw["rewards"].mean())
    with th.no_grad():
        for critic in (model.critic, model.critic_target):
            for qnet in critic.q_networks:
                qnet[-1].bias.fill_(bias)
        model.value_net.v_net[-1].bias.fill_(bias)
    _select_path(monkeypatch, model, path)
    assert (model.expectile, model.beta, model.exp_adv_max, model.tau, model.gamma, model.lr_schedule(1)) == (0.7, 3.0, 100.0, 0.005, 0.99, 3e-4)
    refm = ref.RefIQL(_ref_policy(model, arch), 3e-4, model.gamma, model.tau, 0.7, 3.0, 100.0)
    index = {a.tobytes(): i for i, a in enumerate(raw["actions"])}
    model.debug_capture = True
    lab = f"iql_{tag}_{path}"
    rs = np.random.RandomState(5)  # the sampler's stream (seed_sampler(5)): every path draws NumPy's indices, so the same batches
    for k in range(2):
        model.train(gradient_steps=1, batch_size=B)
        b = model._static_batch
        idx = np.array([index[r.tobytes()] for r in b.actions.cpu().numpy()])
        want_idx = rs.randint(0, raw["rewards"].shape[0], size=B)
        rs.randint(0, 1, size=B)
        np.testing.assert_array_equal(idx, want_idx)
        for name in ("observations", "actions", "next_observations", "rewards", "dones"):
            np.testing.assert_array_equal(getattr(b, name).cpu().numpy().reshape(B, -1), raw[name][idx].reshape(B, -1), err_msg=f"{lab} step {k} {name}")
        want = refm.step(raw["observations"][idx], raw["actions"][idx], raw["next_observations"][idx], raw["rewards"][idx], raw["dones"][idx])
        t = {k_: ([x.cpu().numpy().astype(np.float64).reshape(-1) for x in v] if isinstance(v, list) else v.cpu().numpy().astype(np.float64).reshape(-1))
             for k_, v in model.last_train_tensors.items()}
        e_q = [q_err(t["q"][i], want["q"][i], lab) for i in range(2)]
        e_v, e_y = q_err(t["v"], want["v"], lab), q_err(t["y"], want["y"], lab)
        qt = want["u"] + want["v"]
        big = lambda x: np.maximum(np.abs(x), np.abs(x).mean())  # noqa: E731
        bar_u = 1e-5 * (big(qt) + big(want["v"]))
        e_u = float((np.abs(t["u"] - want["u"]) / bar_u).max())
        e_w = float((np.abs(t["w"] - want["w"]) / (want["w"] * (3.0 * bar_u + 1e-5))).max())
        a_ref = raw["actions"][idx].astype(np.float64)
        bar_lp = 1e-5 * big(want["logp"]) + 4 * 2.0 ** -23 * (1.0 / (1 - a_ref ** 2 + 1e-6)).sum(axis=1)
        e_lp = float((np.abs(t["logp"] - want["logp"]) / bar_lp).max())
        e_l = [rel_err(t["losses"][i], want["losses"][i], 1e-3) for i in range(3)]
        lv = model.logger.name_to_value
        logged = [float(lv[f"train/{n}"]) for n in ("value_loss", "critic_loss", "actor_loss")]
        assert all(abs(a - g) <= 2 * np.spacing(np.float32(abs(g))) for a, g in zip(logged, t["losses"])), (logged, t["losses"])
        assert rel_err(float(lv["train/adv_mean"]), want["u"].mean(), 1e-3) < 1e-4 and rel_err(float(lv["train/weight_mean"]), want["w"].mean(), 1e-3) < 1e-4
        assert rel_err(float(lv["train/logp_mean"]), want["logp"].mean(), 1e-3) < 1e-4
        assert abs(float(lv["train/weight_clip_frac"]) - float((np.exp(3.0 * want["u"]) > 100.0).mean())) <= 1.0 / B
        line = (f"{lab} step {k}: q {e_q[0]:.2e} {e_q[1]:.2e} v {e_v:.2e} y {e_y:.2e} (of their scale); u {e_u:.3f} w {e_w:.3f} logp {e_lp:.3f} "
                f"(of their bars); losses " + " ".join(f"{e:.2e}" for e in e_l))
        print(line)
        assert max(e_q) < 1e-5 and e_v < 1e-5 and e_y < 1e-5 and e_u < 1.0 and e_w < 1.0 and e_lp < 1.0 and max(e_l) < 1e-5, line
    assert model._n_updates == 2 and all(o.step_count == 2 for o in (model.actor.optimizer, model.critic.optimizer, model.value_net.optimizer))
    worst = 0.0
    for nm in MODS:
        wsd = getattr(refm.p, nm).state_dict()
        for k, v in getattr(model.policy, nm).state_dict().items():
            got, w = v.detach().cpu().numpy().astype(np.float64), wsd[k].numpy()
            scale = max(float(np.abs(w).max()), 1e-3)
            worst = max(worst, float((np.abs(got - w) / (2e-5 * scale + 1e-4 * np.abs(w))).max()))
    print(f"{lab}: weights of the four networks after 2 steps, worst err / (2e-5 scale + 1e-4 |w|) = {worst:.3f}")
    assert worst < 1.0, worst


# ------------------------------------------------------------------------------------ graph replay, allocations, launches, paths
def _digest(model):
    pol = model.policy
    parts = [pol.actor_arena.flat, pol.critic_arena.flat, pol.critic_target_arena.flat, pol.value_arena.flat]
    for o in (model.actor.optimizer, model.critic.optimizer, model.value_net.optimizer):
        parts += [o.exp_avg, o.exp_avg_sq, o.ctl[:1].float()]
    parts += [model.replay_buffer.sampler_stream.float(), model._loss_sum_buf]
    return [p.detach().clone() for p in parts]


@pytest.mark.parametrize("unroll", [1, 4])
def test_graph_replay_equals_eager(unroll):
    outs = []
    warm, n = 16, 9
    for graph in (False, True):
        model = _model(B=64, seed=3)
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
    assert model._graph_eligible(model._noop_callback())  # the step draws nothing: nothing queued can keep it eager


def test_nothing_is_allocated_after_the_second_step():
    model = _model(B=64)
    model.train(1, 64)
    model.train(1, 64)
    th.cuda.synchronize()
    ptrs = lambda: [t.data_ptr() for t in (model._g_v, model._gq, model._g_params, model._adv, model._logp, model._target_q,  # noqa: E731
                                           model._packed.x_data, model._packed.x_pn)]
    before, mem = ptrs(), th.cuda.memory_allocated()
    model.train(1, 64)
    th.cuda.synchronize()
    assert ptrs() == before and th.cuda.memory_allocated() == mem


STEP_ABI_CALLS = 27  # sample 1; target critics 3, V 3, critics 3, actor trunk 2 + head epilogue 1; loss 1; V backward 3, critics 3, actor 4; 3 optimiser steps


def test_abi_calls_of_a_step_and_the_one_launch_between_forwards_and_backwards(monkeypatch):
    """Every launching entry point reports through hip_ops' `check`: a recording wrapper sees a gradient step's calls in order. Exactly one
    of them is cstr_iql_loss_f32; the call in front of it is a forward launch, the one behind it a backward launch, every call in front
    of it a sampler or forward launch and none behind it a forward one. The count per step is pinned (profiles/iql_probe.txt has it too)."""
    from core.common import hip_ops

    names = []
    orig = hip_ops.check

    def recording(rc, what):
        names.append(what)
        return orig(rc, what)

    model = _model(B=256, arch=None)
    model.train(1, 256)
    model.train(1, 256)
    monkeypatch.setattr(hip_ops, "check", recording)
    model.train(1, 256)
    first = list(names)
    names.clear()
    model.train(1, 256)
    print(f"ABI calls of one IQL gradient step at the class defaults: {len(names)}: " + " ".join(n.replace("cstr_", "").replace("_f32", "") for n in names))
    assert names == first and names.count("cstr_iql_loss_f32") == 1
    i = names.index("cstr_iql_loss_f32")
    fwd = lambda n: "_fwd" in n  # noqa: E731
    assert fwd(names[i - 1]) and "_bwd" in names[i + 1], names
    assert all(fwd(n) or "replay_sample" in n for n in names[:i]) and not any(fwd(n) for n in names[i + 1:]), names
    assert len(names) == STEP_ABI_CALLS, len(names)


def test_path_selection(monkeypatch):
    from core.common import hip_ops

    calls = {}
    orig = hip_ops.iql_loss

    def wrapped(*a, **k):
        calls["iql_loss"] = calls.get("iql_loss", 0) + 1
        return orig(*a, **k)

    monkeypatch.setattr(hip_ops, "iql_loss", wrapped)
    model = _model(B=32, arch=(32, 32))
    assert model.fused_learner and model._chain_for(32) is None and type(model).chain_type is None
    model.train(gradient_steps=2, batch_size=32)
    assert calls == dict(iql_loss=2), calls
    calls.clear()
    model.fused_learner = False
    model.train(gradient_steps=2, batch_size=32)
    assert not calls
    for extra in (dict(policy_kwargs=dict(net_arch=[32, 32], n_critics=3)), dict(policy_kwargs=dict(net_arch=[32, 32], optimizer_class=th.optim.AdamW))):
        calls.clear()
        m = _model(B=32, arch=(32, 32), **extra)
        assert not m.fused_learner, extra
        m.debug_capture = True
        m.train(gradient_steps=2, batch_size=32)
        t = m.last_train_tensors
        assert len(t["q"]) == (3 if "n_critics" in str(extra) else 2) and not calls and m._n_updates == 2
        assert all(bool(th.isfinite(t[k]).all()) for k in ("u", "w", "y", "logp", "v", "losses", "aux"))
    for kw in (dict(gradient_steps=3), dict(target_update_interval=2), dict(expectile=0.9, beta=0.0, exp_adv_max=5.0)):
        m = _model(B=32, arch=(32, 32), **kw)
        m.debug_capture = True
        calls.clear()
        m.train(gradient_steps=m.gradient_steps, batch_size=32)
        assert m.fused_learner and calls == dict(iql_loss=m.gradient_steps), (kw, calls)
        assert np.isfinite(m._loss_sum_buf.cpu().numpy()).all()
        if kw.get("beta") == 0.0:
            assert bool((m.last_train_tensors["w"] == 1.0).all())


# ------------------------------------------------------------------------------------ dataset forms, predict
def test_dataset_forms_and_the_callers_buffer(tmp_path):
    from core.common.save_util import save_to_pkl
    from core.iql import IQL

    raw = _raw_dataset(rows=300)
    src = _buffer(raw)
    before = _fields(src)
    pkl, npz = str(tmp_path / "data.pkl"), str(tmp_path / "data.npz")
    save_to_pkl(pkl, src)
    np.savez(npz, **{k: getattr(src, k).cpu().numpy() for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")})
    models = []
    for dataset in (src, pkl, npz):
        m = IQL("MlpPolicy", _env(), dataset=dataset, seed=0, batch_size=32, policy_kwargs=dict(net_arch=[32, 32]))
        rb = m.replay_buffer
        assert rb.size() == 300 and rb.n_envs == 1 and m.n_envs == 1
        assert all(th.equal(getattr(rb, k), getattr(src, k)) for k in ("observations", "next_observations", "actions", "rewards", "dones"))
        m.replay_buffer.seed_sampler(5)
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
            "train/n_updates", "train/value_loss", "train/critic_loss", "train/actor_loss", "train/adv_mean", "train/weight_mean",
            "train/weight_clip_frac", "train/logp_mean", "train/learning_rate"}
    for step, row in dumps.rows:
        assert set(row) == want, (step, sorted(set(row) ^ want))
        assert row["dataset/size"] == 2048 and row["train/n_updates"] == step
        assert all(np.isfinite(float(row[k])) for k in want if k.startswith("train/"))
        assert 0.0 <= float(row["train/weight_clip_frac"]) <= 1.0 and 0.0 < float(row["train/weight_mean"]) <= 100.0
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
    assert multi._n_updates == 4 and multi.value_net.optimizer.step_count == 4
    lv, sums = multi.logger.name_to_value, multi._loss_sum_buf.cpu().numpy().astype(np.float64)
    assert float(lv["train/value_loss"]) == pytest.approx(sums[0] / 4, rel=1e-6) and float(lv["train/logp_mean"]) == pytest.approx(sums[6] / 4, rel=1e-6)
    assert float(multi.last_train_tensors["aux"][3]) != pytest.approx(sums[6] / 4, rel=1e-7)


def test_checkpoint_round_trip_continues_identically(tmp_path):
    import json
    import zipfile

    from core.iql import IQL

    raw = _raw_dataset()
    model = _model(raw, B=32, arch=(32, 32), expectile=0.8, beta=2.0, exp_adv_max=50.0, target_update_interval=2)
    model.learn(5)
    path = str(tmp_path / "iql_ckpt")
    model.save(path)
    with zipfile.ZipFile(path + ".zip") as z:
        assert {"data", "policy.pth", "actor.optimizer.pth", "critic.optimizer.pth", "value_net.optimizer.pth"} <= set(z.namelist())
        data = json.loads(z.read("data"))
    assert (data["expectile"], data["beta"], data["exp_adv_max"], data["target_update_interval"]) == (0.8, 2.0, 50.0, 2) and "dataset" not in data
    assert "ent_coef" not in data
    clone = IQL.load(path, env=_env(), dataset=_buffer(raw))
    assert clone._n_updates == 5 and clone.num_timesteps == 5 and clone.fused_learner
    assert (clone.expectile, clone.beta, clone.exp_adv_max, clone.target_update_interval) == (0.8, 2.0, 50.0, 2)
    sd = model.policy.state_dict()
    assert any(k.startswith("value_net.") for k in sd)
    for a, b in zip(sd.values(), clone.policy.state_dict().values()):
        assert th.equal(a, b)
    for o, c in ((model.actor.optimizer, clone.actor.optimizer), (model.critic.optimizer, clone.critic.optimizer),
                 (model.value_net.optimizer, clone.value_net.optimizer)):
        assert o.step_count == c.step_count == 5 and th.equal(o.exp_avg, c.exp_avg) and th.equal(o.exp_avg_sq, c.exp_avg_sq)
    obs = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(model.predict(obs, deterministic=True)[0], clone.predict(obs, deterministic=True)[0])
    outs = []
    for m in (model, clone):
        m.replay_buffer.seed_sampler(99)
        m.train(gradient_steps=3, batch_size=32)
        outs.append([p.detach().clone() for p in m.policy.parameters()])
    for a, b in zip(*outs):
        assert th.equal(a, b)
    # a dataset path travels in the archive: load() without dataset= reads it again
    from core.common.save_util import save_to_pkl

    pkl = str(tmp_path / "data.pkl")
    save_to_pkl(pkl, _buffer(raw))
    by_path = IQL("MlpPolicy", _env(), dataset=pkl, seed=0, batch_size=32, policy_kwargs=dict(net_arch=[32, 32]))
    by_path.save(path + "_p")
    again = IQL.load(path + "_p", env=_env())
    assert again.dataset == pkl and again.replay_buffer.size() == 2048 and again.expectile == 0.7


def test_every_refusal():
    from core.common.vec_env import VecNormalize
    from core.iql import IQL

    ds = _buffer(_raw_dataset(rows=64))
    with pytest.raises(ValueError, match="VecNormalize"):
        IQL("MlpPolicy", VecNormalize(_env()), dataset=ds)
    with pytest.raises(ValueError, match="does not support a Dict observation space"):
        IQL("MlpPolicy", _env(goal_conditioned=True, goal_range=(0.10, 0.40)), dataset=ds)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        IQL("MlpPolicy", _env(discrete_actions=3), dataset=ds)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        IQL("MlpPolicy", _env(multi_discrete_actions=(3, 5)), dataset=ds)
    with pytest.raises(ValueError, match="does not support gSDE"):
        IQL("MlpPolicy", _env(), dataset=ds, policy_kwargs=dict(use_sde=True))
    with pytest.raises(ValueError, match="the model does not support multiple envs"):
        IQL("MlpPolicy", _env(8), dataset=ds)
    from core.common import distributed as dist_util

    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            IQL("MlpPolicy", _env(), dataset=ds)
    finally:
        dist_util.rank_world = orig
    with pytest.raises(ValueError, match="Policy MultiInputPolicy unknown|MultiInputPolicy"):
        IQL("MultiInputPolicy", _env(), dataset=ds)
    import inspect

    assert "replay_buffer_class" not in inspect.signature(IQL.__init__).parameters  # HER: the goal face is refused above, and no buffer class is taken
    for kw, msg in ((dict(expectile=0.0), "expectile"), (dict(expectile=1.0), "expectile"), (dict(expectile=float("nan")), "expectile"),
                    (dict(beta=-1.0), "beta"), (dict(beta=float("nan")), "beta"), (dict(exp_adv_max=0.0), "exp_adv_max"),
                    (dict(exp_adv_max=float("nan")), "exp_adv_max")):
        with pytest.raises(ValueError, match=msg):
            IQL("MlpPolicy", _env(), dataset=ds, **kw)
    with pytest.raises(ValueError, match="needs `env`"):
        IQL("MlpPolicy", None, dataset=ds)
    from core.common.buffers import ReplayBuffer

    with pytest.raises(ValueError, match="Loaded dataset is empty"):
        IQL("MlpPolicy", _env(), dataset=ReplayBuffer(64, *_spaces(), device=DEV, n_envs=1))
    m = IQL("MlpPolicy", _env(), dataset=ds, policy_kwargs=dict(net_arch=[32, 32]), behavior_cloning_warmup=3)
    assert m.behavior_cloning_warmup == 3 and m.n_eval_episodes == 10 and m.log_ent_coef is None and m.ent_coef_optimizer is None
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


def test_fused_evaluation_and_collection_cover_an_iql_model():
    """evaluate_policy_fused against evaluate_policy, order and lengths equal, returns within 4 x d0: d0 = the worst |fused - loop| episode
    return of a plain SAC model of the same shape and seed (two float32 implementations of one network, propagated through the episodes),
    floor one float32 ulp of a step reward per step."""
    from core.bcq import BCQ
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy_fused, evaluate_trajectories, supported
    from core.common.offline_dataset import collect_offline_dataset
    from core.cql import CQL
    from core.iql import IQL
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
    print(f"IQL (32, 32): worst |fused - loop| return {float(np.abs(loop - fused).max()):.3e}, bar {4 * d0:.3e}")
    assert float(np.abs(loop - fused).max()) <= 4 * d0
    ev = EvalCallback(_short_env(4, 7), n_eval_episodes=4, eval_freq=5, verbose=0, warn=False)  # fused=None: the one-launch evaluation where it applies
    model.learn(10, callback=ev)
    assert ev.n_calls == 10 and np.isfinite(ev.last_mean_reward)
    tr = evaluate_trajectories(model, _short_env(4, 3), n_eval_episodes=4)
    rets, lens = evaluate_policy_fused(model, _short_env(4, 3), n_eval_episodes=4, return_episode_rewards=True, warn=False)
    assert tr["states"].shape == (4, 20, 4) and list(tr["episode_lengths"]) == lens
    np.testing.assert_allclose(tr["episode_rewards"], rets, rtol=1e-6)
    rb, stats = collect_offline_dataset(model, _short_env(8, 5), num_episodes=16, random_action_prob=0.2, seed=1)
    assert rb.size() == 40 and rb.n_envs == 8 and stats["num_episodes"] >= 16
    # the four offline algorithms beside each other on that one buffer; the caller's buffer stays bit-identical
    before = _fields(rb)
    pk = dict(net_arch=[32, 32])
    iql = IQL("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=pk)
    cql = CQL("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=pk, cql_n_actions=4)
    bcq = BCQ("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=dict(critic_net_arch=[32, 32]))
    tbc = TD3BC("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=pk)
    for m in (iql, cql, bcq, tbc):
        m.learn(20)
    th.cuda.synchronize()
    assert iql._n_updates == 20 and iql.fused_learner and all(bool(th.isfinite(p).all()) for m in (iql, cql, bcq, tbc) for p in m.policy.parameters())
    assert all(th.equal(a, b) for a, b in zip(before, _fields(rb)))
    from twoseriescstr import evaluate_model

    ep_rewards, ep_states = evaluate_model(iql, _short_env(4, 3), num_episodes=4, plot=False)
    assert len(ep_rewards) == 4 and np.asarray(ep_states).shape == (4, 20, 4) and np.isfinite(ep_rewards).all()


# ------------------------------------------------------------------------------------ what the expectile does, and a learning run
def test_expectile_orders_the_value_function():
    """tests/_iql_reference.py ORDER_ARGS on `ordering_dataset` (300 steps at (32, 32) / batch 64 / lr 3e-3 / seed 0): the dataset mean of V
    after expectile 0.9 is above that after expectile 0.5. The reference alone: -3.237 and -2.512 (asserted in tests/test_iql_abi.py). Here
    only the inequality, on the device path."""
    from core.iql import IQL

    args = ref.ORDER_ARGS
    data = ref.ordering_dataset()
    vals = {}
    for tau_e in (0.5, 0.9):
        m = IQL("MlpPolicy", _env(), dataset=_buffer(data, sampler_seed=args["seed"] + 1), seed=args["seed"], batch_size=args["B"],
                learning_rate=args["lr"], expectile=tau_e, policy_kwargs=dict(net_arch=list(args["arch"])))
        assert m.fused_learner
        m.learn(args["steps"])
        vals[tau_e] = ref.dataset_value(_ref_policy(m, args["arch"]), data)
    print(f"device path: mean V after expectile 0.5: {vals[0.5]:.3f}, after 0.9: {vals[0.9]:.3f}")
    assert vals[0.9] > vals[0.5], vals


def test_iql_learns_the_behaviour_policy():
    """test_bcq_learns_the_behaviour_policy's dataset: actions = clip(tanh(obs K) + N(0, 0.05)), 20 000 rows, default_rng(0); after
    learn(1000) at the class defaults the deterministic predict() is within 0.2 (mean absolute error) of tanh(obs K): the siblings'
    criterion. The fp64 reference on the CPU (tests/_iql_reference.py RefIQL at (256, 256) / 256, seed 0) reaches 0.014 after 250 steps
    and 0.009 after 1000, from 0.409."""
    from core.iql import IQL

    data = ref.synthetic_dataset()
    K = data["K"]
    test_obs = np.random.default_rng(99).uniform(-1, 1, (200, 4)).astype(np.float32)
    model = IQL("MlpPolicy", _env(), dataset=_buffer(data, sampler_seed=None), seed=0)
    assert model.fused_learner and model.batch_size == 256 and (model.expectile, model.beta, model.exp_adv_max) == (0.7, 3.0, 100.0)

    def score():
        pred = model.policy.scale_action(model.predict(test_obs, deterministic=True)[0])
        return float(np.abs(pred - np.tanh(test_obs @ K)).mean())

    before = score()
    model.learn(1000)
    after = score()
    print(f"behaviour cloning error: untrained {before:.3f}, after learn(1000) {after:.3f}; "
          f"weight_mean {float(model._loss_sums['weight_mean']):.3f}, logp_mean {float(model._loss_sums['logp_mean']):.3f}")
    assert model._n_updates == 1000
    assert after < 0.2, f"mean |predict - tanh(obs K)| = {after:.3f} after learn(1000) (untrained {before:.3f})"
