"""TD3+BC on the HIP learner (core/td3bc, csrc/cstr_td3bc.hip) against the fp64 statements of tests/_td3bc_reference.py.

The loss launch: lam, the loss and the three aux values within 4 x the distance of the float32 torch evaluation of the same statement
from fp64, measured here on the same inputs (CPU ATen), floor 2 float32 ulp of the value; gq one value in every row within 2 ulp of
-lam / B. The backward-rows launch: bit for bit against the NumPy float32 statement. Teacher-forced learning: Q values and targets
through `q_err`, weights within 2e-5 of the tensor's scale + 1e-4 relative (tests/_parity_helpers.py); the actor loss, lam and
bc_loss at the loss launch's bar ON THE LAUNCH'S OWN INPUTS (the captured Q1(s, pi(s)) and pi(s); the float32 torch evaluation is
taken on the model's device there, which is what the torch-statement path itself runs), the captured inputs themselves against the
fp64 steps through `q_err` / the tanh-output bar of tests/test_sde.py.

Measured on MI355X: the loss launch within 0.5 ulp of fp64 for lam and bc, about 1 ulp for the Q term (it follows from the float32
lam), about 2 ulp for the loss, their sum; teacher-forced Q values and targets within 3e-6 of their scale on every path, weights at
most 0.28 of their bar after six steps at (400, 300); launches and times in profiles/td3bc_probe.txt (tools/td3bc_probe.py)."""
import numpy as np
import pytest
import torch as th

import _td3bc_reference as ref
from _parity_helpers import q_err, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]

DEV = "cuda"
SENT = float(np.float32(12345.678))
PAD = 64
MODS = ["actor", "actor_target", "critic", "critic_target"]


def _env(n=1, **kw):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n, **kw)


def _spaces():
    from core.common.spaces import Box

    return Box(-1, 1, (4,)), Box(-1, 1, (2,))


def _ulp(v) -> float:
    return float(np.spacing(np.abs(np.float32(v))))


def _out(*shape):
    """a sentinel-filled output with 64 sentinel floats in front of it and behind it -> (whole buffer, the output view)"""
    n = int(np.prod(shape))
    f = th.full((n + 2 * PAD,), SENT, dtype=th.float32, device=DEV)
    return f, f[PAD:PAD + n].view(*shape)


def _pads_clean(f) -> bool:
    return bool((f[:PAD] == SENT).all()) and bool((f[-PAD:] == SENT).all())


def _rows_view(a: np.ndarray, extra: int):
    """[B, A] values as the last A columns of rows A + extra floats wide, the base pointer on a 4-byte boundary only"""
    B, A = a.shape
    flat = th.zeros(B * (A + extra) + 1, dtype=th.float32, device=DEV)
    rows = flat[1:].view(B, A + extra)
    v = rows[:, extra:]
    v.copy_(th.as_tensor(a))
    return v


# ------------------------------------------------------------------------------------ the loss launch
def _loss_inputs(B, A, sign, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 2.0, B).astype(np.float32)
    if sign == "negative":
        q = -np.abs(q) - np.float32(0.25)
    if sign == "positive":
        q = np.abs(q) + np.float32(0.25)
    if sign == "mixed" and B > 1:
        q[0], q[1] = np.float32(-1.5), np.float32(0.75)
    pi = np.tanh(rng.normal(0, 1, (B, A))).astype(np.float32)
    a = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    return q, pi, a


@pytest.mark.parametrize("A", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 5, 255, 256, 257, 1030, 16384])
def test_actor_loss_launch_against_fp64(B, A):
    from core import _native as nv
    from core.common import hip_ops

    assert nv.TD3BC_MAX_BATCH == 16384
    alpha = 2.5
    worst = {}
    for extra in (0, 4):
        for si, sign in enumerate(("negative", "positive", "mixed")):
            q, pi, a = _loss_inputs(B, A, sign, 1000 * B + 10 * A + si)
            want = ref.actor_loss_f64(q, pi, a, alpha)
            aten = ref.actor_loss_torch(q, pi, a, alpha, th.float32)
            qd = th.as_tensor(q).to(DEV).reshape(B, 1)
            pid, ad = _rows_view(pi, extra), _rows_view(a, extra)
            assert pid.stride(0) == A + extra and pid.data_ptr() % 4 == 0
            (f_gq, gq), (f_lo, lo), (f_ls, ls), (f_aux, aux) = _out(B, 1), _out(1), _out(1), _out(3)
            ls.fill_(1.5)
            hip_ops.td3bc_actor_loss(qd, pid, ad, alpha, gq, lo, ls, aux)
            th.cuda.synchronize()
            got = dict(lam=float(aux[0]), q_term=float(aux[1]), bc=float(aux[2]), loss=float(lo))
            for k in ("lam", "q_term", "bc", "loss"):
                bar = max(4 * abs(aten[k] - want[k]), 2 * _ulp(want[k]))
                err = abs(got[k] - want[k])
                worst[k] = max(worst.get(k, 0.0), err / _ulp(want[k]))
                assert err <= bar, (k, sign, extra, got[k], want[k], aten[k], err / _ulp(want[k]))
            g = gq.cpu().numpy().reshape(-1)
            assert (g == g[0]).all() and abs(float(g[0]) - want["gq"][0]) <= 2 * _ulp(want["gq"][0])
            # accumulate mode: one float32 add to what was there; store mode wrote the value itself
            assert float(ls) == float(np.float32(1.5) + np.float32(got["loss"]))
            assert all(_pads_clean(f) for f in (f_gq, f_lo, f_ls, f_aux))
            snap = [t.clone() for t in (f_gq, f_lo, f_aux)]
            ls.fill_(1.5)
            first_sum = float(np.float32(1.5) + np.float32(got["loss"]))
            hip_ops.td3bc_actor_loss(qd, pid, ad, alpha, gq, lo, ls, aux)  # a second launch: the same bits
            th.cuda.synchronize()
            assert all(th.equal(s, t) for s, t in zip(snap, (f_gq, f_lo, f_aux))) and float(ls) == first_sum
            # each of loss_out / loss_sum / aux alone
            (f2, lo2), (f3, ls3) = _out(1), _out(1)
            ls3.fill_(-0.25)
            hip_ops.td3bc_actor_loss(qd, pid, ad, alpha, gq, lo2, None, None)
            hip_ops.td3bc_actor_loss(qd, pid, ad, alpha, gq, None, ls3, None)
            th.cuda.synchronize()
            assert float(lo2) == got["loss"] and float(ls3) == float(np.float32(-0.25) + np.float32(got["loss"]))
            assert _pads_clean(f2) and _pads_clean(f3) and th.equal(f_aux, snap[2])
    print(f"td3bc_actor_loss B={B} A={A}: worst |got - fp64| in float32 ulp of the value: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("alpha", [2.5, 0.0])
def test_actor_loss_launch_q_zero_matches_the_float32_torch_pattern(alpha):
    from core.common import hip_ops

    B, A = 257, 2
    _, pi, a = _loss_inputs(B, A, "mixed", 7)
    q = np.zeros(B, np.float32)
    with np.errstate(all="ignore"):
        aten = ref.actor_loss_torch(q, pi, a, alpha, th.float32)
    (f_gq, gq), (f_lo, lo), (f_aux, aux) = _out(B, 1), _out(1), _out(3)
    hip_ops.td3bc_actor_loss(th.zeros(B, 1, device=DEV), _rows_view(pi, 4), _rows_view(a, 4), alpha, gq, lo, None, aux)
    th.cuda.synchronize()
    got = dict(lam=float(aux[0]), q_term=float(aux[1]), bc=float(aux[2]), loss=float(lo))
    for k in got:
        assert (np.isnan(got[k]), np.isposinf(got[k]), np.isneginf(got[k])) == (np.isnan(aten[k]), np.isposinf(aten[k]), np.isneginf(aten[k])), (k, got, aten)
    assert np.isfinite(got["bc"]) and not np.isfinite(got["loss"]) and (np.isposinf(got["lam"]) if alpha > 0 else np.isnan(got["lam"]))
    want_g = -np.float32(aten["lam"]) / np.float32(B)
    g = gq.cpu().numpy().reshape(-1)
    assert (np.isneginf(g).all() and np.isneginf(want_g)) if alpha > 0 else (np.isnan(g).all() and np.isnan(want_g))
    assert all(_pads_clean(f) for f in (f_gq, f_lo, f_aux))


def test_loss_wrapper_refuses_mis_shaped_operands():
    from core.common import hip_ops

    z = lambda *s: th.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(ValueError):
        hip_ops.td3bc_actor_loss(z(8, 1), z(8, 2), z(7, 2), 2.5, z(8, 1))
    with pytest.raises(ValueError):
        hip_ops.td3bc_actor_loss(z(8, 1), z(8, 2), z(8, 2), 2.5, z(7, 1))
    with pytest.raises(ValueError):
        hip_ops.td3bc_actor_loss(z(8, 1), z(8, 2), z(8, 2), 2.5, z(8, 1), aux=z(2))
    with pytest.raises(ValueError):
        hip_ops.td3bc_actor_loss(z(8, 1), z(2, 8).t(), z(8, 2), 2.5, z(8, 1))
    with pytest.raises(RuntimeError, match="cstr_td3bc_actor_loss_f32"):
        hip_ops.td3bc_actor_loss(z(8, 1), z(8, 9), z(8, 9), 2.5, z(8, 1))  # act_dim beyond the launch's width


# ------------------------------------------------------------------------------------ the backward-rows launch
@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("m", [1, 17, 256, 1030])
def test_act_bwd_rows_launch_bit_for_bit(m, n):
    from core.common import hip_ops

    rng = np.random.default_rng(100 * m + n)
    gy = rng.normal(0, 1e-2, (m, n)).astype(np.float32)
    gy[0, 0] = np.float32(-0.0)
    z = rng.normal(0, 1.2, (m, n)).astype(np.float32)
    act = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    coef = 2.0 / (m * n)
    for kind in (2, 0):
        y = np.tanh(z).astype(np.float32) if kind == 2 else z
        for extra in (0, 4):
            gyd, yd, ad = _rows_view(gy, extra), _rows_view(y, extra), _rows_view(act, extra)
            f, gz = _out(m, n)
            hip_ops.td3bc_act_bwd_rows(gyd, yd, ad, coef, kind, gz)
            th.cuda.synchronize()
            want = ref.act_bwd_rows_f32(gy, y, act, np.float32(coef), kind)
            assert np.array_equal(gz.cpu().numpy().view(np.uint32), want.view(np.uint32)), (kind, extra)
            assert _pads_clean(f)
            snap = f.clone()
            hip_ops.td3bc_act_bwd_rows(gyd, yd, ad, coef, kind, gz)
            th.cuda.synchronize()
            assert th.equal(f, snap)
            # coef = 0: the kernel it stands in for, bit for bit
            f0, gz0 = _out(m, n)
            hip_ops.td3bc_act_bwd_rows(gyd, yd, ad, 0.0, kind, gz0)
            base = hip_ops.bias_act_bwd_rows(gyd, yd, kind, th.empty(m, n, device=DEV)) if kind != 0 else gyd.contiguous()
            th.cuda.synchronize()
            assert th.equal(gz0.view(th.int32), base.view(th.int32)) and _pads_clean(f0)
    # ReLU keeps that kernel's expression too
    y = np.maximum(z, 0).astype(np.float32)
    f, gz = _out(m, n)
    hip_ops.td3bc_act_bwd_rows(_rows_view(gy, 4), _rows_view(y, 4), _rows_view(act, 4), coef, 1, gz)
    th.cuda.synchronize()
    assert np.array_equal(gz.cpu().numpy().view(np.uint32), ref.act_bwd_rows_f32(gy, y, act, np.float32(coef), 1).view(np.uint32)) and _pads_clean(f)


# ------------------------------------------------------------------------------------ datasets and models
def _raw_dataset(rows=2048, seed=3):
    """one seeded dataset on the host; observation columns of different offsets and widths, so that normalising matters"""
    rng = np.random.default_rng(seed)
    obs = (rng.uniform(-1, 1, (rows, 4)) * np.array([1.0, 0.5, 0.2, 1.0]) + np.array([0.1, -0.3, 0.5, 0.0])).astype(np.float32)
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
    from core.td3bc import TD3BC

    raw = _raw_dataset() if raw is None else raw
    pk = dict(kw.pop("policy_kwargs", {}))
    if arch is not None:
        pk.setdefault("net_arch", list(arch))
    model = TD3BC("MlpPolicy", _env(), dataset=_buffer(raw), seed=seed, batch_size=B, policy_kwargs=pk, **kw)
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
    from core.td3.policies import TD3Policy

    pk = {} if arch is None else dict(net_arch=list(arch))
    p = TD3Policy(*_spaces(), lambda _: 1e-3, **pk)
    p.load_state_dict({k: v.detach().cpu() for k, v in model.policy.state_dict().items()})
    return p.double()


_BATCHES = {}  # (arch, B, normalize) -> the sampled batches of the first path that ran: every path must draw the same ones


def _loss_bar_check(name, got, q_pi, pi, act, alpha, path):
    """the loss launch's bar on the launch's own inputs: 4 x the float32 torch evaluation's distance from fp64, floor 2 ulp"""
    want = ref.actor_loss_f64(q_pi, pi, act, alpha)
    aten = ref.actor_loss_torch(q_pi, pi, act, alpha, th.float32, device=DEV)
    out = {}
    for k in ("lam", "q_term", "bc", "loss"):
        bar = max(4 * abs(aten[k] - want[k]), 2 * _ulp(want[k]))
        out[k] = abs(got[k] - want[k]) / _ulp(want[k])
        assert abs(got[k] - want[k]) <= bar, (name, path, k, got[k], want[k], aten[k])
    return out


@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("tag", ["small", "default"])
def test_td3bc_teacher_forced(tag, normalize, path, monkeypatch):
    arch, B = ((64, 64), 64) if tag == "small" else (None, 256)
    raw = _raw_dataset()
    model = _model(raw, arch=arch, B=B, normalize_states=normalize)
    _select_path(monkeypatch, model, path)
    delay, n_steps = model.policy_delay, 3 * model.policy_delay
    assert (delay, model.alpha, model.tau, model.gamma, model.lr_schedule(1)) == (2, 2.5, 0.005, 0.99, 1e-3)
    refm = ref.RefTD3BC(_ref_policy(model, arch), 1e-3, model.gamma, model.tau, delay, model.target_noise_clip, model.alpha)
    mean, std = ref.statistics_f64(raw["observations"]) if normalize else (np.zeros(4), np.ones(4))
    if normalize:  # the statistics in float32 storage are what normalises: the fp64 statement uses the stored values
        mean, std = model.obs_mean.cpu().numpy().astype(np.float64), model.obs_std.cpu().numpy().astype(np.float64)
        m64, s64 = ref.statistics_f64(raw["observations"])
        assert np.abs(mean - m64).max() <= 2.0 ** -24 * np.abs(m64).max() and np.abs(std - s64).max() <= 2.0 ** -24 * np.abs(s64).max()
    index = {a.tobytes(): i for i, a in enumerate(raw["actions"])}
    assert len(index) == raw["actions"].shape[0]
    model.debug_capture = True
    gen = th.Generator().manual_seed(11)
    lab = f"td3bc_{tag}_{path}"
    key = (tag, normalize)
    for k in range(n_steps):
        noise = th.randn(B, 2, generator=gen) * model.target_policy_noise
        model.noise_queue = [noise.clone()]
        model.train(gradient_steps=1, batch_size=B)
        assert not model.noise_queue
        b = model._static_batch
        acts = b.actions.cpu().numpy()
        idx = np.array([index[r.tobytes()] for r in acts])
        batch = [getattr(b, n).cpu().numpy().copy() for n in ("observations", "actions", "next_observations", "rewards", "dones")]
        if (key, k) in _BATCHES:  # bit-equal across paths
            assert all(np.array_equal(x, y) for x, y in zip(batch, _BATCHES[(key, k)])), (lab, k)
        else:
            _BATCHES[(key, k)] = batch
        np.testing.assert_array_equal(batch[3][:, 0], raw["rewards"][idx])
        obs64, nobs64 = ref.normalize_f64(raw["observations"][idx], mean, std), ref.normalize_f64(raw["next_observations"][idx], mean, std)
        assert np.abs(batch[0] - obs64).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(obs64).max())  # the buffer holds the float32 normalisation
        want = refm.step(obs64, raw["actions"][idx], nobs64, raw["rewards"][idx][:, None], raw["dones"][idx][:, None], noise.numpy())
        t = model.last_train_tensors
        e_t = q_err(t["target_q"].cpu().numpy(), want["target_q"], lab)
        e_q = [q_err(t["current_q"][i].cpu().numpy(), want["current_q"][i], lab) for i in range(2)]
        e_c = rel_err(float(t["critic_loss"]), want["critic_loss"], 1e-3)
        lv = model.logger.name_to_value
        assert rel_err(float(lv["train/critic_loss"]), want["critic_loss"], 1e-3) < 1e-5
        line = f"{lab} norm={normalize} step {k}: target_q {e_t:.2e} q {e_q[0]:.2e} {e_q[1]:.2e} critic_loss {e_c:.2e}"
        assert e_t < 1e-5 and max(e_q) < 1e-5 and e_c < 1e-5, line
        if (k + 1) % delay == 0:
            assert t["actor_loss"] is not None and want["actor_loss"] is not None
            a = model.last_actor_tensors
            q_pi, pi, aux = a["q_pi"].cpu().numpy(), a["pi"].cpu().numpy(), a["aux"].cpu().numpy()
            e_qpi = q_err(q_pi, want["q_pi"], lab)
            e_pi = float(np.abs(pi - want["pi"]).max())
            assert e_qpi < 1e-5 and e_pi < 2e-5, (lab, k, e_qpi, e_pi)  # tanh-bounded outputs: tests/test_sde.py's bar
            got = dict(lam=float(aux[0]), q_term=float(aux[1]), bc=float(aux[2]), loss=float(t["actor_loss"]))
            ulps = _loss_bar_check(lab, got, q_pi, pi, acts, model.alpha, path)
            logged = dict(lam=float(lv["train/lambda"]), bc=float(lv["train/bc_loss"]), loss=float(lv["train/actor_loss"]))
            assert all(abs(logged[n] - got[n]) <= _ulp(got[n]) for n in logged), (logged, got)
            # and against the fp64 steps themselves, at what the bars of their inputs allow: Q1 within 1e-5 of its scale moves lam
            # and mean(q) by 1e-5 each; pi within 2e-5 moves mean((pi - a)^2) by at most 2 |pi - a| 2e-5 <= 8e-5
            assert rel_err(got["lam"], want["lam"], 1e-3) < 1e-5 and abs(got["bc"] - want["bc"]) < 8e-5
            assert abs(got["loss"] - want["actor_loss"]) < 8e-5 + 2e-5 * abs(want["q_term"])
            line += f" | q_pi {e_qpi:.2e} pi {e_pi:.2e} loss-launch ulps " + ", ".join(f"{n} {v:.2f}" for n, v in ulps.items())
        else:
            assert t["actor_loss"] is None and want["actor_loss"] is None
        print(line)
    assert model._n_updates == n_steps and model.actor.optimizer.step_count == n_steps // delay and model.critic.optimizer.step_count == n_steps
    worst = 0.0
    for nm in MODS:
        wsd = getattr(refm.p, nm).state_dict()
        for k, v in getattr(model.policy, nm).state_dict().items():
            got, w = v.detach().cpu().numpy().astype(np.float64), wsd[k].numpy()
            scale = max(float(np.abs(w).max()), 1e-3)
            worst = max(worst, float((np.abs(got - w) / (2e-5 * scale + 1e-4 * np.abs(w))).max()))
    print(f"{lab} norm={normalize}: weights after {n_steps} steps, worst err / (2e-5 scale + 1e-4 |w|) = {worst:.3f}")
    assert worst < 1.0, worst


# ------------------------------------------------------------------------------------ graph replay
def _digest(model):
    pol = model.policy
    parts = [pol.actor_arena.flat, pol.critic_arena.flat, pol.actor_target_arena.flat, pol.critic_target_arena.flat]
    for o in (model.actor.optimizer, model.critic.optimizer):
        parts += [o.exp_avg, o.exp_avg_sq, o.ctl[:1].float()]
    parts += [model.replay_buffer.sampler_stream.float(), model._loss_sum_buf]
    return [p.detach().clone() for p in parts]


@pytest.mark.parametrize("unroll", [1, 4])
def test_graph_replay_equals_eager(unroll):
    """4 * policy_delay + 1 iterations, eager against replayed (one graph per policy_delay residue and unroll rung). Every graph key
    warms up eagerly before it is recorded, so a first learn() of 16 iterations goes in front, in both runs alike: the compared 9 then
    start with recorded graphs (unroll 4: two replays of four bodies and an eager tail; unroll 1: replays throughout)."""
    outs = []
    warm, n = 16, 4 * 2 + 1
    for graph in (False, True):
        model = _model(B=64, seed=3)
        assert model.policy_delay == 2
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
            assert st["active"] and st["replays"] - before >= 8 and st["error"] is None, st
            # one graph per residue of the update counter; four bodies per graph keep the residue, so unroll 4 records residue 0 alone
            assert set(st["abi_launches_per_iteration"]) >= ({0, 1} if unroll == 1 else {0})
        else:
            assert st["replays"] == 0
        outs.append((start, _digest(model)))
    for a, b in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]):
        assert th.equal(a, b)
    assert not all(th.equal(a, b) for a, b in zip(outs[0][0], outs[0][1]))  # the nine iterations did change the state
    model.noise_queue = [th.zeros(64, 2)]  # a queued draw keeps the iteration eager
    assert not model._graph_eligible(model._noop_callback())
    model.noise_queue = []
    assert model._graph_eligible(model._noop_callback())


# ------------------------------------------------------------------------------------ launches and paths
def _abi_calls(fn) -> int:
    from core import _native as nv

    th.cuda.synchronize()
    before = nv.ABI_CALLS[0]
    fn()
    return nv.ABI_CALLS[0] - before


def test_actor_step_makes_as_many_abi_calls_as_td3s_with_its_loss_launch(monkeypatch):
    """TD3's per-layer actor step with -mean(Q1) as a launch of its own (the non-riding branch of PerLayerTwinCritic.neg_mean_pass)
    against TD3BC's: the loss launch and the last layer's backward launch are replaced one for one. Actor step = a train() call with
    the policy update minus one without, per model (the critic steps cancel)."""
    from core.common import fused, hip_ops
    from core.td3 import TD3

    calls = {}
    for name in ("td3bc_actor_loss", "td3bc_act_bwd_rows", "neg_mean_loss", "bias_act_bwd_rows"):
        orig = getattr(hip_ops, name)

        def wrapped(*a, _o=orig, _n=name, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _o(*a, **k)

        monkeypatch.setattr(hip_ops, name, wrapped)
    bc = _model(B=64)
    assert bc.fused_learner and bc._chain_for(64) is None
    bc.train(2, 64)  # scratch buffers exist from here on
    calls.clear()
    bc_plain, bc_actor = _abi_calls(lambda: bc.train(1, 64)), _abi_calls(lambda: bc.train(1, 64))
    assert bc._n_updates == 4 and calls == dict(td3bc_actor_loss=1, td3bc_act_bwd_rows=1), calls
    monkeypatch.setattr(fused, "USE_LOSS_ROOT", False)  # TD3's losses as launches of their own
    from core.common import chain

    monkeypatch.setattr(chain, "USE_CHAIN", False)      # ... on the per-layer path
    td3 = TD3("MlpPolicy", _env(4), seed=0, batch_size=64, buffer_size=4 * 64, learning_starts=0, policy_kwargs=dict(net_arch=[64, 64]))
    td3.learn(4 * 40)
    assert td3.fused_learner and td3._chain_for(64) is None
    td3._n_updates = 0
    td3.train(2, 64)
    calls.clear()
    td3_plain, td3_actor = _abi_calls(lambda: td3.train(1, 64)), _abi_calls(lambda: td3.train(1, 64))
    assert calls == dict(neg_mean_loss=1, bias_act_bwd_rows=1), calls
    print(f"ABI calls per train(): TD3BC {bc_plain} / {bc_actor} (without / with the actor step), TD3 per-layer, losses as launches: {td3_plain} / {td3_actor}")
    assert bc_actor - bc_plain == td3_actor - td3_plain and bc_actor > bc_plain


def test_path_selection(monkeypatch):
    from core.common import hip_ops

    calls = {}
    for name in ("td3bc_actor_loss", "td3bc_act_bwd_rows", "neg_mean_loss"):
        orig = getattr(hip_ops, name)

        def wrapped(*a, _o=orig, _n=name, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _o(*a, **k)

        monkeypatch.setattr(hip_ops, name, wrapped)
    model = _model(B=32, arch=(32, 32))
    assert model.fused_learner and model._chain_for(32) is None and type(model).chain_type is None
    model.train(gradient_steps=2, batch_size=32)  # one actor step
    assert calls == dict(td3bc_actor_loss=1, td3bc_act_bwd_rows=1), calls
    calls.clear()
    model.fused_learner = False
    model.train(gradient_steps=2, batch_size=32)
    assert not calls
    # three critics, one critic and another optimiser class take the torch statements
    for extra in (dict(n_critics=3), dict(n_critics=1), dict(optimizer_class=th.optim.AdamW)):
        calls.clear()
        m = _model(B=32, policy_kwargs=dict(net_arch=[32, 32], **extra))
        assert not m.fused_learner, extra
        m.debug_capture = True
        m.train(gradient_steps=2, batch_size=32)
        t, a = m.last_train_tensors, m.last_actor_tensors
        assert len(t["current_q"]) == extra.get("n_critics", 2) and t["actor_loss"] is not None and not calls
        assert all(bool(th.isfinite(v).all()) for v in (t["critic_loss"], t["actor_loss"], t["target_q"], a["aux"]))
        assert float(a["aux"][0]) > 0 and m._n_updates == 2


# ------------------------------------------------------------------------------------ dataset forms, normalisation, predict
def test_dataset_forms_and_the_callers_buffer(tmp_path):
    from core.common.save_util import save_to_pkl
    from core.td3bc import TD3BC

    raw = _raw_dataset(rows=300)
    src = _buffer(raw)
    before = _fields(src)
    pkl, npz = str(tmp_path / "data.pkl"), str(tmp_path / "data.npz")
    save_to_pkl(pkl, src)
    np.savez(npz, **{k: getattr(src, k).cpu().numpy() for k in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")})
    pk = dict(net_arch=[32, 32])
    m64, s64 = ref.statistics_f64(raw["observations"])
    for normalize in (True, False):
        models = []
        for dataset in (src, pkl, npz):
            m = TD3BC("MlpPolicy", _env(), dataset=dataset, seed=0, batch_size=32, policy_kwargs=pk, normalize_states=normalize)
            rb = m.replay_buffer
            assert rb.size() == 300 and rb.n_envs == 1 and m.n_envs == 1
            if normalize:
                assert rb is not src and rb.observations.data_ptr() != src.observations.data_ptr()
                np.testing.assert_allclose(m.obs_mean.cpu().numpy(), m64, rtol=2e-7, atol=1e-9)
                np.testing.assert_allclose(m.obs_std.cpu().numpy(), s64, rtol=2e-7)
                want = ref.normalize_f64(raw["observations"], m.obs_mean.cpu().numpy(), m.obs_std.cpu().numpy())
                np.testing.assert_allclose(rb.observations.cpu().numpy()[:, 0], want, rtol=0, atol=4 * 2.0 ** -24 * np.abs(want).max())
                wantn = ref.normalize_f64(raw["next_observations"], m.obs_mean.cpu().numpy(), m.obs_std.cpu().numpy())
                np.testing.assert_allclose(rb.next_observations.cpu().numpy()[:, 0], wantn, rtol=0, atol=4 * 2.0 ** -24 * np.abs(wantn).max())
            else:
                assert m.obs_mean is None and (dataset is not src or rb is src) and th.equal(rb.observations, src.observations)
            assert th.equal(rb.actions, src.actions) and th.equal(rb.rewards, src.rewards) and th.equal(rb.dones, src.dones)
            m.learn(3)
            assert m._n_updates == 3 and m.fused_learner
            models.append(m)
        for m in models[1:]:
            assert th.equal(m.replay_buffer.observations, models[0].replay_buffer.observations)
        # the caller's object: bit-identical after construction and after learning on the model's copy
        assert all(th.equal(a, b) for a, b in zip(before, _fields(src))), normalize
    # rows loaded later go through the same hook: normalised with the model's statistics (raw for a model that does not normalise)
    first = TD3BC("MlpPolicy", _env(), dataset=src, seed=0, batch_size=32, policy_kwargs=pk)
    want_obs, want_mean = first.replay_buffer.observations.clone(), first.obs_mean.clone()
    half = dict(raw, observations=(raw["observations"] * 0.5).astype(np.float32))
    save_to_pkl(pkl, _buffer(half))
    first.load_replay_buffer(pkl)
    assert th.equal(first.obs_mean, want_mean) and th.equal(first.policy.obs_norm[0], want_mean)
    assert th.equal(first.replay_buffer.observations, (th.as_tensor(half["observations"], device=DEV).reshape(300, 1, 4) - first.obs_mean) / first.obs_std)
    save_to_pkl(pkl, src)
    first.load_replay_buffer(pkl)
    assert th.equal(first.replay_buffer.observations, want_obs) and first.replay_buffer is not src
    first.learn(2)
    plain = TD3BC("MlpPolicy", _env(), dataset=src, seed=0, batch_size=32, policy_kwargs=pk, normalize_states=False)
    plain.load_replay_buffer(pkl)
    assert th.equal(plain.replay_buffer.observations, src.observations) and plain.obs_mean is None
    assert all(th.equal(a, b) for a, b in zip(before, _fields(src)))
    # statistics over the VALID rows only
    part = _buffer(raw)
    part._adds = 100
    part.ring.ctl[0], part.ring.ctl[1] = 100, 0
    m = TD3BC("MlpPolicy", _env(), dataset=part, seed=0, batch_size=32, policy_kwargs=pk)
    mp, sp = ref.statistics_f64(raw["observations"][:100])
    np.testing.assert_allclose(m.obs_mean.cpu().numpy(), mp, rtol=2e-7, atol=1e-9)
    np.testing.assert_allclose(m.obs_std.cpu().numpy(), sp, rtol=2e-7)
    assert m.replay_buffer.size() == 100


def test_predict_normalises_what_it_is_given():
    model = _model(B=32, arch=(32, 32))
    model.learn(4)
    rng = np.random.default_rng(0)
    obs = rng.uniform(-1, 1, (7, 4)).astype(np.float32)
    act, state = model.predict(obs, deterministic=True)
    assert state is None and act.shape == (7, 2)
    with th.no_grad():
        norm = (th.as_tensor(obs, device=DEV) - model.obs_mean) / model.obs_std
        want = model.policy.unscale_action(model.actor(norm).cpu().numpy())
        raw_net = model.policy.unscale_action(model.actor(th.as_tensor(obs, device=DEV)).cpu().numpy())
    np.testing.assert_array_equal(act, np.clip(want, model.action_space.low, model.action_space.high))
    assert np.abs(act - raw_net).max() > 1e-3
    off = _model(B=32, arch=(32, 32), normalize_states=False)
    act_off, _ = off.predict(obs, deterministic=True)
    with th.no_grad():
        want_off = off.policy.unscale_action(off.actor(th.as_tensor(obs, device=DEV)).cpu().numpy())
    np.testing.assert_array_equal(act_off, np.clip(want_off, off.action_space.low, off.action_space.high))


# ------------------------------------------------------------------------------------ learn(), checkpoints, callbacks
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
            "train/n_updates", "train/actor_loss", "train/critic_loss", "train/bc_loss", "train/lambda", "train/learning_rate"}
    for step, row in dumps.rows:
        assert set(row) == want, (step, sorted(row))
        assert row["dataset/size"] == 2048 and row["training/conservative_weight"] == 0.0 and row["train/n_updates"] == step
        assert all(np.isfinite(float(row[k])) for k in ("train/actor_loss", "train/critic_loss", "train/bc_loss", "train/lambda"))
        assert float(row["train/lambda"]) > 0 and float(row["train/bc_loss"]) > 0
    with pytest.warns(UserWarning, match="do not collect rollouts"):
        assert model.collect_rollouts(model.env, None, None, model.replay_buffer) is None

    class Stop(BaseCallback):
        def _on_step(self):
            return self.n_calls < 3

    stopped = _model(B=32, arch=(32, 32))
    stopped.learn(8, callback=Stop())
    assert stopped.num_timesteps == 3 and stopped._n_updates == 3
    # gradient_steps > 1: counters, and the logged values are means over the call's actor steps
    multi = _model(B=32, arch=(32, 32), gradient_steps=4)
    multi.debug_capture = True
    multi.learn(1)
    assert multi._n_updates == 4 and multi.actor.optimizer.step_count == 2
    lv = multi.logger.name_to_value
    sums = multi._loss_sum_buf.cpu().numpy().astype(np.float64)  # [actor | critic | lambda | -lambda mean(q) | bc] over the two actor steps
    assert float(lv["train/lambda"]) == pytest.approx(sums[2] / 2, rel=1e-6) and float(lv["train/bc_loss"]) == pytest.approx(sums[4] / 2, rel=1e-6)
    assert float(lv["train/actor_loss"]) == pytest.approx((sums[3] + sums[4]) / 2, rel=1e-5, abs=1e-6)
    assert float(multi.last_actor_tensors["aux"][0]) != pytest.approx(sums[2] / 2, rel=1e-7)  # a mean of two steps, not the last value


def test_checkpoint_round_trip_continues_identically(tmp_path):
    import json
    import zipfile

    from core.td3bc import TD3BC

    raw = _raw_dataset()
    model = _model(raw, B=32, arch=(32, 32), alpha=1.75)
    model.learn(5)
    path = str(tmp_path / "td3bc_ckpt")
    model.save(path)
    with zipfile.ZipFile(path + ".zip") as z:
        assert {"data", "policy.pth", "actor.optimizer.pth", "critic.optimizer.pth"} <= set(z.namelist())
        data = json.loads(z.read("data"))
    assert data["alpha"] == 1.75 and data["normalize_states"] is True and data["policy_delay"] == 2
    assert np.array_equal(np.asarray(data["obs_mean"], np.float32), model.obs_mean.cpu().numpy())
    assert np.array_equal(np.asarray(data["obs_std"], np.float32), model.obs_std.cpu().numpy())
    clone = TD3BC.load(path, env=_env(), dataset=_buffer(raw))
    # load() normalises the dataset it is given with the ARCHIVE's statistics, not with ones computed again
    other = TD3BC.load(path, env=_env(), dataset=_buffer(dict(raw, observations=(raw["observations"] * 0.5).astype(np.float32))))
    assert th.equal(other.obs_mean, model.obs_mean) and th.equal(other.obs_std, model.obs_std)
    assert clone._n_updates == 5 and clone.num_timesteps == 5 and clone.alpha == 1.75 and clone.normalize_states and clone.fused_learner
    assert th.equal(clone.obs_mean, model.obs_mean) and th.equal(clone.obs_std, model.obs_std)
    assert th.equal(clone.policy.obs_norm[0], model.obs_mean) and clone.policy.normalize_states
    assert th.equal(clone.replay_buffer.observations, model.replay_buffer.observations)
    assert list(clone.policy.state_dict()) == list(model.policy.state_dict())
    for a, b in zip(model.policy.state_dict().values(), clone.policy.state_dict().values()):
        assert th.equal(a, b)
    for name in ("actor", "critic"):
        o, c = getattr(model, name).optimizer, getattr(clone, name).optimizer
        assert o.step_count == c.step_count and th.equal(o.exp_avg, c.exp_avg) and th.equal(o.exp_avg_sq, c.exp_avg_sq)
    obs = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(model.predict(obs)[0], clone.predict(obs)[0])
    outs = []
    for m in (model, clone):
        m.set_random_seed(7)
        m.replay_buffer.seed_sampler(99)
        m.train(gradient_steps=3, batch_size=32)
        outs.append([p.detach().clone() for p in m.policy.parameters()])
    for a, b in zip(*outs):
        assert th.equal(a, b)
    raw_model = _model(raw, B=32, arch=(32, 32), normalize_states=False)
    raw_model.save(path + "_raw")
    again = TD3BC.load(path + "_raw", env=_env(), dataset=_buffer(raw))
    assert not again.normalize_states and again.obs_mean is None and again.policy.obs_norm is None


def test_every_refusal():
    from core.common.vec_env import VecNormalize
    from core.td3bc import TD3BC

    ds = _buffer(_raw_dataset(rows=64))
    with pytest.raises(ValueError, match="VecNormalize"):
        TD3BC("MlpPolicy", VecNormalize(_env()), dataset=ds)
    with pytest.raises(ValueError, match="does not support a Dict observation space"):
        TD3BC("MlpPolicy", _env(goal_conditioned=True, goal_range=(0.10, 0.40)), dataset=ds)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        TD3BC("MlpPolicy", _env(discrete_actions=3), dataset=ds)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        TD3BC("MlpPolicy", _env(multi_discrete_actions=(3, 5)), dataset=ds)
    with pytest.raises(ValueError, match="does not support gSDE"):
        TD3BC("MlpPolicy", _env(), dataset=ds, policy_kwargs=dict(use_sde=True))
    with pytest.raises(ValueError, match="the model does not support multiple envs"):
        TD3BC("MlpPolicy", _env(8), dataset=ds)
    from core.common import distributed as dist_util

    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            TD3BC("MlpPolicy", _env(), dataset=ds)
    finally:
        dist_util.rank_world = orig
    with pytest.raises(ValueError, match="Policy MultiInputPolicy unknown|MultiInputPolicy"):
        TD3BC("MultiInputPolicy", _env(), dataset=ds)
    with pytest.raises(ValueError, match="needs `env`"):
        TD3BC("MlpPolicy", None, dataset=ds)
    from core.common.buffers import ReplayBuffer

    with pytest.raises(ValueError, match="Loaded dataset is empty"):
        TD3BC("MlpPolicy", _env(), dataset=ReplayBuffer(64, *_spaces(), device=DEV, n_envs=1))
    m = TD3BC("MlpPolicy", _env(), dataset=ds, policy_kwargs=dict(net_arch=[32, 32]))
    assert m.conservative_weight == 0.0 and m.behavior_cloning_warmup == 0 and m.n_eval_episodes == 10


# ------------------------------------------------------------------------------------ evaluation
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


def test_fused_evaluation_against_the_loop_with_and_without_folding():
    """evaluate_policy_fused against evaluate_policy on TD3BC models, order and lengths equal, returns within a tolerance that is
    measured, not fixed: d0 = the worst |fused - loop| episode return of a plain TD3 model of the same shape and seed (two float32
    implementations of one network, propagated through the episodes). normalize_states=False gets 4 x d0. With folding, the first
    layer's pre-activation moves by the float32 storage of W1' and b1' (at most (sum_k |W1'_jk| + |b1'_j|) 2^-24 for |o| <= 1, the
    fp64 folded-vs-unfolded distance tests/test_td3bc_abi.py bounds) on top of the float32 evaluation's own rounding of that layer
    ((K + 1) roundings of terms of that size): a perturbation of the same kind at the same place, r = fold / own times as large, so
    the bar is 4 x d0 x (1 + r), both factors computed here from the model's weights. Floor for d0: one float32 ulp of a step reward
    per step, the resolution of the rewards the returns are sums of.
    Measured on MI355X: plain TD3 0 (floor 2.4e-6), TD3BC without normalisation 0 (bar 9.5e-6), with the folded first layer 1.0e-7
    (r = 3.75, bar 4.5e-5); the launch on the unfolded network differs from it by more than 100 bars."""
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import supported
    from core.td3 import TD3

    td3 = TD3("MlpPolicy", _env(1), seed=0, policy_kwargs=dict(net_arch=[64, 64]))
    loop, fused = _both_ways(td3)
    floor = 20 * _ulp(np.abs(loop).max() / 20)
    d0 = max(float(np.abs(loop - fused).max()), floor)
    raw = _raw_dataset()
    lines = [f"plain TD3 (64, 64), seed 0, 8 episodes of 20 steps on 4 envs: worst |fused - loop| return {float(np.abs(loop - fused).max()):.3e} "
             f"(floor {floor:.3e}); returns around {loop.mean():.3f}"]
    for normalize in (False, True):
        model = _model(raw, arch=(64, 64), B=64, normalize_states=normalize)
        assert supported(model, _short_env(4, 21))
        loop, fused = _both_ways(model)
        d = float(np.abs(loop - fused).max())
        r = 0.0
        if normalize:
            l1 = model.actor.mu[0]
            w, b = l1.weight.detach().cpu().numpy().astype(np.float64), l1.bias.detach().cpu().numpy().astype(np.float64)
            fw, fb = ref.fold_first_layer_f64(w, b, model.obs_mean.cpu().numpy(), model.obs_std.cpu().numpy())
            fold = ((np.abs(fw).sum(axis=1) + np.abs(fb)) * 2.0 ** -24).max()
            own = ((np.abs(w).sum(axis=1) + np.abs(b)) * 2.0 ** -24).max()  # one rounding of terms of the unfolded layer's size
            r = float(fold / own)
        bar = 4 * d0 * (1 + r)
        lines.append(f"TD3BC normalize_states={normalize}: worst |fused - loop| return {d:.3e}, bar {bar:.3e} (r = {r:.2f})")
        print(lines[-1])
        assert d <= bar, lines
        if normalize:  # the launch saw the folded network, not the raw one
            model.policy.normalize_states = False
            raw_fused = _fused_returns(model)
            model.policy.normalize_states = True
            assert np.abs(raw_fused - fused).max() > 100 * bar
            model.policy.obs_norm = None
            with pytest.raises(RuntimeError, match="statistics are missing"):
                supported(model, _short_env(4, 21))
            model.policy.obs_norm = (model.obs_mean, model.obs_std)
    print("\n".join(lines))
    # EvalCallback(fused=None) takes the launch for a TD3BC model
    model = _model(raw, arch=(32, 32), B=32)
    ev = EvalCallback(_short_env(4, 7), n_eval_episodes=4, eval_freq=5, verbose=0, warn=False)
    model.learn(10, callback=ev)
    assert ev.n_calls == 10 and np.isfinite(ev.last_mean_reward)


def _fused_returns(model, n_envs=4, episodes=8):
    from core.common.evaluation import evaluate_policy_fused

    return np.asarray(evaluate_policy_fused(model, _short_env(n_envs, 21), n_eval_episodes=episodes, return_episode_rewards=True, warn=False)[0], np.float64)


def test_one_launch_functions_cover_a_td3bc_model():
    from core.common.evaluation import evaluate_policy_fused, evaluate_trajectories
    from core.common.offline_dataset import collect_offline_dataset
    from core.td3bc import TD3BC

    model = _model(arch=(32, 32), B=32)
    model.learn(4)
    tr = evaluate_trajectories(model, _short_env(4, 3), n_eval_episodes=4)
    rets, lens = evaluate_policy_fused(model, _short_env(4, 3), n_eval_episodes=4, return_episode_rewards=True, warn=False)
    assert tr["states"].shape == (4, 20, 4) and list(tr["episode_lengths"]) == lens
    np.testing.assert_allclose(tr["episode_rewards"], rets, rtol=1e-6)
    rb, stats = collect_offline_dataset(model, _short_env(8, 5), num_episodes=16, random_action_prob=0.2, seed=1)
    assert rb.size() == 40 and rb.n_envs == 8 and stats["num_episodes"] >= 16
    before = _fields(rb)
    again = TD3BC("MlpPolicy", _env(), dataset=rb, seed=0, batch_size=32, policy_kwargs=dict(net_arch=[32, 32]))
    again.learn(50)
    th.cuda.synchronize()
    assert again._n_updates == 50 and again.fused_learner and all(bool(th.isfinite(p).all()) for p in again.policy.parameters())
    assert all(th.equal(a, b) for a, b in zip(before, _fields(rb)))
    from twoseriescstr import evaluate_model

    ep_rewards, ep_states = evaluate_model(again, _short_env(4, 3), num_episodes=4, plot=False)
    assert len(ep_rewards) == 4 and np.asarray(ep_states).shape == (4, 20, 4) and np.isfinite(ep_rewards).all()


# ------------------------------------------------------------------------------------ it learns the behaviour it was given
def test_td3bc_learns_the_behaviour_policy():
    """test_bcq_learns_the_behaviour_policy's dataset: actions = clip(tanh(obs K) + N(0, 0.05)), 20 000 rows, default_rng(0); after
    learn(1000) at the class defaults predict() is within 0.2 (mean absolute error) of tanh(obs K). The plain torch statement on the
    CPU reaches 0.060 / 0.066 / 0.080 (normalised) and 0.067 / 0.073 / 0.081 (raw) for seeds 0 / 1 / 2 from 0.44 - 0.46, lam ending
    at 0.21 - 0.23."""
    from core.common.buffers import ReplayBuffer
    from core.td3bc import TD3BC

    rng = np.random.default_rng(0)
    rows = 20_000
    K = rng.normal(0, 0.8, (4, 2))
    obs = rng.uniform(-1, 1, (rows, 4))
    act = np.clip(np.tanh(obs @ K) + rng.normal(0, 0.05, (rows, 2)), -1, 1)
    nobs = np.clip(obs + rng.normal(0, 0.05, (rows, 4)), -1, 1)
    rb = ReplayBuffer(rows, *_spaces(), device=DEV, n_envs=1)
    f = lambda a, *sh: th.as_tensor(a.astype(np.float32)).reshape(*sh)  # noqa: E731
    rb.observations.copy_(f(obs, rows, 1, 4)), rb.next_observations.copy_(f(nobs, rows, 1, 4)), rb.actions.copy_(f(act, rows, 1, 2))
    rb.rewards.copy_(f(rng.uniform(-8, 0, rows), rows, 1)), rb.dones.copy_(f((rng.uniform(size=rows) < 0.05).astype(np.float64), rows, 1))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    test_obs = rng.uniform(-1, 1, (200, 4)).astype(np.float32)
    for normalize in (True, False):
        model = TD3BC("MlpPolicy", _env(), dataset=rb, seed=0, normalize_states=normalize)
        assert model.fused_learner and model.batch_size == 256 and model.alpha == 2.5

        def score():
            pred = model.policy.scale_action(model.predict(test_obs)[0])
            return float(np.abs(pred - np.tanh(test_obs @ K)).mean())

        before = score()
        model.learn(1000)
        after = score()
        lam = float(model._loss_sums["lambda"])  # one gradient step per train(): the slot holds the last actor step's value
        print(f"behaviour cloning error, normalize_states={normalize}: untrained {before:.3f}, after learn(1000) {after:.3f}, lambda {lam:.3f}")
        assert model._n_updates == 1000
        assert after < 0.2, f"mean |predict - tanh(obs K)| = {after:.3f} after learn(1000) (untrained {before:.3f})"
        assert 0.05 < lam < 1.0, lam  # alpha / mean|Q1|: rewards in [-8, 0] put |Q| at a few units
