"""cstr_collect_episodes_f32 (a policy rolled out into replay-ring rows in one launch, optionally epsilon-uniform) through the C ABI
against the launches that already exist, bit for bit, and the functions built on it: `collect_offline_dataset`, `evaluate_trajectories`,
`evaluate_model` (the last against the reference-written fixture tests/golden/evaluate_model_kat.npz).

The step-by-step statement, per vec-step on a twin state and a twin ring: cstr_policy_rows_fwd_f32 on the same cstr_policy_mlp_t (head 0:
eps = 0); the rows the NumPy statement of the exploration draw (tests/_collect_reference.py) flags get its uniform action instead; for
unsquashed nets predict()'s clip; cstr_collect_step_f32 without noise. The host accounting on the twin ring's rewards / dones gives the
episode outputs (f64 sums of the f32 step rewards).

evaluate_model's bars (tools/collect_probe.py, profiles/collect_probe.txt): the yardstick is the step-by-step path that existed before the
launch -- `model.predict` + `env.step` on the GPU with the fixture's weights and seed -- whose distance to the float64-NumPy / CPU-torch
reference was measured per state component (max abs, raw units) and per episode reward; the bar is 4 x that distance (the project's
allowance for summation-order scatter), never below one float32 ulp of the component's span."""
import json
import os
import pickle

import numpy as np
import pytest
import torch as th

import _collect_reference as CR
from core import _native as nv
from core.common import hip_ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RELU, TANH, NONE = 1, 2, 0
UNIT = ((-1.0, -1.0), (1.0, 1.0))
SKEW = ((-1.0, -0.5), (0.5, 1.0))     # bounds other than (-1, 1) for a squashed actor
BOX = ((-0.5, -0.5), (0.25, 0.25))    # an unsquashed actor's box: narrow enough for the clip to engage
SENT = -777.25

# (n_envs, h1, h2, act, head, out_act, squashed, (low, high), integrator, tile-major W2, init_mode, episode limit, n_steps, explore_prob,
#  row0, ring rows, ep_stride, index_offset, step_offset, seed) -- the seeds of the mixed cases were chosen on the CPU so that the
# statement's own flags hold at least 20 explored and 20 policy rows (asserted below)
CASES = [
    (1, 16, 16, RELU, 0, NONE, True, UNIT, "euler", True, "random", 1, 1, 0.0, 0, 1, 2, 0, 0, 1),
    (16, 36, 20, TANH, 1, TANH, True, SKEW, "rk4", False, "static", 2, 5, 0.25, 2, 9, 3, 5, 3, 1),
    (17, 256, 256, RELU, 0, NONE, True, UNIT, "euler", True, "random", 3, 7, 1.0, 0, 7, 1, 0, 0, 2),
    (48, 400, 300, RELU, 1, NONE, False, BOX, "euler", True, "random", 3, 7, 0.25, 1, 9, 3, (1 << 32) - 20, 0, (3 << 32) + 1),
    (48, 256, 256, TANH, 1, TANH, True, SKEW, "rk4", False, "static", 2, 5, 0.25, 0, 5, 3, 0, (1 << 32) - 5, 1),
    (17, 36, 20, RELU, 0, NONE, True, SKEW, "rk4", True, "static", 1, 3, 0.0, 0, 3, 4, 0, 0, 1),
    (16, 16, 16, TANH, 1, NONE, False, BOX, "euler", False, "random", 400, 801, 0.25, 0, 801, 3, 0, 0, 1),
    (1, 400, 300, TANH, 0, NONE, True, UNIT, "euler", False, "random", 2, 5, 1.0, 0, 5, 3, 0, 0, 4),
    (17, 16, 16, RELU, 1, TANH, True, UNIT, "euler", True, "random", 3, 7, 0.0, 3, 12, 3, 0, 0, 1),
    (48, 36, 20, TANH, 0, NONE, True, SKEW, "euler", False, "random", 1, 3, 0.25, 0, 3, 1, 7, 0, 1),
    (16, 256, 256, RELU, 1, NONE, False, BOX, "rk4", True, "static", 2, 5, 1.0, 0, 5, 3, 0, 0, 6),
]


def _case_id(c):
    n, h1, h2, act, head, out_act, sq, bounds, integ, swz, init, limit, T, prob = c[:14]
    return (f"n{n}-{h1}x{h2}-{'relu' if act == RELU else 'tanh'}-head{head}-{'squashed' if sq else 'clipped'}-{integ}-{'swz' if swz else 'rows'}-"
            f"{init}-limit{limit}-T{T}-p{prob}")


def _pcg_words(seeds):
    m = (1 << 64) - 1
    words = np.empty((len(seeds), 4), np.uint64)
    for i, s in enumerate(seeds):
        st = np.random.PCG64(np.random.SeedSequence(int(s))).state["state"]
        words[i] = (st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)
    return th.from_numpy(words.view(np.int64)).to(DEV)


def _host_accounting(rew, done, stride):
    """ep_return [N, stride] (f64 sums of the f32 rewards), ep_len, ep_done of [T, N] rewards / dones; slots never reached keep SENT"""
    T, n = rew.shape
    ret, ln, cnt = np.full((n, stride), SENT), np.full((n, stride), -777, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        acc, k = 0.0, 0
        for t in range(T):
            acc += float(rew[t, i])
            k += 1
            if done[t, i] > 0:
                if cnt[i] < stride:
                    ret[i, cnt[i]], ln[i, cnt[i]] = acc, k
                cnt[i] += 1
                acc, k = 0.0, 0
    return ret, ln, cnt


class _Setup:
    """Weights, env state and the step-by-step result of one case (computed once, then only read)."""

    def __init__(self, case, nan_weight=False):
        (n, h1, h2, act, head, out_act, squashed, (low, high), integ, swz, init, limit, T, prob, row0, rows, stride, ioff, soff, seed) = case
        self.case, self.n = case, n
        g = th.Generator(device=DEV).manual_seed(1000 * n + h1 + h2 + 7 * head + limit)
        r = lambda *sh: th.randn(*sh, device=DEV, generator=g)  # noqa: E731
        n_out = 4 if head == 0 else 2
        self.w = [r(h1, 4) / 2.0, r(h1) * 0.1, r(h2, h1) / h1 ** 0.5, r(h2) * 0.1, r(n_out, h2) * (2.0 / h2 ** 0.5), r(n_out) * 0.1]
        if nan_weight:
            self.w[4][0, 0] = float("nan")
        self.swz = ops.policy_swizzle(self.w[2]) if swz else None
        self.coef = nv.default_coef(max_steps=limit)
        self.low, self.high = list(low), list(high)
        self.pcg0 = _pcg_words([11 + 3 * i for i in range(n)])
        self.static0 = None
        if init == "static":
            self.static0 = th.tensor([0.45, 310.0, 0.25, 290.0], dtype=th.float64, device=DEV).repeat(n, 1).contiguous()
        self.obs0 = th.zeros(n, 4, device=DEV)
        pcg, st = self.pcg0.clone(), None if self.static0 is None else self.static0.clone()
        ops.reset_draw(pcg, None, self.obs0, 2, static_init=st)  # the state env.reset() leaves
        self.pcg1, self.static1 = pcg, st
        self.flags, self.v = CR.explore_draw(seed, ioff, soff, T, n, prob, squashed, low, high)
        self._reference()

    def padded_state(self, pad=3):
        """(obs, steps, pcg, static) as views of sentinel-padded arrays, and the arrays themselves"""
        n = self.n
        obs = th.full((n + pad, 4), SENT, device=DEV)
        steps = th.full((n + pad,), -777, dtype=th.int32, device=DEV)
        pcg = th.full((n + pad, 4), -777, dtype=th.int64, device=DEV)
        static = None if self.static1 is None else th.full((n + pad, 4), SENT, dtype=th.float64, device=DEV)
        obs[:n], steps[:n], pcg[:n] = self.obs0, 0, self.pcg1
        if static is not None:
            static[:n] = self.static1
        return (obs[:n], steps[:n], pcg[:n], None if static is None else static[:n]), (obs, steps, pcg, static)

    def ring(self):
        rows = self.case[15]
        ring = ops.DeviceRing(rows, self.n, 4, 2, DEV)
        for f in (ring.observations, ring.next_observations, ring.actions, ring.rewards, ring.dones, ring.timeouts):
            f.fill_(SENT)
        return ring

    def _reference(self):
        (n, h1, h2, act, head, out_act, squashed, _, integ, swz, init, limit, T, prob, row0, rows, stride, ioff, soff, seed) = self.case
        (obs, steps, pcg, static), _ = self.padded_state(0)
        ring = self.ring()
        ring.ctl[0] = row0  # cstr_collect_step_f32 writes at the ring's position and advances it
        low, high = th.tensor(self.low, device=DEV), th.tensor(self.high, device=DEV)
        flags, v = th.from_numpy(self.flags).to(DEV), th.from_numpy(self.v).to(DEV)
        action, eps = th.empty(n, 2, device=DEV), (th.zeros(n, 2, device=DEV) if head == 0 else None)
        self.clipped = 0
        for t in range(T):
            ops.policy_rows_fwd(obs, *self.w, act, head, out_act, action, eps=eps, w2_swz=self.swz)
            u = th.where(flags[t][:, None], v[t], action)
            if not squashed:
                self.clipped += int(((u < low) | (u > high)).sum())
                u = th.minimum(th.maximum(u, low), high)  # np.clip: NaN passes through
            ops.collect_step(self.coef, integ, ring, obs, steps, u.contiguous(), int(squashed), self.low, self.high, pcg_state=pcg, static_init=static)
        self.ring_ref = [f.cpu().numpy() for f in (ring.observations, ring.next_observations, ring.actions, ring.rewards, ring.dones, ring.timeouts)]
        self.state_ref = [x.cpu().numpy() for x in (obs, steps, pcg)] + [None if static is None else static.cpu().numpy()]
        self.acc_ref = _host_accounting(self.ring_ref[3][row0:row0 + T], self.ring_ref[4][row0:row0 + T], stride)

    def launch(self, pad=3, T=None, row0=None, soff=None, state=None, ring=None, outputs=True):
        """One launch into sentinel-filled buffers; returns everything it may have written, on the host."""
        (n, h1, h2, act, head, out_act, squashed, _, integ, swz, init, limit, T0, prob, r0, rows, stride, ioff, s0, seed) = self.case
        T, row0, soff = T0 if T is None else T, r0 if row0 is None else row0, s0 if soff is None else soff
        (obs, steps, pcg, static), full = self.padded_state(pad) if state is None else state
        ring = self.ring() if ring is None else ring
        ret = th.full((n + pad, stride), SENT, dtype=th.float64, device=DEV) if outputs else None
        ln = th.full((n + pad, stride), -777, dtype=th.int32, device=DEV) if outputs else None
        dn = th.full((n + pad,), -777, dtype=th.int32, device=DEV)
        ex_full = th.full((rows * n + 16,), 7, dtype=th.uint8, device=DEV) if outputs else None
        ops.collect_episodes_into(*self.w, act, head, out_act, self.swz, self.coef, integ, obs, steps, pcg, squashed, self.low, self.high, ring, T, row0,
                                  prob, seed, ioff, soff, ret, ln, stride if outputs else 0, dn, None if ex_full is None else ex_full[:rows * n], static)
        host = lambda x: None if x is None else x.cpu().numpy()  # noqa: E731
        return dict(ring=[host(f) for f in (ring.observations, ring.next_observations, ring.actions, ring.rewards, ring.dones, ring.timeouts)],
                    state=[host(x) for x in full], ret=host(ret), ln=host(ln), dn=host(dn), ex=host(ex_full), keep=((obs, steps, pcg, static), full), ring_obj=ring)


_cache = {}


def _setup(case):
    if case not in _cache:
        _cache[case] = _Setup(case)
    return _cache[case]


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_matches(s, out, pad=3, T=None, row0=None, soff=0):
    n, stride, rows = s.n, s.case[16], s.case[15]
    for name, got, want in zip(("obs", "next_obs", "act", "rew", "done", "timeout"), out["ring"], s.ring_ref):
        assert _same(got, want), name  # rows outside row0 .. row0 + T - 1 keep the sentinel on both sides
    for name, got, want in zip(("env_obs", "step_count", "pcg_state", "static_init"), out["state"], s.state_ref):
        if want is not None:
            assert _same(got[:n], want), name
            assert (got[n:] == (SENT if got.dtype.kind == "f" else -777)).all(), name
    assert np.array_equal(out["dn"][:n], s.acc_ref[2]) and (out["dn"][n:] == -777).all()
    if out["ret"] is not None:
        assert _same(out["ret"][:n], s.acc_ref[0]) and _same(out["ln"][:n], s.acc_ref[1])  # f64 sums bit for bit; unreached slots keep the sentinel
        assert (out["ret"][n:] == SENT).all() and (out["ln"][n:] == -777).all()
        T, row0 = s.case[12] if T is None else T, s.case[14] if row0 is None else row0
        ex = out["ex"][:rows * n].reshape(rows, n)
        assert np.array_equal(ex[row0:row0 + T], s.flags[soff:soff + T].astype(np.uint8))
        assert (ex[:row0] == 7).all() and (ex[row0 + T:] == 7).all() and (out["ex"][rows * n:] == 7).all()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_collect_episodes_match_the_step_by_step_launches_bit_for_bit(case):
    s = _setup(case)
    (n, h1, h2, act, head, out_act, squashed, _, integ, swz, init, limit, T, prob, row0, rows, stride, ioff, soff, seed) = case
    if 0.0 < prob < 1.0:  # the mixed case's condition, on the statement's own flags
        assert s.flags.sum() >= 20 and (~s.flags).sum() >= 20, (int(s.flags.sum()), int((~s.flags).sum()))
    else:
        assert s.flags.all() == (prob == 1.0) and s.flags.any() == (prob == 1.0)
    if not squashed and prob < 1.0:
        assert s.clipped > 0  # the clip does something
    assert (s.ring_ref[4][row0:row0 + T].sum(axis=0) == T // limit).all()  # every env's episodes end at the limit
    if stride < T // limit:
        assert (s.acc_ref[2] > stride).all()  # episodes beyond ep_stride: counted, not stored
    out = s.launch()
    _assert_matches(s, out)
    again = s.launch()  # a relaunch from the same state: the same bits
    for k in ("ring", "state"):
        for x, y in zip(out[k], again[k]):
            assert (x is None and y is None) or _same(x, y)
    for k in ("ret", "ln", "dn", "ex"):
        assert _same(out[k], again[k])


def test_collect_episodes_two_launches_continue_one():
    """row0 / step_offset continuation: 3 + 4 vec-steps from the state the first launch left equal the 7 of one launch -- ring rows,
    env state and flags; the episode accounting restarts with each launch, so the first launch's outputs are those of its 3 steps."""
    case = CASES[3]
    s = _setup(case)
    T, row0, soff = case[12], case[14], case[18]
    first = s.launch(T=3)
    second = s.launch(T=T - 3, row0=row0 + 3, soff=soff + 3, state=first["keep"], ring=first["ring_obj"])
    for name, got, want in zip(("obs", "next_obs", "act", "rew", "done", "timeout"), second["ring"], s.ring_ref):
        assert _same(got, want), name
    for got, want in zip(second["state"], s.state_ref):
        if want is not None:
            assert _same(got[:s.n], want)
    rows, n = case[15], s.n
    assert np.array_equal(first["ex"][:rows * n].reshape(rows, n)[row0:row0 + 3], s.flags[:3].astype(np.uint8))
    assert np.array_equal(second["ex"][:rows * n].reshape(rows, n)[row0 + 3:row0 + T], s.flags[3:].astype(np.uint8))
    want = _host_accounting(s.ring_ref[3][row0:row0 + 3], s.ring_ref[4][row0:row0 + 3], case[16])
    assert _same(first["ret"][:n], want[0]) and _same(first["ln"][:n], want[1]) and np.array_equal(first["dn"][:n], want[2])


def test_collect_episodes_optional_outputs_left_out():
    """ep_stride = 0 without ep_return / ep_len, no `explored`: the ring, the env state and ep_done are the same."""
    s = _setup(CASES[1])
    out = s.launch(outputs=False)
    assert out["ret"] is None and out["ex"] is None
    _assert_matches(s, out)


def test_collect_episodes_nan_weight_takes_the_nan_path():
    """A NaN in the head's weights: every policy row takes the env's NaN path (old state, -10, truncated), every exploring row a normal
    step -- an episode per policy step, far more than ep_stride: counted, not stored."""
    case = (16, 36, 20, RELU, 1, TANH, True, UNIT, "euler", True, "random", 3, 7, 0.25, 0, 7, 2, 0, 0, 3)
    s = _Setup(case, nan_weight=True)
    rew, done = s.ring_ref[3], s.ring_ref[4]
    assert s.flags.sum() >= 20 and (~s.flags).sum() >= 20
    assert (rew[~s.flags] == -10.0).all() and (done[~s.flags] == 1.0).all() and (rew[s.flags] != -10.0).all()
    assert np.isnan(s.ring_ref[2][~s.flags][:, 0]).all() and not np.isnan(s.ring_ref[2][s.flags]).any()  # the NaN weight feeds valve 0
    assert (s.acc_ref[2] > 2).all()
    _assert_matches(s, s.launch())


def test_collect_episodes_wrapper_allocates_and_checks():
    s = _setup(CASES[1])
    (n, h1, h2, act, head, out_act, squashed, _, integ, swz, init, limit, T, prob, row0, rows, stride, ioff, soff, seed) = s.case
    (obs, steps, pcg, static), _ = s.padded_state(0)
    ring = s.ring()
    ret, ln, dn, ex = ops.collect_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, steps, pcg, squashed, s.low, s.high, ring, T, row0=row0,
                                           explore_prob=prob, seed=seed, index_offset=ioff, step_offset=soff, ep_stride=stride, static_init=static,
                                           record_explored=True)
    assert ret.shape == (n, stride) and ret.dtype == th.float64 and ln.dtype == th.int32 and ex.shape == (rows, n) and ex.dtype == th.uint8
    assert np.array_equal(dn.cpu().numpy(), s.acc_ref[2]) and np.array_equal(ex.cpu().numpy()[row0:row0 + T], s.flags.astype(np.uint8))
    filled = np.arange(stride)[None, :] < s.acc_ref[2][:, None]
    assert _same(ret.cpu().numpy()[filled], s.acc_ref[0][filled]) and (ret.cpu().numpy()[~filled] == 0).all()
    assert _same(ring.rewards.cpu().numpy(), s.ring_ref[3]) and ring.ctl.tolist() == [0, 0, 0, 0]  # the control words are the caller's
    out3 = ops.collect_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, steps, pcg, squashed, s.low, s.high, ring, 1)
    assert len(out3) == 3 and out3[0].shape == (n, 0)
    with pytest.raises(ValueError, match="rows"):
        ops.collect_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, steps, pcg, squashed, s.low, s.high, ring, T, row0=rows - T + 1)
    with pytest.raises(ValueError, match="pcg_state"):
        ops.collect_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, steps, pcg[:, :3].contiguous(), squashed, s.low, s.high, ring, T)
    with pytest.raises(ValueError, match="ring is"):
        ops.collect_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, steps, pcg, squashed, s.low, s.high, ops.DeviceRing(rows, n + 1, 4, 2, DEV), T)


# ---- collect_offline_dataset --------------------------------------------------------------------------------------------------------

def _short_env(n, seed, limit=7, **kw):
    from core.common.vec_env import CSTRVecEnv

    cls = type("Short", (CSTRVecEnv,), dict(max_steps=limit))
    env = cls(n, **kw)
    env.seed(seed)
    return env


def _models():
    from core.ppo import PPO
    from core.sac import SAC
    from core.td3 import TD3

    td3 = TD3("MlpPolicy", _short_env(8, 0), seed=0, batch_size=16, buffer_size=8 * 16, learning_starts=16, policy_kwargs=dict(net_arch=[16, 16]))
    td3.learn(8 * 6)  # briefly trained
    sac = SAC("MlpPolicy", _short_env(8, 0), seed=0, batch_size=16, buffer_size=8 * 16, policy_kwargs=dict(net_arch=[32, 32]))
    ppo = PPO("MlpPolicy", _short_env(4, 0), n_steps=8, batch_size=32, seed=1, device=DEV)
    with th.no_grad():
        ppo.policy.action_net.weight.mul_(40.0)  # drive some actions out of the box: the clip does something
    return dict(td3=td3, sac=sac, ppo=ppo)


@pytest.fixture(scope="module")
def models():
    return _models()


@pytest.mark.parametrize("name", ["td3", "sac", "ppo"])
def test_collect_offline_dataset_buffer_stats_and_files(models, name, tmp_path):
    from core.common.offline_dataset import collect_offline_dataset
    from core.common.save_util import load_from_pkl

    model, n, limit = models[name], 5, 7
    env = _short_env(n, 3)
    rb, stats = collect_offline_dataset(model, env, num_episodes=12, random_action_prob=0.25, dataset_path=str(tmp_path), dataset_name=name, seed=9)
    T = 3 * limit  # ceil(12 / 5) episodes per env
    assert rb.buffer_size == T and rb.n_envs == n and rb.pos == 0 and rb.full and rb.size() == T and rb.ring.ctl.tolist() == [0, 1, 0, T]
    assert tuple(rb.observations.shape) == (T, n, 4) and tuple(rb.actions.shape) == (T, n, 2) and tuple(rb.rewards.shape) == (T, n)
    rew, done = rb.rewards.cpu().numpy(), rb.dones.cpu().numpy()
    assert np.array_equal(done, rb.timeouts.cpu().numpy()) and np.array_equal(np.nonzero(done.sum(axis=1))[0], [6, 13, 20])
    rets = rew.reshape(3, limit, n).astype(np.float64).sum(axis=1).reshape(-1)
    assert stats["num_episodes"] == 15 and stats["total_transitions"] == T * n
    np.testing.assert_allclose([stats["mean_reward"], stats["std_reward"], stats["min_reward"], stats["max_reward"]],
                               [rets.mean(), rets.std(), rets.min(), rets.max()], rtol=1e-12)
    act, obs, nxt = rb.actions.cpu().numpy(), rb.observations.cpu().numpy(), rb.next_observations.cpu().numpy()
    assert np.isfinite(act).all() and np.abs(act).max() <= 1.0 and len(np.unique(act)) > 20  # scaled buffer actions, mixed policy
    assert np.array_equal(nxt[:limit - 1], obs[1:limit]) and not np.array_equal(nxt[limit - 1], obs[limit])  # terminal, not reset, observation
    assert np.array_equal(obs[limit], env_reset_after(n, 3, 1)) and np.array_equal(env.obs.cpu().numpy(), env_reset_after(n, 3, 3))
    assert env.step_count.tolist() == [0] * n
    with open(os.path.join(str(tmp_path), f"{name}_stats.json")) as f:
        assert json.load(f) == stats
    back = load_from_pkl(os.path.join(str(tmp_path), f"{name}_buffer.pkl"))
    again = pickle.loads(pickle.dumps(rb))
    for b in (back, again):
        assert b.pos == 0 and b.full and b.size() == T and b.n_envs == n
        for f in rb._FIELDS:
            assert th.equal(getattr(b, f), getattr(rb, f)), f
    # use_mixed_policy=False: the deterministic policy alone, whatever the probability says -- and it is reproducible
    rb0, _ = collect_offline_dataset(model, _short_env(n, 3), 12, 0.9, use_mixed_policy=False)
    rb1, _ = collect_offline_dataset(model, _short_env(n, 3), 12, 0.0)
    assert th.equal(rb0.actions, rb1.actions) and th.equal(rb0.rewards, rb1.rewards) and not th.equal(rb0.actions, rb.actions)


def env_reset_after(n, seed, resets):
    """observations of the `resets`-th auto-reset after env.reset() of an identically seeded env (random init: independent of the actions)"""
    env = _short_env(n, seed)
    env.reset_device()
    obs = th.empty(n, 4, device=DEV)
    for _ in range(resets):
        ops.reset_draw(env.pcg_state, None, obs, 2)
    return obs.cpu().numpy()


def test_bcq_trains_on_the_collected_dataset(models, tmp_path):
    from core.bcq import BCQ
    from core.common.offline_dataset import collect_offline_dataset

    rb, _ = collect_offline_dataset(models["td3"], _short_env(8, 1), 40, 0.1, dataset_path=str(tmp_path), dataset_name="d")
    for dataset in (rb, os.path.join(str(tmp_path), "d_buffer.pkl")):
        bcq = BCQ("MlpPolicy", _short_env(1, 0), dataset=dataset, seed=0, batch_size=16, policy_kwargs=dict(critic_net_arch=[16, 16]))
        bcq.learn(50)
        th.cuda.synchronize()
        assert bcq._n_updates == 50 and all(bool(th.isfinite(p).all()) for p in bcq.policy.parameters())


def test_collectors_decline_what_the_launch_does_not_cover(models):
    import twoseriescstr
    from core.bcq import BCQ
    from core.common.evaluation import evaluate_trajectories
    from core.common.offline_dataset import collect_offline_dataset
    from core.common.vec_env import VecNormalize
    from core.dqn import DQN
    from core.maddpg import MADDPG
    from core.ppo import PPO
    from core.sac import SAC

    env = _short_env(4, 0)
    sac = models["sac"]
    denv, menv = _short_env(4, 0, discrete_actions=3), _short_env(4, 0, multi_discrete_actions=(3, 5))
    genv = _short_env(4, 0, goal_conditioned=True, goal_range=(0.1, 0.4))
    bcq = BCQ("MlpPolicy", _short_env(1, 0), dataset=models["td3"].replay_buffer, seed=0, batch_size=16, policy_kwargs=dict(critic_net_arch=[16, 16]))
    maddpg = MADDPG(2, "MlpPolicy", env, [[0, 1], [2, 3]], [[0], [1]], learning_rate_list=[1e-3, 1e-3], seed=0, batch_size=16, buffer_size=64,
                    policy_kwargs=dict(net_arch=[[16, 16], [16, 16]]))
    declined = [
        (sac, VecNormalize(_short_env(4, 0))),                                                               # a VecNormalize wrapper
        (SAC("MlpPolicy", env, seed=0, use_sde=True, policy_kwargs=dict(net_arch=[16, 16])), env),           # gSDE
        (SAC("MlpPolicy", env, seed=0, policy_kwargs=dict(net_arch=[16, 16, 16])), env),                     # other depths
        (DQN("MlpPolicy", denv, seed=0, batch_size=16, buffer_size=64), denv),                               # the Discrete face
        (PPO("MlpPolicy", menv, n_steps=8, batch_size=32, seed=0, device=DEV), menv),                        # the MultiDiscrete face
        (PPO("MultiInputPolicy", genv, n_steps=8, batch_size=32, seed=0, device=DEV), genv),                 # the goal face
        (sac, genv),
        (bcq, env), (maddpg, env),
        (SAC("MlpPolicy", _short_env(4, 0, obs_dim=8), seed=0, policy_kwargs=dict(net_arch=[16, 16])), _short_env(4, 0, obs_dim=8)),  # (8, 2)
    ]
    for model, e in declined:
        with pytest.raises(ValueError, match="collect_offline_dataset does not cover"):
            collect_offline_dataset(model, e, 2)
        with pytest.raises(ValueError, match="evaluate_trajectories does not cover"):
            evaluate_trajectories(model, e, 2)
        with pytest.raises(ValueError, match="evaluate_model"):
            twoseriescstr.evaluate_model(model, e, 2, plot=False)
    with pytest.raises(ValueError, match="probability"):
        collect_offline_dataset(sac, env, 2, 1.5)
    with pytest.raises(ValueError, match="positive"):
        collect_offline_dataset(sac, env, 0)


# ---- evaluate_trajectories / evaluate_model -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["td3", "sac", "ppo"])
def test_evaluate_trajectories_against_the_fused_evaluation(models, name):
    from core.common.evaluation import evaluate_policy_fused, evaluate_trajectories
    from twoseriescstr import TwoSeriesCSTREnv as E

    model, n, limit = models[name], 4, 7
    env = _short_env(n, 5)
    tr = evaluate_trajectories(model, env, n_eval_episodes=8)  # splits evenly: two episodes per env
    rets, lens = evaluate_policy_fused(model, _short_env(n, 5), n_eval_episodes=8, return_episode_rewards=True, warn=False)
    assert tr["episode_rewards"].dtype == np.float64 and tr["episode_rewards"].tolist() == rets and tr["episode_lengths"].tolist() == lens == [limit] * 8
    assert tr["states"].shape == (8, limit, 4) and tr["actions"].shape == (8, limit, 2) and tr["rewards"].shape == (8, limit)
    assert all(v.dtype == np.float64 for v in (tr["states"], tr["actions"], tr["rewards"])) and not np.isnan(tr["states"]).any()
    twin = _short_env(n, 5)
    o0 = twin.reset_device().cpu().numpy()
    raw0 = E.raw_state_low + (o0 + np.float32(1.0)) * (E.raw_state_high - E.raw_state_low) / np.float32(2.0)
    assert np.array_equal(tr["states"][:n, 0], raw0.astype(np.float64))  # the first row is the reset state
    assert np.array_equal(tr["states"][n:, 0], (E.raw_state_low + (env_reset_after(n, 5, 1) + np.float32(1.0)) * (E.raw_state_high - E.raw_state_low)
                                                / np.float32(2.0)).astype(np.float64))
    assert (tr["actions"] >= 30.0).all() and (tr["actions"] <= 250.0).all()  # L/min
    assert np.array_equal(tr["rewards"].sum(axis=1), tr["episode_rewards"]) or np.allclose(tr["rewards"].sum(axis=1), tr["episode_rewards"], rtol=1e-12)
    # the env is left where the step-by-step loop leaves it: behind the auto-reset of its last episode
    assert np.array_equal(env.obs.cpu().numpy(), env_reset_after(n, 5, 2)) and env.step_count.tolist() == [0] * n
    # only the first n_eval_episodes by (end step, env) are returned
    tr5 = evaluate_trajectories(model, _short_env(n, 5), n_eval_episodes=5)
    assert tr5["states"].shape == (5, limit, 4) and np.array_equal(tr5["states"], tr["states"][:5]) and tr5["episode_rewards"].tolist() == rets[:5]


# Measured on the GPU by tools/collect_probe.py (profiles/collect_probe.txt): distance of the step-by-step path (model.predict + env.step
# with the fixture's weights and seed) to the fixture, and the bars = max(4 x distance, one float32 ulp of the component's span).
PARENT_STATE_DISTANCE = {"static": (8.940696716308594e-08, 3.0517578125e-05, 1.7881393432617188e-07, 3.0517578125e-05),  # [C1, T1, C2, T2]
                         "random": (4.172325134277344e-07, 3.0517578125e-05, 2.980232238769531e-07, 6.103515625e-05)}    # max abs, raw units
PARENT_REWARD_DISTANCE = {"static": 3.0517578125e-05, "random": 0.00018310546875}
SPAN_ULP = tuple(float(np.spacing(np.float32(s))) for s in (0.7, 400.0 - 273.15, 0.7, 400.0 - 273.15))
REWARD_ULP = float(np.spacing(np.float32(400.0)))  # |episode reward| < 400: one float32 ulp of the reference's float32 running sum


def _fixture_model(g):
    from core.td3 import TD3

    model = TD3("MlpPolicy", _short_env(1, 0, limit=400), seed=0, policy_kwargs=dict(net_arch=[16, 16]))
    with th.no_grad():
        for k, name in ((0, "1"), (2, "2"), (4, "3")):
            model.actor.mu[k].weight.copy_(th.from_numpy(g["w" + name]))
            model.actor.mu[k].bias.copy_(th.from_numpy(g["b" + name]))
    return model


@pytest.mark.parametrize("mode", ["static", "random"])
def test_evaluate_model_against_the_reference_fixture(golden, mode, capsys):
    import twoseriescstr
    from core.common.vec_env import CSTRVecEnv, DummyVecEnv

    g = golden("evaluate_model_kat.npz")
    env_seed, _, n_ep = (int(v) for v in g["dims"][:3])
    model = _fixture_model(g)
    env = DummyVecEnv([lambda: twoseriescstr.TwoSeriesCSTREnv(init_mode=mode)])
    assert isinstance(env, CSTRVecEnv)
    env.seed(env_seed)
    rewards, states = twoseriescstr.evaluate_model(model, env, num_episodes=n_ep, plot=False)
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == n_ep + 2 and printed[0].startswith("Episode 1 ") and str(np.mean(rewards)) in printed[-2]
    want_s, want_r = g[f"{mode}/episode_states"].astype(np.float64), g[f"{mode}/episode_rewards"]
    assert states.shape == want_s.shape == (n_ep, 400, 4) and len(rewards) == n_ep
    dist_s = np.abs(states - want_s).max(axis=(0, 1))
    dist_r = np.abs(np.asarray(rewards, np.float64) - want_r).max()
    bars = [max(4.0 * d, u) for d, u in zip(PARENT_STATE_DISTANCE[mode], SPAN_ULP)]
    bar_r = max(4.0 * PARENT_REWARD_DISTANCE[mode], REWARD_ULP)
    print(f"evaluate_model {mode}: state distance {dist_s.tolist()} (bars {bars}), reward distance {dist_r} (bar {bar_r})")
    assert (np.abs(states[:, 0] - want_s[:, 0]).max(axis=0) <= SPAN_ULP).all()  # the reset states: float64 draws rounded to float32 once
    assert (dist_s <= bars).all(), (dist_s.tolist(), bars)
    assert dist_r <= bar_r, (dist_r, bar_r)
    # the env's state afterwards is what the reference's loop leaves: per episode an explicit reset and the auto-reset at its end
    twin = CSTRVecEnv(1, init_mode=mode)
    twin.seed(env_seed)
    buf = th.empty(1, 4, device=DEV)
    for _ in range(n_ep):
        twin.reset_device()
        ops.reset_draw(twin.pcg_state, None, buf, 2, static_init=twin.static_init)
    assert th.equal(env.pcg_state, twin.pcg_state) and th.equal(env.obs, buf) and env.step_count.tolist() == [0]
    if mode == "static":
        assert th.equal(env.static_init, twin.static_init)


def test_evaluate_model_spreads_episodes_over_several_envs(models):
    import twoseriescstr
    from core.common.evaluation import evaluate_trajectories

    rewards, states = twoseriescstr.evaluate_model(models["td3"], _short_env(3, 2), num_episodes=5, plot=False)
    tr = evaluate_trajectories(models["td3"], _short_env(3, 2), 5)
    assert rewards == tr["episode_rewards"].tolist() and np.array_equal(states, tr["states"]) and states.shape == (5, 7, 4)
