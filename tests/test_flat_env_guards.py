"""The flat learner kernels (csrc/cstr_learner.hip), the env kernels (csrc/cstr_env.hip) and the ring / sampler kernels
(csrc/cstr_replay.hip) under guard (tests/_sentinel_bufs.py: GuardedBufs). Their values are already compared with the oracle and with
torch in tests/test_hip_kernels.py; here the same references are asserted at the sizes where a float4 body hands over to its scalar
tail (n = 1, 3, 4, 5, 1023, 1026) and at one env less / more than a wave (n_envs = 1, 63, 65), and the new assertions are the guards:
all arenas of a launch lie back to back in ONE block, so that one arena's tail overrun lands in the next arena's front band; ring
arrays, outputs and per-env state (int32 steps, uint64 PCG words included) have sentinel bands on both sides; ring rows other than
the one written keep their bits; inputs keep theirs; a second launch from the same state gives the same bits."""
import numpy as np
import pytest
import torch as th

from conftest import rel_err
from oracle import cstr_oracle as orc
from _sentinel_bufs import SENT, GuardedBufs
from test_hip_kernels import OBS_FLOOR, _twin_expected, obs8

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1026]
LAYOUTS = [(4, 2), (8, 2), (8, 4)]


@pytest.fixture(scope="module")
def ops():
    assert th.cuda.is_available()
    from core import _native as nv
    from core.common import hip_ops

    nv.lib()
    return hip_ops


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- learner kernels
@pytest.mark.parametrize("n", SIZES)
def test_polyak_guarded(ops, n):
    g = th.Generator().manual_seed(n)
    p, t = th.randn(n, generator=g), th.randn(n, generator=g)
    b = GuardedBufs()
    dp, dt = b.new_pack("arenas", [n, n])
    for tau in (0.005, 1.0):
        dp.copy_(p), dt.copy_(t)
        ops.polyak(dp, dt, tau)
        b.check(("arenas",))
        assert th.equal(dp.cpu(), p)
        np.testing.assert_array_equal(_np(dt), orc.polyak(p.numpy(), t.numpy(), tau))
        snap = b.snapshot()
        dt.copy_(t)
        ops.polyak(dp, dt, tau)
        b.check(("arenas",))
        b.same_as(snap)
    # 4-byte aligned arenas: refused (the float4 body would fault or tear), nothing written
    m = GuardedBufs()
    mp, mt, ap, at = m.put_ro("p", p, misalign=1), m.put_ro("t", t, misalign=1), m.put_ro("p16", p), m.put_ro("t16", t)
    for args in ((mp, at), (ap, mt)):
        with pytest.raises(RuntimeError):
            ops.polyak(*args, 0.005)
    m.check()


def _ulps(got, want):
    return np.abs(_np(got).view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("n", SIZES)
def test_adam_guarded(ops, n):
    """two steps of cstr_adam_f32 on [param | grad | exp_avg | exp_avg_sq] in one block, against the oracle at test_adam_vs_torch_and_oracle's
    bars: at most 4 ulp anywhere and 1e-6 against torch.optim.Adam; its third bar -- fewer than 1 in 1000 elements beyond 1 ulp -- is a
    statement about large arenas and is asked from 1000 elements on."""
    g = th.Generator().manual_seed(n)
    p0 = th.randn(n, generator=g)
    ref = th.nn.Parameter(p0.clone())
    opt = th.optim.Adam([ref], lr=3e-4)
    b = GuardedBufs()
    p, gr, m, v = b.new_pack("arenas", [n, n, n, n])
    p.copy_(p0), m.zero_(), v.zero_()
    ctl, lr = b.put("ctl", ops.new_adam_ctl("cuda"), dtype=th.int64), b.put_ro("lr", th.tensor([3e-4], dtype=th.float64), dtype=th.float64)
    op, om, ov = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in (1, 2):
        grad = th.randn(n, generator=g) * 0.1
        gr.copy_(grad)
        ref.grad = grad.clone()
        opt.step()
        before = [t.clone() for t in (p, m, v, ctl)]
        ops.adam(p, gr, m, v, ctl, lr)
        b.check(("arenas",))
        op, om, ov = orc.adam_step(op, grad.numpy(), om, ov, step, 3e-4)
        assert int(ctl[0]) == step and int(ctl[1]) == 0 and th.equal(gr.cpu(), grad)
        for got, want in ((p, op), (m, om), (v, ov)):
            u = _ulps(got, want)
            assert u.max() <= 4 and (n < 1000 or (u > 1).mean() < 1e-3)
        assert rel_err(_np(p), ref.detach().numpy(), 1e-3) < 1e-6
        snap = b.snapshot()
        for t, s in zip((p, m, v, ctl), before):
            t.copy_(s)
        ops.adam(p, gr, m, v, ctl, lr)
        b.check(("arenas",))
        b.same_as(snap)
    # misaligned arenas: refused, nothing written (the control words included)
    x = GuardedBufs()
    al = [x.put_ro(f"a{i}", p0) for i in range(4)]
    c2 = x.put_ro("ctl", ops.new_adam_ctl("cuda"), dtype=th.int64)
    for i in range(4):
        args = list(al)
        args[i] = x.put_ro(f"m{i}", p0, misalign=1)
        with pytest.raises(RuntimeError):
            ops.adam(*args, c2, lr)
    x.check()


@pytest.mark.parametrize("n", SIZES)
def test_adam_multi_guarded(ops, n):
    """cstr_adam_multi_f32 with an Adam segment of n elements carrying its own target (own_target), an Adam segment of ONE element, and a
    polyak segment of n + 1 elements, every arena of the launch in one block: bit for bit the separate cstr_adam_f32 / cstr_polyak_f32
    launches (test_multi_update_launch_equals_separate_calls / test_adam_segment_with_its_own_soft_target_update)."""
    g = th.Generator().manual_seed(100 + n)
    r = lambda k: th.randn(k, generator=g)  # noqa: E731
    b = GuardedBufs()
    names = ["p", "g", "m", "v", "own", "p1", "g1", "m1", "v1", "src", "tgt"]
    sizes = [n, n, n, n, n, 1, 1, 1, 1, n + 1, n + 1]
    d = dict(zip(names, b.new_pack("arenas", sizes)))
    init = {k: (th.zeros(s) if k in ("m", "v", "m1", "v1") else r(s)) for k, s in zip(names, sizes)}
    for k in names:
        d[k].copy_(init[k])
    sep = {k: v.clone().cuda() for k, v in init.items()}
    ca, cb = b.put("ctl_a", ops.new_adam_ctl("cuda", 0, 0.9, 0.999), dtype=th.int64), b.put("ctl_b", ops.new_adam_ctl("cuda", 0, 0.8, 0.99), dtype=th.int64)
    sa, sb = ops.new_adam_ctl("cuda", 0, 0.9, 0.999), ops.new_adam_ctl("cuda", 0, 0.8, 0.99)
    lra, lrb = th.tensor([3e-4], dtype=th.float64, device="cuda"), th.tensor([1e-2], dtype=th.float64, device="cuda")

    def multi():
        ops.adam_multi([(d["p"], d["g"], d["m"], d["v"], ca, lra, 0.9, 0.999, 1e-8, 1.0, None, (d["own"], 0.005)),
                        (d["p1"], d["g1"], d["m1"], d["v1"], cb, lrb, 0.8, 0.99, 1e-6, 0.5), ("polyak", d["src"], d["tgt"], 0.005)])

    for _ in range(2):
        ops.adam(sep["p"], sep["g"], sep["m"], sep["v"], sa, lra, 0.9, 0.999, 1e-8, 1.0)
        ops.polyak(sep["p"], sep["own"], 0.005)
        ops.adam(sep["p1"], sep["g1"], sep["m1"], sep["v1"], sb, lrb, 0.8, 0.99, 1e-6, 0.5)
        ops.polyak(sep["src"], sep["tgt"], 0.005)
        before = {k: d[k].clone() for k in names}
        cab, cbb = ca.clone(), cb.clone()
        multi()
        b.check(("arenas",))
        for k in names:
            assert th.equal(d[k], sep[k]), k
        assert th.equal(ca, sa) and th.equal(cb, sb)
        snap = b.snapshot()
        for k in names:
            d[k].copy_(before[k])
        ca.copy_(cab), cb.copy_(cbb)
        multi()
        b.check(("arenas",))
        b.same_as(snap)
    # one misaligned arena in any segment: the whole launch is refused, nothing written
    x = GuardedBufs()
    al = {k: x.put_ro(k, init[k]) for k in names}
    mis = {k: x.put_ro(k + "_mis", init[k], misalign=1) for k in ("p", "g", "m", "v", "own", "src", "tgt")}
    c3 = x.put_ro("ctl", ops.new_adam_ctl("cuda"), dtype=th.int64)
    for k in mis:
        a = dict(al)
        a[k] = mis[k]
        with pytest.raises(RuntimeError):
            ops.adam_multi([(a["p"], a["g"], a["m"], a["v"], c3, lra, 0.9, 0.999, 1e-8, 1.0, None, (a["own"], 0.005)),
                            ("polyak", a["src"], a["tgt"], 0.005)])
    x.check()


@pytest.mark.parametrize("sac", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_td_target_min_guarded(ops, n, sac):
    """cstr_td_target_min_f32 has no alignment term (scalar loads): the same launch on arenas 4 bytes off a 16-byte boundary must give the
    same bits."""
    g = th.Generator().manual_seed(n)
    q1, q2, lp = th.randn(n, generator=g) * 5, th.randn(n, generator=g) * 5, th.randn(n, generator=g)
    rew, done = -th.rand(n, generator=g) * 8, (th.rand(n, generator=g) < 0.2).float()
    exp = orc.td_target_min(q1.numpy(), q2.numpy(), lp.numpy() if sac else None, rew.numpy(), done.numpy(), 0.731, 0.99)
    outs = []
    for mis in (0, 1):
        b = GuardedBufs()
        arenas = b.new_pack("arenas", [n] * 6, misalign=mis)
        for t, s in zip(arenas, (q1, q2, lp, rew, done)):
            t.copy_(s)
        out = arenas[5]
        ent = b.put_ro("ent", th.tensor([0.731]))
        launch = lambda: ops.td_target_min(arenas[0], arenas[1], arenas[2] if sac else None, arenas[3], arenas[4], ent if sac else None, 0.99, out)  # noqa: E731
        launch()
        b.check(("arenas",))
        snap = b.snapshot()
        launch()
        b.check(("arenas",))
        b.same_as(snap)
        for t, s in zip(arenas, (q1, q2, lp, rew, done)):
            assert th.equal(t.cpu(), s)
        np.testing.assert_array_equal(_np(out), exp)
        outs.append(out.clone())
    assert th.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------ env and ring kernels
class GuardedRing:
    """hip_ops.DeviceRing with its six arrays and control words in guarded buffers"""

    def __init__(self, b, rows, n_envs, obs_dim, act_dim, tag="ring"):
        from core import _native as nv

        z = lambda name, *s: b.put(f"{tag}_{name}", th.zeros(*s))  # noqa: E731
        self.observations, self.next_observations = z("obs", rows, n_envs, obs_dim), z("next_obs", rows, n_envs, obs_dim)
        self.actions = z("act", rows, n_envs, act_dim)
        self.rewards, self.dones, self.timeouts = z("rew", rows, n_envs), z("done", rows, n_envs), z("timeout", rows, n_envs)
        self.ctl = b.put(f"{tag}_ctl", th.zeros(nv.RING_CTL_WORDS, dtype=th.int64), dtype=th.int64)
        self.rows, self.n_envs, self.obs_dim, self.act_dim = rows, n_envs, obs_dim, act_dim
        self.c = nv.Ring(self.observations.data_ptr(), self.next_observations.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr(),
                         self.dones.data_ptr(), self.timeouts.data_ptr(), rows, n_envs, obs_dim, act_dim)

    def fields(self):
        return (self.observations, self.next_observations, self.actions, self.rewards, self.dones, self.timeouts)

    def fill_random(self, seed):
        g = th.Generator().manual_seed(seed)
        for t in (self.observations, self.next_observations, self.actions, self.rewards):
            t.copy_(th.randn(t.shape, generator=g))
        self.dones.copy_((th.rand(self.rows, self.n_envs, generator=g) < 0.3).float())
        self.timeouts.copy_((th.rand(self.rows, self.n_envs, generator=g) < 0.5).float().cuda() * self.dones)


def _env_inputs(n, D, A, seed):
    rng = np.random.default_rng(seed)
    o4 = rng.uniform(-1, 1, (n, 4 if D == 8 and A == 2 else D)).astype(np.float32)
    r4 = rng.uniform(-1, 1, o4.shape).astype(np.float32)
    act = rng.uniform(-1.2, 1.2, (n, A)).astype(np.float32)
    steps = np.where(np.arange(n) % 3 == 0, 399, rng.integers(0, 398, n)).astype(np.int32)  # every third env ends its episode
    full = (lambda x: obs8(x)) if (D, A) == (8, 2) else (lambda x: x)  # noqa: E731
    return o4, r4, act, steps, full


def _env_expected(o4, act, steps, r4, D, A):
    """next_obs, obs_after (first 4 columns for the (8, 2) layout), reward, done, timeout, steps"""
    return _twin_expected(o4, act, steps, r4) if A == 4 else orc.vec_step(o4, act, steps, r4)


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("D,A", LAYOUTS)
def test_vec_step_guarded(ops, D, A, n):
    from core import _native as nv

    o4, r4, act, steps, full = _env_inputs(n, D, A, 10 * n + D + A)
    b = GuardedBufs()
    obs, ro, a = b.put_ro("obs", full(o4)), b.put_ro("reset_obs", full(r4)), b.put_ro("act", act)
    st = b.put("steps", steps, dtype=th.int32)
    nxt, after = b.new("next_obs", n, D), b.new("obs_after", n, D)
    rew, done, tout = b.new("reward", n), b.new("done", n), b.new("timeout", n)
    outs = ("next_obs", "obs_after", "reward", "done", "timeout")
    ops.vec_step(nv.default_coef(), "euler", obs, a, st, ro, nxt, after, rew, done, tout)
    b.check(outs)
    e = _env_expected(o4, act, steps, r4, D, A)
    w = 4 if (D, A) == (8, 2) else D
    assert rel_err(_np(nxt)[:, :w], e[0], OBS_FLOOR) < 5e-7 and rel_err(_np(after)[:, :w], e[1], OBS_FLOOR) < 5e-7
    assert rel_err(_np(rew), e[2], 1.0) < 2e-6
    np.testing.assert_array_equal(_np(done), e[3])
    np.testing.assert_array_equal(_np(tout), e[4])
    np.testing.assert_array_equal(_np(st), e[5])
    fin = e[3] > 0
    assert fin.any() and np.array_equal(_np(after)[fin], full(r4)[fin])  # the reset source, copied bit for bit (raw half included)
    snap = b.snapshot()
    st.copy_(th.as_tensor(steps))
    ops.vec_step(nv.default_coef(), "euler", obs, a, st, ro, nxt, after, rew, done, tout)
    b.check(outs)
    b.same_as(snap)
    # a 4-byte aligned observation matrix is refused: nothing written
    x = GuardedBufs()
    mo = x.put_ro("obs", full(o4), misalign=1)
    xs = x.put_ro("steps", steps, dtype=th.int32)
    xo = [x.new(k, n, D) for k in ("next_obs", "obs_after")] + [x.new(k, n) for k in ("reward", "done", "timeout")]
    with pytest.raises(RuntimeError):
        ops.vec_step(nv.default_coef(), "euler", mo, a, xs, ro, *xo)
    x.check()
    assert all(bool((t == SENT).all()) for t in xo)


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("D,A", LAYOUTS)
def test_reset_draw_guarded(ops, D, A, n):
    st = orc.pcg64_states_from_seeds(np.arange(100, 100 + n))
    b = GuardedBufs()
    dst = b.put("pcg", st.view(np.uint64).reshape(n, 4).view(np.int64), dtype="uint64")
    for rnd in range(2):
        mask = None if rnd == 0 else (np.arange(n) % 2 == 0).astype(np.uint8)
        dmask = None if mask is None else th.as_tensor(mask).cuda()
        out = b.new(f"obs_out{rnd}", n, D)
        dst_before = dst.clone()
        ops.reset_draw(dst, dmask, out, act_dim=A)
        b.check()
        exp = orc.reset_draw(st, mask)
        if A == 4:
            exp = np.concatenate([exp, orc.reset_draw(st, mask)], 1)  # train B continues the env's stream
        sel = np.ones(n, bool) if mask is None else mask.astype(bool)
        got = _np(out)
        np.testing.assert_array_equal(got[sel][:, :exp.shape[1]], exp[sel])
        if (D, A) == (8, 2):
            assert rel_err(got[sel][:, 4:], obs8(exp)[sel][:, 4:], 1.0) < 1e-6
        assert np.all(got[~sel] == np.float32(SENT))  # rows the mask leaves out are not written
        np.testing.assert_array_equal(_np(dst).view(np.uint64).reshape(-1), st.view(np.uint64).reshape(-1))
        assert dmask is None or np.array_equal(_np(dmask), mask)
        snap = b.snapshot()
        dst.copy_(dst_before)
        out.fill_(SENT)
        ops.reset_draw(dst, dmask, out, act_dim=A)
        b.check()
        b.same_as(snap)


def _ring_on_last_row(b, n, D, A, seed):
    ring = GuardedRing(b, 3, n, D, A)
    ring.fill_random(seed)
    ring.ctl[0] = 2  # the write cursor on the last row: this add wraps
    return ring


def _check_ring_add(ring, before, ctl_adds=1):
    """rows 0 and 1 keep their bits; the cursor wrapped"""
    for t, t0 in zip(ring.fields(), before):
        assert th.equal(t[:2], t0[:2])
    assert ring.ctl.tolist() == [0, 1, 0, ctl_adds]


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("D,A", LAYOUTS)
def test_replay_add_guarded(ops, D, A, n):
    rng = np.random.default_rng(n + D)
    f = [rng.uniform(-1, 1, (n, D)).astype(np.float32), rng.uniform(-1, 1, (n, D)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
         rng.uniform(-8, 0, n).astype(np.float32), (rng.uniform(size=n) < 0.3).astype(np.float32), (rng.uniform(size=n) < 0.2).astype(np.float32)]
    b = GuardedBufs()
    ring = _ring_on_last_row(b, n, D, A, n)
    ins = [b.put_ro(f"in{i}", x) for i, x in enumerate(f)]
    before = [t.clone() for t in ring.fields()]
    ops.replay_add(ring, *ins)
    b.check()
    _check_ring_add(ring, before)
    for t, x in zip(ring.fields(), f):
        np.testing.assert_array_equal(_np(t[2]), x)
    snap = b.snapshot()
    ring.ctl.copy_(th.tensor([2, 0, 0, 0]))
    ops.replay_add(ring, *ins)
    b.check()
    b.same_as(snap)


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("D,A", LAYOUTS)
def test_collect_step_guarded(ops, D, A, n):
    from core import _native as nv

    o4, r4, _, steps, full = _env_inputs(n, D, A, 20 * n + D + A)
    rng = np.random.default_rng(n)
    pol = np.tanh(rng.normal(0, 1.5, (n, A))).astype(np.float32)
    low, high = -np.ones(A, np.float32), np.ones(A, np.float32)
    b = GuardedBufs()
    ring = _ring_on_last_row(b, n, D, A, n + 1)
    env_obs, st = b.put("env_obs", full(o4)), b.put("steps", steps, dtype=th.int32)
    d_pol, d_reset = b.put_ro("policy_out", pol), b.put_ro("reset_obs", full(r4))
    rew_o, done_o = b.new("reward_out", n), b.new("done_out", n)
    before = [t.clone() for t in ring.fields()]

    def launch():
        ops.collect_step(nv.default_coef(), "euler", ring, env_obs, st, d_pol, True, low, high, reset_obs=d_reset, reward_out=rew_o, done_out=done_o)

    launch()
    b.check(("reward_out", "done_out"))
    _check_ring_add(ring, before)
    buf_a, env_a = orc.action_scale_chain(pol, True, low, high)
    e = _env_expected(o4, env_a, steps, r4, D, A)
    w = 4 if (D, A) == (8, 2) else D
    assert rel_err(_np(env_obs)[:, :w], e[1], OBS_FLOOR) < 5e-7 and rel_err(_np(ring.next_observations[2])[:, :w], e[0], OBS_FLOOR) < 5e-7
    np.testing.assert_array_equal(_np(ring.observations[2]), full(o4))
    np.testing.assert_array_equal(_np(ring.actions[2]), buf_a)
    np.testing.assert_array_equal(_np(ring.dones[2]), e[3])
    np.testing.assert_array_equal(_np(ring.timeouts[2]), e[4])
    np.testing.assert_array_equal(_np(done_o), e[3])
    np.testing.assert_array_equal(_np(st), e[5])
    assert rel_err(_np(ring.rewards[2]), e[2], 1.0) < 2e-6 and th.equal(rew_o, ring.rewards[2]) and (e[3] > 0).any()
    snap = b.snapshot()
    env_obs.copy_(th.as_tensor(full(o4))), st.copy_(th.as_tensor(steps)), ring.ctl.copy_(th.tensor([2, 0, 0, 0]))
    launch()
    b.check(("reward_out", "done_out"))
    b.same_as(snap)


@pytest.mark.parametrize("B", [1, 100])
@pytest.mark.parametrize("D,A", LAYOUTS)
def test_samplers_guarded(ops, D, A, B):
    """cstr_replay_sample_mt19937_f32, cstr_replay_sample_packed_mt19937_f32 and cstr_replay_gather_packed_f32 on a full 3-row ring of 65
    envs: indices against numpy's RandomState, gathered values against the ring itself, the ring and the index inputs bit-unchanged, and
    a second launch from the restored MT state the same bits."""
    n, W = 65, D + A
    b = GuardedBufs()
    ring = GuardedRing(b, 3, n, D, A)
    ring.fill_random(D * 10 + A + B)
    ring.ctl.copy_(th.tensor([0, 1, 0, 3]))
    for name in list(b.bufs):
        b.freeze(name)  # the samplers only read the ring
    mt = b.new("mt", 628, dtype=th.int32)
    ops.mt19937_seed(mt, 5)
    mt0 = mt.clone()
    rs = np.random.RandomState(5)
    ebi, eei = rs.randint(0, 3, size=B), rs.randint(0, n, size=B)
    bi, ei = th.as_tensor(ebi).cuda(), th.as_tensor(eei).cuda()
    want_done = (ring.dones * (1 - ring.timeouts))[bi, ei].reshape(B, 1)
    # plain sampler
    o, a, no = b.new("out_obs", B, D), b.new("out_act", B, A), b.new("out_next_obs", B, D)
    dn, rw = b.new("out_done", B, 1), b.new("out_rew", B, 1)
    ri, ci = b.new("row_idx", B, dtype=th.int64), b.new("env_idx", B, dtype=th.int64)
    names = ("out_obs", "out_act", "out_next_obs", "out_done", "out_rew", "row_idx", "env_idx")
    ops.replay_sample(ring, mt, B, o, a, no, dn, rw, ri, ci)
    b.check(names)
    assert np.array_equal(_np(ri), ebi) and np.array_equal(_np(ci), eei)
    assert th.equal(o, ring.observations[bi, ei]) and th.equal(a, ring.actions[bi, ei]) and th.equal(no, ring.next_observations[bi, ei])
    assert th.equal(dn, want_done) and th.equal(rw, ring.rewards[bi, ei].reshape(B, 1))
    snap, mt1 = b.snapshot(), mt.clone()
    mt.copy_(mt0)
    ops.replay_sample(ring, mt, B, o, a, no, dn, rw, ri, ci)
    b.check(names)
    b.same_as(snap)
    # packed sampler: the same draw into (obs | act), (next_obs | .), (obs | .) rows; the action columns of x_next / x_pi are not its
    xd, xn, xp = b.new("x_data", B, W), b.new("x_next", B, W), b.new("x_pi", B, W)
    pdn, prw = b.new("p_done", B, 1), b.new("p_rew", B, 1)
    pri, pci = b.new("p_row_idx", B, dtype=th.int64), b.new("p_env_idx", B, dtype=th.int64)
    mt.copy_(mt0)
    ops.replay_sample_packed(ring, mt, B, xd, xn, xp, pdn, prw, pri, pci)
    b.check(("x_data", "p_done", "p_rew", "p_row_idx", "p_env_idx"))
    assert th.equal(mt, mt1) and th.equal(pri, ri) and th.equal(pci, ci) and th.equal(pdn, dn) and th.equal(prw, rw)
    assert th.equal(xd[:, :D], o) and th.equal(xd[:, D:], a) and th.equal(xn[:, :D], no) and th.equal(xp[:, :D], o)
    assert bool((xn[:, D:] == SENT).all()) and bool((xp[:, D:] == SENT).all())
    snap = b.snapshot()
    mt.copy_(mt0)
    ops.replay_sample_packed(ring, mt, B, xd, xn, xp, pdn, prw, pri, pci)
    b.check()
    b.same_as(snap)
    # the gather alone, from index pairs given as int32 [2, B]
    idx = b.put_ro("sample_idx", np.stack([ebi, eei]), dtype=th.int32)
    gd, gn, gp = b.new("g_data", B, W), b.new("g_next", B, W), b.new("g_pi", B, W)
    gdn, grw = b.new("g_done", B, 1), b.new("g_rew", B, 1)
    ops.replay_gather_packed(ring, idx, B, gd, gn, gp, gdn, grw)
    b.check(("g_data", "g_done", "g_rew"))
    assert th.equal(gd, xd) and th.equal(gn, xn) and th.equal(gp, xp) and th.equal(gdn, dn) and th.equal(grw, rw)
    snap = b.snapshot()
    ops.replay_gather_packed(ring, idx, B, gd, gn, gp, gdn, grw)
    b.check()
    b.same_as(snap)
