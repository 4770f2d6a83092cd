"""CPU-side checks of cstr_collect_episodes_f32 (a policy rolled out into replay-ring rows in one launch) and of the functions built on
it: the symbol, every CSTR_E_BADARG / CSTR_E_UNSUPPORTED case of the header on pointers that are never dereferenced (the pattern of
tests/test_goal_eval_abi.py), the wrappers' refusals that need no device, the Python signatures, the NumPy restatement of the exploration
draw (tests/_collect_reference.py) against the existing Philox restatement, the host episode segmentation on synthetic arrays, and the
reference-written fixture tests/golden/evaluate_model_kat.npz against oracle/cstr_oracle.py driven by the fixture's own actions."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch as th

import _collect_reference as CR
from _rowkernel_reference import philox4x32_10
from conftest import rel_err
from core import _native as nv

BAD, UNS = -1, -2


def test_collect_episodes_symbol_is_exported():
    lib = nv.lib()
    assert "cstr_collect_episodes_f32" in nv.SYMBOLS and hasattr(lib, "cstr_collect_episodes_f32")
    assert nv.COLLECT_TAG == CR.COLLECT_TAG and nv.COLLECT_TAG not in (nv.HER_GOAL_TAG, 0x5DE5DE5D, 0xBC0BC0B1, 0x990A11C7, 0x3CA7A11C, 0xD09A11C7,
                                                                      0xCA7A11C7)


def test_collect_episodes_entry_point_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    coef = nv.default_coef()
    null = C.c_void_p(None)
    A = lambda i: C.c_void_p(0x100000 * (i + 1))  # noqa: E731  distinct, 16-byte aligned, 1 MiB apart: nothing overlaps
    off = lambda p, d: C.c_void_p(p.value + d)  # noqa: E731
    lo, hi = (C.c_float * 2)(-1, -1), (C.c_float * 2)(1, 1)
    good_net = dict(k0=4, h1=64, h2=64, act_dim=2, act=1, head=0, out_act=0, reserved=0, w1=A(0).value, b1=A(1).value, w2=A(2).value, b2=A(3).value,
                    w3=A(4).value, b3=A(5).value, w2_swizzled=A(6).value)
    good_ring = dict(obs=A(20).value, next_obs=A(21).value, act=A(22).value, rew=A(23).value, done=A(24).value, timeout=A(25).value, rows=12, n_envs=3,
                     obs_dim=4, act_dim=2)

    def call(net=None, ring=None, ring_ptr=True, coef_=C.byref(coef), integrator=0, obs_dim=4, env_obs=A(7), steps=A(8), pcg=A(9), static=null,
             squashed=1, lo_=lo, hi_=hi, row0=2, n=3, n_steps=10, prob=0.25, seed=(1 << 40) + 3, index_offset=5, step_offset=0, ret=A(10), ln=A(11),
             stride=4, dn=A(12), explored=A(13)):
        f = dict(good_net, **(net or {}))
        pm = nv.PolicyMlp(*[f[k] for k in ("k0", "h1", "h2", "act_dim", "act", "head", "out_act", "reserved", "w1", "b1", "w2", "b2", "w3", "b3",
                                           "w2_swizzled")])
        r = dict(good_ring, **(ring or {}))
        rg = nv.Ring(*[r[k] for k in ("obs", "next_obs", "act", "rew", "done", "timeout", "rows", "n_envs", "obs_dim", "act_dim")])
        return lib.cstr_collect_episodes_f32(C.byref(pm), coef_, integrator, obs_dim, env_obs, steps, pcg, static, squashed, lo_, hi_,
                                             C.byref(rg) if ring_ptr else null, C.c_int64(row0), C.c_int64(n), C.c_int64(n_steps), C.c_float(prob),
                                             C.c_uint64(seed), C.c_int64(index_offset), C.c_int64(step_offset), ret, ln, C.c_int64(stride), dn, explored,
                                             null)

    # NULL required pointers (static_init and explored are optional; ep_return / ep_len only with ep_stride == 0)
    rg0 = nv.Ring(*[good_ring[k] for k in ("obs", "next_obs", "act", "rew", "done", "timeout", "rows", "n_envs", "obs_dim", "act_dim")])
    assert lib.cstr_collect_episodes_f32(null, C.byref(coef), 0, 4, A(7), A(8), A(9), null, 1, lo, hi, C.byref(rg0), C.c_int64(0), C.c_int64(3),
                                         C.c_int64(5), C.c_float(0), C.c_uint64(0), C.c_int64(0), C.c_int64(0), A(10), A(11), C.c_int64(1), A(12),
                                         null, null) == BAD
    for kw in (dict(coef_=null), dict(env_obs=null), dict(steps=null), dict(pcg=null), dict(lo_=null), dict(hi_=null), dict(ring_ptr=False),
               dict(dn=null), dict(ret=null), dict(ln=null), dict(net=dict(w1=None)), dict(net=dict(b2=None)), dict(net=dict(w3=None)),
               dict(ring=dict(obs=None)), dict(ring=dict(next_obs=None)), dict(ring=dict(act=None)), dict(ring=dict(rew=None)),
               dict(ring=dict(done=None)), dict(ring=dict(timeout=None))):
        assert call(**kw) == BAD, kw
    # sizes and the row window
    assert call(n=0, ring=dict(n_envs=0)) == BAD and call(n=-3, ring=dict(n_envs=-3)) == BAD
    assert call(n_steps=0) == BAD and call(n_steps=-1) == BAD
    assert call(row0=-1) == BAD and call(row0=3) == BAD and call(n_steps=13, row0=0) == BAD and call(ring=dict(rows=0)) == BAD
    assert call(row0=(1 << 62), n_steps=(1 << 62)) == BAD
    # the ring is not this env's
    assert call(ring=dict(n_envs=4)) == BAD and call(ring=dict(obs_dim=8)) == BAD and call(ring=dict(act_dim=4)) == BAD
    # the exploration probability, the stream window, the episode slots
    for p in (-0.25, 1.5, float("nan"), float("inf")):
        assert call(prob=p) == BAD, p
    assert call(step_offset=-1) == BAD and call(step_offset=(1 << 32) - 9) == BAD and call(step_offset=1 << 32) == BAD
    assert call(stride=-1) == BAD
    assert call(squashed=2) == BAD and call(net=dict(reserved=1)) == BAD
    assert call(net=dict(k0=8)) == BAD and call(net=dict(k0=6)) == BAD  # the policy reads the env's observation rows
    assert call(hi_=(C.c_float * 2)(1, -1)) == BAD                       # empty action interval
    # misaligned arrays
    for kw in (dict(env_obs=off(A(7), 4)), dict(pcg=off(A(9), 8)), dict(ret=off(A(10), 4)), dict(ln=off(A(11), 2)), dict(dn=off(A(12), 2)),
               dict(steps=off(A(8), 2)), dict(static=off(A(14), 4)), dict(net=dict(w1=A(0).value + 4)), dict(net=dict(w2=A(2).value + 4)),
               dict(net=dict(w3=A(4).value + 8)), dict(net=dict(w2_swizzled=A(6).value + 8)), dict(ring=dict(obs=A(20).value + 8)),
               dict(ring=dict(next_obs=A(21).value + 4)), dict(ring=dict(act=A(22).value + 4)), dict(ring=dict(rew=A(23).value + 2)),
               dict(ring=dict(done=A(24).value + 1)), dict(ring=dict(timeout=A(25).value + 2))):
        assert call(**kw) == BAD, kw
    # anything written overlapping anything read, or anything else written
    for kw in (dict(ret=A(7)), dict(ln=A(9)), dict(dn=A(8)), dict(ret=A(2)), dict(explored=A(0)), dict(explored=A(10)), dict(env_obs=A(4)),
               dict(pcg=A(2)), dict(steps=A(1)), dict(static=A(9)), dict(static=A(3)), dict(ring=dict(obs=A(7).value)),
               dict(ring=dict(next_obs=A(20).value)), dict(ring=dict(act=A(9).value)), dict(ring=dict(rew=A(0).value)),
               dict(ring=dict(done=A(10).value)), dict(ring=dict(timeout=A(24).value)), dict(ring=dict(rew=A(13).value)),
               dict(ln=off(A(10), 16)), dict(dn=off(A(7), 32)), dict(explored=off(A(23), 8)), dict(ring=dict(next_obs=A(20).value + 16)),
               dict(ring=dict(act=A(12).value + 8))):
        assert call(**kw) == BAD, kw
    # unsupported layouts, integrators and network shapes
    assert call(obs_dim=8, net=dict(k0=8), ring=dict(obs_dim=8)) == UNS                             # (8, 2)
    assert call(obs_dim=8, net=dict(k0=8, act_dim=4), ring=dict(obs_dim=8, act_dim=4)) == UNS      # (8, 4)
    assert call(obs_dim=5, net=dict(k0=5), ring=dict(obs_dim=5)) == UNS and call(net=dict(act_dim=3), ring=dict(act_dim=3)) == UNS
    assert call(integrator=7) == UNS
    assert call(net=dict(h1=66)) == UNS and call(net=dict(act=3)) == UNS and call(net=dict(head=2)) == UNS and call(net=dict(out_act=5)) == UNS
    assert call(net=dict(h1=1024, h2=512)) == UNS                                                   # more than 64 KB of LDS


def test_collect_episodes_supported_shapes():
    from core.common import hip_ops as ops

    for h1, h2 in ((16, 16), (36, 20), (256, 256), (400, 300), (528, 32)):
        assert ops.collect_episodes_supported(4, h1, h2, 4, 0, 2) and ops.collect_episodes_supported(4, h1, h2, 2, 1, 2)
    assert not ops.collect_episodes_supported(8, 64, 64, 4, 0, 2) and not ops.collect_episodes_supported(8, 64, 64, 4, 1, 4)  # other layouts
    assert not ops.collect_episodes_supported(4, 64, 64, 2, 0, 2) and not ops.collect_episodes_supported(4, 66, 64, 4, 0, 2)
    assert not ops.collect_episodes_supported(4, 1024, 512, 4, 0, 2)


def test_collect_episodes_wrapper_refuses_host_tensors():
    from core.common import hip_ops as ops

    ring = ops.DeviceRing(4, 2, 4, 2, "cpu")
    w = [th.zeros(16, 4), th.zeros(16), th.zeros(16, 16), th.zeros(16), th.zeros(2, 16), th.zeros(2)]
    with pytest.raises(ValueError, match="HBM"):
        ops.collect_episodes(*w, 1, 1, 2, None, nv.default_coef(), "euler", th.zeros(2, 4), th.zeros(2, dtype=th.int32),
                             th.zeros(2, 4, dtype=th.int64), True, [-1, -1], [1, 1], ring, 4)
    # and what it checks before any tensor: the row window, the probability, the layout
    for kw, n_steps in ((dict(row0=1), 4), (dict(explore_prob=1.5), 4), (dict(step_offset=-1), 4), (dict(ep_stride=-1), 4), ({}, 0), ({}, 5)):
        with pytest.raises(ValueError):
            ops.collect_episodes(*w, 1, 1, 2, None, nv.default_coef(), "euler", th.zeros(2, 4), th.zeros(2, dtype=th.int32),
                                 th.zeros(2, 4, dtype=th.int64), True, [-1, -1], [1, 1], ring, n_steps, **kw)
    with pytest.raises(ValueError, match="layout"):
        ops.collect_episodes(th.zeros(16, 8), *w[1:], 1, 1, 2, None, nv.default_coef(), "euler", th.zeros(2, 8), th.zeros(2, dtype=th.int32),
                             th.zeros(2, 4, dtype=th.int64), True, [-1, -1], [1, 1], ring, 4)


def test_signatures_and_defaults_of_the_python_functions():
    import twoseriescstr
    from core.common import evaluation, offline_dataset

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert sig(offline_dataset.collect_offline_dataset) == [("model", E), ("env", E), ("num_episodes", 100), ("random_action_prob", 0.1),
                                                            ("use_mixed_policy", True), ("dataset_path", None), ("dataset_name", "offline_dataset"),
                                                            ("seed", 0)]
    assert sig(evaluation.evaluate_trajectories) == [("model", E), ("env", E), ("n_eval_episodes", 10)]
    assert sig(twoseriescstr.evaluate_model) == [("model", E), ("env", E), ("num_episodes", 10), ("plot", None)]
    # the functions that were there keep their signatures
    assert list(inspect.signature(evaluation.evaluate_policy_fused).parameters) == [
        "model", "env", "n_eval_episodes", "deterministic", "reward_threshold", "return_episode_rewards", "warn"]


# ---- the exploration draw's restatement ------------------------------------------------------------------------------------------

def test_philox_restatement_agrees_with_the_existing_one_on_shared_counters():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1 << 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
    c[0] = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, CR.COLLECT_TAG)
    c[1] = (0, 0, 0, 0)
    for key in ((9, 5), (0xFFFFFFFF, 0), (0x9E3779B9, 0xBB67AE85)):
        want = philox4x32_10(c, np.array(key, np.uint64))
        got = np.array([CR.philox_block(row, key) for row in c], np.uint32)
        assert np.array_equal(got, want)
    # the collector's counter layout: (idx lo, idx hi, step, tag), key = (seed lo, seed hi) -- with an index that carries into word 1 and
    # a seed above 2^32
    seed, off = (7 << 32) + 11, (1 << 32) - 2
    for i in range(4):
        idx = off + i
        row = np.array([[idx & 0xFFFFFFFF, idx >> 32, 17, CR.COLLECT_TAG]], np.uint32)
        assert tuple(philox4x32_10(row, np.array([11, 7], np.uint64))[0]) == CR.collect_block(seed, idx, 17)
    assert CR.collect_block(seed, off + 1, 17) != CR.collect_block(seed, off + 2, 17) != CR.collect_block(seed & 0xFFFFFFFF, off + 2, 17)
    assert CR.collect_block(seed, -1, 3) == CR.collect_block(seed, (1 << 64) - 1, 3)  # int64 index taken modulo 2^64, as the kernel's cast does


def test_explore_draw_flag_action_forms_and_continuation():
    low, high = [-0.5, 0.25], [0.25, 2.0]
    f, v = CR.explore_draw(3, 0, 0, 40, 5, 0.25, True, [-1, -1], [1, 1])
    assert f.shape == (40, 5) and v.shape == (40, 5, 2) and v.dtype == np.float32
    assert 20 <= f.sum() <= 80 and (v >= -1).all() and (v < 1).all()
    # both forms from the same words; the flag does not depend on the form
    f2, v2 = CR.explore_draw(3, 0, 0, 40, 5, 0.25, False, low, high)
    assert np.array_equal(f, f2)
    u = (v + np.float32(1)) / np.float32(2)  # exact: v = 2u - 1 with u a multiple of 2^-24
    lo32, hi32 = np.asarray(low, np.float32), np.asarray(high, np.float32)
    assert np.array_equal(v2, lo32 + (u * (hi32 - lo32)).astype(np.float32)) and (v2 >= lo32).all() and (v2 <= hi32).all()
    w = CR.collect_block(3, 2, 7)
    assert f[7, 2] == (CR.uniform(w[0]) < np.float32(0.25)) and v[7, 2, 0] == np.float32(2) * CR.uniform(w[1]) - np.float32(1)
    assert CR.uniform(0xFFFFFFFF) < 1 and CR.uniform(0xFF) == 0 and CR.uniform(0x100) == np.float32(2.0 ** -24)
    # probabilities 0 and 1
    f0, v0 = CR.explore_draw(3, 0, 0, 6, 3, 0.0, True, [-1, -1], [1, 1])
    f1, _ = CR.explore_draw(3, 0, 0, 6, 3, 1.0, True, [-1, -1], [1, 1])
    assert not f0.any() and not v0.any() and f1.all()
    # step_offset continuation: two halves equal one whole; index_offset shifts the envs
    fa, va = CR.explore_draw(3, 0, 0, 17, 5, 0.25, True, [-1, -1], [1, 1])
    fb, vb = CR.explore_draw(3, 0, 17, 23, 5, 0.25, True, [-1, -1], [1, 1])
    assert np.array_equal(np.concatenate([fa, fb]), f) and np.array_equal(np.concatenate([va, vb]), v)
    fo, vo = CR.explore_draw(3, 2, 0, 40, 3, 0.25, True, [-1, -1], [1, 1])
    assert np.array_equal(fo, f[:, 2:]) and np.array_equal(vo, v[:, 2:])
    # a counter carry in the index and a seed above 2^32 change the draw and stay reproducible
    fc, vc = CR.explore_draw((5 << 32) + 3, (1 << 32) - 2, (1 << 32) - 6, 6, 4, 0.5, True, [-1, -1], [1, 1])
    fd, vd = CR.explore_draw(3, (1 << 32) - 2, (1 << 32) - 6, 6, 4, 0.5, True, [-1, -1], [1, 1])
    assert not np.array_equal(vc, vd) and np.array_equal(vc, CR.explore_draw((5 << 32) + 3, (1 << 32) - 2, (1 << 32) - 6, 6, 4, 0.5, True, [-1, -1], [1, 1])[1])
    with pytest.raises(AssertionError):
        CR.collect_block(3, 0, 1 << 32)


# ---- the host episode segmentation ---------------------------------------------------------------------------------------------------

def _synthetic():
    T, N = 9, 3
    rew = (np.arange(T * N, dtype=np.float32).reshape(T, N) + np.float32(0.1)) * np.float32(0.37)
    done = np.zeros((T, N), np.float32)
    done[2, 1] = done[3, 0] = done[3, 2] = done[5, 1] = done[8, 0] = done[8, 1] = 1  # env 2's second episode does not end
    return rew, done


def test_segment_episodes_order_sums_and_nan_padding():
    from core.common.evaluation import pad_episodes, segment_episodes

    rew, done = _synthetic()
    spans, rets = segment_episodes(rew, done)
    assert spans == [(1, 0, 3), (0, 0, 4), (2, 0, 4), (1, 3, 3), (0, 4, 5), (1, 6, 3)]  # by the vec-step an episode ends at, then by env
    for (i, s, ln), r in zip(spans, rets):
        acc = 0.0
        for x in rew[s:s + ln, i]:
            acc += float(x)  # float64 sum of the float32 rewards, one add per step
        assert r == acc
    assert rets.dtype == np.float64
    field = np.arange(9 * 3 * 2, dtype=np.float32).reshape(9, 3, 2)
    pad = pad_episodes(field, spans)
    assert pad.shape == (6, 5, 2) and pad.dtype == np.float64
    assert np.array_equal(pad[0, :3], field[0:3, 1]) and np.isnan(pad[0, 3:]).all() and np.array_equal(pad[4], field[4:9, 0])
    assert np.isnan(pad).sum() == 2 * (2 + 1 + 1 + 2 + 0 + 2)
    none, r0 = segment_episodes(rew, np.zeros_like(done))
    assert none == [] and r0.shape == (0,) and pad_episodes(field, none).shape == (0, 0, 2)


def test_ended_returns_recomputes_when_an_env_overflows_its_slots():
    from core.common.evaluation import segment_episodes
    from core.common.offline_dataset import ended_returns, episode_stats

    rew, done = _synthetic()
    spans, rets = segment_episodes(rew, done)
    per_env = {i: [r for (e, _, _), r in zip(spans, rets) if e == i] for i in range(3)}
    ep_done = np.array([2, 3, 1], np.int32)

    def slots(stride):
        out = np.full((3, stride), -7.0)
        for i in range(3):
            out[i, :min(stride, len(per_env[i]))] = per_env[i][:stride]
        return out

    def never():
        raise AssertionError("the ring is only read back on overflow")

    got = ended_returns(slots(3), ep_done, never, never)       # every episode has a slot: the launch's values, env-major
    assert sorted(got.tolist()) == sorted(rets.tolist()) and got.tolist() == per_env[0] + per_env[1] + per_env[2]
    got = ended_returns(slots(2), ep_done, lambda: rew, lambda: done)  # env 1 ended 3 episodes, 2 slots: recomputed from the ring
    assert got.tolist() == rets.tolist()
    st = episode_stats(len(got), 27, got)
    assert list(st) == ["num_episodes", "total_transitions", "mean_reward", "std_reward", "min_reward", "max_reward"]
    assert st["num_episodes"] == 6 and st["total_transitions"] == 27 and st["mean_reward"] == float(np.mean(rets)) and st["max_reward"] == float(rets.max())


# ---- the reference-written fixture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["static", "random"])
def test_evaluate_model_fixture_states_follow_the_oracle_on_its_own_actions(golden, mode):
    """episode_states of the reference's evaluate_model are the states BEFORE each step: from row 0, the oracle env driven by the recorded
    actions reproduces rows 1 .. 399 at the bound tests/test_oracle_env.py asserts for 400-step trajectories (1e-5 relative to the box)."""
    from oracle import cstr_oracle as orc

    g = golden("evaluate_model_kat.npz")
    states, actions = g[f"{mode}/episode_states"], g[f"{mode}/actions"]
    assert states.shape == (3, 400, 4) and actions.shape == (3, 400, 2) and g[f"{mode}/episode_rewards"].shape == (3,)
    lo, hi = np.array([0.0, 273.15, 0.0, 273.15]), np.array([0.7, 400.0, 0.7, 400.0])
    norm = 2.0 * (states.astype(np.float64) - lo) / (hi - lo) - 1.0
    obs, steps = norm[:, 0].astype(np.float32), np.zeros(3, np.int32)
    worst, ret = 0.0, np.zeros(3)
    for k in range(400):
        nxt, _, rew, done, tout, steps = orc.vec_step(obs, actions[:, k], steps, reset_obs=obs)
        ret += rew
        if k < 399:
            worst = max(worst, rel_err(nxt, norm[:, k + 1], 1.0))
            assert not done.any()
        obs = nxt
    assert done.all() and tout.all() and worst < 1e-5, worst
    assert rel_err(ret, g[f"{mode}/episode_rewards"], 1.0) < 1e-4  # 400 float32 adds on the reference's side
    assert len({tuple(s) for s in states[:, 0]}) == 3                # three different reset states


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------

def test_evaluate_model_and_collect_refuse_without_touching_a_device():
    import twoseriescstr
    from core.common import evaluation, offline_dataset

    class NotAnEnv:
        num_envs = 1

    for f, kw in ((twoseriescstr.evaluate_model, {}), (twoseriescstr.evaluate_model, dict(plot=False))):
        with pytest.raises(ValueError, match="CSTRVecEnv"):
            f(object(), NotAnEnv(), **kw)
    with pytest.raises(ValueError, match="bare CSTRVecEnv"):
        offline_dataset.collect_offline_dataset(object(), NotAnEnv())
    with pytest.raises(ValueError, match="bare CSTRVecEnv"):
        evaluation.evaluate_trajectories(object(), NotAnEnv())
