"""CPU-side checks of HER: the three entry points of csrc/cstr_her.hip are exported and reject bad arguments on the host (nothing is
dereferenced or launched), `from core import HerReplayBuffer` resolves, the `Dict` space, the goal face's reward statement and
`her_ratio` / `nb_virtual`, and the NumPy restatement of tests/_her_reference.py against the fixture written by the unmodified reference
(tests/golden/her_buffer_kat.npz, tools/refharness/gen_golden.py --only her), bit for bit: bookkeeping after every add, drawn indices,
goal indices, the five outputs and the MT19937 state after every seeded sample, and the truncate_last_trajectory case. The restatement
is the yardstick of the GPU tests (tests/test_her.py), so it is checked here first."""
import ctypes as C
import os

import numpy as np
import pytest

from _her_reference import HerNp, goal_of_target, goal_reward, mt_image
from core import _native as nv

i64, f32, u64 = C.c_int64, C.c_float, C.c_uint64
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
HER_SYMBOLS = ("cstr_goal_vec_step_f32", "cstr_her_add_f32", "cstr_her_sample_f32")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "her_buffer_kat.npz")
TAGS = ("r4a", "r4b", "r12a", "r12b")


def P(k: int) -> C.c_void_p:
    """the k-th of a set of fake, well separated, 256-byte-aligned device addresses (never dereferenced)"""
    return C.c_void_p(0x1000000 * (k + 1))


def off(p: C.c_void_p, nbytes: int) -> C.c_void_p:
    return C.c_void_p(p.value + nbytes)


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(GOLDEN))


def test_her_symbols_declared_and_exported():
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in HER_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive


def step(coef=None, integ=0, d=4, obs=P(0), act=P(1), st=P(2), pcg=P(3), init=null, tgt=P(4), ep=null, lo=0.1, hi=0.4, nxt=P(5), after=P(6),
         rew=P(7), done=P(8), tout=P(9), n=64):
    coef = C.byref(nv.default_coef()) if coef is None else coef
    return nv.lib().cstr_goal_vec_step_f32(coef, integ, d, obs, act, st, pcg, init, tgt, ep, u64(0), i64(0), f32(lo), f32(hi), nxt, after, rew,
                                           done, tout, i64(n), null)


def test_goal_step_rejects_bad_arguments_on_the_host():
    for name in ("coef", "obs", "act", "st", "pcg", "tgt", "nxt", "after", "rew", "done", "tout"):
        assert step(**{name: null}) == BAD, name
    assert step(n=0) == BAD and step(n=-3) == BAD
    assert step(d=8) == UNSUP and step(d=6) == UNSUP and step(integ=2) == UNSUP
    assert step(obs=off(P(0), 8)) == BAD and step(act=off(P(1), 4)) == BAD and step(nxt=off(P(5), 4)) == BAD and step(after=off(P(6), 4)) == BAD
    assert step(pcg=off(P(3), 8)) == BAD and step(tgt=off(P(4), 2)) == BAD and step(ep=off(P(10), 2)) == BAD
    assert step(after=P(5)) == BAD and step(after=off(P(5), 24 * 63)) == BAD  # the two outputs overlap
    assert step(nxt=P(0)) == BAD and step(after=off(P(0), 16 * 32)) == BAD    # an output on the env state
    assert step(ep=P(10), lo=0.4, hi=0.1) == BAD


def ring(obs=P(20), nxt=P(21), act=P(22), rew=P(23), done=P(24), tout=P(25), rows=12, n=3, d=4, a=2):
    return nv.Ring(obs.value, nxt.value, act.value, rew.value, done.value, tout.value, rows, n, d, a)


def her(goal=P(30), start=P(31), length=P(32), cur=P(33), valid=P(34), bits=P(35)):
    return nv.Her(goal.value, start.value, length.value, cur.value, valid.value, bits.value)


def add(r=None, h=None, ctl=P(40), obs=P(41), nxt=P(42), act=P(43), rew=P(44), done=P(45), tout=P(46)):
    r, h = ring() if r is None else r, her() if h is None else h
    return nv.lib().cstr_her_add_f32(C.byref(r), C.byref(h), ctl, obs, nxt, act, rew, done, tout, null)


def test_add_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    assert lib.cstr_her_add_f32(null, C.byref(her()), P(40), P(41), P(42), P(43), P(44), P(45), P(46), null) == BAD
    assert lib.cstr_her_add_f32(C.byref(ring()), null, P(40), P(41), P(42), P(43), P(44), P(45), P(46), null) == BAD
    for name in ("ctl", "obs", "nxt", "act", "rew", "done", "tout"):
        assert add(**{name: null}) == BAD, name
    for name in ("obs", "nxt", "act", "rew", "done", "tout"):
        assert add(r=ring(**{name: null})) == BAD, name
    for name in ("goal", "start", "length", "cur", "valid", "bits"):
        assert add(h=her(**{name: null})) == BAD, name
    assert add(r=ring(rows=0)) == BAD and add(r=ring(n=0)) == BAD
    assert add(r=ring(d=8)) == UNSUP and add(r=ring(d=8, a=4)) == UNSUP and add(r=ring(d=6)) == UNSUP
    assert add(r=ring(rows=nv.HER_MAX_ROWS + 1)) == UNSUP and add(r=ring(rows=8192, n=1 << 18)) == UNSUP  # 2^31 transitions
    assert add(r=ring(obs=off(P(20), 8))) == BAD and add(r=ring(act=off(P(22), 4))) == BAD and add(h=her(bits=off(P(35), 4))) == BAD
    assert add(obs=off(P(41), 4)) == BAD and add(nxt=off(P(42), 4)) == BAD and add(act=off(P(43), 4)) == BAD and add(h=her(start=off(P(31), 2))) == BAD
    assert add(obs=off(P(20), 16 * 5)) == BAD and add(nxt=off(P(21), 16 * 35)) == BAD  # input rows inside the ring


def sample(coef=None, r=None, h=None, mt=P(50), b=10, nbv=8, strat=0, frow=null, fenv=null, fgoal=null, obs=P(51), act=P(52), nxt=P(53),
           done=P(54), rew=P(55), status=P(56)):
    coef = C.byref(nv.default_coef()) if coef is None else coef
    r, h = ring() if r is None else r, her() if h is None else h
    return nv.lib().cstr_her_sample_f32(coef, C.byref(r), C.byref(h), mt, i64(b), i64(nbv), strat, frow, fenv, fgoal, obs, act, nxt, done, rew,
                                        null, null, null, status, null)


def test_sample_rejects_bad_arguments_on_the_host():
    for name in ("coef", "mt", "obs", "act", "nxt", "done", "rew", "status"):
        assert sample(**{name: null}) == BAD, name
    assert sample(b=0) == BAD and sample(b=-1) == BAD
    assert sample(nbv=11) == BAD and sample(nbv=-1) == BAD       # nb_virtual > batch
    assert sample(strat=3) == BAD and sample(strat=-1) == BAD    # unknown strategy
    assert sample(r=ring(d=8)) == UNSUP and sample(r=ring(d=8, a=4)) == UNSUP and sample(b=nv.HER_MAX_BATCH + 1, nbv=0) == UNSUP
    assert sample(r=ring(rows=nv.HER_MAX_ROWS + 1)) == UNSUP
    assert sample(r=ring(rows=0)) == BAD and sample(h=her(length=null)) == BAD and sample(r=ring(nxt=null)) == BAD
    assert sample(frow=P(57)) == BAD and sample(fenv=P(58)) == BAD and sample(fgoal=P(59)) == BAD  # the pair goes together; goals need it
    assert sample(obs=off(P(51), 4)) == BAD and sample(nxt=off(P(53), 4)) == BAD and sample(act=off(P(52), 4)) == BAD
    assert sample(done=off(P(54), 2)) == BAD and sample(status=off(P(56), 2)) == BAD
    assert sample(nxt=P(51)) == BAD and sample(nxt=off(P(51), 24 * 9)) == BAD and sample(rew=P(54)) == BAD and sample(act=off(P(51), 8)) == BAD


def test_core_exports_her():
    import core
    from core import HerReplayBuffer
    from core.common.type_aliases import DictReplayBufferSamples
    from core.her import GoalSelectionStrategy, HerReplayBuffer as H2
    from core.her.goal_selection_strategy import KEY_TO_GOAL_STRATEGY

    assert HerReplayBuffer is H2 and "HerReplayBuffer" in core.__all__
    assert [s.name for s in GoalSelectionStrategy] == ["FUTURE", "FINAL", "EPISODE"] and [s.value for s in GoalSelectionStrategy] == [0, 1, 2]
    assert {k: v.value for k, v in KEY_TO_GOAL_STRATEGY.items()} == nv.HER_STRATEGIES
    assert DictReplayBufferSamples._fields == ("observations", "actions", "next_observations", "dones", "rewards")


def test_dqn_policy_aliases_untouched():
    from core.dqn import DQN

    assert set(DQN.policy_aliases) == {"MlpPolicy"}


@pytest.mark.parametrize("algo, net_arch, mods", [("sac", [64, 64], ("actor", "critic", "critic_target")),
                                                  ("td3", [48, 32], ("actor", "actor_target", "critic", "critic_target"))])
def test_multi_input_policy_keys_and_seeded_initial_weights(algo, net_arch, mods):
    """`MultiInputPolicy` = the algorithm's own policy class with a CombinedExtractor: state-dict keys, construction order and seeded
    initial weights of the reference's (`{algo}_her_train_kat_small.npz`, written by the unmodified reference)."""
    import importlib

    import torch as th

    from core.common.spaces import Box, Dict
    from core.common.torch_layers import CombinedExtractor

    g = np.load(os.path.join(os.path.dirname(GOLDEN), f"{algo}_her_train_kat_small.npz"))
    one = np.ones(1, np.float32)
    space = Dict({"observation": Box(-1, 1, (4,)), "achieved_goal": Box(-one, one), "desired_goal": Box(-one, one)})
    algo_mod = importlib.import_module(f"core.{algo}.{algo}")
    cls = getattr(algo_mod, algo.upper()).policy_aliases["MultiInputPolicy"]
    assert set(getattr(algo_mod, algo.upper()).policy_aliases) == {"MlpPolicy", "MultiInputPolicy"}
    from core.td3 import DDPG

    assert DDPG.policy_aliases["MultiInputPolicy"] is importlib.import_module("core.td3.policies").MultiInputPolicy
    th.manual_seed(0)
    pol = cls(space, Box(-1, 1, (2,)), lambda _: 1e-3, net_arch=net_arch)
    fe = pol.actor.features_extractor
    assert isinstance(fe, CombinedExtractor) and fe.features_dim == 6 and not list(fe.parameters()) and fe.keys == list(space.keys())
    for nm in mods:
        sd = getattr(pol, nm).state_dict()
        want = sorted(k[len(f"before/{nm}/"):] for k in g.files if k.startswith(f"before/{nm}/"))
        assert sorted(sd) == want, nm
        for k, v in sd.items():
            np.testing.assert_array_equal(v.numpy(), g[f"before/{nm}/{k}"], err_msg=f"{nm}/{k}")
    rows = np.random.default_rng(0).uniform(-1, 1, (5, 6)).astype(np.float32)
    as_dict = {"achieved_goal": rows[:, 0:1], "desired_goal": rows[:, 1:2], "observation": rows[:, 2:]}
    t, vectorized = pol.obs_to_tensor(as_dict)
    assert vectorized and np.array_equal(t.numpy(), rows) and not pol.obs_to_tensor({k: v[0] for k, v in as_dict.items()})[1]
    a_dict, a_flat = pol.predict(as_dict, deterministic=True)[0], pol.predict(rows, deterministic=True)[0]
    assert a_dict.shape == (5, 2) and np.array_equal(a_dict, a_flat) and pol.predict(rows[0], deterministic=True)[0].shape == (2,)
    with pytest.raises(ValueError, match="Dict observation space"):
        cls(Box(-1, 1, (6,)), Box(-1, 1, (2,)), lambda _: 1e-3)


def test_dict_space():
    from core.common.spaces import Box, Dict

    one = np.ones(1, np.float32)
    d = Dict({"observation": Box(-1, 1, (4,)), "desired_goal": Box(-one, one), "achieved_goal": Box(-one, one)}, seed=3)
    assert list(d.keys()) == ["achieved_goal", "desired_goal", "observation"] == list(d.spaces) == [k for k, _ in d.items()]
    assert d["observation"].shape == (4,) and [s.shape for s in d.values()] == [(1,), (1,), (4,)] and d.flat_dim() == 6
    assert repr(d) == "Dict('achieved_goal': Box(-1.0, 1.0, (1,), float32), 'desired_goal': Box(-1.0, 1.0, (1,), float32), " \
                      "'observation': Box(-1.0, 1.0, (4,), float32))"
    x = d.sample()
    assert list(x) == list(d.keys()) and d.contains(x) and x["observation"].shape == (4,) and x["observation"].dtype == np.float32
    assert not d.contains({k: v for k, v in x.items() if k != "desired_goal"}) and not d.contains(x["observation"])
    assert not d.contains(dict(x, achieved_goal=np.array([2.0], np.float32)))
    assert d == Dict({"achieved_goal": Box(-one, one), "desired_goal": Box(-one, one), "observation": Box(-1, 1, (4,))})
    assert d != Dict({"observation": Box(-1, 1, (4,))}) and d != Box(-1, 1, (6,))
    with pytest.raises(ValueError):
        Dict({"a": 3})


def test_compute_reward_matches_the_fixture_bit_for_bit(kat):
    from core.common.vec_env.cstr_vec_env import goal_dict_to_rows, goal_reward_np, goal_rows_to_dict

    coef = nv.default_coef()
    for tag in TAGS:
        nxt, obs, rew = kat[f"{tag}/next"], kat[f"{tag}/obs"], kat[f"{tag}/rew"]
        got = goal_reward_np(coef, nxt[..., 0].reshape(-1, 1), obs[..., 1].reshape(-1, 1))
        assert got.dtype == np.float32 and np.array_equal(got, rew.reshape(-1))
        assert np.array_equal(goal_reward(nxt[..., 0], obs[..., 1]), rew)  # the test's own statement
        assert np.array_equal(goal_dict_to_rows(goal_rows_to_dict(obs[0])), obs[0])
    # the goals of the fixture's three targets through the env's affine map
    assert np.array_equal(goal_of_target(np.array([0.12, 0.20, 0.33], np.float32)), kat["r4a/obs"][0, :, 1])


@pytest.mark.parametrize("nsg, ratio, nbv10, nbv256", [(0, 0.0, 0, 0), (1, 0.5, 5, 128), (4, 0.8, 8, 204)])
def test_her_ratio_and_nb_virtual(nsg, ratio, nbv10, nbv256):
    h = HerNp(4, 1, n_sampled_goal=nsg)
    assert h.her_ratio == 1 - (1.0 / (nsg + 1)) and abs(h.her_ratio - ratio) < 1e-12
    assert int(h.her_ratio * 10) == nbv10 and int(h.her_ratio * 256) == nbv256


def replay_adds(kat, tag, check=True):
    R, N, T, pos, full = (int(v) for v in kat[f"{tag}/meta"])
    h = HerNp(R, N)
    for t in range(T):
        h.add(*(kat[f"{tag}/{k}"][t] for k in ("obs", "next", "act", "rew", "done", "timeout")))
        if check:
            assert np.array_equal(h.ep_start, kat[f"{tag}/ep_start"][t]), (tag, t)
            assert np.array_equal(h.ep_length, kat[f"{tag}/ep_length"][t]), (tag, t)
            assert np.array_equal(h.cur, kat[f"{tag}/cur"][t]), (tag, t)
    assert (h.pos, int(h.full)) == (pos, full)
    return h


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_bookkeeping_after_every_add(kat, tag):
    h = replay_adds(kat, tag)
    assert (h.ep_length > 0).any() and (h.ep_length == 0).any()  # the fixture holds valid and invalidated transitions


def sample_cases(kat, tag):
    for key in sorted(k[:-len("/flat_idx")] for k in kat if k.startswith(tag + "/") and k.endswith("/flat_idx")):
        _, strategy, nsg, B = key.split("/")
        yield key, strategy, int(nsg), int(B)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_seeded_samples(kat, tag):
    h = replay_adds(kat, tag, check=False)
    n = 0
    for key, strategy, nsg, B in sample_cases(kat, tag):
        h.strategy, h.her_ratio = strategy, 1 - (1.0 / (nsg + 1))
        rs = np.random.RandomState(1000 + B + nsg)
        s = h.sample(rs, B)
        assert np.array_equal(s["flat_idx"], kat[key + "/flat_idx"]), key
        assert np.array_equal(s["goal_idx"], kat[key + "/goal_idx"]) or (strategy == "final" and kat[key + "/goal_idx"].size == 0), key
        for k in ("obs", "next", "act", "done", "rew"):
            assert s[k].dtype == np.float32 and np.array_equal(s[k], kat[f"{key}/{k}"]), (key, k)
        st = rs.get_state()
        assert np.array_equal(st[1], kat[key + "/mt_key"]) and [st[2], st[3]] == kat[key + "/mt_pos"].tolist(), key
        assert np.array_equal(mt_image(rs)[:624], kat[key + "/mt_key"])
        n += 1
    assert n == (12 if tag in ("r4a", "r12b") else 6)


def test_array_randint_is_one_scalar_draw_per_element():
    """What the sampler kernel walks: RandomState.randint(low[], high[]) consumes the stream like one scalar call per element, in order,
    and takes no draw where high - low == 1 (values and final stream state)."""
    gen = np.random.default_rng(0)
    for case in range(50):
        low = gen.integers(0, 9, 40)
        high = low + gen.choice([1, 1, 2, 3, 4, 5, 8, 9, 16, 17, 400], 40)
        a, b = np.random.RandomState(case), np.random.RandomState(case)
        want = a.randint(low, high)
        got = np.array([b.randint(lo, hi) if hi - lo > 1 else lo for lo, hi in zip(low, high)])
        assert np.array_equal(want, got) and np.array_equal(a.get_state()[1], b.get_state()[1]) and a.get_state()[2] == b.get_state()[2]
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    assert np.array_equal(a.choice(np.arange(3, 40, 3), size=33, replace=True), np.arange(3, 40, 3)[b.randint(0, 13, 33)])
    assert a.get_state()[2] == b.get_state()[2]


@pytest.mark.parametrize("tag", TAGS)
def test_truncate_last_trajectory_restated(kat, tag):
    h = replay_adds(kat, tag, check=False)
    warned = bool((h.cur != h.pos).any())
    for env_idx in np.where(h.cur != h.pos)[0]:  # her_replay_buffer.py:400-408
        h.dones[h.pos - 1, env_idx] = 1.0
        h._compute_episode_length(env_idx)
        h.timeouts[h.pos - 1, env_idx] = 1.0
    assert warned == bool(kat[f"{tag}/trunc/warned"][0])
    assert np.array_equal(h.ep_length, kat[f"{tag}/trunc/ep_length"]) and np.array_equal(h.cur, kat[f"{tag}/trunc/cur"])
    assert np.array_equal(h.dones, kat[f"{tag}/trunc/dones"]) and np.array_equal(h.timeouts, kat[f"{tag}/trunc/timeouts"])


def test_constructor_assertions():
    """Everything the constructor refuses before it allocates device memory."""
    from core.common.spaces import Box, Dict
    from core.her import HerReplayBuffer

    one = np.ones(1, np.float32)
    space = Dict({"achieved_goal": Box(-one, one), "desired_goal": Box(-one, one), "observation": Box(-1, 1, (4,))})
    act = Box(-1, 1, (2,))

    class Env:
        goal_conditioned, coef = True, None

    with pytest.raises(ValueError, match="copy_info_dict"):
        HerReplayBuffer(12, space, act, Env(), copy_info_dict=True)
    with pytest.raises(ValueError, match="optimize_memory_usage"):
        HerReplayBuffer(12, space, act, Env(), optimize_memory_usage=True)
    with pytest.raises(ValueError, match="goal face"):
        HerReplayBuffer(12, Box(-1, 1, (4,)), act, Env())
    with pytest.raises(ValueError, match="goal face"):
        HerReplayBuffer(12, space, act, object())
    with pytest.raises(AssertionError, match="Invalid goal selection strategy"):
        HerReplayBuffer(12, space, act, Env(), goal_selection_strategy="nearest")
    with pytest.raises(AssertionError, match="Invalid goal selection strategy"):
        HerReplayBuffer(12, space, act, Env(), goal_selection_strategy=2)
