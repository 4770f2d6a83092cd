"""CPU-side checks of PPO / A2C on the goal face: cstr_goal_rollout_add_f32 and cstr_goal_ppo_gather_f32 are exported and reject bad
arguments on the host (never-dereferenced pointers: nothing is launched), the Box-face entry points keep refusing the 6-float row,
"MultiInputPolicy" resolves for both classes, MultiInputActorCriticPolicy built on the CPU has the reference's state-dict keys, shapes
and seeded initial weights (tests/golden/*_goal_train_kat_small.npz, written by the unmodified reference: tools/refharness/gen_golden.py
gen_ppo_goal / gen_a2c_goal), the dict views of a flat row array alias it, and what can be refused without a device is refused.
`add_numpy` / `gather_numpy` are the NumPy restatement of the two launches that tests/test_goal_onpolicy.py compares the kernels with."""
import ctypes as C

import numpy as np
import pytest

from core import _native as nv
from test_ppo_abi import BAD, UNSUP, P, f32, i64, null, rollout

GOAL_SYMBOLS = ("cstr_goal_rollout_add_f32", "cstr_goal_ppo_gather_f32")
KEYS = ("achieved_goal", "desired_goal", "observation")


def off(p: C.c_void_p, nbytes: int) -> C.c_void_p:
    return C.c_void_p(p.value + nbytes)


# ---- the NumPy restatement (reference core/common/buffers.py:763-803 + on_policy_algorithm.py:236-256, buffers.py:805-840) ------------
def add_numpy(buf: dict, ctl: list, rows, act, reward, episode_start, value, log_prob, timeout=None, terminal_value=None, gamma=0.99,
              done=None, ep_return=None, ep_len=None, ep_stats=None) -> None:
    """One add launch on host arrays, in place: buf = {observations [T, N, 6], actions [T, N, 2], rewards, episode_starts, values,
    log_probs, advantages, returns [T, N]}, ctl = [pos, full, ticket, adds]; episode_start / ep_return / ep_len / ep_stats are updated
    as the launch updates them. A full buffer takes no row."""
    pos, T = ctl[0], buf["rewards"].shape[0]
    if not 0 <= pos < T:
        return
    rw = np.asarray(reward, np.float32).copy()
    if ep_stats is not None:
        ret, length, d = ep_return + rw, ep_len + 1, done != 0
        ep_stats[0] += d.sum()
        ep_stats[1] += ret[d].astype(np.float64).sum()
        ep_stats[2] += length[d].sum()
        ep_return[:], ep_len[:] = np.where(d, np.float32(0), ret), np.where(d, 0, length)
    if timeout is not None:
        rw = np.where(timeout != 0, rw + np.float32(gamma) * terminal_value, rw).astype(np.float32)
    buf["observations"][pos], buf["actions"][pos], buf["rewards"][pos] = rows, act, rw
    buf["episode_starts"][pos], buf["values"][pos], buf["log_probs"][pos] = episode_start, value, log_prob
    buf["advantages"][pos], buf["returns"][pos] = 0.0, 0.0
    if done is not None:
        episode_start[:] = done
    ctl[0], ctl[3] = pos + 1, ctl[3] + 1
    if pos + 1 == T:
        ctl[1] = 1


def gather_numpy(buf: dict, idx) -> tuple:
    """The gather launch: flat index i (swap_and_flatten) = env i // T, step i % T, clamped into [0, T N) -> (rows, actions, old_values,
    old_log_prob, advantages, returns)"""
    T, N = buf["rewards"].shape
    i = np.clip(np.asarray(idx, np.int64), 0, T * N - 1)
    env, step = i // T, i % T
    return tuple(buf[f][step, env] for f in ("observations", "actions", "values", "log_probs", "advantages", "returns"))


def test_numpy_restatement_is_swap_and_flatten():
    rng = np.random.default_rng(0)
    T, N = 3, 5
    buf = {f: rng.normal(size=(T, N) + s).astype(np.float32) for f, s in (("observations", (6,)), ("actions", (2,)), ("rewards", ()),
           ("episode_starts", ()), ("values", ()), ("log_probs", ()), ("advantages", ()), ("returns", ()))}
    idx = rng.permutation(T * N)
    got = gather_numpy(buf, idx)
    flat = lambda a: a.swapaxes(0, 1).reshape(T * N, *a.shape[2:])  # noqa: E731  (buffers.py:86-99)
    for g, f in zip(got, ("observations", "actions", "values", "log_probs", "advantages", "returns")):
        np.testing.assert_array_equal(g, flat(buf[f])[idx])
    np.testing.assert_array_equal(gather_numpy(buf, [-3, T * N + 4])[0], np.stack([buf["observations"][0, 0], buf["observations"][T - 1, N - 1]]))
    # add: bootstrap where timeout, episode_start <- done, statistics on the raw reward, a full buffer takes nothing
    ctl, start = [T - 1, 0, 0, T - 1], np.ones(N, np.float32)
    rew, tv = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    done, tout = np.array([1, 0, 1, 0, 1], np.float32), np.array([1, 0, 0, 0, 1], np.float32)
    er, el, st = np.zeros(N, np.float32), np.zeros(N, np.int32), np.zeros(4)
    rows = rng.normal(size=(N, 6)).astype(np.float32)
    add_numpy(buf, ctl, rows, rows[:, :2], rew, start, rew, rew, tout, tv, 0.99, done, er, el, st)
    assert ctl == [T, 1, 0, T] and np.array_equal(start, done) and st[0] == 3 and st[2] == 3
    np.testing.assert_array_equal(buf["rewards"][T - 1], np.where(tout != 0, rew + np.float32(0.99) * tv, rew).astype(np.float32))
    np.testing.assert_array_equal(buf["observations"][T - 1], rows)
    before = {k: v.copy() for k, v in buf.items()}
    add_numpy(buf, ctl, rows + 1, rows[:, :2], rew, start, rew, rew)
    assert ctl == [T, 1, 0, T] and all(np.array_equal(before[k], buf[k]) for k in buf)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_goal_symbols_declared_and_exported():
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in GOAL_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive


def goal_rb(**kw):
    kw.setdefault("d", 6)
    return rollout(**kw)


def add(lib, rb=None, ctl=P(8), rows=P(9), act=P(10), rew=P(11), es=P(12), val=P(13), lp=P(14), tout=null, tv=null, done=null, er=null, el=null,
        st=null, entry="cstr_goal_rollout_add_f32"):
    rb = goal_rb() if rb is None else rb
    return getattr(lib, entry)(C.byref(rb), ctl, rows, act, rew, es, val, lp, tout, tv, f32(0.99), done, er, el, st, null)


def gather(lib, rb=None, idx=P(8), b=12, rows=P(9), act=P(10), ov=P(11), olp=P(12), adv=P(13), ret=P(14), entry="cstr_goal_ppo_gather_f32"):
    rb = goal_rb() if rb is None else rb
    return getattr(lib, entry)(C.byref(rb), idx, i64(b), rows, act, ov, olp, adv, ret, null)


def test_goal_add_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    # every call below fails a host check: one with valid-looking fake pointers would enqueue a launch, so none is made
    assert lib.cstr_goal_rollout_add_f32(null, P(8), P(9), P(10), P(11), P(12), P(13), P(14), null, null, f32(0.99), null, null, null, null, null) == BAD
    for name in ("ctl", "rows", "act", "rew", "es", "val", "lp"):
        assert add(lib, **{name: null}) == BAD, name
    for field in ("obs", "act", "rew", "es", "val", "lp", "adv", "ret"):
        assert add(lib, rb=goal_rb(**{field: null})) == BAD, field
    assert add(lib, rb=goal_rb(rows=0)) == BAD and add(lib, rb=goal_rb(n=0)) == BAD and add(lib, rb=goal_rb(rows=-1)) == BAD
    assert add(lib, rb=goal_rb(d=0)) == BAD and add(lib, rb=goal_rb(a=0)) == BAD
    for d in (4, 8):
        assert add(lib, rb=goal_rb(d=d)) == UNSUP, d
    for a in (1, 3, 4):
        assert add(lib, rb=goal_rb(a=a)) == UNSUP, a
    assert add(lib, rb=goal_rb(rows=1 << 20, n=1 << 20)) == UNSUP
    assert add(lib, rows=off(P(9), 4)) == BAD and add(lib, rb=goal_rb(obs=off(P(0), 4))) == BAD  # a 4-byte-misaligned observation row
    assert add(lib, act=off(P(10), 4)) == BAD and add(lib, ctl=off(P(8), 4)) == BAD and add(lib, val=off(P(13), 2)) == BAD
    assert add(lib, tout=P(15)) == BAD and add(lib, tv=P(15)) == BAD          # a timeout flag without terminal values, and the reverse
    assert add(lib, er=P(15), el=P(16), st=P(17)) == BAD                        # episode statistics need `done`
    assert add(lib, done=P(18), er=P(15)) == BAD                                # ... all three or none
    assert add(lib, rows=P(0)) == BAD and add(lib, rows=off(P(0), 24 * 31)) == BAD  # an input row inside the buffer it is copied into
    assert add(lib, act=P(1)) == BAD and add(lib, val=P(4)) == BAD and add(lib, lp=P(5)) == BAD and add(lib, rew=P(2)) == BAD
    assert add(lib, done=P(12)) == BAD                                          # done over the episode starts it replaces


def test_goal_gather_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    assert lib.cstr_goal_ppo_gather_f32(null, P(8), i64(12), P(9), P(10), P(11), P(12), P(13), P(14), null) == BAD
    for name in ("idx", "rows", "act", "ov", "olp", "adv", "ret"):
        assert gather(lib, **{name: null}) == BAD, name
    assert gather(lib, b=0) == BAD and gather(lib, b=-4) == BAD and gather(lib, rb=goal_rb(rows=0)) == BAD
    for d in (4, 8):
        assert gather(lib, rb=goal_rb(d=d)) == UNSUP, d
    for a in (1, 3, 4):
        assert gather(lib, rb=goal_rb(a=a)) == UNSUP, a
    assert gather(lib, b=(1 << 30) + 1) == UNSUP
    assert gather(lib, rows=off(P(9), 4)) == BAD and gather(lib, idx=off(P(8), 4)) == BAD and gather(lib, act=off(P(10), 4)) == BAD
    assert gather(lib, rows=P(0)) == BAD and gather(lib, adv=P(12)) == BAD and gather(lib, ret=P(7)) == BAD  # overlapping rows
    assert gather(lib, rows=off(P(10), -8)) == BAD                               # two outputs over each other


def test_box_face_entry_points_keep_refusing_the_goal_row():
    lib = nv.lib()
    assert add(lib, entry="cstr_rollout_add_f32") == UNSUP and gather(lib, entry="cstr_ppo_gather_f32") == UNSUP
    assert add(lib, rb=rollout(d=4), entry="cstr_rollout_add_f32", rows=off(P(9), 8)) == BAD  # and their 16-byte rows


def test_hip_ops_wrappers_and_device_rollout_widths():
    import torch as th

    from core.common import hip_ops

    assert hip_ops.goal_onpolicy_supported(6, 2) and not hip_ops.goal_onpolicy_supported(6, 4) and not hip_ops.goal_onpolicy_supported(4, 2)
    assert not hip_ops.ppo_supported(6, 2) and not hip_ops.rollout_supported(6, 2)  # the Box face's own checks are what they were
    with pytest.raises(ValueError, match="obs_dim 6 and act_dim 2"):
        hip_ops.DeviceRollout(8, 4, 4, 2, "cpu", goal=True)
    with pytest.raises(ValueError, match="obs_dim"):
        hip_ops.DeviceRollout(8, 4, 6, 2, "cpu")
    rb = hip_ops.DeviceRollout(3, 4, 6, 2, "cpu", goal=True)
    box = hip_ops.DeviceRollout(3, 4, 4, 2, "cpu")
    assert tuple(rb.observations.shape) == (3, 4, 6) and rb.goal and not box.goal
    z = lambda *s: th.zeros(*s)  # noqa: E731
    with pytest.raises(ValueError, match="No CPU fallback|device"):
        hip_ops.goal_rollout_add(rb, z(4, 6), z(4, 2), z(4), z(4), z(4), z(4))
    with pytest.raises(ValueError, match="No CPU fallback|device"):
        hip_ops.goal_ppo_gather(rb, th.zeros(5, dtype=th.int64), z(5, 6), z(5, 2), z(5), z(5), z(5), z(5))
    with pytest.raises(ValueError, match="goal face"):
        hip_ops.goal_rollout_add(box, z(4, 6), z(4, 2), z(4), z(4), z(4), z(4))
    with pytest.raises(ValueError, match="goal face"):
        hip_ops.goal_ppo_gather(box, th.zeros(5, dtype=th.int64), z(5, 6), z(5, 2), z(5), z(5), z(5), z(5))


# ---- classes ----------------------------------------------------------------------------------------------------------------------
def goal_space():
    from core.common.spaces import Box, Dict

    g1, o4 = np.ones(1, np.float32), np.ones(4, np.float32)
    return Dict({"observation": Box(-o4, o4), "achieved_goal": Box(-g1, g1), "desired_goal": Box(-g1, g1)})


def action_space():
    from core.common.spaces import Box

    return Box(-np.ones(2, np.float32), np.ones(2, np.float32))


def test_multi_input_policy_resolves_for_ppo_and_a2c():
    from core.a2c import A2C, MultiInputPolicy as A2cMulti
    from core.common.policies import ActorCriticPolicy, MultiInputActorCriticPolicy, MultiInputMixin
    from core.ppo import PPO, MultiInputPolicy as PpoMulti

    assert PpoMulti is A2cMulti is MultiInputActorCriticPolicy
    assert issubclass(MultiInputActorCriticPolicy, ActorCriticPolicy) and issubclass(MultiInputActorCriticPolicy, MultiInputMixin)
    for cls in (PPO, A2C):
        assert cls.policy_aliases["MultiInputPolicy"] is MultiInputActorCriticPolicy and cls.policy_aliases["MlpPolicy"] is ActorCriticPolicy
        assert cls.goal_face_support


@pytest.mark.parametrize("name,module", [("ppo_goal_train_kat_small.npz", "ppo"), ("a2c_goal_train_kat_small.npz", "a2c"),
                                         ("ppo_goal_train_kat_default.npz", "ppo")])
def test_policy_keys_shapes_and_seeded_initial_weights(golden, name, module):
    import importlib

    import torch as th

    from core.common.torch_layers import CombinedExtractor

    g = golden(name)
    th.manual_seed(int(g["seed"]))
    kw = {}
    if module == "a2c":  # what A2C's constructor puts into policy_kwargs (a2c.py:123-127)
        kw = dict(optimizer_class=th.optim.RMSprop, optimizer_kwargs=dict(alpha=0.99, eps=1e-5, weight_decay=0))
    pol = importlib.import_module(f"core.{module}").MultiInputPolicy(goal_space(), action_space(), lambda _: 3e-4,
                                                                      net_arch=[int(w) for w in g["net_arch"]], **kw)
    sd = pol.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_dict_keys"]]
    assert isinstance(pol.features_extractor, CombinedExtractor) and pol.features_dim == 6
    assert tuple(sd["mlp_extractor.policy_net.0.weight"].shape) == (int(g["net_arch"][0]), 6) == tuple(sd["mlp_extractor.value_net.0.weight"].shape)
    assert list(pol.goal_space.spaces) == list(KEYS) and pol.observation_space.shape == (6,)
    for k, v in sd.items():
        key = f"before/policy/{k}"
        if key not in g.files:  # the default nets' large tensors are stored as digests
            head = g[key + "#head"]
            np.testing.assert_allclose(v.numpy().reshape(-1)[:head.size], head, rtol=0, atol=1e-6, err_msg=k)
            assert tuple(v.shape) == tuple(g[key + "#shape"])
            continue
        want = g[key]
        assert tuple(v.shape) == want.shape, k
        if k == "log_std" or k.endswith(".bias"):
            np.testing.assert_array_equal(v.numpy(), want, err_msg=k)
        else:  # orthogonal_: QR through LAPACK, whose last bits may depend on the host CPU
            np.testing.assert_allclose(v.numpy(), want, rtol=0, atol=1e-6, err_msg=k)


def test_policy_torch_statements_take_dicts_and_flat_rows(golden):
    import torch as th

    from core.ppo import MultiInputPolicy

    g = golden("ppo_goal_predict_kat.npz")
    pol = MultiInputPolicy(goal_space(), action_space(), lambda _: 3e-4, net_arch=[int(w) for w in g["net_arch"]])
    with th.no_grad():
        for k, v in pol.state_dict().items():
            v.copy_(th.as_tensor(g[f"policy/{k}"]))
    rows = g["rows"]
    obs = {"achieved_goal": rows[:, 0:1], "desired_goal": rows[:, 1:2], "observation": rows[:, 2:6]}
    for given in (obs, rows, {k: th.as_tensor(v) for k, v in obs.items()}):
        act, state = pol.predict(given, deterministic=True)
        assert state is None and act.shape == (16, 2)
        np.testing.assert_allclose(act, g["deterministic"], rtol=0, atol=2e-6)
    one, _ = pol.predict({k: v[3] for k, v in obs.items()}, deterministic=True)
    assert one.shape == (2,)
    np.testing.assert_allclose(one, g["deterministic"][3], rtol=0, atol=2e-6)
    with th.no_grad():
        values = pol.predict_values({k: th.as_tensor(v) for k, v in obs.items()})
        values_flat = pol.predict_values(th.as_tensor(rows))
        v2, lp, ent = pol.evaluate_actions({k: th.as_tensor(v) for k, v in obs.items()}, th.as_tensor(g["sampled"]))
    np.testing.assert_allclose(values.numpy(), g["values"], rtol=1e-5, atol=1e-6)
    assert th.equal(values, values_flat) and th.equal(v2, values) and lp.shape == (16,) and ent.shape == (16,)
    pol.action_dist.eps_queue.append(th.as_tensor(g["eps"]))
    act, _ = pol.predict(obs, deterministic=False)
    np.testing.assert_allclose(act, g["sampled"], rtol=0, atol=2e-6)


def test_dict_views_alias_the_flat_rows_and_samples_carry_them():
    import torch as th

    from core.common.buffers import DictRolloutBuffer, RolloutBuffer
    from core.common.type_aliases import DictRolloutBufferSamples, GoalRolloutBufferSamples, RolloutBufferSamples

    assert issubclass(DictRolloutBuffer, RolloutBuffer)
    rows = th.arange(3 * 4 * 6, dtype=th.float32).reshape(3, 4, 6)
    views = DictRolloutBuffer.split(rows)
    assert list(views) == list(KEYS) and [tuple(v.shape) for v in views.values()] == [(3, 4, 1), (3, 4, 1), (3, 4, 4)]
    for k, col in zip(KEYS, (0, 1, 2)):
        assert views[k].data_ptr() == rows.data_ptr() + 4 * col
    rows[1, 2, 1] = -7.0
    assert float(views["desired_goal"][1, 2, 0]) == -7.0
    assert DictRolloutBufferSamples._fields == RolloutBufferSamples._fields  # the reference's six fields, in its order
    flat = th.zeros(5, 6)
    mb = GoalRolloutBufferSamples(DictRolloutBuffer.split(flat), *(th.zeros(5) for _ in range(5)))
    mb.rows = flat
    assert isinstance(mb, DictRolloutBufferSamples) and len(mb) == 6 and mb.rows is flat and mb.observations["observation"].shape == (5, 4)


def test_refusals_that_need_no_device():
    from core.a2c import A2C
    from core.common.buffers import DictRolloutBuffer
    from core.common.spaces import Box, Dict
    from core.ppo import PPO, MultiInputPolicy

    one = np.ones(4, np.float32)
    with pytest.raises(ValueError, match="MultiInputPolicy needs a Dict observation space"):
        MultiInputPolicy(Box(-one, one), action_space(), lambda _: 3e-4)
    with pytest.raises(ValueError, match="does not support gSDE"):
        MultiInputPolicy(goal_space(), action_space(), lambda _: 3e-4, use_sde=True)
    with pytest.raises(AssertionError, match="DictRolloutBuffer must be used with Dict obs space only"):
        DictRolloutBuffer(8, Box(-one, one), action_space(), device="cuda", n_envs=4)
    with pytest.raises(ValueError, match="CSTR goal face"):
        DictRolloutBuffer(8, Dict({"a": Box(-one, one), "b": Box(-one, one)}), action_space(), device="cuda", n_envs=4)
    for cls in (PPO, A2C):
        with pytest.raises(ValueError, match="does not support gSDE"):
            cls("MultiInputPolicy", None, use_sde=True)
        msg = cls._goal_face_policy_message(cls.__new__(cls), "MlpPolicy")
        assert "does not support a Dict observation space" in msg and "MultiInputPolicy" in msg and cls.__name__ in msg
