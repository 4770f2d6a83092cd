"""CPU-side checks of the training callbacks (core/common/callbacks.py) and of cstr_eval_episodes_f32's argument checks: constructor
signatures against the reference's (written out), the `calls_until_event()` / `skip_calls()` arithmetic against a brute-force count,
file names and the evaluations.npz layout against the reference-written tests/golden/callbacks_kat.npz, the `parent` assertions, and
the entry point's error codes without anything being dereferenced or launched."""
import ctypes as C
import inspect
import math
import os
import types

import numpy as np
import pytest

from core import _native as nv
from core.common import callbacks as cbs
from core.common.callbacks import (BaseCallback, CallbackList, CheckpointCallback, ConvertCallback, EvalCallback, EventCallback,
                                   EveryNTimesteps, NoopCallback, StopTrainingOnMaxEpisodes, StopTrainingOnNoModelImprovement,
                                   StopTrainingOnRewardThreshold)


pytestmark = pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")


class _Logger:
    def __init__(self):
        self.records, self.dumps = [], []

    def record(self, key, value, exclude=None):
        self.records.append((key, value, exclude))

    def dump(self, step=0):
        self.dumps.append(step)


class _Model:
    """What the callbacks touch of an algorithm."""

    def __init__(self, n_envs):
        self.num_timesteps, self.n_envs = 0, n_envs
        self.env = types.SimpleNamespace(num_envs=n_envs)
        self.logger = _Logger()
        self.saved = []

    def get_env(self):
        return self.env

    def get_vec_normalize_env(self):
        return None

    def save(self, path):
        path = path if path.endswith(".zip") else path + ".zip"
        self.saved.append((self.num_timesteps, os.path.basename(path)))
        open(path, "w").close()

    def save_replay_buffer(self, path):
        self.saved.append((self.num_timesteps, os.path.basename(path)))
        open(path, "w").close()

    replay_buffer = object()


def _params(cls):
    return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]


E = inspect.Parameter.empty


def test_constructor_signatures_and_defaults_are_the_references():
    assert _params(EventCallback) == [("callback", None), ("verbose", 0)]
    assert _params(CheckpointCallback) == [("save_freq", E), ("save_path", E), ("name_prefix", "rl_model"), ("save_replay_buffer", False),
                                           ("save_vecnormalize", False), ("verbose", 0)]
    assert _params(EvalCallback) == [("eval_env", E), ("callback_on_new_best", None), ("callback_after_eval", None), ("n_eval_episodes", 5),
                                     ("eval_freq", 10000), ("log_path", None), ("best_model_save_path", None), ("deterministic", True),
                                     ("render", False), ("verbose", 1), ("warn", True), ("fused", None)]  # `fused`: this package's, last
    assert _params(StopTrainingOnRewardThreshold) == [("reward_threshold", E), ("verbose", 0)]
    assert _params(EveryNTimesteps) == [("n_steps", E), ("callback", E)]
    assert _params(StopTrainingOnMaxEpisodes) == [("max_episodes", E), ("verbose", 0)]
    assert _params(StopTrainingOnNoModelImprovement) == [("max_no_improvement_evals", E), ("min_evals", 0), ("verbose", 0)]
    assert not hasattr(cbs, "ProgressBarCallback")
    for cls in (EvalCallback, EveryNTimesteps):
        assert issubclass(cls, EventCallback)
    # attributes
    ev = EvalCallback(_stub_env(), log_path="/tmp/x")
    assert (ev.n_eval_episodes, ev.eval_freq, ev.best_mean_reward, ev.last_mean_reward, ev.deterministic, ev.render, ev.warn, ev.fused) == (
        5, 10000, -np.inf, -np.inf, True, False, True, None)
    assert ev.log_path == os.path.join("/tmp/x", "evaluations") and ev.best_model_save_path is None
    assert ev.evaluations_results == ev.evaluations_timesteps == ev.evaluations_length == ev.evaluations_successes == []
    ck = CheckpointCallback(10, "/tmp/y")
    assert (ck.save_freq, ck.save_path, ck.name_prefix, ck.save_replay_buffer, ck.save_vecnormalize) == (10, "/tmp/y", "rl_model", False, False)
    st = StopTrainingOnMaxEpisodes(3)
    assert (st.max_episodes, st._total_max_episodes, st.n_episodes) == (3, 3, 0)
    nm = StopTrainingOnNoModelImprovement(4)
    assert (nm.max_no_improvement_evals, nm.min_evals, nm.last_best_mean_reward, nm.no_improvement_evals) == (4, 0, -np.inf, 0)
    en = EveryNTimesteps(5, BaseCallback())
    assert (en.n_steps, en.last_time_trigger) == (5, 0) and en.callback.parent is en


class _Rec(BaseCallback):
    def __init__(self):
        super().__init__()
        self.seen = []

    def _on_step(self):
        self.seen.append((self.n_calls, self.num_timesteps))
        return True


def _make(kind, freq, tmp):
    """(callback, events()) where events() lists what has fired so far, as (num_timesteps at the event) values"""
    if kind == "checkpoint":
        cb = CheckpointCallback(freq, str(tmp), name_prefix="m")
        return cb, lambda: [t for t, _ in cb.model.saved]
    if kind == "eval":
        cb = EvalCallback(_stub_env(), eval_freq=freq, verbose=0)
        cb._evaluate = lambda: ([-1.0, -2.0], [400, 400])
        return cb, lambda: list(cb.model.logger.dumps)
    if kind == "every":
        rec = _Rec()
        cb = EveryNTimesteps(freq, rec)
        return cb, lambda: [t for _, t in rec.seen]
    if kind == "list":
        a, ea = _make("checkpoint", freq, tmp)
        b, eb = _make("every", 2 * freq + 1, tmp)
        inner = CallbackList([b, NoopCallback()])
        return CallbackList([a, inner]), lambda: sorted(ea() + eb())
    raise AssertionError(kind)


def _stub_env():
    from core.common.vec_env.base_vec_env import VecEnv

    class _Env(VecEnv):
        def __init__(self):
            self.num_envs = 2

    return _Env()


@pytest.mark.parametrize("kind", ["checkpoint", "eval", "every", "list"])
@pytest.mark.parametrize("n_envs", [1, 4])
@pytest.mark.parametrize("freq", [1, 3, 7])
def test_calls_until_event_and_skip_calls_against_a_brute_force_count(kind, n_envs, freq, tmp_path):
    calls = 60

    def fresh(sub):
        d = tmp_path / sub
        d.mkdir()
        cb, events = _make(kind, freq, d)
        model = _Model(n_envs)
        cb.init_callback(model)
        cb.on_training_start({}, {})
        return cb, events, model

    # brute force: every call goes through on_step(); the calls at which something fired
    cb, events, model = fresh("a")
    fired_at, announced = [], []
    for c in range(1, calls + 1):
        announced.append(cb.calls_until_event())
        before = len(events())
        model.num_timesteps += n_envs
        assert cb.on_step() is True
        if len(events()) > before:
            fired_at.append(c)
    assert fired_at, "the case has events"
    for c0, k in enumerate(announced):  # c0 calls done: the next event is call c0 + k
        nxt = [c for c in fired_at if c > c0]
        if nxt:
            assert k == nxt[0] - c0, (c0, k, nxt[0])
        else:
            assert k >= calls + 1 - c0
    brute_events, brute_calls = events(), cb.n_calls
    # the skipping walk: eventless calls are skipped in one go; the same events at the same timesteps, the same counters
    cb, events, model = fresh("b")
    done, real = 0, 0
    while done < calls:
        k = cb.calls_until_event()
        n = min(k - 1, calls - done)
        if n > 0:
            model.num_timesteps += n * n_envs
            cb.skip_calls(n)
            done += n
        if done < calls:
            model.num_timesteps += n_envs
            assert cb.on_step() is True
            done, real = done + 1, real + 1
    assert events() == brute_events and cb.n_calls == brute_calls == calls and cb.num_timesteps == calls * n_envs
    assert real == len(fired_at) or kind == "list"  # (a list's two children may fire at the same call)
    if kind == "list":
        assert all(ch.n_calls == calls for ch in cb.callbacks) and cb.callbacks[1].callbacks[0].n_calls == calls


def test_calls_until_event_of_the_other_classes():
    assert BaseCallback().calls_until_event() is None and ConvertCallback(lambda l, g: True).calls_until_event() is None
    assert NoopCallback().calls_until_event() == math.inf
    assert StopTrainingOnMaxEpisodes(2).calls_until_event() is None
    assert EvalCallback(_stub_env(), eval_freq=0).calls_until_event() == math.inf
    assert EvalCallback(_stub_env(), eval_freq=-5).calls_until_event() == math.inf

    class Mine(BaseCallback):
        pass

    assert Mine().calls_until_event() is None
    assert CallbackList([NoopCallback(), CheckpointCallback(5, "/tmp/z")]).calls_until_event() == 5
    assert CallbackList([NoopCallback(), CallbackList([CheckpointCallback(5, "/tmp/z"), Mine()])]).calls_until_event() is None
    assert CallbackList([]).calls_until_event() == math.inf


def test_checkpoint_names_and_evaluations_layout_match_the_reference_fixture(golden, tmp_path):
    """Run (a) of tests/golden/callbacks_kat.npz (written by the reference: SAC on 4 envs, EvalCallback(eval_freq=50, 3 episodes) +
    CheckpointCallback(save_freq=60, "m", save_replay_buffer=True), 520 steps) on a stub model: the same files, the same
    evaluations.npz keys / timesteps / ep_lengths / result shape, the same counters."""
    g = golden("callbacks_kat.npz")
    n_envs, _, n_ep, eval_freq, save_freq, steps = (int(v) for v in g["a/dims"])
    ev = EvalCallback(_stub_env(), n_eval_episodes=n_ep, eval_freq=eval_freq, log_path=str(tmp_path / "log"),
                      best_model_save_path=str(tmp_path / "best"), verbose=0, warn=False)
    tape = iter(np.linspace(-3.0, -1.0, 64))
    ev._evaluate = lambda: ([float(next(tape)) for _ in range(n_ep)], [400] * n_ep)
    ck = CheckpointCallback(save_freq=save_freq, save_path=str(tmp_path / "ck"), name_prefix="m", save_replay_buffer=True)
    cb = CallbackList([ev, ck])
    model = _Model(n_envs)
    cb.init_callback(model)
    cb.on_training_start({}, {})
    while model.num_timesteps < steps:
        model.num_timesteps += n_envs
        assert cb.on_step()
    assert sorted(os.listdir(tmp_path / "ck")) == g["a/ck_files"].tolist()
    assert sorted(os.listdir(tmp_path / "log")) == g["a/log_files"].tolist()
    assert sorted(os.listdir(tmp_path / "best")) == g["a/best_files"].tolist()
    e = np.load(tmp_path / "log" / "evaluations.npz")
    assert sorted(e.files) == g["a/eval_keys"].tolist()
    assert e["timesteps"].tolist() == g["a/timesteps"].tolist() and e["ep_lengths"].tolist() == g["a/ep_lengths"].tolist()
    assert list(e["results"].shape) == g["a/results_shape"].tolist()
    assert [ev.n_calls, ck.n_calls, ev.num_timesteps, model.num_timesteps] == g["a/counters"].tolist()[:4]
    keys = [k for k, _, _ in model.logger.records]
    assert keys[:3] == ["eval/mean_reward", "eval/mean_ep_length", "time/total_timesteps"] and model.logger.records[2][2] == "tensorboard"
    assert model.logger.dumps == g["a/timesteps"].tolist() and ev.best_mean_reward == ev.last_mean_reward  # the tape improves every time


def test_stop_children_assert_their_parent_and_stop_where_the_reference_does(golden):
    with pytest.raises(AssertionError, match="``StopTrainingOnMinimumReward`` callback must be used with an ``EvalCallback``"):
        StopTrainingOnRewardThreshold(1.0)._on_step()
    with pytest.raises(AssertionError, match="``StopTrainingOnNoModelImprovement`` callback must be used with an ``EvalCallback``"):
        StopTrainingOnNoModelImprovement(1)._on_step()
    with pytest.raises(AssertionError, match="`dones` variable is not defined, please check your code next to `callback.on_step\\(\\)`"):
        StopTrainingOnMaxEpisodes(1)._on_step()
    # reward threshold: the child of a new best
    stop = StopTrainingOnRewardThreshold(-np.inf)
    ev = EvalCallback(_stub_env(), callback_on_new_best=stop, eval_freq=3, verbose=0)
    ev._evaluate = lambda: ([-5.0], [400])
    model = _Model(4)
    ev.init_callback(model)
    results = []
    for _ in range(3):
        model.num_timesteps += 4
        results.append(ev.on_step())
    assert results == [True, True, False] and stop.parent is ev and stop.n_calls == 1
    # max episodes: host arrays and (on the device rollout path) tensors are both counted
    import torch as th

    g = golden("callbacks_kat.npz")
    n_envs, max_ep, n_episodes, n_calls, _ = (int(v) for v in g["b/stop"])
    for kind in (np.asarray, lambda d: th.as_tensor(np.asarray(d, np.float32))):
        cb = StopTrainingOnMaxEpisodes(max_ep)
        model = _Model(n_envs)
        cb.init_callback(model)
        assert cb._total_max_episodes == max_ep * n_envs
        calls = 0
        while True:
            calls += 1
            cb.update_locals(dict(dones=kind([calls % 400 == 0] * n_envs)))
            if not cb.on_step():
                break
        assert (cb.n_episodes, calls) == (n_episodes, n_calls)
    # no model improvement: (2, min_evals=1) against a best that improves twice and then stalls
    stop = StopTrainingOnNoModelImprovement(2, min_evals=1)
    stop.init_callback(_Model(1))
    stop.parent = types.SimpleNamespace(best_mean_reward=-np.inf)
    outs = []
    for best in (-9.0, -8.0, -7.0, -7.0, -7.0, -7.0):
        stop.parent.best_mean_reward = best
        outs.append(stop.on_step())
    assert outs == [True, True, True, True, True, False] and stop.no_improvement_evals == 3


def test_every_n_timesteps_fires_at_the_recorded_timesteps(golden):
    g = golden("callbacks_kat.npz")
    for n_envs in (4, 3):
        rec = _Rec()
        cb = EveryNTimesteps(100, rec)
        model = _Model(n_envs)
        cb.init_callback(model)
        while model.num_timesteps < 650:
            model.num_timesteps += n_envs
            cb.on_step()
        assert [t for _, t in rec.seen] == g[f"e/fired_{n_envs}"].tolist() and model.num_timesteps == int(g[f"e/final_{n_envs}"][0])


def test_eval_episodes_entry_point_rejects_bad_arguments_on_the_host():
    """Every CSTR_E_BADARG / CSTR_E_UNSUPPORTED case of the header, on pointers that are never dereferenced (`targets` is a host array)."""
    lib = nv.lib()
    assert "cstr_eval_episodes_f32" in nv.SYMBOLS and hasattr(lib, "cstr_eval_episodes_f32")
    coef = nv.default_coef()
    null = C.c_void_p(None)
    A = lambda i: C.c_void_p(0x100000 * (i + 1))  # noqa: E731  distinct, 16-byte aligned, 1 MiB apart: nothing overlaps
    lo, hi = (C.c_float * 4)(-1, -1, -1, -1), (C.c_float * 4)(1, 1, 1, 1)
    good_net = dict(k0=4, h1=64, h2=64, act_dim=2, act=1, head=0, out_act=0, reserved=0, w1=A(0).value, b1=A(1).value, w2=A(2).value, b2=A(3).value,
                    w3=A(4).value, b3=A(5).value, w2_swizzled=A(6).value)

    def call(net=None, coef_=C.byref(coef), integrator=0, obs_dim=4, env_obs=A(7), steps=A(8), pcg=A(9), static=null, squashed=1, lo_=lo, hi_=hi,
             targets=(1, 0, 2), n=3, max_steps=10, ret=A(10), ln=A(11), dn=A(12)):
        f = dict(good_net, **(net or {}))
        pm = nv.PolicyMlp(*[f[k] for k in ("k0", "h1", "h2", "act_dim", "act", "head", "out_act", "reserved", "w1", "b1", "w2", "b2", "w3", "b3",
                                           "w2_swizzled")])
        tg = null if targets is None else (C.c_int32 * len(targets))(*targets)
        return lib.cstr_eval_episodes_f32(C.byref(pm), coef_, integrator, obs_dim, env_obs, steps, pcg, static, squashed, lo_, hi_, tg, C.c_int64(n),
                                          C.c_int64(max_steps), ret, ln, dn, null)

    BAD, UNS = -1, -2
    # NULL pointers
    assert lib.cstr_eval_episodes_f32(null, C.byref(coef), 0, 4, A(7), A(8), A(9), null, 1, lo, hi, (C.c_int32 * 1)(1), C.c_int64(1), C.c_int64(5), A(10),
                                      A(11), A(12), null) == BAD
    for kw in (dict(coef_=null), dict(env_obs=null), dict(steps=null), dict(pcg=null), dict(lo_=null), dict(hi_=null), dict(targets=None), dict(ret=null),
               dict(ln=null), dict(dn=null), dict(net=dict(w1=None)), dict(net=dict(b2=None)), dict(net=dict(w3=None))):
        assert call(**kw) == BAD, kw
    # sizes and targets
    assert call(n=0) == BAD and call(n=-3) == BAD
    assert call(targets=(1, -1, 2)) == BAD
    assert call(max_steps=0) == BAD and call(max_steps=-1) == BAD
    assert call(squashed=2) == BAD and call(net=dict(reserved=1)) == BAD
    assert call(net=dict(k0=8)) == BAD                                      # the policy reads the env's observation rows
    assert call(hi_=(C.c_float * 4)(1, -1, 1, 1)) == BAD                    # empty action interval
    # misaligned rows
    for kw in (dict(env_obs=C.c_void_p(A(7).value + 4)), dict(pcg=C.c_void_p(A(9).value + 8)), dict(ret=C.c_void_p(A(10).value + 4)),
               dict(ln=C.c_void_p(A(11).value + 2)), dict(net=dict(w2=A(2).value + 4)), dict(net=dict(w2_swizzled=A(6).value + 8))):
        assert call(**kw) == BAD, kw
    # outputs overlapping inputs, or each other
    assert call(ret=A(7)) == BAD and call(ln=A(9)) == BAD and call(dn=A(8)) == BAD and call(ret=A(2)) == BAD
    assert call(ln=C.c_void_p(A(10).value + 16)) == BAD and call(dn=C.c_void_p(A(7).value + 32)) == BAD
    # unsupported layouts, integrators and network shapes
    assert call(obs_dim=5, net=dict(k0=5)) == UNS and call(net=dict(act_dim=4)) == UNS and call(net=dict(act_dim=3)) == UNS
    assert call(integrator=7) == UNS
    assert call(net=dict(h1=66)) == UNS and call(net=dict(act=3)) == UNS and call(net=dict(head=2)) == UNS and call(net=dict(out_act=5)) == UNS
    assert call(net=dict(h1=1024, h2=512)) == UNS                           # more than 64 KB of LDS


def test_a_subclass_with_its_own_on_step_sees_every_call(tmp_path):
    """The event schedules describe the classes' own `_on_step`. Overriding it (per-step work on top of `super()._on_step()` is a
    common pattern) turns the answer into None, so graph replay keeps every iteration eager for such a callback."""
    class PerStepCheckpoint(CheckpointCallback):
        def _on_step(self):
            return super()._on_step()

    class PerStepEval(EvalCallback):
        def _on_step(self):
            return super()._on_step()

    class PerStepEvery(EveryNTimesteps):
        def _on_step(self):
            return super()._on_step()

    class OnlyNewMethods(CheckpointCallback):  # no override of `_on_step`: the schedule still holds
        def extra(self):
            return 1

    model = _Model(2)
    for cb in (PerStepCheckpoint(5, str(tmp_path)), PerStepEval(_stub_env(), eval_freq=5), PerStepEvery(10, BaseCallback())):
        cb.init_callback(model)
        assert cb.calls_until_event() is None
        assert CallbackList([NoopCallback(), cb]).calls_until_event() is None
    plain = OnlyNewMethods(5, str(tmp_path))
    plain.init_callback(model)
    assert plain.calls_until_event() == 5


class _HostEnv:
    """A two-env host VecEnv with 400-step episodes, enough for `evaluate_policy`'s host loop."""

    def __new__(cls):
        from core.common.vec_env.base_vec_env import VecEnv

        class Env(VecEnv):
            def __init__(self):
                self.num_envs, self.t, self.actions_seen = 2, np.zeros(2, np.int64), []

            def reset(self):
                self.t[:] = 0
                return np.zeros((2, 4), np.float32)

            def step(self, actions):
                self.actions_seen.append(np.asarray(actions).copy())
                self.t += 1
                dones = self.t >= 400
                rewards = -np.abs(np.asarray(actions, np.float32)).sum(axis=1)
                infos = [{"TimeLimit.truncated": bool(d)} for d in dones]
                self.t[dones] = 0
                return np.zeros((2, 4), np.float32), rewards, dones, infos

        return Env()


def test_eval_callback_evaluates_a_tape_policy_through_evaluate_policy(golden, tmp_path):
    """Run (a) of the fixture once more, this time through `EvalCallback._evaluate` itself: a stub model whose `predict` replays an
    action tape, a host VecEnv with 400-step episodes, `fused=False` and `fused=None` (the launch does not cover a stub: the loop
    runs). The evaluation's arguments arrive (`n_eval_episodes`, `deterministic`), the files and evaluations.npz are the fixture's,
    and the recorded returns are the f64 sums of the tape's f32 rewards."""
    g = golden("callbacks_kat.npz")
    n_envs, _, n_ep, eval_freq, save_freq, steps = (int(v) for v in g["a/dims"])
    tape = np.random.default_rng(4).uniform(-1, 1, size=(1000, 2, 2)).astype(np.float32)
    for fused in (False, None):
        d = tmp_path / str(fused)
        env = _HostEnv()
        model = _Model(n_envs)
        seen = []

        def predict(observations, state=None, episode_start=None, deterministic=False):
            seen.append(deterministic)
            return tape[(len(seen) - 1) % len(tape)].copy(), state

        model.predict = predict
        ev = EvalCallback(env, n_eval_episodes=n_ep, eval_freq=eval_freq, log_path=str(d / "log"), best_model_save_path=str(d / "best"), verbose=0,
                          warn=False, fused=fused)
        ck = CheckpointCallback(save_freq=save_freq, save_path=str(d / "ck"), name_prefix="m", save_replay_buffer=True)
        cb = CallbackList([ev, ck])
        cb.init_callback(model)
        cb.on_training_start({}, {})
        while model.num_timesteps < steps:
            model.num_timesteps += n_envs
            assert cb.on_step()
        e = np.load(d / "log" / "evaluations.npz")
        assert sorted(e.files) == g["a/eval_keys"].tolist() and e["timesteps"].tolist() == g["a/timesteps"].tolist()
        assert e["ep_lengths"].tolist() == g["a/ep_lengths"].tolist() and list(e["results"].shape) == g["a/results_shape"].tolist()
        assert sorted(os.listdir(d / "ck")) == g["a/ck_files"].tolist() and sorted(os.listdir(d / "best")) == g["a/best_files"].tolist()
        # 3 episodes over 2 envs: targets [1, 2] -> 800 vec-steps per evaluation, all deterministic, actions straight from the tape
        assert len(seen) == 2 * 800 and all(seen) and np.array_equal(env.actions_seen[5], tape[5])
        rew = -np.abs(tape).sum(axis=2)  # [t, env] float32
        first = [np.sum(rew[:400, 0].astype(np.float64)), np.sum(rew[:400, 1].astype(np.float64)), np.sum(rew[400:800, 1].astype(np.float64))]
        np.testing.assert_allclose(e["results"][0], first, rtol=1e-12)
    with pytest.raises(ValueError, match="evaluate_policy_fused does not cover"):
        ev = EvalCallback(_HostEnv(), eval_freq=1, verbose=0, warn=False, fused=True)
        ev.init_callback(_Model(2))
        ev.on_step()


def test_vecnormalize_checkpoint_name_and_the_wrapping_mismatch_message(tmp_path):
    from core.common.vec_env import VecNormalize

    written = []
    model = _Model(4)
    model.get_vec_normalize_env = lambda: types.SimpleNamespace(save=lambda path: (written.append(os.path.basename(path)), open(path, "w").close()))
    ck = CheckpointCallback(2, str(tmp_path), name_prefix="m", save_vecnormalize=True)
    ck.init_callback(model)
    for _ in range(2):
        model.num_timesteps += 4
        ck.on_step()
    assert written == ["m_vecnormalize_8_steps.pkl"] and sorted(os.listdir(tmp_path)) == ["m_8_steps.zip", "m_vecnormalize_8_steps.pkl"]
    # the training env is wrapped, the evaluation env is not: the reference's message
    wrapped = VecNormalize.__new__(VecNormalize)  # never initialised: only its type is looked at
    model = _Model(4)
    model.env = wrapped
    model.get_vec_normalize_env = lambda: wrapped
    ev = EvalCallback(_stub_env(), eval_freq=1, verbose=0, warn=False)
    ev._evaluate = lambda: pytest.fail("the evaluation must not start")
    with pytest.warns(UserWarning, match="Training and eval env are not of the same type"):
        ev.init_callback(model)
    model.num_timesteps += 4
    with pytest.raises(AssertionError, match="Training and eval env are not wrapped the same way, see https://stable-baselines3.readthedocs.io/"
                                             "en/master/guide/callbacks.html#evalcallback and warning above."):
        ev.on_step()
    # two bare envs: nothing to synchronise
    cbs.sync_envs_normalization(_stub_env(), _stub_env())
