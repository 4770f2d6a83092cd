"""The training callbacks on real learn() loops: graph replay between callback events (SAC, DQN), the stop callbacks against the
reference-written tests/golden/callbacks_kat.npz, checkpoints that load, the on-policy eager loop, and `EvalCallback(fused=...)`."""
import os

import numpy as np
import pytest
import torch as th

from core.common.callbacks import (BaseCallback, CheckpointCallback, EvalCallback, EveryNTimesteps, StopTrainingOnMaxEpisodes,
                                   StopTrainingOnNoModelImprovement, StopTrainingOnRewardThreshold)
from core.common.vec_env import CSTRVecEnv

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]


class ShortEnv(CSTRVecEnv):
    max_steps = 20


def _env(n, seed, cls=CSTRVecEnv, **kw):
    e = cls(n, **kw)
    e.seed(seed)
    return e


def _run_with_events(make_model, mode, tmp, iters, n_envs, calls_per_iter=1, **eval_env_kw):
    from core.common import legacy_rng

    d = tmp / str(mode)
    ev = EvalCallback(_env(8, 21, ShortEnv, **eval_env_kw), n_eval_episodes=3, eval_freq=37, log_path=str(d / "log"), verbose=0, warn=False)
    ck = CheckpointCallback(save_freq=50, save_path=str(d / "ck"), name_prefix="m")
    model = make_model()
    if mode != "eager":
        model.enable_graph_capture(True, unroll=8 if mode == "unroll8" else 1)
    model.learn(n_envs * calls_per_iter * iters, callback=[ev, ck])
    th.cuda.synchronize()
    env, rb = model.get_env().unwrapped, model.replay_buffer
    e = np.load(d / "log" / "evaluations.npz")
    state = dict(weights=np.concatenate([p.detach().cpu().numpy().ravel() for p in model.policy.parameters()]),
                 ring_obs=rb.ring.observations.cpu().numpy(), ring_act=rb.ring.actions.cpu().numpy(), ring_rew=rb.ring.rewards.cpu().numpy(),
                 ring_ctl=rb.ring.ctl.cpu().numpy(), sampler=legacy_rng.global_stream(model.device).cpu().numpy().copy(),
                 env_obs=env.obs.cpu().numpy(), env_steps=env.step_count.cpu().numpy(), env_pcg=env.pcg_state.cpu().numpy(),
                 eval_timesteps=e["timesteps"], eval_results=e["results"], eval_lengths=e["ep_lengths"])
    return state, model, ev, ck, sorted(os.listdir(d / "ck"))


def _compare_runs(make_model, tmp, iters, n_envs, calls_per_iter=1, **eval_env_kw):
    from core.common.graph_replay import GRAPH_WARMUP_ITERATIONS

    runs = {m: _run_with_events(make_model, m, tmp, iters, n_envs, calls_per_iter, **eval_env_kw) for m in ("eager", "graph", "unroll8")}
    base, model0, ev0, ck0, files0 = runs["eager"]
    calls = iters * calls_per_iter
    assert ev0.n_calls == ck0.n_calls == calls and base["eval_timesteps"].tolist() == [37 * n_envs * k for k in range(1, calls // 37 + 1)]
    assert files0 == sorted(f"m_{50 * n_envs * k}_steps.zip" for k in range(1, calls // 50 + 1))
    for mode in ("graph", "unroll8"):
        state, model, ev, ck, files = runs[mode]
        for k in base:  # print each figure before asserting
            a, b = np.asarray(base[k], np.float64), np.asarray(state[k], np.float64)
            print(f"{mode} {k}: max |diff| = {np.abs(a - b).max() if a.size else 0.0:.3e}, equal bits = {base[k].tobytes() == state[k].tobytes()}")
        for k in base:
            assert base[k].tobytes() == state[k].tobytes(), (mode, k)
        assert (ev.n_calls, ck.n_calls, files) == (ev0.n_calls, ck0.n_calls, files0) and model.num_timesteps == model0.num_timesteps
        st = model.graph_status()
        assert st["replays"] > 0 and st["error"] is None
        # eager iterations: what runs before the replays can start (learning_starts, warm-up per graph) plus one per event, no more
        events = len(set(range(37, calls + 1, 37)) | set(range(50, calls + 1, 50)))
        event_iters = len({(c - 1) // calls_per_iter for c in set(range(37, calls + 1, 37)) | set(range(50, calls + 1, 50))})
        assert event_iters <= events
        print(f"{mode}: replays {st['replays']}, eager iterations {st['eager_iterations']}, graphs {st['graphs']}, event iterations {event_iters}")
        assert st["replays"] + st["eager_iterations"] == iters
        warm = sum(model._graph_warm.values())
        assert warm <= GRAPH_WARMUP_ITERATIONS * (st["graphs"] + 1)
        assert st["eager_iterations"] == model._eager_before_replay + warm + event_iters


def test_sac_graph_replay_between_callback_events_equals_the_eager_run(tmp_path):
    """SAC, 16 envs, [EvalCallback(eval_freq=37, 3 episodes on 8 short-episode envs), CheckpointCallback(save_freq=50)], 300
    iterations: eager, replayed one iteration per graph, and eight per graph. Policy weights, ring, sampler stream, env state and
    evaluations.npz bit for bit; equal callback counters; replays happened; eager iterations = start-up + warm-up + one per event."""
    from core.sac import SAC

    def make():
        m = SAC("MlpPolicy", _env(16, 4), seed=5, batch_size=32, buffer_size=16 * 64, learning_starts=64, policy_kwargs=dict(net_arch=[32, 32]))
        m._eager_before_replay = 64 // 16
        return m

    _compare_runs(make, tmp_path, 300, 16)


def test_dqn_graph_replay_with_events_in_the_middle_of_an_iteration(tmp_path):
    """DQN with train_freq=4: an iteration is four on_step() calls, so events at calls 37, 50, 74, ... fall inside iterations; those
    iterations run eagerly, the others replay."""
    from core.dqn import DQN

    def make():
        m = DQN("MlpPolicy", _env(16, 4, discrete_actions=3), seed=5, batch_size=32, buffer_size=16 * 64, learning_starts=64, train_freq=4,
                policy_kwargs=dict(net_arch=[32, 32]))
        m._eager_before_replay = 1
        return m

    _compare_runs(make, tmp_path, 80, 16, calls_per_iter=4, discrete_actions=3)


def test_a_user_callback_keeps_every_iteration_eager():
    from core.sac import SAC

    class Mine(BaseCallback):
        def _on_step(self):
            return True

    model = SAC("MlpPolicy", _env(16, 4), seed=5, batch_size=32, buffer_size=16 * 64, learning_starts=64, policy_kwargs=dict(net_arch=[32, 32]))
    model.enable_graph_capture(True)
    cb = Mine()
    model.learn(16 * 40, callback=cb)
    st = model.graph_status()
    assert cb.n_calls == 40 and st["replays"] == 0 and st["eager_iterations"] == 40 and st["graphs"] == 0


def _idle_sac(n, **kw):
    from core.sac import SAC

    return SAC("MlpPolicy", _env(n, 3), seed=0, batch_size=16, buffer_size=4096, learning_starts=10 ** 6, policy_kwargs=dict(net_arch=[16, 16]), **kw)


def test_stop_callbacks_end_learn_where_the_reference_fixture_says(golden):
    g = golden("callbacks_kat.npz")
    # StopTrainingOnRewardThreshold(-inf) behind a new best: the first evaluation ends the run
    n_envs, eval_freq, ev_calls, stop_t = (int(v) for v in g["c/stop"])
    ev = EvalCallback(_env(2, 7), callback_on_new_best=StopTrainingOnRewardThreshold(-np.inf), n_eval_episodes=2, eval_freq=eval_freq, verbose=0,
                      warn=False)
    model = _idle_sac(n_envs)
    model.learn(2000, callback=ev)
    assert (ev.n_calls, model.num_timesteps) == (ev_calls, stop_t)
    # StopTrainingOnMaxEpisodes: `dones` is a device tensor on this path
    n_envs, max_ep, n_episodes, n_calls, stop_t = (int(v) for v in g["b/stop"])
    cb = StopTrainingOnMaxEpisodes(max_episodes=max_ep)
    model = _idle_sac(n_envs)
    model.enable_graph_capture(True)  # answers None: every iteration stays eager
    model.learn(10 ** 5, callback=cb)
    assert (cb.n_episodes, cb.n_calls, model.num_timesteps) == (n_episodes, n_calls, stop_t) and model.graph_status()["replays"] == 0
    # StopTrainingOnNoModelImprovement(2, min_evals=1) with the fixture's action tape in place of the policy
    n_envs, eval_freq, stop_calls, ev_calls, stop_t, no_imp, tape_t = (int(v) for v in g["d/stop"])
    tape = th.as_tensor(g["d/tape"]).cuda()
    stop = StopTrainingOnNoModelImprovement(max_no_improvement_evals=2, min_evals=1)
    ev = EvalCallback(_env(2, 7), callback_after_eval=stop, n_eval_episodes=2, eval_freq=eval_freq, verbose=0, warn=False, fused=False)
    model = _idle_sac(n_envs)
    t = [0]

    def replay(obs, deterministic=False):
        t[0] += 1
        return tape[(t[0] - 1) % tape.shape[0]]

    model.policy._predict = replay
    model.learn(10 ** 5, callback=ev)
    assert (stop.n_calls, ev.n_calls, model.num_timesteps, stop.no_improvement_evals, t[0]) == (stop_calls, ev_calls, stop_t, no_imp, tape_t)


@pytest.mark.parametrize("graph", [False, True])
def test_every_n_timesteps_fires_at_the_recorded_timesteps(golden, graph):
    from core.sac import SAC

    g = golden("callbacks_kat.npz")

    class Rec(BaseCallback):
        def __init__(self):
            super().__init__()
            self.seen = []

        def _on_step(self):
            self.seen.append(self.num_timesteps)
            return True

    for n in (4, 3):
        rec = Rec()
        model = SAC("MlpPolicy", _env(n, 3), seed=0, batch_size=16, buffer_size=4096, learning_starts=n, policy_kwargs=dict(net_arch=[16, 16]))
        model.enable_graph_capture(graph)
        model.learn(650, callback=EveryNTimesteps(n_steps=100, callback=rec))
        assert rec.seen == g[f"e/fired_{n}"].tolist() and model.num_timesteps == int(g[f"e/final_{n}"][0])
        assert (model.graph_status()["replays"] > 0) == graph


def test_checkpoints_and_best_model_load(tmp_path):
    from core.sac import SAC

    ev = EvalCallback(_env(4, 21, ShortEnv), n_eval_episodes=4, eval_freq=10, best_model_save_path=str(tmp_path / "best"), verbose=0, warn=False)
    ck = CheckpointCallback(save_freq=15, save_path=str(tmp_path / "ck"), name_prefix="m", save_replay_buffer=True)
    model = SAC("MlpPolicy", _env(8, 4), seed=5, batch_size=16, buffer_size=8 * 32, learning_starts=16, policy_kwargs=dict(net_arch=[16, 16]))
    model.learn(8 * 30, callback=[ev, ck])
    assert sorted(os.listdir(tmp_path / "ck")) == ["m_120_steps.zip", "m_240_steps.zip", "m_replay_buffer_120_steps.pkl", "m_replay_buffer_240_steps.pkl"]
    best = SAC.load(str(tmp_path / "best" / "best_model.zip"), env=_env(8, 4))
    assert all(bool(th.isfinite(p).all()) for p in best.policy.parameters())
    last = SAC.load(str(tmp_path / "ck" / "m_240_steps.zip"), env=_env(8, 4))
    assert last.num_timesteps == 240 and all(bool(th.isfinite(p).all()) for p in last.policy.parameters())
    last.load_replay_buffer(str(tmp_path / "ck" / "m_replay_buffer_240_steps.pkl"))
    for name in ("observations", "next_observations", "actions", "rewards"):  # the hook fires behind the 30th add: the ring is the final one
        assert th.equal(getattr(last.replay_buffer.ring, name), getattr(model.replay_buffer.ring, name)), name


@pytest.mark.parametrize("algo", ["ppo", "a2c"])
def test_on_policy_eager_loop_with_an_eval_callback(algo, tmp_path):
    from core.a2c import A2C
    from core.ppo import PPO

    ev = EvalCallback(_env(4, 21, ShortEnv), n_eval_episodes=4, eval_freq=12, log_path=str(tmp_path), verbose=0, warn=False, fused=True)
    if algo == "ppo":
        model = PPO("MlpPolicy", _env(8, 4), n_steps=8, batch_size=32, n_epochs=2, seed=0, device="cuda:0")
    else:
        model = A2C("MlpPolicy", _env(8, 4), seed=0, device="cuda:0")
    model.learn(8 * 40, callback=ev)
    e = np.load(tmp_path / "evaluations.npz")
    assert e["timesteps"].tolist() == [96, 192, 288] and e["ep_lengths"].tolist() == [[20] * 4] * 3 and ev.n_calls == 40
    best = e["results"].mean(axis=1).max()
    assert np.isfinite(e["results"]).all() and abs(ev.best_mean_reward - best) <= 1e-12 * abs(best)


def test_eval_callback_fused_modes(tmp_path):
    from core.common import evaluation
    from core.common.vec_env import VecNormalize
    from core.sac import SAC

    model = SAC("MlpPolicy", _env(8, 4), seed=5, batch_size=16, buffer_size=8 * 32, learning_starts=16, policy_kwargs=dict(net_arch=[16, 16]))
    # fused=True on what the launch does not cover raises at the first evaluation
    with pytest.raises(ValueError, match="evaluate_policy_fused does not cover"):
        model.learn(8 * 10, callback=EvalCallback(VecNormalize(_env(4, 21, ShortEnv)), eval_freq=5, verbose=0, warn=False, fused=True))
    with pytest.raises(ValueError, match="evaluate_policy_fused does not cover"):
        model.learn(8 * 10, callback=EvalCallback(_env(4, 21, ShortEnv), eval_freq=5, deterministic=False, verbose=0, warn=False, fused=True))
    # fused=True and fused=False give the same evaluations (lengths equal, returns at the loop-vs-launch rtol of the evaluation tests).
    # 8 episodes over 4 envs: every env runs two, so loop and launch leave the eval env in the same state for the second evaluation
    # (with an uneven split the loop keeps stepping the envs that are done, the launch does not: see evaluate_policy_fused)
    got = {}
    for fused in (True, False, None):
        m = SAC("MlpPolicy", _env(8, 4), seed=5, batch_size=16, buffer_size=8 * 32, learning_starts=16, policy_kwargs=dict(net_arch=[16, 16]))
        ev = EvalCallback(_env(4, 21, ShortEnv), n_eval_episodes=8, eval_freq=10, log_path=str(tmp_path / str(fused)), verbose=0, warn=False, fused=fused)
        m.learn(8 * 20, callback=ev)
        got[fused] = np.load(tmp_path / str(fused) / "evaluations.npz")
    assert got[True]["ep_lengths"].tolist() == got[False]["ep_lengths"].tolist() == [[20] * 8] * 2
    np.testing.assert_allclose(got[True]["results"], got[False]["results"], rtol=1e-4)
    default = got[True] if evaluation.FUSED_BY_DEFAULT else got[False]
    assert got[None]["results"].tobytes() == default["results"].tobytes()


def test_eval_callback_fused_true_on_an_unsupported_model_raises():
    """`fused=True` with models the launch does not cover: a one-hidden-layer actor, gSDE, DQN's Discrete face."""
    from core.dqn import DQN
    from core.sac import SAC

    kw = dict(seed=5, batch_size=16, buffer_size=8 * 32, learning_starts=16)
    models = [(SAC("MlpPolicy", _env(8, 4), policy_kwargs=dict(net_arch=[16]), **kw), {}),
              (SAC("MlpPolicy", _env(8, 4), use_sde=True, policy_kwargs=dict(net_arch=[16, 16]), **kw), {}),
              (DQN("MlpPolicy", _env(8, 4, discrete_actions=3), policy_kwargs=dict(net_arch=[16, 16]), **kw), dict(discrete_actions=3))]
    for model, env_kw in models:
        ev = EvalCallback(_env(4, 21, ShortEnv, **env_kw), eval_freq=5, verbose=0, warn=False, fused=True)
        with pytest.raises(ValueError, match="evaluate_policy_fused does not cover"):
            model.learn(8 * 10, callback=ev)
        assert ev.n_calls == 5 and ev.evaluations_timesteps == []
        # the same model evaluates through the loop
        ok = EvalCallback(_env(4, 21, ShortEnv, **env_kw), eval_freq=5, n_eval_episodes=4, verbose=0, warn=False, fused=None)
        model.learn(8 * 5, callback=ok)
        assert np.isfinite(ok.last_mean_reward)


@pytest.mark.parametrize("graph", [False, True])
def test_the_reference_run_with_both_callbacks(golden, tmp_path, graph):
    """Run (a) of tests/golden/callbacks_kat.npz as the reference ran it: SAC on 4 envs, learning_starts 40, EvalCallback(3 episodes on
    2 envs, eval_freq 50) + CheckpointCallback(save_freq 60, "m", replay buffer), 520 steps. Files, evaluations.npz and the final
    counters -- `_n_updates` included -- are the reference's, eagerly and with graph replay between the events."""
    from core.sac import SAC

    g = golden("callbacks_kat.npz")
    n_envs, n_eval_envs, n_ep, eval_freq, save_freq, steps = (int(v) for v in g["a/dims"])
    ev = EvalCallback(_env(n_eval_envs, 7), n_eval_episodes=n_ep, eval_freq=eval_freq, log_path=str(tmp_path / "log"),
                      best_model_save_path=str(tmp_path / "best"), verbose=0, warn=False)
    ck = CheckpointCallback(save_freq=save_freq, save_path=str(tmp_path / "ck"), name_prefix="m", save_replay_buffer=True)
    model = SAC("MlpPolicy", _env(n_envs, 3), seed=0, batch_size=16, buffer_size=4096, learning_starts=40, policy_kwargs=dict(net_arch=[16, 16]))
    model.enable_graph_capture(graph)
    model.learn(steps, callback=[ev, ck])
    e = np.load(tmp_path / "log" / "evaluations.npz")
    assert sorted(os.listdir(tmp_path / "ck")) == g["a/ck_files"].tolist() and sorted(os.listdir(tmp_path / "log")) == g["a/log_files"].tolist()
    assert sorted(os.listdir(tmp_path / "best")) == g["a/best_files"].tolist() and sorted(e.files) == g["a/eval_keys"].tolist()
    assert e["timesteps"].tolist() == g["a/timesteps"].tolist() and e["ep_lengths"].tolist() == g["a/ep_lengths"].tolist()
    assert list(e["results"].shape) == g["a/results_shape"].tolist()
    assert [ev.n_calls, ck.n_calls, ev.num_timesteps, model.num_timesteps, model._n_updates] == g["a/counters"].tolist()
    assert (model.graph_status()["replays"] > 0) == graph


def test_vecnormalize_statistics_reach_the_evaluation_env_and_the_checkpoint(tmp_path):
    from core.common.callbacks import sync_envs_normalization
    from core.common.vec_env import VecNormalize
    from core.sac import SAC

    train_env = VecNormalize(_env(8, 4))
    eval_env = VecNormalize(_env(4, 21, ShortEnv), training=False)
    ev = EvalCallback(eval_env, n_eval_episodes=4, eval_freq=10, verbose=0, warn=False)
    ck = CheckpointCallback(save_freq=20, save_path=str(tmp_path), name_prefix="m", save_vecnormalize=True)
    model = SAC("MlpPolicy", train_env, seed=5, batch_size=16, buffer_size=8 * 32, learning_starts=16, policy_kwargs=dict(net_arch=[16, 16]))
    before = eval_env._state.clone()
    model.learn(8 * 20, callback=[ev, ck])  # the last call is an evaluation: nothing moves the training statistics after it
    assert not th.equal(eval_env._state, before) and th.equal(eval_env._state, train_env._state)
    assert len(ev.evaluations_timesteps) == 0 and np.isfinite(ev.last_mean_reward)
    assert sorted(os.listdir(tmp_path)) == ["m_160_steps.zip", "m_vecnormalize_160_steps.pkl"]
    loaded = VecNormalize.load(str(tmp_path / "m_vecnormalize_160_steps.pkl"), _env(8, 4))
    assert th.equal(loaded._state, train_env._state)
    # an evaluation env that is not wrapped like the training env
    bad = EvalCallback(_env(4, 21, ShortEnv), eval_freq=5, verbose=0, warn=False)
    with pytest.raises(AssertionError, match="Training and eval env are not wrapped the same way"):
        model.learn(8 * 10, callback=bad)
    with pytest.raises(AttributeError, match="observations"):
        sync_envs_normalization(train_env, VecNormalize(_env(4, 21, obs_dim=8)))
