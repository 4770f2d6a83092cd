"""core.ARS (core/ars): constructor contract, the flat parameter vector, one learn() on the kernel path against the restatement's update
(tests/_ars_reference.py) applied to the returns the population launch produced, the kernel path against the published statements on
one env, bookkeeping (num_timesteps, logger keys, callbacks), save / load, predict() on a LinearPolicy, the refusals, evaluation.
Bars: the update 1e-6 |want| + 1e-7 (tests/test_ars_abi.py); returns max(4 d, 2e-6 |R64|) with d the distance between the restatement's
two precisions on the same state (tests/test_ars_abi.py), each path against the fp64 restatement."""
import warnings

import numpy as np
import pytest
import torch as th
from torch import nn

import _ars_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_STEPS = 7


def _env(n, **kw):
    from core import _native as nv
    from core.common.vec_env import CSTRVecEnv

    env = CSTRVecEnv(n, device=DEV, **kw)
    env.max_steps = MAX_STEPS
    env.coef = nv.default_coef(0.20, 0.05, 0.45, MAX_STEPS)  # 7-step episodes
    return env


class _Record:
    """a callback that keeps what every update left"""

    def __init__(self, stop_after=None):
        from core.common.callbacks import BaseCallback

        outer = self
        self.returns, self.lengths, self.weights, self.kept, self.steps, self.stop_after = [], [], [], [], [], stop_after

        class CB(BaseCallback):
            def _on_step(self) -> bool:
                m = self.model
                outer.returns.append(m.last_returns.cpu().numpy().copy())
                outer.lengths.append(m._lengths.cpu().numpy().copy())
                outer.weights.append(m.weights.cpu().numpy().copy())
                outer.kept.append(m._kept.cpu().numpy().copy())
                outer.steps.append(m.num_timesteps)
                return outer.stop_after is None or len(outer.returns) < outer.stop_after

        self.cb = CB()


def test_constructor_defaults_and_n_top_clamp():
    from core import ARS
    from core.ars import ARSLinearPolicy, ARSPolicy

    m = ARS("MlpPolicy", _env(2), device=DEV)
    assert (m.n_delta, m.n_top, m.learning_rate, m.delta_std, m.zero_policy, m.alive_bonus_offset, m.n_eval_episodes) == (8, 8, 0.02, 0.05, True, 0, 1)
    assert type(m.policy) is ARSPolicy and m.policy.net_arch == [64, 64] and m.policy.with_bias and m.policy.squash_output
    assert [type(x) for x in m.policy.action_net] == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear, nn.Tanh] and m.fused_learner
    lin = ARS("LinearPolicy", _env(2), device=DEV)
    assert type(lin.policy) is ARSLinearPolicy and lin.policy.net_arch == [] and not lin.policy.with_bias and lin.fused_learner
    assert [type(x) for x in lin.policy.action_net] == [nn.Linear, nn.Tanh] and lin.policy.action_net[0].bias is None and lin.n_params == 8
    assert set(ARS.policy_aliases) == {"MlpPolicy", "LinearPolicy"}
    with pytest.warns(UserWarning, match="n_top"):
        assert ARS("LinearPolicy", _env(1), n_delta=4, n_top=9, device=DEV).n_top == 4
    assert ARS("LinearPolicy", _env(1), n_delta=4, n_top=2, device=DEV).n_top == 2
    assert not ARS("MlpPolicy", _env(1), policy_kwargs=dict(net_arch=[65]), device=DEV).fused_learner  # wider than the kernels take


def test_zero_policy_and_parameter_order():
    from core import ARS

    z = ARS("MlpPolicy", _env(1), seed=1, device=DEV, policy_kwargs=dict(net_arch=[5, 3]))
    assert z.weights.shape == (4 * 5 + 5 + 5 * 3 + 3 + 3 * 2 + 2,) and not bool(z.weights.any())
    assert all(not bool(p.any()) for p in z.policy.parameters())
    m = ARS("MlpPolicy", _env(1), seed=1, zero_policy=False, device=DEV, policy_kwargs=dict(net_arch=[5, 3]))
    assert bool(m.weights.any()) and th.equal(m.weights, th.nn.utils.parameters_to_vector(m.policy.parameters()))
    m.weights[0] = 7.0  # the modules view the vector
    assert float(m.policy.action_net[0].weight[0, 0]) == 7.0


@pytest.mark.parametrize("policy,n_envs", [("LinearPolicy", 6), ("MlpPolicy", 3)])
def test_learn_on_the_kernel_path_applies_the_update_to_its_returns(policy, n_envs):
    from core import ARS

    kw = dict(policy_kwargs=dict(net_arch=[16, 8])) if policy == "MlpPolicy" else {}
    m = ARS(policy, _env(n_envs), n_delta=3, n_top=2, zero_policy=False, n_eval_episodes=2, alive_bonus_offset=-1, seed=4, device=DEV, **kw)
    assert m.fused_learner
    w = [m.weights.cpu().numpy().copy()]
    rec = _Record()
    per_update = 6 * 2 * MAX_STEPS
    m.learn(3 * per_update, callback=rec.cb)
    assert m._n_updates == 3 and len(rec.returns) == 3 and rec.cb.n_calls == 3
    assert m.num_timesteps == sum(int(x.sum()) for x in rec.lengths) == 3 * per_update and rec.steps == [per_update, 2 * per_update, 3 * per_update]
    for u in range(3):
        want, step, std, kept = ref.update(w[u], rec.returns[u], 3, 2, 0.02, ref.deltas(m.delta_seed, u, 3, m.n_params))
        assert np.array_equal(rec.kept[u], kept)
        err, bar = np.abs(rec.weights[u].astype(np.float64) - want), 1e-6 * np.abs(want) + 1e-7
        print(f"ARS learn {policy} update {u}: worst err / bar = {float((err / bar).max()):.3f}")
        assert (err <= bar).all()
        w.append(rec.weights[u])


def test_kernel_path_and_published_statements_agree_on_one_env():
    from core import ARS
    from oracle import cstr_oracle as orc

    models = []
    for fused in (True, False):
        m = ARS("MlpPolicy", _env(1), n_delta=2, zero_policy=False, seed=3, device=DEV, policy_kwargs=dict(net_arch=[8]))
        assert m.fused_learner
        m.fused_learner = fused
        models.append(m)
    probe = _env(1)
    probe.seed(3)
    probe.reset_device()  # the state learn()'s seeded reset leaves
    spec = dict(obs_dim=4, act_dim=2, hidden=[8], act="relu", with_bias=True, squash=True)
    args = (models[0].weights.cpu().numpy(), spec, 0.05, models[0].delta_seed, 0, 2, 1, 0.0, orc.default_coef(0.20, 0.05, 0.45, MAX_STEPS), "euler",
            probe.obs.cpu().numpy(), probe.step_count.cpu().numpy(), probe.pcg_state.cpu().numpy().view(np.uint64), None, [-1.0, -1.0], [1.0, 1.0])
    r64, r32 = ref.run_population(*args, np.float64), ref.run_population(*args, np.float32)
    bar = np.maximum(4.0 * np.abs(r32["returns"] - r64["returns"]).max(), 2e-6 * np.abs(r64["returns"]))
    for m in models:
        m.learn(4 * MAX_STEPS)
        assert m._n_updates == 1 and m.num_timesteps == 4 * MAX_STEPS
        err = np.abs(m.last_returns.cpu().numpy() - r64["returns"])
        print(f"ARS paths (fused_learner={m.fused_learner}): worst err / bar = {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), (err, bar)
        assert np.array_equal(m.env.pcg_state.cpu().numpy().view(np.uint64), r64["pcg"])  # the same reset-draw stream
    assert th.equal(models[0].env.pcg_state, models[1].env.pcg_state)
    assert th.equal(models[0]._kept, models[1]._kept)
    np.testing.assert_allclose(models[0].weights.cpu().numpy(), models[1].weights.cpu().numpy(), rtol=1e-4, atol=1e-6)


def test_logger_keys_and_callback_stop():
    from core import ARS
    from core.common.logger import Logger

    m = ARS("LinearPolicy", _env(4), n_delta=2, seed=0, device=DEV)
    logger, seen = Logger(), {}
    dump = logger.dump
    logger.dump = lambda step=0: (seen.update(logger.resolved()), dump(step))
    m.set_logger(logger)
    rec = _Record(stop_after=2)
    m.learn(10 * 4 * MAX_STEPS, callback=rec.cb)
    assert m._n_updates == 2 and rec.cb.n_calls == 2 and m.num_timesteps == 2 * 4 * MAX_STEPS  # False stops learn()
    for key in ("train/iterations", "train/delta_std", "train/learning_rate", "train/step_size", "rollout/return_std", "rollout/ep_rew_mean",
                "rollout/ep_len_mean", "time/fps", "time/time_elapsed", "time/total_timesteps"):
        assert key in seen, key
    assert seen["train/iterations"] == 2 and seen["rollout/ep_len_mean"] == MAX_STEPS and seen["train/delta_std"] == 0.05
    assert abs(seen["rollout/ep_rew_mean"] - rec.returns[-1].mean()) <= 1e-12 * abs(rec.returns[-1].mean())


def test_save_load_round_trip(tmp_path):
    from core import ARS

    m = ARS("LinearPolicy", _env(4), n_delta=2, n_top=1, seed=0, device=DEV, policy_kwargs=dict(with_bias=True))
    m.learn(2 * 4 * MAX_STEPS)
    assert bool(m.weights.any())
    obs = np.random.default_rng(0).uniform(-1, 1, (5, 4)).astype(np.float32)
    want, _ = m.predict(obs, deterministic=True)
    path = str(tmp_path / "ars")
    m.save(path)
    back = ARS.load(path, env=_env(4), device=DEV)
    assert (back.n_delta, back.n_top, back._n_updates, back.num_timesteps, back.delta_seed) == (2, 1, m._n_updates, m.num_timesteps, m.delta_seed)
    assert th.equal(back.weights, m.weights) and th.equal(back.weights, th.nn.utils.parameters_to_vector(back.policy.parameters()))
    got, _ = back.predict(obs, deterministic=True)
    assert np.array_equal(got, want)


def test_predict_on_a_linear_policy_is_the_unscaled_gain():
    from core import ARS
    from core.common.spaces import Box

    m = ARS("LinearPolicy", _env(1), zero_policy=False, seed=2, device=DEV)
    m.action_space = m.policy.action_space = Box(np.array([-2.0, 0.5], np.float32), np.array([1.0, 3.0], np.float32), dtype=np.float32)
    obs = np.random.default_rng(1).uniform(-1, 1, (9, 4)).astype(np.float32)
    got, state = m.predict(obs, deterministic=True)
    k = m.policy.action_net[0].weight
    low, high = th.tensor([-2.0, 0.5], device=DEV), th.tensor([1.0, 3.0], device=DEV)
    want = low + 0.5 * (th.tanh(th.as_tensor(obs, device=DEV) @ k.T) + 1.0) * (high - low)
    assert state is None and got.shape == (9, 2)
    np.testing.assert_allclose(got, want.cpu().numpy(), rtol=2e-6, atol=1e-6)


def test_refusals():
    from core import ARS
    from core.common.vec_env import CSTRVecEnv, VecNormalize

    refusal = (ValueError, NotImplementedError, AssertionError)
    with pytest.raises(refusal):
        ARS("MlpPolicy", VecNormalize(_env(2)), device=DEV)
    with pytest.raises(refusal):
        ARS("MlpPolicy", CSTRVecEnv(2, goal_conditioned=True, device=DEV), device=DEV)
    with pytest.raises(refusal):
        ARS("MlpPolicy", CSTRVecEnv(2, discrete_actions=3, device=DEV), device=DEV)
    with pytest.raises(refusal):
        ARS("MlpPolicy", CSTRVecEnv(2, multi_discrete_actions=(3, 5), device=DEV), device=DEV)
    for bad in (dict(n_delta=0), dict(n_eval_episodes=0), dict(delta_std=0.0), dict(delta_std=-0.1)):
        with pytest.raises(ValueError):
            ARS("MlpPolicy", _env(1), device=DEV, **bad)
    m = ARS("LinearPolicy", _env(1), device=DEV)
    with pytest.raises(NotImplementedError):
        m.enable_graph_capture(True)
    m.enable_graph_capture(False)
    with pytest.raises(NotImplementedError):
        m.learn(10, async_eval=object())
    with pytest.raises(ValueError):
        ARS("CnnPolicy", _env(1), device=DEV)


def test_refuses_data_parallel_runs(monkeypatch):
    from core import ARS
    from core.common import distributed as dist_util

    monkeypatch.setattr(dist_util, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        ARS("LinearPolicy", _env(1), device=DEV)


def test_evaluation_takes_the_model():
    from core import ARS
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused, supported

    m = ARS("LinearPolicy", _env(2), n_delta=2, seed=0, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rets, lens = evaluate_policy(m, _env(2), n_eval_episodes=3, return_episode_rewards=True)
        assert len(rets) == 3 and lens == [MAX_STEPS] * 3
        assert not supported(m, _env(2))
        with pytest.raises(ValueError, match="does not cover"):  # it says so, it does not crash
            evaluate_policy_fused(m, _env(2), n_eval_episodes=2)
        cb = EvalCallback(_env(2), n_eval_episodes=2, eval_freq=1, verbose=0)
        m.learn(2 * 4 * MAX_STEPS, callback=cb)
    assert len(cb.evaluations_results) == 2 or cb.last_mean_reward > -np.inf
