"""cstr_eval_episodes_f32 (whole evaluation episodes in one launch) through the C ABI against the step-by-step launches, bit for bit,
and `evaluate_policy_fused` against the reference-written fixture and against `evaluate_policy`.

The step-by-step statement: cstr_policy_rows_fwd_f32 on the same cstr_policy_mlp_t (head 0: eps = 0), predict()'s post-processing,
cstr_vec_step_f32 with reset observations from cstr_reset_draw_f32 -- the launches `CSTRVecEnv.step_device` makes -- and the host
accounting of evaluation.py (f64 sums of the f32 step rewards). An env's pcg_state is compared as it stands right after the reset draw
behind its last counted episode: the host loop keeps stepping finished envs, the kernel does not (see the header)."""
import numpy as np
import pytest
import torch as th

from core import _native as nv
from core.common import hip_ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RELU, TANH, NONE = 1, 2, 0

# (n_envs, h1, h2, act, head, out_act, squashed, (obs_dim, act_dim), integrator, tile-major W2, init_mode, max_steps)
CASES = [
    (1, 16, 16, RELU, 0, NONE, True, (4, 2), "euler", True, "random", 5),
    (16, 64, 64, TANH, 1, TANH, True, (4, 2), "rk4", False, "random", 6),
    (17, 256, 256, RELU, 0, NONE, True, (8, 2), "euler", True, "static", 7),
    (48, 400, 300, RELU, 1, TANH, True, (4, 2), "euler", True, "random", 8),
    (17, 36, 20, TANH, 0, NONE, True, (8, 4), "rk4", False, "static", 9),
    (48, 36, 20, RELU, 1, NONE, False, (8, 4), "euler", True, "random", 5),
    (16, 256, 256, TANH, 1, NONE, False, (4, 2), "rk4", False, "random", 7),
    (48, 400, 300, TANH, 0, NONE, True, (8, 2), "rk4", False, "random", 6),
    (1, 64, 64, RELU, 1, NONE, False, (8, 2), "euler", True, "static", 9),
    (17, 16, 16, TANH, 0, NONE, False, (8, 4), "euler", True, "random", 8),
    (48, 256, 256, RELU, 0, NONE, True, (4, 2), "euler", False, "random", 5),
    (17, 528, 32, RELU, 0, NONE, True, (4, 2), "euler", True, "random", 6),  # wider than the split-K head's 512: shuffle-tree head on the tile-major W2
]


def _case_id(c):
    n, h1, h2, act, head, out_act, sq, lay, integ, swz, init, ms = c
    return f"n{n}-{h1}x{h2}-{'relu' if act == RELU else 'tanh'}-head{head}-{'squashed' if sq else 'clipped'}-{lay[0]}_{lay[1]}-{integ}-{'swz' if swz else 'rows'}-{init}"


def _targets(n):
    return np.array(([0, 1, 3, 2] * ((n + 3) // 4))[:n] if n > 1 else [3], np.int32)


def _pcg_words(seeds):
    m = (1 << 64) - 1
    words = np.empty((len(seeds), 4), np.uint64)
    for i, s in enumerate(seeds):
        st = np.random.PCG64(np.random.SeedSequence(int(s))).state["state"]
        words[i] = (st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)
    return th.from_numpy(words.view(np.int64)).to(DEV)


class _Setup:
    """Weights, env state and the step-by-step result of one case (computed once, then only read)."""

    def __init__(self, case):
        n, h1, h2, act, head, out_act, squashed, (d, a), integ, swz, init, max_steps = case
        self.case, self.n, self.d, self.a = case, n, d, a
        g = th.Generator(device=DEV).manual_seed(1000 * n + h1 + h2 + 7 * head)
        r = lambda *sh: th.randn(*sh, device=DEV, generator=g)  # noqa: E731
        n_out = 2 * a if head == 0 else a
        self.w = [r(h1, d) / d ** 0.5, r(h1) * 0.1, r(h2, h1) / h1 ** 0.5, r(h2) * 0.1, r(n_out, h2) * (2.0 / h2 ** 0.5), r(n_out) * 0.1]
        self.swz = ops.policy_swizzle(self.w[2]) if swz else None
        self.coef = nv.default_coef(max_steps=max_steps)
        self.low = [-1.0, -0.5, -1.0, -0.75][:a] if squashed else [-0.5] * a
        self.high = [1.0, 1.0, 0.5, 1.0][:a] if squashed else [0.25] * a
        self.targets = _targets(n)
        self.pcg0 = _pcg_words([11 + 3 * i for i in range(n)])
        self.static0 = None
        if init == "static":
            self.static0 = th.tensor([0.45, 310.0, 0.25, 290.0], dtype=th.float64, device=DEV).repeat(n, 2 if a == 4 else 1).contiguous()
        self.obs0 = th.zeros(n, d, device=DEV)
        pcg, st = self.pcg0.clone(), None if self.static0 is None else self.static0.clone()
        ops.reset_draw(pcg, None, self.obs0, a, static_init=st)  # the state evaluate_policy starts from: env.reset()
        self.pcg1, self.static1 = pcg, st
        self._reference()

    def state(self):
        return (self.obs0.clone(), th.zeros(self.n, dtype=th.int32, device=DEV), self.pcg1.clone(),
                None if self.static1 is None else self.static1.clone())

    def _reference(self):
        n, h1, h2, act, head, out_act, squashed, (d, a), integ, swz, init, max_steps = self.case
        obs, steps, pcg, static = self.state()
        low, high = th.tensor(self.low, device=DEV), th.tensor(self.high, device=DEV)
        action, eps = th.empty(n, a, device=DEV), (th.zeros(n, a, device=DEV) if head == 0 else None)
        nxt, buf = th.empty(n, d, device=DEV), th.empty(n, d, device=DEV)
        rew, done, tout = (th.empty(n, device=DEV) for _ in range(3))
        tg = self.targets
        counts, cur_ret, cur_len = np.zeros(n, np.int64), np.zeros(n), np.zeros(n, np.int64)
        stride = int(tg.max())
        self.ret, self.len = np.zeros((n, stride)), np.zeros((n, stride), np.int32)
        self.end_step = np.zeros((n, stride), np.int64)  # vec-step (1-based) at which episode [i][j] ended
        self.pcg_ref = pcg.cpu().numpy().copy()            # envs with target 0 keep their state
        t = 0
        while (counts < tg).any():
            assert t < stride * max_steps, "every episode is truncated by max_steps"
            ops.policy_rows_fwd(obs, *self.w, act, head, out_act, action, eps=eps, w2_swz=self.swz)
            env_act = (low + (0.5 * (action + 1.0)) * (high - low)) if squashed else th.minimum(th.maximum(action, low), high)
            ops.vec_step(self.coef, integ, obs, env_act.contiguous(), steps, obs, nxt, buf, rew, done, tout)
            ops.reset_draw(pcg, done.to(th.uint8), buf, a, static_init=static)
            obs.copy_(buf)
            t += 1
            rew_h, done_h, pcg_h = rew.cpu().numpy(), done.cpu().numpy() > 0, pcg.cpu().numpy()
            cur_ret += rew_h  # float64 += float32, as evaluation.py:97
            cur_len += 1
            for i in np.nonzero(done_h & (counts < tg))[0]:
                self.ret[i, counts[i]], self.len[i, counts[i]], self.end_step[i, counts[i]] = cur_ret[i], cur_len[i], t
                counts[i] += 1
                cur_ret[i], cur_len[i] = 0.0, 0
                if counts[i] == tg[i]:
                    self.pcg_ref[i] = pcg_h[i]
        self.vec_steps = t

    def launch(self, max_vec_steps, pad=3):
        """One launch from the case's initial state into sentinel-filled buffers with `pad` rows behind the envs'."""
        n, h1, h2, act, head, out_act, squashed, (d, a), integ, swz, init, max_steps = self.case
        obs, steps, pcg, static = self.state()
        stride = int(self.targets.max())
        ret = th.full((n + pad, stride), -777.25, dtype=th.float64, device=DEV)
        ln = th.full((n + pad, stride), -777, dtype=th.int32, device=DEV)
        dn = th.full((n + pad,), -777, dtype=th.int32, device=DEV)
        ops.eval_episodes_into(*self.w, act, head, out_act, self.swz, self.coef, integ, obs, steps, pcg, squashed, self.low, self.high,
                               self.targets, max_vec_steps, ret, ln, dn, static)
        return ret.cpu().numpy(), ln.cpu().numpy(), dn.cpu().numpy(), pcg.cpu().numpy(), steps.cpu().numpy()


_cache = {}


def _setup(case):
    if case not in _cache:
        _cache[case] = _Setup(case)
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_eval_episodes_match_the_step_by_step_launches_bit_for_bit(case):
    s = _setup(case)
    n, tg = s.n, s.targets
    assert min(s.len[i, j] for i in range(n) for j in range(tg[i])) >= 1 and s.vec_steps > case[-1]  # several resets per env
    # max_vec_steps exact: the number of vec-steps the step-by-step loop needed is enough
    ret, ln, dn, pcg, steps = s.launch(s.vec_steps)
    assert np.array_equal(dn[:n], tg)
    filled = np.arange(ret.shape[1])[None, :] < tg[:, None]
    assert np.array_equal(ln[:n][filled], s.len[filled])
    assert np.array_equal(ret[:n][filled].view(np.int64), s.ret[filled].view(np.int64))  # f64 sums, bit for bit
    assert np.array_equal(pcg, s.pcg_ref)
    # slots at and beyond targets[i] and the padding rows keep the sentinel
    assert (ret[:n][~filled] == -777.25).all() and (ln[:n][~filled] == -777).all()
    assert (ret[n:] == -777.25).all() and (ln[n:] == -777).all() and (dn[n:] == -777).all()
    # a relaunch from the same state gives the same bits, and so does the host's own bound max(targets) * max_steps
    again = s.launch(s.vec_steps)
    roomy = s.launch(int(tg.max()) * case[-1])
    for x, y, z in zip((ret, ln, dn, pcg, steps), again, roomy):
        assert x.tobytes() == y.tobytes() == z.tobytes()


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[5]], ids=_case_id)
def test_eval_episodes_end_at_the_step_bound(case):
    """The termination guarantee, exercised without provoking anything: one vec-step short of what the targets need the launch returns,
    with ep_done < targets exactly for the envs whose last episode ends at the last vec-step, and the wrapper raises."""
    s = _setup(case)
    n, tg = s.n, s.targets
    cap = s.vec_steps - 1
    ret, ln, dn, pcg, steps = s.launch(cap)
    want = np.array([sum(1 for j in range(tg[i]) if s.end_step[i, j] <= cap) for i in range(n)], np.int32)
    assert np.array_equal(dn[:n], want) and (want < tg).any()
    for i in range(n):
        assert np.array_equal(ln[i, :want[i]], s.len[i, :want[i]]) and ret[i, :want[i]].tobytes() == s.ret[i, :want[i]].tobytes()
        assert (ln[i, want[i]:] == -777).all()
    n_, h1, h2, act, head, out_act, squashed, (d, a), integ, swz, init, max_steps = case
    obs, st, pcg_t, static = s.state()
    with pytest.raises(RuntimeError, match="max_vec_steps"):
        ops.eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, st, pcg_t, squashed, s.low, s.high, tg, cap, static_init=static)


def test_eval_episodes_wrapper_checks_its_operands():
    s = _setup(CASES[0])
    n_, h1, h2, act, head, out_act, squashed, (d, a), integ, swz, init, max_steps = s.case
    obs, st, pcg, static = s.state()
    with pytest.raises(ValueError, match="non-negative"):
        ops.eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, st, pcg, squashed, s.low, s.high, [-1], 5)
    with pytest.raises(ValueError, match="targets"):
        ops.eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, st, pcg, squashed, s.low, s.high, [1, 1], 5)
    with pytest.raises(nv.NativeError, match="bad argument"):
        ops.eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, st, pcg, squashed, s.low, s.high, [1], 0)
    # all targets zero: nothing runs, nothing is an error
    ret, ln, dn = ops.eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, obs, st, pcg, squashed, s.low, s.high, [0], 5)
    assert ret.shape == (1, 0) and dn.tolist() == [0] and th.equal(pcg, s.pcg1)


# ---- evaluate_policy_fused ------------------------------------------------------------------------------------------------

def _fresh_env(n, seed, **kw):
    from core.common.vec_env import CSTRVecEnv

    env = CSTRVecEnv(n, **kw)
    env.seed(seed)
    return env


@pytest.mark.parametrize("name", ["sac", "td3"])
def test_evaluate_policy_fused_matches_the_reference_fixture(golden, name):
    """The seeded untrained class-default SAC / TD3 policies of tests/golden/evaluate_policy_kat.npz (written by the reference):
    lengths equal, returns at the rtol tests/test_learner_parity.py asserts for the same arrays; the list order and the (mean, std) form
    against `evaluate_policy` on the same seeds."""
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused, supported
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC
    from core.td3 import TD3

    g = golden("evaluate_policy_kat.npz")
    n_envs, n_ep, env_seed, model_seed = (int(v) for v in g["model_dims"])
    model = {"sac": SAC, "td3": TD3}[name]("MlpPolicy", CSTRVecEnv(2), seed=model_seed)
    env = _fresh_env(n_envs, env_seed)
    assert supported(model, env) and supported(model.policy, env, deterministic=True)
    with pytest.warns(UserWarning, match="Monitor"):
        rets, lens = evaluate_policy_fused(model, env, n_eval_episodes=n_ep, return_episode_rewards=True)
    assert lens == g[f"{name}_lengths"].tolist()
    np.testing.assert_allclose(np.asarray(rets, np.float64), g[f"{name}_returns"], rtol=1e-4, err_msg=name)
    rets_l, lens_l = evaluate_policy(model, _fresh_env(n_envs, env_seed), n_eval_episodes=n_ep, return_episode_rewards=True, warn=False)
    assert lens == [int(v) for v in lens_l]
    np.testing.assert_allclose(np.asarray(rets, np.float64), np.asarray(rets_l, np.float64), rtol=1e-4)
    mean, std = evaluate_policy_fused(model, _fresh_env(n_envs, env_seed), n_eval_episodes=n_ep, warn=False)
    assert abs(mean - np.mean(rets)) <= 1e-12 * abs(mean) and abs(std - np.std(rets)) <= 1e-9
    with pytest.raises(AssertionError, match="Mean reward below threshold"):
        evaluate_policy_fused(model, _fresh_env(n_envs, env_seed), n_eval_episodes=n_ep, warn=False, reward_threshold=0.0)


def test_evaluate_policy_fused_list_order_on_short_episodes():
    """13 episodes over 5 envs (targets [2, 2, 3, 3, 3]) of a 7-step env with the (8, 2) layout: the lists come back sorted by (vec-step
    at which the episode ended, env index), like the loop appends them -- every env's returns differ, so a per-env concatenation
    would not pass."""
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused
    from core.common.vec_env import CSTRVecEnv
    from core.td3 import TD3

    class Short(CSTRVecEnv):
        max_steps = 7

    def env():
        e = Short(5, obs_dim=8)
        e.seed(5)
        return e

    model = TD3("MlpPolicy", env(), seed=3, policy_kwargs=dict(net_arch=[32, 32]))
    rets, lens = evaluate_policy_fused(model, env(), n_eval_episodes=13, return_episode_rewards=True, warn=False)
    rets_l, lens_l = evaluate_policy(model, env(), n_eval_episodes=13, return_episode_rewards=True, warn=False)
    assert len(rets) == 13 and lens == [int(v) for v in lens_l] == [7] * 13 and len(set(rets)) == 13
    np.testing.assert_allclose(np.asarray(rets, np.float64), np.asarray(rets_l, np.float64), rtol=1e-4)


def test_evaluate_policy_fused_ppo_policy_against_the_loop():
    """`ActorCriticPolicy`: policy_net + action_net as a deterministic head without output activation, clipped into the action box."""
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused, supported
    from core.ppo import PPO

    model = PPO("MlpPolicy", _fresh_env(4, 0), n_steps=8, batch_size=32, seed=1, device=DEV)
    with th.no_grad():
        model.policy.action_net.weight.mul_(40.0)  # drive some actions out of the box: the clip does something
    env = _fresh_env(4, 9)
    assert supported(model, env)
    rets, lens = evaluate_policy_fused(model, env, n_eval_episodes=6, return_episode_rewards=True, warn=False)
    rets_l, lens_l = evaluate_policy(model, _fresh_env(4, 9), n_eval_episodes=6, return_episode_rewards=True, warn=False)
    assert lens == [int(v) for v in lens_l]
    np.testing.assert_allclose(np.asarray(rets, np.float64), np.asarray(rets_l, np.float64), rtol=1e-4)


def test_evaluate_policy_fused_declines_what_it_does_not_cover():
    from core.common.evaluation import evaluate_policy_fused, supported
    from core.common.vec_env import VecNormalize
    from core.dqn import DQN
    from core.sac import SAC

    env = _fresh_env(4, 0)
    sac = SAC("MlpPolicy", env, seed=0, policy_kwargs=dict(net_arch=[16, 16]))
    declined = [
        (sac, env, False),                                                                            # stochastic evaluation
        (sac, VecNormalize(_fresh_env(4, 0)), True),                                                  # a VecNormalize wrapper
        (SAC("MlpPolicy", env, seed=0, use_sde=True, policy_kwargs=dict(net_arch=[16, 16])), env, True),   # gSDE
        (SAC("MlpPolicy", env, seed=0, policy_kwargs=dict(net_arch=[16, 16, 16])), env, True),            # other depths
        (SAC("MlpPolicy", env, seed=0, policy_kwargs=dict(net_arch=[16])), env, True),
    ]
    denv = _fresh_env(4, 0, discrete_actions=3)
    declined.append((DQN("MlpPolicy", denv, seed=0, batch_size=16, buffer_size=64), denv, True))      # the Discrete face
    for model, e, det in declined:
        assert not supported(model, e, det)
        with pytest.raises(ValueError, match="evaluate_policy_fused does not cover"):
            evaluate_policy_fused(model, e, n_eval_episodes=2, deterministic=det, warn=False)


def test_evaluate_policy_fused_declines_multi_agent_and_offline_policies():
    from core.bcq import BCQ
    from core.common.evaluation import supported
    from core.maddpg import MADDPG
    from core.sac import SAC

    env = _fresh_env(4, 0)
    data = SAC("MlpPolicy", _fresh_env(16, 0), seed=0, batch_size=16, buffer_size=16 * 8, policy_kwargs=dict(net_arch=[16, 16]))
    data.learn(16 * 4)
    bcq = BCQ("MlpPolicy", _fresh_env(1, 0), dataset=data.replay_buffer, seed=0, batch_size=16, policy_kwargs=dict(critic_net_arch=[16, 16]))
    assert not supported(bcq, env)
    maddpg = MADDPG(2, "MlpPolicy", env, [[0, 1], [2, 3]], [[0], [1]], learning_rate_list=[1e-3, 1e-3], seed=0, batch_size=16, buffer_size=64,
                    policy_kwargs=dict(net_arch=[[16, 16], [16, 16]]))
    assert not supported(maddpg, env)
