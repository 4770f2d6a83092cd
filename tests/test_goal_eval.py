"""cstr_eval_goal_episodes_f32 (whole evaluation episodes on the goal face in one launch) through the C ABI against the step-by-step
launches, bit for bit; `evaluate_policy_fused` / `evaluate_goal_tracking` / `EvalCallback` on HER models against `evaluate_policy`.

The step-by-step statement: cstr_policy_rows_fwd_f32 on the flat rows [achieved | desired | observation] (k0 = 6; head 0: eps = 0),
predict()'s post-processing, cstr_goal_vec_step_f32 -- the launches `CSTRVecEnv.step_device` makes on the goal face -- and the host
accounting of evaluation.py (f64 sums of the f32 step rewards); the tracking outputs are NumPy statements on that launch's `next_rows`.
An env's state is compared as it stands right after the reset draw and the target redraw behind its last counted episode: the host loop
keeps stepping finished envs, the kernel does not (see the header)."""
import numpy as np
import pytest
import torch as th

from core import _native as nv
from core.common import hip_ops as ops
from core.common.vec_env.cstr_vec_env import draw_goal_targets

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]

DEV = "cuda:0"
RELU, TANH, NONE = 1, 2, 0
GOAL_SEED, INDEX_OFFSET, GOAL_LO, GOAL_HI = (1 << 40) + 12345, 1000, 0.10, 0.40  # a seed above 2^32, a non-zero index offset
SENT_F, SENT_I = -777.25, -777

# (n_envs, h1, h2, act, head, out_act, squashed, integrator, tile-major W2, init_mode, max_steps, goal redraw, targets, NaN in b3)
CASES = [
    (1, 16, 16, RELU, 0, NONE, True, "euler", True, "random", 5, True, "uneven", False),
    (16, 36, 20, TANH, 1, TANH, True, "rk4", False, "static", 6, True, "uneven", False),
    (17, 256, 256, RELU, 0, NONE, True, "euler", True, "static", 7, False, "uneven", False),
    (48, 400, 300, RELU, 1, TANH, True, "euler", True, "random", 6, True, "uneven", False),
    (17, 36, 20, TANH, 0, NONE, False, "rk4", False, "random", 7, True, "uneven", False),
    (48, 16, 16, RELU, 1, NONE, False, "euler", True, "random", 5, False, "uneven", False),
    (16, 256, 256, TANH, 1, NONE, False, "rk4", False, "random", 7, True, "uneven", False),
    (48, 400, 300, TANH, 0, NONE, True, "rk4", False, "static", 6, True, "uneven", False),
    (17, 528, 32, RELU, 0, NONE, True, "euler", True, "random", 6, True, "uneven", False),  # wider than the split-K head's 512
    (16, 64, 64, RELU, 0, NONE, True, "euler", True, "random", 400, True, "ones", False),  # the default episode length, one episode each
    (1, 16, 16, TANH, 0, NONE, True, "euler", False, "random", 5, True, "uneven", True),   # the NaN path: every action is NaN
]
GRID, DEFAULT_LENGTH, NAN_CASE = CASES[:9], CASES[9], CASES[10]


def _case_id(c):
    n, h1, h2, act, head, out_act, sq, integ, swz, init, ms, redraw, tg, nan = c
    return (f"n{n}-{h1}x{h2}-{'relu' if act == RELU else 'tanh'}-head{head}-{'squashed' if sq else 'clipped'}-{integ}-{'swz' if swz else 'rows'}-"
            f"{init}-{'redraw' if redraw else 'fixed'}-T{ms}{'-nan' if nan else ''}")


def _targets(n, kind):
    if kind == "ones":
        return np.ones(n, np.int32)
    return np.array(([0, 1, 3, 2] * ((n + 3) // 4))[:n] if n > 1 else [3], np.int32)


def _pcg_words(seeds):
    m = (1 << 64) - 1
    words = np.empty((len(seeds), 4), np.uint64)
    for i, s in enumerate(seeds):
        st = np.random.PCG64(np.random.SeedSequence(int(s))).state["state"]
        words[i] = (st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)
    return th.from_numpy(words.view(np.int64)).to(DEV)


def _goal_of_target(coef, t):
    return np.float32(2) * (np.asarray(t, np.float32) - np.float32(coef.s_lo[2])) / np.float32(coef.s_span[2]) - np.float32(1)


STATE = ("obs", "steps", "pcg", "target", "episode", "static")
OUTS = ("ret", "len", "goal", "gap", "abs")


class _Setup:
    """Weights, env state and the step-by-step result of one case (computed once, then only read)."""

    def __init__(self, case):
        n, h1, h2, act, head, out_act, squashed, integ, swz, init, max_steps, redraw, tg_kind, nan = case
        self.case, self.n = case, n
        g = th.Generator(device=DEV).manual_seed(1000 * n + h1 + h2 + 7 * head)
        r = lambda *sh: th.randn(*sh, device=DEV, generator=g)  # noqa: E731
        n_out = 4 if head == 0 else 2
        self.w = [r(h1, 6) / 6 ** 0.5, r(h1) * 0.1, r(h2, h1) / h1 ** 0.5, r(h2) * 0.1, r(n_out, h2) * (2.0 / h2 ** 0.5), r(n_out) * 0.1]
        if nan:
            self.w[5][0] = float("nan")
        self.swz = ops.policy_swizzle(self.w[2]) if swz else None
        self.coef = nv.default_coef(max_steps=max_steps)
        self.low = [-1.0, -0.5] if squashed else [-0.5, -0.5]
        self.high = [1.0, 1.0] if squashed else [0.25, 0.25]
        self.targets = _targets(n, tg_kind)
        self.goal_kw = dict(goal_seed=GOAL_SEED, goal_index_offset=INDEX_OFFSET, goal_lo=GOAL_LO, goal_hi=GOAL_HI)
        pcg = _pcg_words([11 + 3 * i for i in range(n)])
        static = th.tensor([0.45, 310.0, 0.25, 290.0], dtype=th.float64, device=DEV).repeat(n, 1).contiguous() if init == "static" else None
        obs = th.zeros(n, 4, device=DEV)
        ops.reset_draw(pcg, None, obs, 2, static_init=static)  # the state evaluate_policy starts from: env.reset()
        target = th.from_numpy(np.linspace(0.12, 0.38, n).astype(np.float32)).to(DEV)
        episode = th.arange(3, 3 + n, dtype=th.int32, device=DEV) if redraw else None
        self.state0 = dict(obs=obs, steps=th.zeros(n, dtype=th.int32, device=DEV), pcg=pcg, target=target, episode=episode, static=static)
        self._reference()

    def state(self, pad=0):
        """A fresh copy of the initial env state; with `pad` sentinel rows behind the envs' (the launch gets the leading views)."""
        out = {}
        for k, t in self.state0.items():
            if t is None:
                out[k] = None
                continue
            full = th.full((self.n + pad,) + tuple(t.shape[1:]), SENT_I, dtype=t.dtype, device=DEV)
            full[:self.n] = t
            out[k] = full
        return out

    def _reference(self):
        n, h1, h2, act, head, out_act, squashed, integ, swz, init, max_steps, redraw, tg_kind, nan = self.case
        s = self.state()
        low, high = th.tensor(self.low, device=DEV), th.tensor(self.high, device=DEV)
        action, eps = th.empty(n, 2, device=DEV), (th.zeros(n, 2, device=DEV) if head == 0 else None)
        next_rows, rows_after = th.empty(n, 6, device=DEV), th.empty(n, 6, device=DEV)
        rew, done, tout = (th.empty(n, device=DEV) for _ in range(3))
        obs_h = s["obs"].cpu().numpy()
        rows = th.from_numpy(np.concatenate([obs_h[:, 2:3], _goal_of_target(self.coef, s["target"].cpu().numpy())[:, None], obs_h], axis=1)).to(DEV)
        tg = self.targets
        counts, cur_ret, cur_len, cur_abs = np.zeros(n, np.int64), np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
        stride = int(tg.max())
        self.ref = dict(ret=np.zeros((n, stride)), len=np.zeros((n, stride), np.int32), goal=np.zeros((n, stride), np.float32),
                        gap=np.zeros((n, stride), np.float32), abs=np.zeros((n, stride)))
        self.end_step = np.zeros((n, stride), np.int64)  # vec-step (1-based) at which episode [i][j] ended
        self.final = {k: (None if v is None else v.cpu().numpy().copy()) for k, v in s.items()}  # envs with target 0 keep their state
        self.raw_targets = np.full((n, stride), np.nan, np.float32)
        t = 0
        while (counts < tg).any():
            assert t < stride * max_steps, "every episode is truncated by max_steps"
            self.raw_targets[np.arange(n)[counts < tg], counts[counts < tg]] = s["target"].cpu().numpy()[counts < tg]
            ops.policy_rows_fwd(rows, *self.w, act, head, out_act, action, eps=eps, w2_swz=self.swz)
            env_act = (low + (0.5 * (action + 1.0)) * (high - low)) if squashed else th.minimum(th.maximum(action, low), high)
            ops.goal_vec_step(self.coef, integ, s["obs"], env_act.contiguous(), s["steps"], s["pcg"], s["target"], next_rows, rows_after, rew, done,
                              tout, static_init=s["static"], episode=s["episode"], **self.goal_kw)
            rows.copy_(rows_after)
            t += 1
            rew_h, done_h, nr = rew.cpu().numpy(), done.cpu().numpy() > 0, next_rows.cpu().numpy()
            gap = nr[:, 0] - nr[:, 1]  # one f32 subtraction
            cur_ret += rew_h           # float64 += float32, as evaluation.py:97
            cur_abs += np.abs(gap).astype(np.float64)
            cur_len += 1
            fin = np.nonzero(done_h & (counts < tg))[0]
            if fin.size:
                now = {k: (None if v is None else v.cpu().numpy()) for k, v in s.items()}
            for i in fin:
                j = counts[i]
                self.ref["ret"][i, j], self.ref["len"][i, j], self.ref["abs"][i, j] = cur_ret[i], cur_len[i], cur_abs[i]
                self.ref["goal"][i, j], self.ref["gap"][i, j], self.end_step[i, j] = nr[i, 1], gap[i], t
                counts[i] += 1
                cur_ret[i], cur_len[i], cur_abs[i] = 0.0, 0, 0.0
                if counts[i] == tg[i]:
                    for k in STATE:
                        if now[k] is not None:
                            self.final[k][i] = now[k][i]
        self.vec_steps = t

    def launch(self, max_vec_steps, pad=3, tracking=True):
        """One launch from the case's initial state into sentinel-filled buffers with `pad` rows behind the envs'."""
        n, h1, h2, act, head, out_act, squashed, integ, swz, init, max_steps, redraw, tg_kind, nan = self.case
        s = self.state(pad)
        v = {k: (None if t is None else t[:n]) for k, t in s.items()}
        stride = int(self.targets.max())
        full = lambda val, dt: th.full((n + pad, stride), val, dtype=dt, device=DEV)  # noqa: E731
        out = dict(ret=full(SENT_F, th.float64), len=full(SENT_I, th.int32), goal=full(SENT_F, th.float32), gap=full(SENT_F, th.float32),
                   abs=full(SENT_F, th.float64))
        dn = th.full((n + pad,), SENT_I, dtype=th.int32, device=DEV)
        track = (out["goal"], out["gap"], out["abs"]) if tracking else (None, None, None)
        ops.goal_eval_episodes_into(*self.w, act, head, out_act, self.swz, self.coef, integ, v["obs"], v["steps"], v["pcg"], v["target"], squashed,
                                    self.low, self.high, self.targets, max_vec_steps, out["ret"], out["len"], dn, *track, static_init=v["static"],
                                    episode=v["episode"], **self.goal_kw)
        res = {k: t.cpu().numpy() for k, t in out.items()}
        res["done"] = dn.cpu().numpy()
        res.update({k: (None if t is None else t.cpu().numpy()) for k, t in s.items()})
        return res


_cache = {}


def _setup(case):
    if case not in _cache:
        _cache[case] = _Setup(case)
    return _cache[case]


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


def _assert_matches(s, res):
    n, tg = s.n, s.targets
    assert np.array_equal(res["done"][:n], tg)
    filled = np.arange(res["ret"].shape[1])[None, :] < tg[:, None]
    for k in OUTS:  # f64 sums and f32 values, bit for bit (a NaN would be compared by its bits too)
        assert _bits(res[k][:n][filled]) == _bits(s.ref[k][filled]), k
        # slots at and beyond targets[i] and the padding rows keep the sentinel
        sent = SENT_I if k == "len" else SENT_F
        assert (res[k][:n][~filled] == sent).all() and (res[k][n:] == sent).all(), k
    assert (res["done"][n:] == SENT_I).all()
    for k in STATE:  # the env state the launch leaves, and the rows behind the envs' untouched
        if s.final[k] is None:
            assert res[k] is None
            continue
        assert _bits(res[k][:n]) == _bits(s.final[k][:n]), k
        assert (res[k][n:] == SENT_I).all(), k


@pytest.mark.parametrize("case", GRID, ids=_case_id)
def test_goal_eval_episodes_match_the_step_by_step_launches_bit_for_bit(case):
    s = _setup(case)
    n, tg, max_steps, redraw = s.n, s.targets, case[10], case[11]
    assert (s.ref["len"][np.arange(s.ref["len"].shape[1])[None, :] < tg[:, None]] == max_steps).all() and s.vec_steps > max_steps  # several resets
    ran = ~np.isnan(s.raw_targets)
    if redraw:  # the reference really redrew: an env's setpoints differ between its episodes, and follow the Philox contract
        i = int(np.argmax(tg))
        assert len(set(s.raw_targets[i, :tg[i]].tolist())) == tg[i]
        want = draw_goal_targets(GOAL_SEED, np.full(tg[i] - 1, INDEX_OFFSET + i), 3 + i + np.arange(tg[i] - 1), GOAL_LO, GOAL_HI)
        assert np.array_equal(s.raw_targets[i, 1:tg[i]], want)
        assert np.array_equal(s.final["episode"], 3 + np.arange(n) + tg)
    else:
        assert np.array_equal(s.final["target"], s.state0["target"].cpu().numpy())
    assert np.array_equal(s.ref["goal"][ran], _goal_of_target(s.coef, s.raw_targets[ran]))
    res = s.launch(s.vec_steps)  # max_vec_steps exact: the number of vec-steps the step-by-step loop needed is enough
    _assert_matches(s, res)
    # a relaunch from the same state gives the same bits, and so does the host's own bound max(targets) * max_steps
    again, roomy = s.launch(s.vec_steps), s.launch(int(tg.max()) * max_steps)
    for k in OUTS + STATE + ("done",):
        if res[k] is not None:
            assert _bits(res[k]) == _bits(again[k]) == _bits(roomy[k]), k
    # the three tracking outputs are optional: without them the rest is the same
    bare = s.launch(s.vec_steps, tracking=False)
    for k in ("ret", "len", "done") + STATE:
        if res[k] is not None:
            assert _bits(res[k]) == _bits(bare[k]), k
    assert all((bare[k] == SENT_F).all() for k in ("goal", "gap", "abs"))


def test_goal_eval_episodes_default_episode_length():
    s = _setup(DEFAULT_LENGTH)
    assert s.vec_steps == 400 and (s.ref["len"] == 400).all()
    _assert_matches(s, s.launch(400))


def test_goal_eval_episodes_nan_path():
    """A NaN in b3 makes every action NaN: goal_step_kernel's NaN path -- old state, -10, the episode ends -- at every step."""
    s = _setup(NAN_CASE)
    assert s.targets.tolist() == [3] and s.ref["len"].tolist() == [[1, 1, 1]] and s.ref["ret"].tolist() == [[-10.0, -10.0, -10.0]]
    res = s.launch(s.vec_steps)
    _assert_matches(s, res)
    assert res["len"][0].tolist() == [1, 1, 1] and res["ret"][0].tolist() == [-10.0, -10.0, -10.0]
    # the old state: the terminal row's achieved goal is the observation the episode started from
    assert res["gap"][0, 0] == s.state0["obs"].cpu().numpy()[0, 2] - _goal_of_target(s.coef, s.state0["target"].cpu().numpy())[0]


@pytest.mark.parametrize("case", [GRID[0], GRID[2], GRID[3], GRID[5]], ids=_case_id)
def test_goal_eval_episodes_end_at_the_step_bound(case):
    """One vec-step short of what the targets need the launch returns, with ep_done < targets exactly for the envs whose last episode
    ends at the last vec-step, and the wrapper raises."""
    s = _setup(case)
    n, tg = s.n, s.targets
    cap = s.vec_steps - 1
    res = s.launch(cap)
    want = np.array([sum(1 for j in range(tg[i]) if s.end_step[i, j] <= cap) for i in range(n)], np.int32)
    assert np.array_equal(res["done"][:n], want) and (want < tg).any()
    for i in range(n):
        for k in OUTS:
            assert _bits(res[k][i, :want[i]]) == _bits(s.ref[k][i, :want[i]]), k
        assert (res["len"][i, want[i]:] == SENT_I).all()
    n_, h1, h2, act, head, out_act, squashed, integ, swz, init, max_steps, redraw, tg_kind, nan = case
    v = s.state()
    with pytest.raises(RuntimeError, match="max_vec_steps"):
        ops.goal_eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, v["obs"], v["steps"], v["pcg"], v["target"], squashed, s.low, s.high,
                               tg, cap, static_init=v["static"], episode=v["episode"], **s.goal_kw)


def test_goal_eval_episodes_wrapper_checks_its_operands():
    s = _setup(GRID[0])
    n_, h1, h2, act, head, out_act, squashed, integ, swz, init, max_steps, redraw, tg_kind, nan = s.case
    v = s.state()
    args = lambda: (*s.w, act, head, out_act, s.swz, s.coef, integ, v["obs"], v["steps"], v["pcg"], v["target"], squashed, s.low, s.high)  # noqa: E731
    with pytest.raises(ValueError, match="non-negative"):
        ops.goal_eval_episodes(*args(), [-1], 5)
    with pytest.raises(ValueError, match="targets"):
        ops.goal_eval_episodes(*args(), [1, 1], 5)
    with pytest.raises(ValueError, match="target"):
        ops.goal_eval_episodes(*s.w, act, head, out_act, s.swz, s.coef, integ, v["obs"], v["steps"], v["pcg"], v["target"].double(), squashed, s.low,
                               s.high, [1], 5)
    with pytest.raises(nv.NativeError, match="bad argument"):
        ops.goal_eval_episodes(*args(), [1], 0)
    # all targets zero: nothing runs, nothing is an error
    out = ops.goal_eval_episodes(*args(), [0], 5, episode=v["episode"], tracking=True, **s.goal_kw)
    assert len(out) == 6 and out[0].shape == (1, 0) and out[2].tolist() == [0] and th.equal(v["pcg"], s.state0["pcg"])
    assert th.equal(v["target"], s.state0["target"]) and th.equal(v["episode"], s.state0["episode"])


# ---- evaluate_policy_fused / evaluate_goal_tracking / EvalCallback on HER models -------------------------------------------------

GOAL_RANGE = (0.10, 0.40)


def _goal_env_class():
    from core.common.vec_env import CSTRVecEnv

    class ShortGoalEnv(CSTRVecEnv):
        max_steps = 7

    return ShortGoalEnv


def _goal_env(n, seed, **kw):
    e = _goal_env_class()(n, device=DEV, goal_conditioned=True, goal_range=GOAL_RANGE, goal_seed=5, **kw)
    e.seed(seed)
    return e


def _her_model(algo, n=4, **kw):
    import core
    from core.her import HerReplayBuffer

    kw.setdefault("policy_kwargs", dict(net_arch=[32, 32]))
    kw.setdefault("buffer_size", 64 * n)
    return getattr(core, algo)("MultiInputPolicy", _goal_env(n, 0), seed=3, replay_buffer_class=HerReplayBuffer, device=DEV, **kw)


@pytest.mark.parametrize("algo", ["SAC", "TD3"])
def test_evaluate_policy_fused_on_the_goal_face_against_the_loop(algo):
    """6 episodes over 4 envs (targets [1, 1, 2, 2]) of a 7-step goal env with redrawn setpoints: episode lists in the loop's order,
    lengths equal, returns at the bar of the Box-face comparison (tests/test_eval_episodes.py: rtol = 1e-4)."""
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused, supported

    model = _her_model(algo)
    env = _goal_env(4, 9)
    assert supported(model, env) and supported(model.policy, env, deterministic=True)
    with pytest.warns(UserWarning, match="Monitor"):
        rets, lens = evaluate_policy_fused(model, env, n_eval_episodes=6, return_episode_rewards=True)
    rets_l, lens_l = evaluate_policy(model, _goal_env(4, 9), n_eval_episodes=6, return_episode_rewards=True, warn=False)
    a, b = np.asarray(rets, np.float64), np.asarray(rets_l, np.float64)
    print(f"{algo} goal face, launch against loop: largest relative difference of an episode return = {np.abs(a / b - 1.0).max():.3e}")
    assert len(rets) == 6 and lens == [int(v) for v in lens_l] == [7] * 6 and len(set(rets)) == 6
    np.testing.assert_allclose(a, b, rtol=1e-4)
    mean, std = evaluate_policy_fused(model, _goal_env(4, 9), n_eval_episodes=6, warn=False)
    assert abs(mean - np.mean(rets)) <= 1e-12 * abs(mean) and abs(std - np.std(rets)) <= 1e-9
    # the env is left as step_device leaves it: flat rows of the state behind the last counted episodes
    obs, tg = env.obs.cpu().numpy(), env.targets.cpu().numpy()
    assert np.array_equal(env.flat.cpu().numpy(), np.concatenate([obs[:, 2:3], env.goal_of_target(tg)[:, None], obs], axis=1))
    assert env.episode.tolist() == [2, 2, 3, 3] and env.step_count.tolist() == [0] * 4  # reset() drew ordinal 0, then one per episode


def test_evaluate_policy_fused_goal_face_refusals():
    from core.common.evaluation import evaluate_goal_tracking, evaluate_policy_fused, supported
    from core.common.vec_env import CSTRVecEnv, VecNormalize
    from core.sac import SAC

    her, goal_env = _her_model("SAC"), _goal_env(4, 0)
    box_env = CSTRVecEnv(4, device=DEV)
    box = SAC("MlpPolicy", box_env, seed=0, policy_kwargs=dict(net_arch=[16, 16]), device=DEV)
    assert supported(her, goal_env) and supported(box, box_env)
    declined = [(her, box_env, True), (box, goal_env, True), (her, goal_env, False), (her, VecNormalize(CSTRVecEnv(4, device=DEV)), True)]
    for model, e, det in declined:
        assert not supported(model, e, det)
        with pytest.raises(ValueError, match="evaluate_policy_fused does not cover"):
            evaluate_policy_fused(model, e, n_eval_episodes=2, deterministic=det, warn=False)
    for model, e in ((box, box_env), (her, box_env), (box, goal_env)):
        with pytest.raises(ValueError, match="evaluate_goal_tracking does not cover"):
            evaluate_goal_tracking(model, e, n_eval_episodes=2, warn=False)


def test_evaluate_goal_tracking_against_the_step_by_step_launches():
    """`target` against draw_goal_targets for the ordinals the envs ran; `final_error` / `mean_abs_error` against the float64 NumPy
    evaluation of the `next_rows` of a twin env stepped through `step_device` with the actor's own launches."""
    from core.common.evaluation import _fused_operands, evaluate_goal_tracking, evaluate_policy_fused

    model, n, n_ep = _her_model("SAC"), 4, 6
    out = evaluate_goal_tracking(model, _goal_env(n, 9), n_eval_episodes=n_ep, warn=False)
    assert set(out) == {"episode_rewards", "episode_lengths", "target", "final_error", "mean_abs_error"}
    rets, lens = evaluate_policy_fused(model, _goal_env(n, 9), n_eval_episodes=n_ep, return_episode_rewards=True, warn=False)
    assert out["episode_rewards"].tolist() == rets and out["episode_lengths"].tolist() == lens == [7] * n_ep
    # the twin, step by step
    twin = _goal_env(n, 9)
    rows = twin.reset_device()
    p = _fused_operands(model.policy)
    (l1, l2), w3, b3 = p["layers"], p["w3"].detach().contiguous(), p["b3"].detach().contiguous()
    w = [t.detach().contiguous() for t in (l1.weight, l1.bias, l2.weight, l2.bias)] + [w3, b3]
    low, high = (th.as_tensor(np.asarray(v, np.float32), device=DEV) for v in (model.policy.action_space.low, model.policy.action_space.high))
    action, eps, swz = th.empty(n, 2, device=DEV), th.zeros(n, 2, device=DEV), ops.policy_swizzle(w[2])
    targets = np.array([(n_ep + i) // n for i in range(n)])
    counts, cur_abs, cur_len, t, recs = np.zeros(n, np.int64), np.zeros(n), np.zeros(n, np.int64), 0, []
    half_span, lo2 = float(twin.coef.s_span[2]) / 2.0, float(twin.coef.s_lo[2])
    while (counts < targets).any():
        raw = twin.targets.cpu().numpy().copy()
        ops.policy_rows_fwd(rows, *w, p["act"], p["head"], p["out_act"], action, eps=eps, w2_swz=swz)
        rows, _, done, _, next_rows = twin.step_device((low + (0.5 * (action + 1.0)) * (high - low)).contiguous())
        t += 1
        nr = next_rows.cpu().numpy()
        gap = nr[:, 0] - nr[:, 1]
        cur_abs += np.abs(gap).astype(np.float64)
        cur_len += 1
        for i in np.nonzero((done.cpu().numpy() > 0) & (counts < targets))[0]:
            recs.append((t, i, float(raw[i]), float(nr[i, 1]), float(gap[i]) * half_span, cur_abs[i] / cur_len[i] * half_span, 1 + counts[i]))
            counts[i] += 1
            cur_abs[i], cur_len[i] = 0.0, 0
    recs.sort(key=lambda r: (r[0], r[1]))
    assert np.array_equal(out["final_error"], np.array([r[4] for r in recs])) and np.array_equal(out["mean_abs_error"], np.array([r[5] for r in recs]))
    assert (out["mean_abs_error"] > 0).all() and (np.abs(out["final_error"]) > 0).all()
    # the setpoints: reset() drew ordinal 0, so episode j of an env ran on ordinal j. `target` is the float64 inverse map of the launch's
    # float32 goal, exactly; against the drawn float32 setpoint it differs by the goal's rounding alone: g = fl(fl(2 t / span) - 1) carries
    # half an ulp of a value below 2 (2^-24) from the division and half an ulp of a value below 1 (2^-25) from the subtraction, i.e.
    # at most 1.5 * 2^-24 in g and 1.5 * 2^-24 * span / 2 in mol/L; the assertion allows 2 * 2^-24 * span / 2
    drawn = draw_goal_targets(5, np.array([r[1] for r in recs]), np.array([r[6] - 1 for r in recs]), *GOAL_RANGE)
    assert np.array_equal(drawn, np.array([r[2] for r in recs], np.float32))
    assert np.array_equal(out["target"], lo2 + (np.array([r[3] for r in recs], np.float64) + 1.0) * half_span)
    assert np.abs(out["target"] - drawn.astype(np.float64)).max() <= 2.0 * 2.0 ** -24 * half_span


def test_eval_callback_on_a_her_run_fused_against_the_loop(tmp_path):
    """A short HER SAC learn() with an EvalCallback: `fused=None` picks the launch, the training state does not depend on how the
    evaluation ran, evaluations.npz has the same layout and agrees at the loop-versus-launch bar; `fused=True` runs.
    8 episodes over 4 envs: every env runs two, so loop and launch leave the eval env in the same state for the next evaluation."""
    from core.common import evaluation, legacy_rng
    from core.common.callbacks import EvalCallback

    n, got, state = 4, {}, {}
    for fused in (None, False, True):
        model = _her_model("SAC", n=n, batch_size=16, learning_starts=8 * n, policy_kwargs=dict(net_arch=[16, 16]))
        ev = EvalCallback(_goal_env(4, 21), n_eval_episodes=8, eval_freq=10, log_path=str(tmp_path / str(fused)), verbose=0, warn=False, fused=fused)
        assert evaluation.supported(model, ev.eval_env)
        model.learn(n * 30, callback=ev)
        th.cuda.synchronize()
        env, rb = model.get_env().unwrapped, model.replay_buffer
        got[fused] = np.load(tmp_path / str(fused) / "evaluations.npz")
        state[fused] = dict(weights=np.concatenate([p.detach().cpu().numpy().ravel() for p in model.policy.parameters()]),
                            ring_obs=rb.ring.observations.cpu().numpy(), ring_act=rb.ring.actions.cpu().numpy(),
                            ring_rew=rb.ring.rewards.cpu().numpy(), ring_ctl=rb.ring.ctl.cpu().numpy(), goals=rb.her.desired_goal.cpu().numpy(),
                            ep_length=np.asarray(rb.ep_length), sampler=legacy_rng.global_stream(model.device).cpu().numpy().copy(),
                            env_obs=env.obs.cpu().numpy(), env_pcg=env.pcg_state.cpu().numpy(), env_targets=env.targets.cpu().numpy(),
                            env_episode=env.episode.cpu().numpy())
        assert model._n_updates > 0 and ev.n_calls == 30
    for k in state[None]:
        assert _bits(state[None][k]) == _bits(state[False][k]) == _bits(state[True][k]), k
    for fused in (None, False, True):
        assert sorted(got[fused].files) == ["ep_lengths", "results", "timesteps"]
        assert got[fused]["timesteps"].tolist() == [40, 80, 120] and got[fused]["ep_lengths"].tolist() == [[7] * 8] * 3
        assert got[fused]["results"].shape == (3, 8)
    print(f"HER SAC EvalCallback, launch against loop: largest relative difference = {np.abs(got[None]['results'] / got[False]['results'] - 1.0).max():.3e}")
    np.testing.assert_allclose(got[None]["results"], got[False]["results"], rtol=1e-4)
    assert _bits(got[None]["results"]) == _bits(got[True]["results"]) and evaluation.FUSED_BY_DEFAULT  # fused=None took the launch
