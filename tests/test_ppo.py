"""GPU checks of PPO on the HIP path.

Kernels (csrc/cstr_ppo.hip) against fp64 / NumPy restatements kept in this file, at rtol 2e-6 / atol 1e-7 (every figure is
printed in units of that bar before it is asserted): the rollout head, the rollout buffer's add, GAE (bit-exact against NumPy's
evaluation of the reference's loop), the minibatch gather, the loss launch (scalars and gradients against an fp64 autograd statement of core/ppo/ppo.py:213-256) and the
gradient clip. Then the classes: the teacher-forced rollout and train() against fixtures written by the unmodified reference
(tests/golden/ppo_*.npz, tools/refharness/gen_golden.py --only ppo) on the kernel path, with CSTR_FUSED_LINEAR=0 and on the
torch-statement path; target_kl, predict, save / load, logger keys, refusals, and a short learning run."""
import numpy as np
import pytest
import torch as th

from _parity_helpers import check_weights, q_err, rel_err
from test_ppo_abi import gae_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-6, 1e-7
LOG_SQRT_2PI = float(np.log(np.sqrt(2 * np.pi)))


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def close(got, want, rtol=RTOL, atol=ATOL, msg=""):
    np.testing.assert_allclose(got.detach().cpu().numpy().astype(np.float64), np.asarray(want, np.float64), rtol=rtol, atol=atol, err_msg=msg)


def bar(got, want, what):
    """max |got - want| / (2e-6 |want| + 1e-7), the project's bar = 1; printed, then asserted"""
    got = got.detach().cpu().numpy() if isinstance(got, th.Tensor) else got
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    units = np.abs(got - want) / (RTOL * np.abs(want) + ATOL)
    worst = int(np.argmax(units))
    print(f"BAR {what}: {units[worst]:.3f} (got {got[worst]:.9g}, want {want[worst]:.9g}, |d| {abs(got[worst] - want[worst]):.3g})")
    assert units[worst] <= 1.0, (what, units[worst], got[worst], want[worst])


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


# ---- GAE ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(1, 1), (8, 4), (5, 130)])
def test_gae_is_bit_identical_to_numpy(ops, T, N):
    rng = np.random.default_rng(100 * T + N)
    rewards = rng.uniform(-8, 0, (T, N)).astype(np.float32)
    values = rng.normal(-20, 10, (T, N)).astype(np.float32)
    starts = (rng.uniform(size=(T, N)) < 0.25).astype(np.float32)
    starts[0, :] = 1.0                      # an episode start at the first step ...
    starts[T - 1, ::2] = 1.0                # ... at the last step ...
    if T >= 3:
        starts[1:3, N // 2] = 1.0           # ... and on consecutive steps
    last_values = rng.normal(-20, 10, N).astype(np.float32)
    dones = (rng.uniform(size=N) < 0.5).astype(np.float32)
    adv, ret = gae_numpy(rewards, values, starts, last_values, dones, 0.99, 0.95)
    rb = ops.DeviceRollout(T, N, 4, 2, DEV)
    rb.rewards.copy_(dev(rewards)), rb.values.copy_(dev(values)), rb.episode_starts.copy_(dev(starts))
    ops.gae(rb, dev(last_values), dev(dones), 0.99, 0.95)
    np.testing.assert_array_equal(rb.advantages.cpu().numpy(), adv)
    np.testing.assert_array_equal(rb.returns.cpu().numpy(), ret)


# ---- rollout head --------------------------------------------------------------------------------------------------------------
def head_f64(mean, log_std, eps, low, high):
    mean, eps = mean.astype(np.float64), eps.astype(np.float64)
    sig = np.exp(log_std.astype(np.float64))
    act = mean + sig * eps
    logp = (-((act - mean) ** 2) / (2 * sig ** 2) - np.log(sig) - LOG_SQRT_2PI).sum(1)
    return act, np.clip(act, low, high), logp


@pytest.mark.parametrize("n,A", [(1, 2), (130, 2), (67, 4)])
def test_head_with_given_eps(ops, n, A):
    rng = np.random.default_rng(n + A)
    mean = rng.uniform(-1.2, 1.2, (n, A)).astype(np.float32)
    log_std = rng.uniform(-1.5, 0.3, A).astype(np.float32)
    eps = rng.normal(size=(n, A)).astype(np.float32)
    low, high = -np.ones(A, np.float32), np.ones(A, np.float32)
    action, env_action, logp = th.empty(n, A, device=DEV), th.empty(n, A, device=DEV), th.empty(n, device=DEV)
    ops.diag_gaussian_act(dev(mean), dev(log_std), dev(eps), None, dev(low), dev(high), False, action, env_action, logp)
    a64, c64, lp64 = head_f64(mean, log_std, eps, low, high)
    bar(action, a64, f"head action n={n} A={A}")
    bar(logp, lp64, f"head log_prob n={n} A={A}")
    # the clip is exact on the f32 action the kernel stored
    np.testing.assert_array_equal(env_action.cpu().numpy(), np.clip(action.cpu().numpy(), low, high))
    # deterministic: action = mean bit for bit, log-prob of the mode
    ops.diag_gaussian_act(dev(mean), dev(log_std), None, None, dev(low), dev(high), True, action, env_action, logp)
    np.testing.assert_array_equal(action.cpu().numpy(), mean)
    bar(logp, np.full(n, (-log_std.astype(np.float64) - LOG_SQRT_2PI).sum()), f"head log_prob of the mode n={n} A={A}")


def test_head_actions_on_and_beyond_the_bounds(ops):
    mean = np.array([[1.0, -1.0], [1.5, -2.0], [0.25, 0.5], [np.nextafter(np.float32(1), np.float32(2)), -1.0]], np.float32)
    zeros, one = np.zeros((4, 2), np.float32), np.ones(2, np.float32)
    action, env_action = th.empty(4, 2, device=DEV), th.empty(4, 2, device=DEV)
    ops.diag_gaussian_act(dev(mean), dev(np.zeros(2, np.float32)), dev(zeros), None, dev(-one), dev(one), False, action, env_action)
    np.testing.assert_array_equal(action.cpu().numpy(), mean)  # stored unclipped
    np.testing.assert_array_equal(env_action.cpu().numpy(), np.array([[1, -1], [1, -1], [0.25, 0.5], [1, -1]], np.float32))


def test_head_philox_draws(ops):
    n, A = 4096, 2
    mean, log_std = th.zeros(n, A, device=DEV), th.zeros(A, device=DEV)

    def draw(ctl):
        action, eps = th.empty(n, A, device=DEV), th.empty(n, A, device=DEV)
        ops.diag_gaussian_act(mean, log_std, None, ctl, None, None, False, action, eps_out=eps)
        return action.cpu().numpy(), eps.cpu().numpy()

    ctl = ops.new_rng_ctl(1234, DEV)
    a1, e1 = draw(ctl)
    a2, _ = draw(ctl)
    assert int(ctl[1]) == 2 * n and int(ctl[2]) == 0        # the offset advanced by the row count, the ticket reset itself
    np.testing.assert_array_equal(a1, e1)                   # mean 0, std 1: the action is the draw
    assert not np.array_equal(a1, a2)                       # two calls differ ...
    a3, _ = draw(ops.new_rng_ctl(1234, DEV))
    np.testing.assert_array_equal(a1, a3)                   # ... a reseed repeats
    assert abs(a1.mean()) < 0.05 and abs(a1.std() - 1) < 0.05 and abs(np.corrcoef(a1[:, 0], a1[:, 1])[0, 1]) < 0.06
    with pytest.raises(Exception, match="code -1"):
        ops.diag_gaussian_act(mean, log_std, None, None, None, None, False, th.empty(n, A, device=DEV))  # no noise source


# ---- rollout buffer add ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A", [(4, 2), (8, 4)])
def test_rollout_add_twice_with_identical_arguments(ops, D, A):
    T, N, gamma = 2, 70, 0.99
    rng = np.random.default_rng(D)
    rb = ops.DeviceRollout(T, N, D, A, DEV)
    for f in rb.FIELDS:
        getattr(rb, f).fill_(7.0)
    obs, act = dev(rng.normal(size=(N, D))), dev(rng.normal(size=(N, A)))
    rew, val, logp, tv = (dev(rng.normal(size=N)) for _ in range(4))
    start, done = dev(np.ones(N)), dev(rng.uniform(size=N) < 0.5)
    timeout = dev((rng.uniform(size=N) < 0.5) & (done.cpu().numpy() > 0))
    ep_ret, ep_len, stats = th.zeros(N, device=DEV), th.zeros(N, dtype=th.int32, device=DEV), th.zeros(4, dtype=th.float64, device=DEV)
    start0 = start.clone()
    for _ in range(2):  # the SAME host arguments: the position is a device control word
        ops.rollout_add(rb, obs, act, rew, start, val, logp, timeout, tv, gamma, done, ep_ret, ep_len, stats)
    boot = np.where(timeout.cpu().numpy() != 0, rew.cpu().numpy() + np.float32(gamma) * tv.cpu().numpy(), rew.cpu().numpy()).astype(np.float32)
    for t in range(2):
        assert th.equal(rb.observations[t], obs) and th.equal(rb.actions[t], act) and th.equal(rb.values[t], val) and th.equal(rb.log_probs[t], logp)
        np.testing.assert_array_equal(rb.rewards[t].cpu().numpy(), boot)  # the bootstrap only where timeout
        assert float(rb.advantages[t].abs().sum()) == 0 and float(rb.returns[t].abs().sum()) == 0
    assert th.equal(rb.episode_starts[0], start0) and th.equal(rb.episode_starts[1], done)  # episode_start <- done for the next step
    assert rb.ctl.tolist() == [2, 1, 0, 2]  # full at T
    got = stats.cpu().tolist()
    # lengths: an env that finishes every step has length 1 twice; return sums follow the raw reward (no bootstrap)
    r, d = rew.cpu().numpy().astype(np.float64), done.cpu().numpy() > 0
    assert got[0] == 2 * d.sum() and got[2] == 2 * d.sum() and abs(got[1] - 2 * r[d].sum()) < 1e-4
    np.testing.assert_allclose(ep_ret.cpu().numpy()[~d], (2 * rew.cpu().numpy())[~d], rtol=1e-6)
    assert ep_len.cpu().numpy()[~d].tolist() == [2] * int((~d).sum())
    # a third add finds the buffer full: nothing is written, nothing faults
    before = rb.rewards.clone()
    ops.rollout_add(rb, obs, act, rew, start, val, logp)
    assert th.equal(rb.rewards, before) and rb.ctl.tolist() == [2, 1, 0, 2]


# ---- gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 12, 100])
def test_gather_in_swap_and_flatten_order(ops, B):
    T, N, D, A = 5, 7, 4, 2
    rng = np.random.default_rng(B)
    rb = ops.DeviceRollout(T, N, D, A, DEV)
    host = {f: rng.normal(size=tuple(getattr(rb, f).shape)).astype(np.float32) for f in rb.FIELDS}
    for f in rb.FIELDS:
        getattr(rb, f).copy_(dev(host[f]))
    idx = rng.integers(0, T * N, B)          # B = 100 > T N: repeated indices
    if B >= 12:
        idx[:3] = idx[3]
    flat = {f: host[f].swapaxes(0, 1).reshape(T * N, -1) for f in rb.FIELDS}
    e = lambda *s: th.empty(*s, device=DEV)  # noqa: E731
    out = (e(B, D), e(B, A), e(B), e(B), e(B), e(B))
    ops.ppo_gather(rb, dev(idx, th.int64), *out)
    for t, f in zip(out, ("observations", "actions", "values", "log_probs", "advantages", "returns")):
        np.testing.assert_array_equal(t.cpu().numpy().reshape(B, -1), flat[f][idx])
    # out-of-range indices are the caller's bug: clamped, never a fault
    ops.ppo_gather(rb, dev(np.array([-5, T * N + 9] + [0] * (B - 2))[:B], th.int64), *out)
    np.testing.assert_array_equal(out[0][0].cpu().numpy(), flat["observations"][0])


# ---- loss --------------------------------------------------------------------------------------------------------------------
def ppo_loss_f64(mean, log_std, actions, values, old_values, old_logp, adv, returns, clip_range, clip_range_vf, normalize, ent_coef, vf_coef):
    """core/ppo/ppo.py:213-256 in fp64 autograd"""
    t = lambda a, g=False: th.tensor(np.asarray(a, np.float64), requires_grad=g)  # noqa: E731
    mean, log_std, values = t(mean, True), t(log_std, True), t(values, True)
    actions, old_values, old_logp, adv, returns = t(actions), t(old_values), t(old_logp), t(adv), t(returns)
    dist = th.distributions.Normal(mean, th.ones_like(mean) * log_std.exp())
    log_prob, entropy = dist.log_prob(actions).sum(1), dist.entropy().sum(1)
    if normalize and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = th.exp(log_prob - old_logp)
    policy_loss = -th.min(adv * ratio, adv * th.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    clip_fraction = th.mean((th.abs(ratio - 1) > clip_range).double())
    values_pred = values if clip_range_vf is None else old_values + th.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = th.nn.functional.mse_loss(returns, values_pred)
    entropy_loss = -th.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    log_ratio = log_prob - old_logp
    approx_kl = th.mean((th.exp(log_ratio) - 1) - log_ratio)
    loss.backward()
    scalars = [float(x) for x in (policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction)]
    return scalars, mean.grad.numpy(), values.grad.numpy(), log_std.grad.numpy(), log_prob.detach().numpy(), ratio.detach().numpy()


def loss_case(B, A, seed, constant_adv=False):
    rng = np.random.default_rng(seed)
    log_std = rng.uniform(-0.7, 0.2, A).astype(np.float32)
    mean = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    actions = (mean + np.exp(log_std) * rng.normal(size=(B, A))).astype(np.float32)
    sig = np.exp(log_std.astype(np.float64))
    logp = (-((actions - mean.astype(np.float64)) ** 2) / (2 * sig ** 2) - np.log(sig) - LOG_SQRT_2PI).sum(1)
    # old log-probs put the ratios on both sides of both clip bounds (0.8 / 1.2) and well inside; none within 1e-3 of a bound
    # (the levels are dealt out in turn and then shuffled, so that every level occurs from B = 6 on, whatever the seed)
    lr = rng.permutation(np.resize([-0.5, 0.4, -0.1, 0.1, 0.0, 0.05], B)) + rng.uniform(-0.02, 0.02, B)
    old_logp = (logp - lr).astype(np.float32)
    values = rng.normal(-20, 5, B).astype(np.float32)
    # value steps on both sides of clip_range_vf = 0.2
    old_values = (values - rng.permutation(np.resize([-1.0, 0.6, -0.1, 0.15, 0.05], B)) + rng.uniform(-0.01, 0.01, B)).astype(np.float32)
    adv = np.full(B, 1.5, np.float32) if constant_adv else rng.normal(0, 3, B).astype(np.float32)
    returns = (values + rng.normal(0, 2, B)).astype(np.float32)
    return mean, log_std, actions, values, old_values, old_logp, adv, returns


def run_loss(ops, case, clip_range, clip_range_vf, normalize, ent_coef=0.01, vf_coef=0.5, sums=None):
    mean, log_std, actions, values, old_values, old_logp, adv, returns = case
    B, A = actions.shape
    g_mean, g_value, g_ls = th.empty(B, A, device=DEV), th.empty(B, device=DEV), th.empty(A, device=DEV)
    scal, logp, ws = th.zeros(6, device=DEV), th.empty(B, device=DEV), ops.new_ppo_workspace(DEV)
    ops.ppo_loss(dev(mean), dev(log_std), dev(actions), dev(values), dev(old_values), dev(old_logp), dev(adv), dev(returns), clip_range,
                 clip_range_vf, normalize, ent_coef, vf_coef, g_mean, g_value, g_ls, ws, scalars_out=scal, scalars_sum=sums, log_prob_out=logp)
    assert int(ws[0]) == 0  # the ticket reset itself
    return scal, g_mean, g_value, g_ls, logp


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("clip_range_vf", [None, 0.2])
@pytest.mark.parametrize("B,A", [(1, 2), (2, 4), (12, 2), (100, 4), (1030, 2)])  # 1030 rows: five workgroups of partials
def test_loss_against_fp64_autograd(ops, B, A, clip_range_vf, normalize):
    case = loss_case(B, A, seed=17 * B + A)
    want, gm, gv, gl, lp, ratio = ppo_loss_f64(*case, 0.2, clip_range_vf, normalize, 0.01, 0.5)
    assert np.min(np.abs(np.abs(ratio - 1) - 0.2)) > 1e-3  # no row sits on a clip bound: clip_fraction compares exactly
    if B >= 12:
        assert 0 < want[5] < 1 and (ratio < 0.8).any() and (ratio > 1.2).any()
    scal, g_mean, g_value, g_ls, logp = run_loss(ops, case, 0.2, clip_range_vf, normalize)
    tag = f"loss B={B} A={A} vf={clip_range_vf} norm={normalize}"
    bar(logp, lp, tag + " log_prob")
    got = scal.cpu().numpy().astype(np.float64)
    for k, name in enumerate(("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl")):
        bar(got[k], want[k], f"{tag} {name}")
    assert got[5] == np.float32(want[5])
    bar(g_mean, gm, tag + " d/d mean"), bar(g_value, gv, tag + " d/d value"), bar(g_ls, gl, tag + " d/d log_std")


def test_loss_constant_advantages_and_accumulating_sums(ops):
    case = loss_case(12, 2, seed=5, constant_adv=True)  # std = 0: the normalised advantages are 0 / 1e-8 = 0
    want, gm, gv, gl, _, _ = ppo_loss_f64(*case, 0.2, None, True, 0.01, 0.5)
    sums = th.zeros(6, device=DEV)
    scal, g_mean, g_value, g_ls, _ = run_loss(ops, case, 0.2, None, True, sums=sums)
    assert float(scal[0]) == 0.0 and float(g_mean.abs().max()) == 0.0 and np.abs(gm).max() == 0.0
    bar(g_value, gv, "constant advantages d/d value"), bar(g_ls, gl, "constant advantages d/d log_std")
    first = scal.clone()
    scal2, *_ = run_loss(ops, case, 0.2, None, True, sums=sums)
    assert th.equal(scal2, first)  # deterministic
    close(sums, 2 * first.cpu().numpy().astype(np.float64), rtol=1e-6)


# ---- gradient clip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 9000])
def test_grad_clip(ops, n):
    rng = np.random.default_rng(n)
    g = rng.normal(size=n).astype(np.float32)
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    ws, out = ops.new_ppo_workspace(DEV), th.zeros(1, device=DEV)
    for max_norm in (2 * norm, float(np.float32(norm)), 0.5):  # below, equal, above
        grad = dev(g)
        ops.grad_clip(grad, max_norm, ws, out)
        coef = min(1.0, max_norm / (norm + 1e-6))
        close(out, [norm], rtol=2e-6)
        close(grad, g.astype(np.float64) * coef, rtol=2e-6, atol=1e-7)
    zero = th.zeros(n, device=DEV)
    ops.grad_clip(zero, 0.5, ws, out)
    assert float(zero.abs().max()) == 0.0 and float(out) == 0.0 and bool(th.isfinite(zero).all())


# ---- the classes against the reference's fixtures ------------------------------------------------------------------------------------
ROLLOUT_FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def make_model(g, prefix="before", **kw):
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the truncated-minibatch warning (checked in test_ppo_abi.py)
        model = PPO("MlpPolicy", CSTRVecEnv(int(g["n_envs"]), device=DEV), seed=int(g["seed"]), n_steps=int(g["n_steps"]),
                    batch_size=int(g["batch_size"]), n_epochs=int(g["n_epochs"]), learning_rate=float(g["learning_rate"]),
                    ent_coef=float(g["ent_coef"]), policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]]), device=DEV, **kw)
    with th.no_grad():
        for k, v in model.policy.state_dict().items():
            v.copy_(th.as_tensor(g[f"{prefix}/policy/{k}"]))
    return model


def scale_err(got, want):
    """max |d| relative to the tensor's scale (its largest magnitude)"""
    want = np.asarray(want, np.float64)
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, th.Tensor) else np.asarray(got, np.float64)
    return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


def test_rollout_teacher_forced(golden):
    """collect_rollouts on the device against the reference's rollout: the `before/` weights, the initial observations and step
    counters injected after _setup_learn's reset, the recorded Normal draws forced. Truncations happen inside the 8 steps."""
    g = golden("ppo_train_kat_small.npz")
    model = make_model(g)
    assert model.fused_learner and model._device_rollout()
    _, cb = model._setup_learn(int(g["n_envs"] * g["n_steps"]), None)
    model.env.set_state(g["init_obs"], g["init_steps"])
    model._fast.eps_queue = [th.as_tensor(e) for e in g["eps"]]
    assert model.collect_rollouts(model.env, cb, model.rollout_buffer, int(g["n_steps"]))
    rb = model.rollout_buffer
    assert rb.full and rb.rb.ctl.tolist() == [int(g["n_steps"]), 1, 0, int(g["n_steps"])] and not model._fast.eps_queue
    np.testing.assert_array_equal(rb.episode_starts.cpu().numpy(), g["rollout/episode_starts"])
    assert g["rollout/episode_starts"][1:].sum() >= 2 and g["timeouts"].sum() >= 2  # the truncations are in the fixture
    for f in ("observations", "actions", "values", "log_probs", "rewards"):
        assert scale_err(getattr(rb, f), g[f"rollout/{f}"]) < 1e-5, f
    # the bootstrap went into the rewards of the truncated steps only: those rewards differ from the env's own by gamma * V(terminal)
    np.testing.assert_array_equal(model._denv._done.cpu().numpy(), g["dones"])
    for f in ("advantages", "returns"):  # the device GAE on the device rollout
        assert scale_err(getattr(rb, f), g[f"rollout/{f}"]) < 1e-5, f
    assert scale_err(model._last_obs, g["last_obs"]) < 1e-5
    n_ep, ret_sum, len_sum, _ = model._ep_stats.cpu().tolist()
    assert n_ep == g["rollout/episode_starts"][1:].sum() + g["dones"].sum() and len_sum > 0 and ret_sum < 0


def run_train(g, path, monkeypatch, prefix="", **kw):
    from core.common import fused
    from core.common.buffers import RolloutBuffer

    if path == "rocblas":  # the kernel path with every GEMM left to PyTorch-ROCm / rocBLAS (CSTR_FUSED_LINEAR=0)
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    model = make_model(g, **kw)
    if path == "torch":
        model.fused_learner = False
    assert model.fused_learner == (path != "torch")
    model.rollout_buffer = RolloutBuffer.from_arrays(model.observation_space, model.action_space, DEV, gamma=model.gamma,
                                                     gae_lambda=model.gae_lambda, **{f: g[f"rollout/{f}"] for f in ROLLOUT_FIELDS})
    model.rollout_buffer.forced_permutations = [p for p in g[f"{prefix}permutations"]]
    model.debug_capture = True
    model.train()
    return model


def check_train(model, g, path, prefix=""):
    label = {"fused": "ppo_fused", "rocblas": "ppo_rocblas", "torch": "ppo_aten"}[path]
    n_mb = int(g[f"{prefix}n_minibatches"])
    assert len(model.last_train_minibatches) == n_mb
    for k, cap in enumerate(model.last_train_minibatches):
        want_v, want_lp, want_s = g[f"{prefix}mb{k}/values"], g[f"{prefix}mb{k}/log_prob"], g[f"{prefix}mb{k}/scalars"].astype(np.float64)
        assert cap["values"].shape[0] == want_v.shape[0]  # the last minibatch of an epoch is the short one
        # values: |dv_i| <= 1e-5 * max(|v_i|, mean|v|), the bar q_err returns. q_err's own per-element assertion (5e-5 of
        # max(|v_i|, 1e-3)) is made for Q values of size 10 ... 300 and is not applied here: a freshly initialised value net gives
        # |v| ~ 0.1 from 64 products whose magnitudes sum to ~1.3, so two correct f32 evaluations differ by several 1e-8, and the
        # fixture's own values (CPU f32) are 3.6e-8 = 3.4e-5 of that floor away from an fp64 forward of the same weights
        assert rel_err(cap["values"].cpu().numpy(), want_v, float(np.abs(want_v).mean())) < 1e-5, (k, "values")
        assert q_err(cap["log_prob"].cpu().numpy(), want_lp, label) < 1e-5, (k, "log_prob")
        got = cap["scalars"].cpu().numpy().astype(np.float64)
        # losses: within 1e-5 of the batch's scale = the size of the terms they average (normalised advantages ~1, squared value
        # errors and entropy as recorded); approx_kl averages (ratio - 1) - log_ratio, whose terms carry the rounding of ratio ~ 1 on
        # either side: 2 ulp(1) = 2.4e-7 absolute on top of the relative part
        floors = (1.0, max(want_s[1], 1.0), max(abs(want_s[2]), 1.0), max(abs(want_s[3]), 1.0))
        for i, fl in enumerate(floors):
            assert abs(got[i] - want_s[i]) <= 1e-5 * max(abs(want_s[i]), fl), (k, i, got[i], want_s[i])
        assert abs(got[4] - want_s[4]) <= 1e-5 * abs(want_s[4]) + 2.4e-7, (k, got[4], want_s[4])
        assert got[5] == want_s[5], (k, "clip_fraction")
        # the gradient norm gathers ~2.4e3 entries whose relative error is ~1e-5 (exp's amplification of the log-prob rounding)
        assert rel_err(cap["grad_norm"].cpu().numpy(), g[f"{prefix}mb{k}/grad_norm"]) < 5e-5, (k, "grad_norm")
    assert model._n_updates == int(g[f"{prefix}n_updates"]) and model.policy.optimizer.step_count == int(g[f"{prefix}optimizer_steps"])
    gg = g if not prefix else {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    check_weights(model, gg, "after", ["policy"])
    logged = model.logger.resolved()
    want = dict(zip([str(k) for k in g[f"{prefix}logged_keys"]], g[f"{prefix}logged_values"]))
    for key in ("train/entropy_loss", "train/policy_gradient_loss", "train/value_loss", "train/clip_fraction", "train/loss",
                "train/explained_variance", "train/std", "train/n_updates", "train/clip_range", "train/learning_rate"):
        assert abs(float(logged[key]) - want[key]) <= 1e-5 * max(abs(want[key]), 1.0), (key, logged[key], want[key])
    assert abs(float(logged["train/approx_kl"]) - want["train/approx_kl"]) <= 1e-5 * abs(want["train/approx_kl"]) + 2.4e-7
    assert set(want) <= set(logged), set(want) - set(logged)


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("name", ["small", "default"])
def test_train_teacher_forced(golden, name, path, monkeypatch):
    g = golden(f"ppo_train_kat_{name}.npz")
    model = run_train(g, path, monkeypatch)
    assert any(float(g[f"mb{k}/scalars"][5]) > 0 for k in range(int(g["n_minibatches"]))) or name == "default"
    check_train(model, g, path)
    if name == "small":
        sizes = [c["values"].shape[0] for c in model.last_train_minibatches]
        assert sizes == [12, 12, 8] * 3  # batch_size 12 over 32 rows: the truncated minibatch


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("normalize", [True, False])
def test_train_teacher_forced_value_clip(golden, normalize, path, monkeypatch):
    g = golden("ppo_train_kat_vfclip.npz")
    prefix = "" if normalize else "raw/"
    model = run_train(g, path, monkeypatch, prefix=prefix, clip_range_vf=float(g["clip_range_vf"]), normalize_advantage=normalize)
    check_train(model, g, path, prefix=prefix)
    assert "train/clip_range_vf" in model.logger.resolved()


@pytest.mark.parametrize("path", ["fused", "torch"])
def test_target_kl_stops_where_the_reference_stopped(golden, path, monkeypatch):
    g = golden("ppo_train_kat_small.npz")
    model = run_train(g, path, monkeypatch, target_kl=float(g["tkl/target_kl"]))
    stop = int(g["tkl/stop_minibatch"])
    assert len(model.last_train_minibatches) == stop + 1  # the minibatch that tripped the threshold is evaluated, not applied
    assert model.policy.optimizer.step_count == int(g["tkl/optimizer_steps"]) == stop and model._n_updates == int(g["tkl/n_updates"])
    check_weights(model, {k[4:]: g[k] for k in g.files if k.startswith("tkl/after/")}, "after", ["policy"])


def test_learn_draws_the_reference_s_permutations(golden, ops, monkeypatch):
    """The un-forced path: learn() of PPO(seed=7) on 4 envs draws RandomState(10)'s permutations (= the fixture's), a second learn()
    runs the same stream on (its reset is unseeded), and another model's seeded reset on the same device in between changes nothing."""
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    g = golden("ppo_train_kat_small.npz")
    assert (int(g["seed"]), int(g["n_envs"]), int(g["n_steps"]), int(g["n_epochs"])) == (7, 4, 8, 3)
    model = make_model(g)
    seen, gather = [], ops.ppo_gather
    monkeypatch.setattr(ops, "ppo_gather", lambda rb, idx, *out: (seen.append(idx.cpu().numpy()), gather(rb, idx, *out))[1])
    model.learn(32)
    want = np.random.RandomState(10)
    assert [len(p) for p in seen] == [12, 12, 8] * 3
    for e in range(3):
        perm = np.concatenate(seen[3 * e:3 * e + 3])
        np.testing.assert_array_equal(perm, want.permutation(32))
        np.testing.assert_array_equal(perm, g["permutations"][e])
    other = PPO("MlpPolicy", CSTRVecEnv(4, device=DEV), n_steps=8, batch_size=32, n_epochs=1, seed=99, device=DEV)
    other._setup_learn(32, None)  # a seeded reset of ANOTHER model's envs
    del seen[:]
    model.learn(32)
    for e in range(3):
        np.testing.assert_array_equal(np.concatenate(seen[3 * e:3 * e + 3]), want.permutation(32))


def test_predict_matches_the_reference(golden):
    g = golden("ppo_predict_kat.npz")
    small = golden("ppo_train_kat_small.npz")
    model = make_model({**{k: small[k] for k in small.files}, **{f"before/policy/{k[7:]}": g[k] for k in g.files if k.startswith("policy/")}})
    act, state = model.predict(g["obs"], deterministic=True)
    assert state is None and act.shape == (16, 2) and act.dtype == np.float32
    assert scale_err(act, g["deterministic"]) < 1e-5
    model._fast.eps_queue.append(th.as_tensor(g["eps"]))
    act, _ = model.predict(g["obs"], deterministic=False)
    assert scale_err(act, g["sampled"]) < 1e-5 and np.abs(act).max() <= 1.0
    one, _ = model.predict(g["obs"][3], deterministic=True)
    assert one.shape == (2,) and scale_err(one, g["deterministic"][3]) < 1e-5
    with th.no_grad():
        values = model.policy.predict_values(dev(g["obs"]))
    assert values.shape == (16, 1) and q_err(values.cpu().numpy(), g["values"], "ppo_fused") < 1e-5
    a1, _ = model.predict(g["obs"], deterministic=False)  # unforced: the Philox stream
    a2, _ = model.predict(g["obs"], deterministic=False)
    assert not np.array_equal(a1, a2)


def test_save_load_round_trip_and_reference_key_layout(golden, tmp_path):
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    g = golden("ppo_train_kat_small.npz")
    model = make_model(g, prefix="after", clip_range_vf=0.3, target_kl=0.05)
    model.learn(2 * int(g["n_envs"] * g["n_steps"]))
    path = str(tmp_path / "ppo_model.zip")
    model.save(path)
    import zipfile

    assert {"data", "policy.pth", "policy.optimizer.pth"} <= set(zipfile.ZipFile(path).namelist())  # the SB3 layout
    loaded = PPO.load(path, env=CSTRVecEnv(int(g["n_envs"]), device=DEV), device=DEV)
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count > 0
    assert th.equal(loaded.policy.optimizer.exp_avg, model.policy.optimizer.exp_avg)
    assert (loaded.n_steps, loaded.batch_size, loaded.n_epochs, loaded.target_kl, loaded.clip_range_vf(1.0)) == (8, 12, 3, 0.05, 0.3)
    assert loaded.num_timesteps == model.num_timesteps and loaded._n_updates == model._n_updates
    obs = np.random.default_rng(0).uniform(-1, 1, (5, 4)).astype(np.float32)
    np.testing.assert_array_equal(model.predict(obs, deterministic=True)[0], loaded.predict(obs, deterministic=True)[0])
    # weights in the reference's key layout (a state dict as the reference's policy.pth holds it)
    ref_sd = {k: th.as_tensor(g[f"before/policy/{k}"]) for k in [str(x) for x in g["state_dict_keys"]]}
    loaded.set_parameters({"policy": ref_sd}, exact_match=False)
    for k, v in loaded.policy.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g[f"before/policy/{k}"])
    with pytest.raises(ValueError, match="do not match"):
        loaded.set_parameters({"policy": {"log_std": ref_sd["log_std"]}, "policy.optimizer": loaded.policy.optimizer.state_dict()})


def test_logger_keys_callbacks_and_refusals(golden):
    from core.common.callbacks import BaseCallback
    from core.common.vec_env import CSTRVecEnv, VecNormalize
    from core.ppo import PPO

    class Count(BaseCallback):
        starts = ends = 0

        def _on_rollout_start(self):
            self.starts += 1

        def _on_rollout_end(self):
            self.ends += 1

        def _on_step(self):
            return self.n_calls < 20

    env = CSTRVecEnv(8, device=DEV)
    model = PPO("MlpPolicy", env, n_steps=8, batch_size=32, n_epochs=2, seed=3, device=DEV)
    cb = Count()
    model.learn(8 * 8 * 3, callback=cb)
    assert cb.starts == 3 and cb.ends == 2 and cb.n_calls == 20 and model.num_timesteps == 160  # the callback stopped the third rollout
    assert model._n_updates == 4
    model.learn(8 * 8 * 2)
    keys = set(model.logger.last_dump) | set(model.logger.resolved())
    for key in ("train/entropy_loss", "train/policy_gradient_loss", "train/value_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
                "train/explained_variance", "train/std", "train/n_updates", "train/clip_range", "train/learning_rate", "time/iterations",
                "time/fps", "time/time_elapsed", "time/total_timesteps"):
        assert key in keys, key
    assert "train/clip_range_vf" not in keys
    with pytest.raises(NotImplementedError, match="hipGraph"):
        model.enable_graph_capture(True)
    model.enable_graph_capture(False)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        PPO("MlpPolicy", VecNormalize(CSTRVecEnv(4, device=DEV)), device=DEV)
    with pytest.raises(ValueError, match="does not support gSDE"):
        PPO("MlpPolicy", env, use_sde=True, device=DEV)
    from core.common import distributed as dist_util

    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            PPO("MlpPolicy", env, device=DEV)
    finally:
        dist_util.rank_world = orig
    # another optimiser class: the torch-statement path, chosen from what the code can observe
    other = PPO("MlpPolicy", CSTRVecEnv(4, device=DEV), n_steps=8, batch_size=16, n_epochs=1, seed=1, device=DEV,
                policy_kwargs=dict(optimizer_class=th.optim.SGD, optimizer_kwargs={}))
    assert not other.fused_learner and isinstance(other.policy.optimizer, th.optim.SGD)
    with pytest.raises(ValueError, match="no kernel path"):
        other.fused_learner = True
    other.learn(32)
    assert other._n_updates == 1 and all(bool(th.isfinite(p).all()) for p in other.policy.parameters())


def test_episode_statistics_reach_the_logger():
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    env = CSTRVecEnv(16, device=DEV)
    model = PPO("MlpPolicy", env, n_steps=16, batch_size=64, n_epochs=1, seed=5, device=DEV)
    _, cb = model._setup_learn(10 ** 6, None)
    env.step_count.fill_(390)  # every env is truncated inside the first rollout
    model.collect_rollouts(env, cb, model.rollout_buffer, 16)
    model._dump_logs(1)
    d = model.logger.last_dump
    # the time limit ends every episode after 10 steps at the latest (an env may end one earlier by itself)
    assert 0 < d["rollout/ep_len_mean"] <= 10.0 and d["rollout/ep_rew_mean"] < 0 and model._episode_num >= 16


def test_it_learns():
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    def score(model):
        env = CSTRVecEnv(8, device=DEV)
        env.seed(1000)
        return evaluate_policy(model, env, n_eval_episodes=8, deterministic=True)[0]

    model = PPO("MlpPolicy", CSTRVecEnv(32, device=DEV), n_steps=64, batch_size=512, n_epochs=4, seed=0, device=DEV)
    before = score(model)
    model.learn(32 * 64 * 20)
    after = score(model)
    print(f"PPO evaluate_policy before {before:.1f}, after {after:.1f}")
    assert np.isfinite(after) and after > before
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters()) and model._n_updates == 80
