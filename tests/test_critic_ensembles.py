"""Critic ensembles (policy_kwargs n_critics = N) in SAC and TD3 on the HIP learner.

The reference's ContinuousCritic builds N Q networks (core/common/policies.py:934-965) and train() uses all of them: the TD target
takes the min over the N target critics (core/sac/sac.py:249-250, core/td3/td3.py:174-175), the critic loss sums N MSE terms
(sac.py:261 with 0.5, td3.py:182), SAC's actor loss takes the min over the N critics (sac.py:273-275). Golden vectors
tests/golden/{sac,td3}_train_kat_ncrit*.npz were written by the unmodified reference (tools/refharness/gen_golden.py,
gen_sac_ncrit / gen_td3_ncrit); the N-critic loss heads (cstr_td_ens_q_loss_f32, cstr_sac_actor_ens_loss_f32) are checked against
an fp64 NumPy statement and, at N = 2, bit for bit against the twin kernels."""
import hashlib
import os
import tempfile

import numpy as np
import pytest
import torch as th

from _parity_helpers import check_init, check_weights, load_ring, q_err, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _make_env(n=4):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n)


def _count_calls(monkeypatch, owner, name):
    """Counts the calls of owner.name (a code base without it keeps the count at 0: the arithmetic checks fail first)."""
    calls = []
    orig = getattr(owner, name, None)

    def wrapped(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    monkeypatch.setattr(owner, name, wrapped, raising=False)
    return calls


def _select_path(monkeypatch, path):
    """path "fused": hand-written MFMA Linear kernels + HIP glue; "rocblas": the same glue with every GEMM in rocBLAS; "aten": stock
    ATen evaluation of the same statements. Returns the ensemble-kernel call counters."""
    from core.common import chain, fused, hip_ops

    monkeypatch.setattr(chain, "USE_CHAIN", True)  # the chain must decline N != 2 by itself
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    chain_calls = _count_calls(monkeypatch, chain.SacChain, "step") + _count_calls(monkeypatch, chain.Td3Chain, "step")
    return chain_calls, _count_calls(monkeypatch, hip_ops, "td_ens_q_loss")


# ------------------------------------------------------------------------------------ teacher-forced parity
@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("tag,n_critics", [("ncrit3", 3), ("ncrit3_default", 3), ("ncrit1", 1)])
def test_sac_ensemble_teacher_forced(golden, tag, n_critics, path, monkeypatch):
    from core.common import legacy_rng
    from core.sac import SAC

    chain_calls, ens_calls = _select_path(monkeypatch, path)
    g = golden(f"sac_train_kat_{tag}.npz")
    gamma, tau, target_entropy, lr, B, n_steps = g["hyper"]
    B, n_steps = int(B), int(n_steps)
    pk = dict(n_critics=n_critics) if tag.endswith("default") else dict(net_arch=[64, 64], n_critics=n_critics)
    model = SAC("MlpPolicy", _make_env(4), seed=0, batch_size=B, buffer_size=64 * 4, policy_kwargs=pk)
    assert len(model.critic.q_networks) == n_critics and model.fused_learner
    model.fused_learner = path != "aten"
    assert model.gamma == gamma and model.tau == tau and model.target_entropy == target_entropy and model.lr_schedule(1) == lr
    mods = ["actor", "critic", "critic_target"]
    check_init(model, g, mods)
    assert float(model.log_ent_coef.detach()) == float(g["before/log_ent_coef"][0])
    load_ring(model, g)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    model.debug_capture = True
    lab = f"sac_{tag}_{path}"
    for k in range(n_steps):
        model.actor.action_dist.eps_queue = [th.as_tensor(g[f"step{k}/eps_pi"]), th.as_tensor(g[f"step{k}/eps_next"])]
        model.train(gradient_steps=1, batch_size=B)
        assert not model.actor.action_dist.eps_queue
        b = model._static_batch
        for name in ("observations", "actions", "next_observations", "dones", "rewards"):
            np.testing.assert_array_equal(getattr(b, name).cpu().numpy(), g[f"step{k}/batch_{name}"], err_msg=f"step {k} batch {name}")
        t = model.last_train_tensors
        assert len(t["current_q"]) == n_critics
        assert q_err(t["target_q"].cpu().numpy(), g[f"step{k}/target_q"], lab) < 1e-5, f"target_q step {k}"
        for i in range(n_critics):
            assert q_err(t["current_q"][i].cpu().numpy(), g[f"step{k}/current_q{i + 1}"], lab) < 1e-5, f"q{i + 1} step {k}"
        lv = model.logger.name_to_value
        for key in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef"):
            assert rel_err(float(lv[f"train/{key}"]), float(g[f"step{k}/{key}"]), 1e-3) < 1e-5, f"{key} step {k}"
    assert model._n_updates == n_steps and not chain_calls
    assert len(ens_calls) == (0 if path == "aten" else n_steps)
    check_weights(model, g, "after", mods)
    assert abs(float(model.log_ent_coef.detach()) - float(g["after/log_ent_coef"][0])) < 1e-6
    assert model.actor.optimizer.step_count == n_steps and model.critic.optimizer.step_count == n_steps


@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
def test_td3_ensemble_teacher_forced(golden, path, monkeypatch):
    """Three critics, four steps (two delayed policy updates): the target is the min over ALL three target critics and every
    critic learns from its own MSE term (scale 1); the actor's loss stays -mean(Q1) (td3.py:194)."""
    from core.common import legacy_rng
    from core.td3 import TD3

    chain_calls, ens_calls = _select_path(monkeypatch, path)
    g = golden("td3_train_kat_ncrit3.npz")
    gamma, tau, tpn, tnc, delay, lr, B, n_steps = g["hyper"]
    B, n_steps = int(B), int(n_steps)
    model = TD3("MlpPolicy", _make_env(4), seed=0, batch_size=B, buffer_size=64 * 4, policy_kwargs=dict(net_arch=[48, 32], n_critics=3))
    assert len(model.critic.q_networks) == 3 and model.fused_learner
    model.fused_learner = path != "aten"
    assert (model.gamma, model.tau, model.target_policy_noise, model.target_noise_clip, model.policy_delay) == (gamma, tau, tpn, tnc, int(delay))
    assert model.lr_schedule(1) == lr
    mods = ["actor", "actor_target", "critic", "critic_target"]
    check_init(model, g, mods)
    load_ring(model, g)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    model.debug_capture = True
    lab = f"td3_ncrit3_{path}"
    for k in range(n_steps):
        model.noise_queue = [th.as_tensor(g[f"step{k}/noise_raw"])]
        model.train(gradient_steps=1, batch_size=B)
        b = model._static_batch
        for name in ("observations", "actions", "next_observations", "dones", "rewards"):
            np.testing.assert_array_equal(getattr(b, name).cpu().numpy(), g[f"step{k}/batch_{name}"])
        t = model.last_train_tensors
        assert len(t["current_q"]) == 3
        assert q_err(t["target_q"].cpu().numpy(), g[f"step{k}/target_q"], lab) < 1e-5, f"target_q step {k}"
        for i in range(3):
            assert q_err(t["current_q"][i].cpu().numpy(), g[f"step{k}/current_q{i + 1}"], lab) < 1e-5, f"q{i + 1} step {k}"
        lv = model.logger.name_to_value
        assert rel_err(float(lv["train/critic_loss"]), float(g[f"step{k}/critic_loss"]), 1e-3) < 1e-5
        if f"step{k}/actor_loss" in g:
            assert rel_err(float(lv["train/actor_loss"]), float(g[f"step{k}/actor_loss"]), 1e-3) < 1e-5
            assert t["actor_loss"] is not None
        else:
            assert t["actor_loss"] is None
    check_weights(model, g, "after", mods)
    assert model.critic.optimizer.step_count == n_steps and model.actor.optimizer.step_count == n_steps // int(delay)
    assert not chain_calls and len(ens_calls) == (0 if path == "aten" else n_steps)


# ------------------------------------------------------------------------------------ the loss heads against fp64 NumPy
def _f32(rng, *shape, lo=-3.0, hi=3.0):
    return rng.uniform(lo, hi, shape).astype(np.float32)


def _dev(a):
    return th.as_tensor(np.ascontiguousarray(a), device=DEV)


def _inject_ties(rng, q):
    """Exact ties in the column minimum: some columns all-equal (the first critic wins), some with two critics j < k tied below the
    others (critic j wins)."""
    n, b = q.shape
    q = q.copy()
    if n == 1:
        return q
    cols = rng.permutation(b)
    q[:, cols[: b // 8]] = q[0, cols[: b // 8]]
    for c in cols[b // 8: b // 4]:
        j, k = sorted(rng.choice(n, 2, replace=False))
        q[j, c] = q[k, c] = q[:, c].min() - np.float32(0.5)
    return q


def _td_np(qt, nlp, rew, done, ec, gamma, q, scale):
    qt, q = qt.astype(np.float64), q.astype(np.float64)
    nxt = qt.min(axis=0)
    if nlp is not None:
        nxt = nxt - ec * nlp.astype(np.float64)
    t = rew.astype(np.float64) + (1.0 - done.astype(np.float64)) * gamma * nxt
    d = q - t
    return t, scale * 2.0 / q.shape[1] * d, scale * sum(float(np.mean(di * di)) for di in d)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 10, 16])
@pytest.mark.parametrize("b", [64, 256, 1000])
@pytest.mark.parametrize("form", ["sac_alpha", "sac_fixed", "td3"])
def test_td_ens_q_loss_against_numpy(n, b, form):
    from core.common import hip_ops as ops

    rng = np.random.default_rng(1000 * n + b)
    qt, q = _inject_ties(rng, _f32(rng, n, b)), _f32(rng, n, b)
    rew, done = _f32(rng, b, lo=-8, hi=0), (rng.uniform(size=b) < 0.2).astype(np.float32)
    nlp, logp_pi = _f32(rng, b, lo=-4, hi=2), _f32(rng, b, lo=-4, hi=2)
    la, fixed_ec, gamma = np.float32(-0.3), np.float32(0.2), 0.99
    scale = 1.0 if form == "td3" else 0.5
    # q_t with a row stride (a slice of a wider buffer), q as the stacked [N, B, 1] output
    qt_buf = _dev(np.concatenate([qt, np.zeros((n, 7), np.float32)], axis=1))
    q_d = _dev(q.reshape(n, b, 1))
    target, gq = th.full((b,), np.nan, device=DEV), th.full((n, b, 1), np.nan, device=DEV)
    loss_out, loss_sum = th.zeros(1, device=DEV), th.full((1,), 2.0, device=DEV)
    alpha = None
    if form == "sac_alpha":
        alpha = dict(log_alpha=_dev(np.array([la])), logp_pi=_dev(logp_pi), target_entropy=-2.0, grad_out=th.zeros(1, device=DEV),
                     ent_coef_out=th.zeros(1, device=DEV), loss_out=th.zeros(1, device=DEV), loss_sum=th.ones(1, device=DEV),
                     ent_coef_sum=th.ones(1, device=DEV))
    ec_dev = _dev(np.array([fixed_ec])) if form == "sac_fixed" else None
    ops.td_ens_q_loss(qt_buf[:, :b], None if form == "td3" else _dev(nlp), _dev(rew), _dev(done), ec_dev, gamma, q_d, scale, target, gq,
                      loss_out, loss_sum, alpha=alpha)
    ec = float(np.exp(np.float32(la))) if form == "sac_alpha" else float(fixed_ec)
    t, g, loss = _td_np(qt, None if form == "td3" else nlp, rew, done, ec, gamma, q, scale)
    th.cuda.synchronize()
    tol = 1e-5 * float(np.abs(t).max())
    np.testing.assert_allclose(target.cpu().numpy(), t, rtol=1e-5, atol=tol)
    np.testing.assert_allclose(gq.cpu().numpy().reshape(n, b), g, rtol=1e-5, atol=scale * 2.0 / b * tol)
    assert rel_err(float(loss_out), loss) < 1e-5 and rel_err(float(loss_sum) - 2.0, loss, 1e-3) < 1e-5
    if alpha is not None:
        mean = float(np.mean(logp_pi.astype(np.float64) - 2.0))
        assert rel_err(float(alpha["grad_out"]), -mean, 1e-6) < 1e-5
        assert rel_err(float(alpha["ent_coef_out"]), np.exp(np.float64(la))) < 1e-6
        assert rel_err(float(alpha["loss_out"]), -float(la) * mean, 1e-6) < 1e-5
        assert rel_err(float(alpha["loss_sum"]) - 1.0, -float(la) * mean, 1e-3) < 1e-5
        assert rel_err(float(alpha["ent_coef_sum"]) - 1.0, np.exp(np.float64(la))) < 1e-5
    if n == 2:  # bit-identical to the twin kernel on the same inputs
        t2, g1, g2 = th.empty(b, device=DEV), th.empty(b, device=DEV), th.empty(b, device=DEV)
        lo2, ls2 = th.zeros(1, device=DEV), th.full((1,), 2.0, device=DEV)
        alpha2 = None
        if alpha is not None:
            alpha2 = dict(alpha, grad_out=th.zeros(1, device=DEV), ent_coef_out=th.zeros(1, device=DEV), loss_out=th.zeros(1, device=DEV),
                          loss_sum=th.ones(1, device=DEV), ent_coef_sum=th.ones(1, device=DEV))
        qt_c = qt_buf[:, :b].contiguous()
        ops.td_twin_q_loss(qt_c[0], qt_c[1], None if form == "td3" else _dev(nlp), _dev(rew), _dev(done), ec_dev, gamma,
                           q_d[0].reshape(b).contiguous(), q_d[1].reshape(b).contiguous(), scale, t2, g1, g2, lo2, ls2, alpha=alpha2)
        assert th.equal(t2, target) and th.equal(g1, gq[0, :, 0]) and th.equal(g2, gq[1, :, 0])
        assert th.equal(lo2, loss_out) and th.equal(ls2, loss_sum)
        if alpha is not None:
            for key in ("grad_out", "ent_coef_out", "loss_out", "loss_sum", "ent_coef_sum"):
                assert th.equal(alpha2[key], alpha[key]), key


@pytest.mark.parametrize("n", [1, 2, 3, 5, 10, 16])
@pytest.mark.parametrize("b", [64, 256, 1000])
def test_sac_actor_ens_loss_against_numpy(n, b):
    from core.common import hip_ops as ops

    rng = np.random.default_rng(77 * n + b)
    q, logp = _inject_ties(rng, _f32(rng, n, b)), _f32(rng, b, lo=-4, hi=2)
    ec = np.float32(0.37)
    q_d = _dev(q.reshape(n, b, 1))
    g_logp, gq = th.full((b,), np.nan, device=DEV), th.full((n, b, 1), np.nan, device=DEV)
    loss_out, loss_sum = th.zeros(1, device=DEV), th.full((1,), 3.0, device=DEV)
    ec_d = _dev(np.array([ec]))
    # N = 1: the one network's [B, 1] output, no stack
    ops.sac_actor_ens_loss(_dev(logp), [q_d[0]] if n == 1 else q_d, ec_d, g_logp, gq, loss_out, loss_sum)
    th.cuda.synchronize()
    arg = q.argmin(axis=0)  # the FIRST index that attains the minimum
    want_gq = np.zeros((n, b), np.float32)
    want_gq[arg, np.arange(b)] = -(np.float32(1.0) / np.float32(b))
    np.testing.assert_array_equal(gq.cpu().numpy().reshape(n, b), want_gq)
    np.testing.assert_allclose(g_logp.cpu().numpy(), np.full(b, np.float64(ec) / b), rtol=1e-6)
    loss = float(np.mean(np.float64(ec) * logp.astype(np.float64) - q.astype(np.float64).min(axis=0)))
    assert rel_err(float(loss_out), loss, 1e-3) < 1e-5 and rel_err(float(loss_sum) - 3.0, loss, 1e-3) < 1e-5
    if n == 2:
        gl2, g1, g2 = th.empty(b, device=DEV), th.empty(b, device=DEV), th.empty(b, device=DEV)
        lo2, ls2 = th.zeros(1, device=DEV), th.full((1,), 3.0, device=DEV)
        ops.sac_actor_loss(_dev(logp), q_d[0].reshape(b).contiguous(), q_d[1].reshape(b).contiguous(), ec_d, gl2, g1, g2, lo2, ls2)
        assert th.equal(gl2, g_logp) and th.equal(g1, gq[0, :, 0]) and th.equal(g2, gq[1, :, 0])
        assert th.equal(lo2, loss_out) and th.equal(ls2, loss_sum)


def test_ensemble_wrappers_validate_operands():
    from core.common import hip_ops as ops

    b = 64
    z = lambda *sh: th.zeros(*sh, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="1..16"):
        ops.sac_actor_ens_loss(z(b), z(17, b, 1), z(1), z(b), z(17, b, 1))
    with pytest.raises(ValueError, match="critics"):
        ops.td_ens_q_loss(z(3, b, 1), None, z(b), z(b), None, 0.99, z(2, b, 1), 1.0, None, z(3, b, 1))
    with pytest.raises(ValueError, match="gq"):
        ops.td_ens_q_loss(z(3, b, 1), None, z(b), z(b), None, 0.99, z(3, b, 1), 1.0, None, z(2, b, 1))
    base = z(4 * b)
    with pytest.raises(ValueError, match="equally spaced"):
        ops.sac_actor_ens_loss(z(b), [base[:b], base[b:2 * b], base[3 * b:]], z(1), z(b), z(3, b, 1))
    with pytest.raises(ValueError, match="device"):
        ops.sac_actor_ens_loss(z(b), th.zeros(3, b, 1), z(1), z(b), z(3, b, 1))
    with pytest.raises(ValueError, match="overlap"):
        ops.sac_actor_ens_loss(z(b), z(b + 2).as_strided((3, b), (1, 1)), z(1), z(b), z(3, b, 1))


# ------------------------------------------------------------------------------------ learn(): graph replay, paths, learning
def _digest(model, env):
    rb = model.replay_buffer
    h = hashlib.sha256()
    for t in [p.detach() for p in model.policy.parameters()] + [rb.observations, rb.next_observations, rb.actions, rb.rewards, rb.dones,
                                                                rb.sampler_stream, rb.ring.ctl, env.obs, env.step_count]:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def test_sac_ensemble_graph_replay_equals_eager():
    """SAC with three critics under learn(): graph replay (8 iterations per graph) leaves weights, ring, sampler stream and env
    state bit-identical to the eager run."""
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    n, iters = 256, 64
    out = []
    for graph in (False, True):
        env = CSTRVecEnv(n, device=DEV)
        model = SAC("MlpPolicy", env, seed=5, device=DEV, learning_starts=n, buffer_size=n * 32, policy_kwargs=dict(n_critics=3))
        assert model.fused_learner and len(model.critic.q_networks) == 3
        model.enable_graph_capture(graph, unroll=8)
        model.learn(n * iters)
        th.cuda.synchronize()
        st = model.graph_status()
        assert model._n_updates == iters - 1
        if graph:
            assert st["active"] and st["replays"] > 0, st
        out.append(_digest(model, env))
    assert out[0] == out[1]


def test_path_selection(monkeypatch):
    """N = 2 still takes the row-chain step; N = 3 is declined by SacChain.supported and runs the ensemble branch."""
    from core.common import chain, hip_ops
    from core.sac import SAC

    assert chain.USE_CHAIN
    chain_calls = _count_calls(monkeypatch, chain.SacChain, "step")
    ens_calls = _count_calls(monkeypatch, hip_ops, "td_ens_q_loss")
    actor_calls = _count_calls(monkeypatch, hip_ops, "sac_actor_ens_loss")
    for n_critics in (2, 3):
        model = SAC("MlpPolicy", _make_env(64), seed=0, batch_size=64, buffer_size=64 * 8, learning_starts=64,
                    policy_kwargs=dict(n_critics=n_critics))
        model.learn(64 * 3)
        assert model._n_updates == 2
        if n_critics == 2:
            assert chain.SacChain.supported(model, 64) and len(chain_calls) == 2 and not ens_calls
        else:
            assert not chain.SacChain.supported(model, 64) and len(chain_calls) == 2 and len(ens_calls) == len(actor_calls) == 2


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_ensemble_checkpoint_round_trip(algo, monkeypatch):
    """save() / load() keep n_critics; after the load training continues on the ensemble path."""
    from core.common import hip_ops
    from core.sac import SAC
    from core.td3 import TD3

    cls = SAC if algo == "sac" else TD3
    model = cls("MlpPolicy", _make_env(16), seed=1, batch_size=32, buffer_size=16 * 8, learning_starts=16,
                policy_kwargs=dict(net_arch=[32, 32], n_critics=4))
    model.learn(16 * 3)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.zip")
        model.save(path)
        loaded = cls.load(path, env=_make_env(16))
    assert len(loaded.critic.q_networks) == len(loaded.critic_target.q_networks) == 4 and loaded.fused_learner
    for a, b in zip(model.policy.state_dict().values(), loaded.policy.state_dict().values()):
        assert th.equal(a.cpu(), b.cpu())
    ens_calls = _count_calls(monkeypatch, hip_ops, "td_ens_q_loss")
    loaded.learn(16 * 3, reset_num_timesteps=False)
    assert len(ens_calls) == 3 and all(bool(th.isfinite(p).all()) for p in loaded.policy.parameters())


def test_sac_ten_critics_learn():
    """SAC with ten critics on device envs: no NaN, and the deterministic evaluation return improves over the untrained policy."""
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    n = 256
    env, eval_env = CSTRVecEnv(n), CSTRVecEnv(64)
    model = SAC("MlpPolicy", env, seed=0, learning_starts=n * 10, policy_kwargs=dict(n_critics=10))
    model.enable_graph_capture()
    eval_env.seed(1234)
    before, _ = evaluate_policy(model, eval_env, n_eval_episodes=64)
    model.learn(n * 8000)
    assert model.graph_status()["active"]
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
    eval_env.seed(1234)
    after, _ = evaluate_policy(model, eval_env, n_eval_episodes=64)
    assert np.isfinite(after) and after > before + 100, (before, after)
