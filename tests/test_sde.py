"""gSDE (SAC use_sde=True) on the HIP path: the draw / head / gradient kernels of csrc/cstr_sde.hip against an fp64 statement of the
reference's expressions (core/common/distributions.py:421-617: get_std, sample_weights, proba_distribution, get_noise, log_prob through
the atanh round trip), and SAC(use_sde=True) end to end: fused, rocBLAS and ATen learner paths agree on teacher-forced draws, the
row-chain and pair passes decline, the reset cadence, graph replay equal to eager, seeding, checkpoints, n_critics and learning."""
import hashlib
import os
import tempfile

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _env(n=4):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n)


def _count_calls(monkeypatch, owner, name):
    calls = []
    orig = getattr(owner, name, None)

    def wrapped(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    monkeypatch.setattr(owner, name, wrapped, raising=False)
    return calls


def _ref_std(ls, expln, full, L, A):
    """get_std in float64 torch (autograd)"""
    if expln:
        std = th.exp(ls) * (ls <= 0) + (th.log1p(ls * (ls > 0) + 1e-6) + 1.0) * (ls > 0)
    else:
        std = th.exp(ls)
    return std if full else th.ones(L, A, dtype=ls.dtype) * std


def _ref_head(h, w, b, clip, ls, z, per_row, expln, full, deterministic=False):
    """The reference's statements in float64: returns action, logp (autograd through h, w, b, log_std)."""
    L, A = w.shape[1], w.shape[0]
    std = _ref_std(ls, expln, full, L, A)
    M = z * std  # [n, L, A]
    pre = h @ w.t() + b
    mean = th.clamp(pre, -clip, clip) if clip > 0 else pre
    var = (h ** 2) @ (std ** 2)
    scale = th.sqrt(var + 1e-6)
    if deterministic:
        x = mean
    elif per_row:
        x = mean + th.bmm(h.unsqueeze(1), M).squeeze(1)
    else:
        x = mean + h @ M[0]
    act = th.tanh(x)
    _ref_head.x = x.detach().numpy()
    eps = float(np.finfo(np.float32).eps)
    c = act.clamp(-1.0 + eps, 1.0 - eps)
    ga = 0.5 * (c.log1p() - (-c).log1p())
    lp = (-((ga - mean) ** 2) / (2 * scale ** 2) - scale.log() - np.log(np.sqrt(2 * np.pi))).sum(1)
    lp = lp - th.log(1.0 - th.tanh(ga) ** 2 + 1e-6).sum(1)
    return act, lp


def _case(B, L, A, seed, wide=False):
    g = np.random.default_rng(seed)
    h = np.maximum(g.normal(0, 1, (B, L)), 0).astype(np.float32)  # a ReLU latent
    w = (g.normal(0, 1, (A, L)) / np.sqrt(L) * (6.0 if wide else 1.0)).astype(np.float32)
    b = g.normal(0, 0.3, A).astype(np.float32)
    if wide:  # rows where the Hardtanh clip engages and rows whose |x| is large enough for the tanh clamp to engage
        h[: B // 2] *= 8.0
    return h, w, b


@pytest.mark.parametrize("expln", [False, True])
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("clip", [2.0, 0.0])
@pytest.mark.parametrize("noise", ["shared", "per_row", "mode"])
def test_sde_kernels_against_fp64(expln, full, clip, noise):
    from core.common import hip_ops

    B, L, A = 96, 64, 2
    h, w, b = _case(B, L, A, 3, wide=True)
    g = np.random.default_rng(7)
    ls = (g.normal(-1.0, 0.8, (L, A if full else 1))).astype(np.float32)  # both sides of 0: expln's two branches
    n = B if noise == "per_row" else 1
    z = g.normal(0, 1, (1 + n, L, A)).astype(np.float32)
    d = lambda x: th.as_tensor(x).to(DEV).contiguous()  # noqa: E731
    zt, mats, std_b = d(z), th.empty(1 + n, L, A, device=DEV), th.empty(L, A, device=DEV)
    hip_ops.sde_draw(d(ls), A, expln, zt, mats, std_b)
    lsd = th.as_tensor(ls, dtype=th.float64).requires_grad_(True)
    std64 = _ref_std(lsd, expln, full, L, A)
    np.testing.assert_allclose(std_b.cpu().numpy(), std64.detach().numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(mats.cpu().numpy(), (th.as_tensor(z, dtype=th.float64) * std64).detach().numpy(), rtol=2e-6, atol=1e-7)

    m = None if noise == "mode" else (mats[1:] if noise == "per_row" else mats[0])
    action, logp, aux = th.empty(B, A, device=DEV), th.empty(B, device=DEV), th.empty(B, 2 * A, device=DEV)
    hd = d(h)
    hip_ops.sde_head_fwd(hd, d(w), d(b), clip, m, std_b, action, logp, aux)
    h64, w64, b64 = (th.as_tensor(x, dtype=th.float64).requires_grad_(True) for x in (h, w, b))
    zz = th.as_tensor(z[1:] if noise == "per_row" else z[:1], dtype=th.float64)
    a_ref, lp_ref = _ref_head(h64, w64, b64, clip, lsd, zz, noise == "per_row", expln, full, deterministic=noise == "mode")
    np.testing.assert_allclose(action.cpu().numpy(), a_ref.detach().numpy(), rtol=1e-4, atol=2e-5)
    ax = np.abs(_ref_head.x)
    # 4 < |x| < 9.5: the atanh round trip of a float32 tanh is ill-conditioned there (fp64 and fp32 act differ in the last bits of
    # 1 - |act|), so those rows are checked for the action and for finite values only. From |x| ~ 8.4 on the tanh clamp is active in
    # float32 and float64 alike, so the clamped rows (|x| >= 9.5) are compared like the others.
    sat = ((ax > 4.0) & (ax < 9.5)).any(1)
    clamped = (ax >= 9.5).any(1) & ~sat
    assert (~sat).sum() >= 8
    if not (noise == "mode" and clip > 0):  # the mean alone stays within +-clip
        assert clamped.sum() >= 4, clamped.sum()
    lp_ref_n = lp_ref.detach().numpy()
    err = np.abs(logp.cpu().numpy() - lp_ref_n) / np.maximum(1.0, np.abs(lp_ref_n))
    assert err[~sat].max() < 2e-4 and np.isfinite(logp.cpu().numpy()).all()
    if clip > 0:  # the pre-clip mean of rows where the Hardtanh clip engages (aux holds it whatever the noise form)
        assert (np.abs(aux.cpu().numpy()[:, :A]) >= clip).sum() >= 4

    # backward: random upstream gradients of action and logp
    ga, gl = g.normal(0, 1, (B, A)).astype(np.float32), g.normal(0, 1, B).astype(np.float32)
    g_pre, g_x, g_var = (th.empty(B, A, device=DEV) for _ in range(3))
    dh = th.empty(B, L, device=DEV)
    hip_ops.sde_head_bwd(d(ga), d(gl), action, aux, hd, d(w), clip, m, std_b, 1, g_pre, g_x, g_var, dh)
    keep = th.as_tensor(~sat)
    loss = (a_ref * th.as_tensor(ga, dtype=th.float64)).sum(1) + lp_ref * th.as_tensor(gl, dtype=th.float64)
    loss[keep].sum().backward()
    dh_ref = (h64.grad * (h64 > 0)).numpy()
    rows = np.flatnonzero(~sat)
    scale = np.abs(dh_ref[rows]).max() + 1e-6
    assert np.abs(dh.cpu().numpy()[rows] - dh_ref[rows]).max() / scale < 2e-3
    if noise != "per_row":
        dw, db, dls = th.empty(A, L, device=DEV), th.empty(A, device=DEV), th.empty(L, ls.shape[1], device=DEV)
        keep_d = th.as_tensor(~sat, device=DEV).float().unsqueeze(1)
        hip_ops.sde_param_grad(hd, (g_pre * keep_d).contiguous(), (g_x * keep_d).contiguous(), (g_var * keep_d).contiguous(),
                               zt[0] if noise == "shared" else None, std_b, d(ls), expln, dw, db, dls)
        for got, ref in ((dw, w64.grad), (db, b64.grad), (dls, lsd.grad)):
            r = ref.numpy()
            assert np.abs(got.cpu().numpy() - r).max() / (np.abs(r).max() + 1e-6) < 2e-3


def test_sde_draw_stream_is_seeded_and_advances():
    from core.common import hip_ops

    L, A, n = 256, 2, 4096
    ls = th.full((L, A), -3.0, device=DEV)
    outs = []
    for _ in range(2):
        ctl = hip_ops.new_rng_ctl(123, DEV)
        z, m = th.empty(1 + n, L, A, device=DEV), th.empty(1 + n, L, A, device=DEV)
        hip_ops.sde_draw(ls, A, False, z, m, rng_ctl=ctl)
        z2 = th.empty_like(z)
        hip_ops.sde_draw(ls, A, False, z2, th.empty_like(m), rng_ctl=ctl)
        outs.append((z.clone(), z2.clone(), m.clone()))
    assert th.equal(outs[0][0], outs[1][0]) and th.equal(outs[0][1], outs[1][1])  # same seed: identical bits
    assert not th.equal(outs[0][0], outs[0][1])  # the offset advanced on the device
    zz = outs[0][0].double()
    assert abs(float(zz.mean())) < 5e-3 and abs(float(zz.std()) - 1.0) < 5e-3
    assert th.allclose(outs[0][2], outs[0][0] * float(np.exp(np.float32(-3.0))), rtol=1e-6, atol=0.0)


def _sde_model(n_envs=4, **kw):
    from core.sac import SAC

    pk = kw.pop("policy_kwargs", dict(net_arch=[64, 64]))
    return SAC("MlpPolicy", _env(n_envs), seed=kw.pop("seed", 0), use_sde=True, policy_kwargs=pk, **kw)


@pytest.mark.parametrize("pk", [dict(net_arch=[64, 64]), dict(net_arch=[64, 64], use_expln=True, full_std=False, clip_mean=0.0)])
def test_actor_gradients_agree_across_paths(pk, monkeypatch):
    """One teacher-forced gradient step on the fused, rocBLAS and ATen paths from the same state: the actor arena's gradient buffer
    (dW / db of every layer, d log_std, written by the gSDE head's backward on the fused paths, by autograd on the ATen path) agrees
    per parameter at a tight relative bar, and d log_std and dW_mu are not zero."""
    from core.common import fused, hip_ops

    grads = {}
    for path in ("fused", "rocblas", "aten"):
        with monkeypatch.context() as mp:
            if path == "rocblas":
                mp.setattr(fused, "USE_FUSED_LINEAR", False)
            model = _sde_model(16, batch_size=64, buffer_size=64 * 16, learning_starts=16 * 8, policy_kwargs=dict(pk))
            assert model.fused_learner
            model.learn(16 * 8)
            model.fused_learner = path != "aten"
            model.actor.action_dist.torch_matrices = path == "aten"
            g = th.Generator().manual_seed(11)
            L = model.actor.log_std.shape[0]
            hip_ops.mt19937_seed(model.replay_buffer.sampler_stream, 5)
            model.actor.action_dist.z_queue = [th.randn(L, 2, generator=g), th.randn(1, L, 2, generator=g)]
            model.train(gradient_steps=1, batch_size=64)
            assert not model.actor.action_dist.z_queue
            grads[path] = {k: p.grad.detach().cpu().double().clone() for k, p in model.actor.named_parameters()}
    f = grads["fused"]
    assert float(f["log_std"].abs().max()) > 0 and float(f["mu.0.weight" if "mu.0.weight" in f else "mu.weight"].abs().max()) > 0
    for path in ("rocblas", "aten"):
        for k, ref in f.items():
            err = float((grads[path][k] - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
            assert err < 1e-3, (path, k, err)


def _sde_pk(tag):
    pk = {} if tag == "default" else dict(net_arch=[64, 64])
    if tag == "variants":
        pk.update(use_expln=True, full_std=False, clip_mean=0.0)
    return pk


@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("tag", ["small", "default", "variants"])
def test_sac_sde_teacher_forced(golden, tag, path, monkeypatch):
    """Teacher-forced gradient steps against the reference (tests/golden/sac_sde_train_kat_*.npz, written by the unmodified reference):
    initial weights and construction draws bit-equal, the sampled batches, Q values / TD targets within the code path's bars, the
    logged losses and every weight after the steps."""
    from _parity_helpers import check_init, check_weights, load_ring, q_err, rel_err

    from core.common import chain, fused, hip_ops, legacy_rng
    from core.sac import SAC

    monkeypatch.setattr(chain, "USE_CHAIN", True)  # SacChain must decline gSDE by itself
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    chain_calls = _count_calls(monkeypatch, chain.SacChain, "step")
    grad_calls = _count_calls(monkeypatch, hip_ops, "sde_param_grad")
    g = golden(f"sac_sde_train_kat_{tag}.npz")
    gamma, tau, target_entropy, lr, B, n_steps = g["hyper"]
    B, n_steps = int(B), int(n_steps)
    model = SAC("MlpPolicy", _env(4), seed=0, batch_size=B, buffer_size=64 * 4, use_sde=True, policy_kwargs=_sde_pk(tag))
    assert model.fused_learner
    model.fused_learner = path != "aten"
    model.actor.action_dist.torch_matrices = path == "aten"
    assert model.gamma == gamma and model.tau == tau and model.target_entropy == target_entropy and model.lr_schedule(1) == lr
    mods = ["actor", "critic", "critic_target"]
    check_init(model, g, mods)
    z1, z2 = model.actor.action_dist._host_z
    np.testing.assert_array_equal(z1.numpy(), g["init/z_mat"])
    np.testing.assert_array_equal(z2.numpy(), g["init/z_mats"])
    load_ring(model, g)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    model.debug_capture = True
    lab = f"sac_sde_{tag}_{path}"
    for k in range(n_steps):
        model.actor.action_dist.z_queue = [th.as_tensor(g[f"step{k}/z_mat"]), th.as_tensor(g[f"step{k}/z_mats"])]
        model.train(gradient_steps=1, batch_size=B)
        assert not model.actor.action_dist.z_queue
        b = model._static_batch
        for name in ("observations", "actions", "next_observations", "dones", "rewards"):
            np.testing.assert_array_equal(getattr(b, name).cpu().numpy(), g[f"step{k}/batch_{name}"], err_msg=f"step {k} batch {name}")
        t = model.last_train_tensors
        assert q_err(t["target_q"].cpu().numpy(), g[f"step{k}/target_q"], lab) < 1e-5, f"target_q step {k}"
        for i in range(2):
            assert q_err(t["current_q"][i].cpu().numpy(), g[f"step{k}/current_q{i + 1}"], lab) < 1e-5, f"q{i + 1} step {k}"
        lv = model.logger.name_to_value
        for key in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef"):
            assert rel_err(float(lv[f"train/{key}"]), float(g[f"step{k}/{key}"]), 1e-3) < 1e-5, f"{key} step {k}"
    assert model._n_updates == n_steps and not chain_calls
    assert len(grad_calls) == (0 if path == "aten" else n_steps)
    check_weights(model, g, "after", mods)
    assert abs(float(model.log_ent_coef.detach()) - float(g["after/log_ent_coef"][0])) < 1e-6


@pytest.mark.parametrize("path", ["fused", "aten"])
def test_sac_sde_predict_against_reference(golden, path):
    """predict() vs the reference (tests/golden/sac_sde_predict_kat.npz): 4 envs with per-env matrices, one env (exploration_mat),
    deterministic, and after a gradient step, whose batch-1 draw makes every row use exploration_mat."""
    from _parity_helpers import check_init, check_weights, load_ring

    from core.common import legacy_rng
    from core.sac import SAC

    g = golden("sac_sde_predict_kat.npz")
    model = SAC("MlpPolicy", _env(4), seed=0, batch_size=64, buffer_size=64 * 4, use_sde=True, policy_kwargs=dict(net_arch=[64, 64]))
    model.fused_learner = path != "aten"
    model.actor.action_dist.torch_matrices = path == "aten"
    check_init(model, g, ["actor", "critic", "critic_target"])
    obs = g["obs"]
    obs_t = th.as_tensor(obs, device=DEV)
    d = model.actor.action_dist

    def actor_out(x, deterministic=False):
        with th.no_grad():
            if path == "fused":
                return model._fast_actor.sde_action_log_prob(x, train_params=False, want_logp=False, deterministic=deterministic)[0]
            return model.actor(x, deterministic=deterministic)

    def close(got, key, tol=2e-5):
        np.testing.assert_allclose(np.asarray(got.cpu() if isinstance(got, th.Tensor) else got), g[key], rtol=0, atol=tol, err_msg=key)

    d.z_queue = [th.as_tensor(g["per_env/z_mat"]), th.as_tensor(g["per_env/z_mats"])]
    model.actor.reset_noise(4)
    assert d.noise_rows(4) and not d.noise_rows(1)
    close(actor_out(obs_t), "per_env/actions")
    close(model.predict(obs)[0], "per_env/predict", 1e-4)
    close(actor_out(obs_t[:1]), "single/actions")
    close(model.predict(obs[:1])[0], "single/predict", 1e-4)
    close(actor_out(obs_t, True), "deterministic/actions")
    close(model.predict(obs, deterministic=True)[0], "deterministic/predict", 1e-4)
    load_ring(model, g)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    d.z_queue = [th.as_tensor(g["train/z_mat"]), th.as_tensor(g["train/z_mats"])]
    model.train(gradient_steps=1, batch_size=64)
    assert not d.z_queue and d.current[3] == 1 and not d.noise_rows(4)
    check_weights(model, g, "after", ["actor"])
    close(actor_out(obs_t), "after_train/actions", 1e-4)
    close(model.predict(obs)[0], "after_train/predict", 2e-4)


def test_path_selection_and_kernels(monkeypatch):
    from core.common import chain, hip_ops

    head_calls = _count_calls(monkeypatch, hip_ops, "sde_head_fwd")
    grad_calls = _count_calls(monkeypatch, hip_ops, "sde_param_grad")
    draw_calls = _count_calls(monkeypatch, hip_ops, "sde_draw")
    chain_calls = _count_calls(monkeypatch, chain.SacChain, "step")
    model = _sde_model(64, batch_size=64, buffer_size=64 * 8, learning_starts=64, policy_kwargs=dict(n_critics=2))
    model.learn(64 * 3)
    assert model.fused_learner and model._n_updates == 2
    assert not chain.SacChain.supported(model, 64) and not chain_calls
    assert model._fast_actor.rollout_operands(model._denv.obs) is None and not model._use_packed_batch()
    assert len(grad_calls) == 2 and len(head_calls) == 2 * 2 + 2 and len(draw_calls) == 1 + 3 + 2
    std = float(model.logger.name_to_value.get("train/std", float("nan"))) if "train/std" in model.logger.name_to_value else None
    assert std is None or np.isfinite(std)


@pytest.mark.parametrize("freq", [-1, 2])
def test_resample_cadence(freq, monkeypatch):
    """train_freq=(4, "step"): the rollout's matrices stay put for its 4 steps with sde_sample_freq=-1 and are redrawn every 2 steps."""
    model = _sde_model(8, batch_size=32, buffer_size=8 * 64, learning_starts=0, train_freq=(4, "step"), sde_sample_freq=freq)
    seen = []
    orig = model.actor.reset_noise

    def rec(batch_size=1):
        seen.append(batch_size)
        return orig(batch_size)

    monkeypatch.setattr(model.actor, "reset_noise", rec)
    model.learn(8 * 4)
    expect = [8] if freq < 0 else [8, 8, 8]  # start of the rollout (+ steps 0 and 2), then the gradient step's batch-1 reset
    assert seen == expect + [1], seen


def test_predict_rules():
    """predict() on n_envs rows uses one matrix per row; on one row exploration_mat; deterministic the mean; after a train step
    the batch-1 draw makes n rows share exploration_mat (the reference's quirk)."""
    model = _sde_model(4, batch_size=16, buffer_size=4 * 64, learning_starts=16)
    model.learn(4 * 6)
    a = model.actor
    d = a.action_dist
    assert d.current[3] == 1  # the last reset was the train step's
    obs = th.rand(4, 4, device=DEV) * 2 - 1
    a.reset_noise(4)
    h = a.latent_pi(obs)
    mean = a.mu(h)
    with th.no_grad():
        per = model._fast_actor.sde_action_log_prob(obs, train_params=False, want_logp=False)[0]
        ref = th.tanh(mean + th.bmm(h.unsqueeze(1), d.exploration_matrices).squeeze(1))
        assert float((per - ref).abs().max()) < 1e-5
        one = model._fast_actor.sde_action_log_prob(obs[:1], train_params=False, want_logp=False)[0]
        assert float((one - th.tanh(mean[:1] + h[:1] @ d.exploration_mat)).abs().max()) < 1e-5
        det = model._fast_actor.sde_action_log_prob(obs, train_params=False, want_logp=False, deterministic=True)[0]
        assert float((det - th.tanh(mean)).abs().max()) < 1e-5
        a.reset_noise()
        shared = model._fast_actor.sde_action_log_prob(obs, train_params=False, want_logp=False)[0]
        assert float((shared - th.tanh(mean + h @ d.exploration_mat)).abs().max()) < 1e-5
        act, _ = model.predict(obs.cpu().numpy())
        assert np.isfinite(act).all()


def _digest(model, env):
    rb = model.replay_buffer
    h = hashlib.sha256()
    for t in [p.detach() for p in model.policy.parameters()] + [rb.observations, rb.next_observations, rb.actions, rb.rewards, rb.dones,
                                                                rb.sampler_stream, rb.ring.ctl, env.obs, env.step_count]:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def test_graph_replay_equals_eager_and_seeding():
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    n, iters = 256, 48
    out = []
    for graph in (False, True, True):
        env = CSTRVecEnv(n, device=DEV)
        model = SAC("MlpPolicy", env, seed=5, device=DEV, learning_starts=n, buffer_size=n * 32, use_sde=True)
        model.enable_graph_capture(graph, unroll=8)
        model.learn(n * iters)
        th.cuda.synchronize()
        st = model.graph_status()
        assert model._n_updates == iters - 1
        if graph:
            assert st["active"] and st["replays"] > 0 and st["error"] is None, st
        out.append(_digest(model, env))
    assert out[0] == out[1] == out[2]


def test_checkpoint_round_trip():
    model = _sde_model(16, batch_size=32, buffer_size=16 * 8, learning_starts=16, policy_kwargs=dict(net_arch=[32, 32], n_critics=3))
    model.learn(16 * 3)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.zip")
        model.save(path)
        from core.sac import SAC

        loaded = SAC.load(path, env=_env(16))
    assert loaded.use_sde and loaded.actor.use_sde and loaded.fused_learner and len(loaded.critic.q_networks) == 3
    sd, sl = model.policy.state_dict(), loaded.policy.state_dict()
    assert "actor.log_std" in sd and "actor.mu.0.weight" in sd and list(sd) == list(sl)
    for k in sd:
        assert th.equal(sd[k].cpu(), sl[k].cpu()), k
    assert loaded.actor.action_dist.current is not None  # load() redrew the matrices
    loaded.learn(16 * 3, reset_num_timesteps=False)
    assert all(bool(th.isfinite(p).all()) for p in loaded.policy.parameters())


def test_gsde_sac_learns():
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC

    n = 256
    env, eval_env = CSTRVecEnv(n), CSTRVecEnv(64)
    model = SAC("MlpPolicy", env, seed=0, learning_starts=n * 10, use_sde=True, policy_kwargs=dict(n_critics=3))
    model.enable_graph_capture()
    eval_env.seed(1234)
    before, _ = evaluate_policy(model, eval_env, n_eval_episodes=64)
    model.learn(n * 6000)
    assert model.graph_status()["active"]
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
    eval_env.seed(1234)
    after, _ = evaluate_policy(model, eval_env, n_eval_episodes=64)
    assert np.isfinite(after) and after > before, (before, after)
