"""BCQ on the HIP learner (core/bcq, core/common/offline_policy_algorithm.py, csrc/cstr_bcq.hip).

Golden vectors tests/golden/bcq_train_kat_{small,default}.npz and bcq_predict_kat.npz were written by the unmodified reference
(tools/refharness/gen_golden.py gen_bcq / gen_bcq_predict). The three draws of a gradient step -- randn_like [B, L] (reference
core/bcq/policies.py:82), randn [10 B, L] (:123) and, on actor steps, randn [B, L] (:123) -- are teacher-forced through
`noise_queue`; the [10 B, L] draw is stored as the seed of the generator that made it plus digests, and regenerated here. The bars are
the project's own for SAC / TD3 (tests/_parity_helpers.py); tanh-bounded outputs use tests/test_sde.py's."""
import types

import numpy as np
import pytest
import torch as th

from _parity_helpers import check_init, check_weights, load_ring, q_err, rel_err, strict_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODS = ["actor", "actor_target", "critic", "critic_target"]


def _env(n=1):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n)


def _spaces():
    from core.common.spaces import Box

    return Box(-1, 1, (4,)), Box(-1, 1, (2,))


def _dataset_from_fixture(g):
    """The fixture's ring as a ReplayBuffer object of this package (one env)."""
    from core.common.buffers import ReplayBuffer

    rows, n = g["ring_rew"].shape
    rb = ReplayBuffer(rows * n, *_spaces(), device=DEV, n_envs=n)
    load_ring(types.SimpleNamespace(replay_buffer=rb), g)
    return rb


def _synthetic_dataset(rows=512, seed=3, sampler_seed=5):
    from core.common.buffers import ReplayBuffer

    rng = np.random.default_rng(seed)
    rb = ReplayBuffer(rows, *_spaces(), device=DEV, n_envs=1)
    obs = rng.uniform(-1, 1, (rows, 1, 4)).astype(np.float32)
    rb.observations.copy_(th.as_tensor(obs))
    rb.next_observations.copy_(th.as_tensor(np.clip(obs + rng.normal(0, 0.05, obs.shape), -1, 1).astype(np.float32)))
    rb.actions.copy_(th.as_tensor(rng.uniform(-1, 1, (rows, 1, 2)).astype(np.float32)))
    rb.rewards.copy_(th.as_tensor(rng.uniform(-8, 0, (rows, 1)).astype(np.float32)))
    rb.dones.copy_(th.as_tensor((rng.uniform(size=(rows, 1)) < 0.1).astype(np.float32)))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    if sampler_seed is not None:
        rb.seed_sampler(sampler_seed)
    return rb


def _draws(g, k, B, L):
    """The step's raw draws, regenerated from the stored generator seed and checked against the stored tensors / digests."""
    gen = th.Generator().manual_seed(int(g[f"step{k}/th_seed"]))
    d1, d2 = th.randn(B, L, generator=gen), th.randn(10 * B, L, generator=gen)
    np.testing.assert_array_equal(d1.numpy(), g[f"step{k}/draw_vae"])
    np.testing.assert_array_equal(d2.reshape(-1)[:64].numpy(), g[f"step{k}/draw_target#head"])
    assert float(d2.double().sum()) == float(g[f"step{k}/draw_target#sum"])
    out = [d1, d2]
    if f"step{k}/draw_actor" in g:
        d3 = th.randn(B, L, generator=gen)
        np.testing.assert_array_equal(d3.numpy(), g[f"step{k}/draw_actor"])
        out.append(d3)
    return out


def _strict(got, want):
    """The per-element figure q_err asserts on (|dq_i| / max(|q_i|, 1e-3)), for the printed record."""
    want = np.asarray(want, np.float64)
    return float((np.abs(got.cpu().numpy().astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)).max())


def _select_path(monkeypatch, model, path):
    from core.common import fused

    assert model.fused_learner
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    if path == "aten":
        model.fused_learner = False
        assert model.policy.fast is None


def _model_for(g, tag, **kw):
    from core.bcq import BCQ

    gamma, tau, delay, lr, B, n_steps, L, mp = g["hyper"]
    pk = dict(critic_net_arch=[64, 64]) if tag == "small" else {}
    model = BCQ("MlpPolicy", _env(), dataset=_dataset_from_fixture(g), seed=0, batch_size=int(B), policy_kwargs=pk, **kw)
    assert (model.gamma, model.tau, model.actor_delay, model.lr_schedule(1)) == (gamma, tau, int(delay), lr)
    assert model.actor.vae.latent_dim == int(L) and model.actor.perturbation.max_perturbation == mp
    return model


def _teacher_forced(g, tag, path, monkeypatch, check=True, **kw):
    from core.common import legacy_rng

    model = _model_for(g, tag, **kw)
    B, n_steps, L = int(g["hyper"][4]), int(g["hyper"][5]), int(g["hyper"][6])
    _select_path(monkeypatch, model, path)
    check_init(model, g, MODS)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    model.debug_capture = True
    lab = f"bcq_{tag}_{path}"
    captured = []
    for k in range(n_steps):
        model.noise_queue = _draws(g, k, B, L)
        model.train(gradient_steps=1, batch_size=B)
        assert not model.noise_queue
        t = model.last_train_tensors
        captured.append(t)
        if not check:
            continue
        b = model._static_batch
        for name in ("observations", "actions", "next_observations", "dones", "rewards"):
            np.testing.assert_array_equal(getattr(b, name).cpu().numpy(), g[f"step{k}/batch_{name}"], err_msg=f"step {k} batch {name}")
        np.testing.assert_allclose(t["recon"].cpu().numpy(), g[f"step{k}/recon"], rtol=1e-4, atol=2e-5, err_msg=f"recon step {k}")
        print(f"{lab} step {k}: per-element target_q {_strict(t['target_q'], g[f'step{k}/target_q']):.2e} "
              f"q1 {_strict(t['current_q'][0], g[f'step{k}/current_q1']):.2e} q2 {_strict(t['current_q'][1], g[f'step{k}/current_q2']):.2e}")
        e_t = q_err(t["target_q"].cpu().numpy(), g[f"step{k}/target_q"], lab)
        e_q = [q_err(t["current_q"][i].cpu().numpy(), g[f"step{k}/current_q{i + 1}"], lab) for i in range(2)]
        lv = model.logger.name_to_value
        e_l = {key: rel_err(float(lv[f"train/{key}"]), float(g[f"step{k}/{key}"]), 1e-3) for key in ("critic_loss", "vae_loss")}
        if f"step{k}/actor_loss" in g:
            assert t["actor_loss"] is not None
            e_l["actor_loss"] = rel_err(float(t["actor_loss"]), float(g[f"step{k}/actor_loss"]), 1e-3)
            assert rel_err(float(lv["train/actor_loss"]), float(g[f"step{k}/actor_loss"]), 1e-3) < 1e-5
        else:
            assert t["actor_loss"] is None
        print(f"{lab} step {k}: target_q {e_t:.2e} q {e_q[0]:.2e} {e_q[1]:.2e} losses {e_l}")
        assert e_t < 1e-5 and max(e_q) < 1e-5, f"step {k}"
        assert all(v < 1e-5 for v in e_l.values()), (k, e_l)
    return model, captured


# ------------------------------------------------------------------------------------ teacher-forced parity with the reference
@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("tag", ["small", "default"])
def test_bcq_teacher_forced(golden, tag, path, monkeypatch):
    g = golden(f"bcq_train_kat_{tag}.npz")
    model, _ = _teacher_forced(g, tag, path, monkeypatch)
    n_steps, delay = int(g["hyper"][5]), int(g["hyper"][2])
    check_weights(model, g, "after", MODS)
    a = model.actor
    assert a.vae_optimizer.step_count == n_steps and model.critic.optimizer.step_count == n_steps
    assert a.perturbation_optimizer.step_count == n_steps // delay and model._n_updates == n_steps
    # actor_target.vae == actor.vae always (the copy after every step); only the perturbation net is really soft-updated
    for (k, v), (_, vt) in zip(a.vae.state_dict().items(), model.actor_target.vae.state_dict().items()):
        assert th.equal(v, vt), k
    assert not th.equal(a.perturbation.model[0].weight, model.actor_target.perturbation.model[0].weight)


@pytest.mark.parametrize("path", ["fused", "aten"])
def test_faithful_quirks_false_takes_a_states_own_candidates(golden, path, monkeypatch):
    """The reference's reshape(B, 10) mixes ten different next states into a target row; faithful_quirks=False is the max over a
    state's own ten candidates: it differs from the fixture and equals a torch statement of the intended grouping."""
    g = golden("bcq_train_kat_small.npz")
    B, L = int(g["hyper"][4]), int(g["hyper"][6])
    model, cap = _teacher_forced(g, "small", path, monkeypatch, check=False, faithful_quirks=False)
    t = cap[0]
    got = t["target_q"].cpu().numpy()
    assert np.abs(got - g["step0/target_q"]).max() > 1e-2  # the quirk is real
    # both groupings as torch statements on the step's own tensors: per-row min over the target critics, [sample][state] order
    # (step 0's tensors: `cap[0]` and the fixture's step-0 batch)
    rew, done = th.as_tensor(g["step0/batch_rewards"]).to(DEV), th.as_tensor(g["step0/batch_dones"]).to(DEV)
    min_q = t["next_q_min"].reshape(-1)
    assert min_q.shape == (10 * B,)
    intended = rew + (1 - done) * model.gamma * min_q.reshape(10, B).max(0)[0].unsqueeze(1)
    quirk = rew + (1 - done) * model.gamma * min_q.reshape(B, 10).max(1)[0].unsqueeze(1)
    assert q_err(got, intended.cpu().numpy(), f"bcq_intended_{path}") < 1e-5
    assert float((quirk - intended).abs().max()) > 1e-2 and L == model.actor.vae.latent_dim


# ------------------------------------------------------------------------------------ kernels against fp64 NumPy
def _t(a):
    return th.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def test_latent_kernels_against_fp64():
    from core.common import hip_ops

    rng = np.random.default_rng(0)
    B, D, L = 96, 4, 32
    params = rng.normal(0, 1.5, (B, 2 * L)).astype(np.float32)
    params[:8, L:] = rng.uniform(-9, -4.5, (8, L))   # clamp engaged at -4
    params[8:16, L:] = rng.uniform(15.5, 20, (8, L))  # ... and at 15
    params[16, L:] = -4.0                             # exactly at the bounds: the gradient passes
    params[17, L:] = 15.0
    obs = rng.uniform(-1, 1, (B, D + 2)).astype(np.float32)  # row-strided observation view
    eps = rng.normal(0, 1, (B, L)).astype(np.float32)
    d_params, d_obs, d_eps = _t(params), _t(obs), _t(eps)
    xdec, std = th.zeros(B, D + L, device=DEV), th.zeros(B, L, device=DEV)
    hip_ops.bcq_latent_fwd(d_params, d_obs[:, :D], d_eps, None, xdec, std)
    p64, e64 = params.astype(np.float64), eps.astype(np.float64)
    ls = np.clip(p64[:, L:], -4, 15)
    std64 = np.exp(ls)
    z64 = p64[:, :L] + std64 * e64
    np.testing.assert_array_equal(xdec[:, :D].cpu().numpy(), obs[:, :D])
    np.testing.assert_allclose(std.cpu().numpy(), std64, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(xdec[:, D:].cpu().numpy(), z64, rtol=2e-6, atol=1e-7 * max(1.0, float(np.abs(z64).max())))
    # backward: g_mean = g_z + dKL/dmean, g_log_std_raw = (g_z eps + dKL/dstd) std on the closed interval [-4, 15]
    g_x = rng.normal(0, 1, (B, D + L)).astype(np.float32)
    gm = rng.normal(0, 0.1, (B, L)).astype(np.float32)
    gs = rng.normal(0, 0.1, (B, L)).astype(np.float32)
    g_params = th.zeros(B, 2 * L, device=DEV)
    hip_ops.bcq_latent_bwd(_t(g_x)[:, D:], _t(gm), _t(gs), d_params, std, d_eps, g_params)
    gz = g_x[:, D:].astype(np.float64)
    mask = (p64[:, L:] >= -4) & (p64[:, L:] <= 15)
    want_m = gz + gm
    want_s = np.where(mask, (gz * e64 + gs) * std64, 0.0)
    assert mask[16].all() and mask[17].all() and not mask[:16].any()
    got = g_params.cpu().numpy().astype(np.float64)
    assert np.abs(got[:, :L] - want_m).max() <= 2e-3 * np.abs(want_m).max()
    # the std = exp(15) rows set the tensor's scale; check the ordinary rows on their own scale too
    assert np.abs(got[:, L:] - want_s).max() <= 2e-3 * np.abs(want_s).max()
    assert np.abs(got[18:, L:] - want_s[18:]).max() <= 2e-3 * np.abs(want_s[18:]).max()
    assert (got[:16, L:] == 0).all()
    # the rows exactly on the bounds, each on its own scale (std = exp(-4) and exp(15)): the closed interval passes the gradient
    for row in (16, 17):
        assert np.abs(got[row, L:] - want_s[row]).max() <= 2e-3 * np.abs(want_s[row]).max()
        assert (got[row, L:] != 0).all()


def test_vae_loss_kernel_against_fp64():
    from core.common import hip_ops

    rng = np.random.default_rng(1)
    for B, A, L in ((64, 2, 32), (256, 2, 32), (37, 3, 5)):
        recon = np.tanh(rng.normal(0, 1, (B, A))).astype(np.float32)
        act = rng.uniform(-1, 1, (B, A + 4)).astype(np.float32)  # actions as a column block of [obs | act] rows
        params = rng.normal(0, 1, (B, 2 * L)).astype(np.float32)
        std = np.exp(np.clip(rng.normal(-1, 2, (B, L)), -4, 15)).astype(np.float32)
        g_recon, g_mean, g_std = th.zeros(B, A, device=DEV), th.zeros(B, L, device=DEV), th.zeros(B, L, device=DEV)
        loss, total = th.zeros(1, device=DEV), th.full((1,), 2.0, device=DEV)
        hip_ops.bcq_vae_loss(_t(recon), _t(act)[:, 4:], _t(params), _t(std), g_recon, g_mean, g_std, loss, total)
        r, a, m, s = (x.astype(np.float64) for x in (recon, act[:, 4:], params[:, :L], std))
        want = ((r - a) ** 2).mean() + 0.5 * (-0.5 * (1 + np.log(s * s) - m * m - s * s).mean())
        assert abs(float(loss) - want) <= 2e-6 * abs(want) + 1e-7, (B, float(loss), want)
        assert abs(float(total) - (2.0 + want)) <= 4e-6 * abs(2.0 + want)
        for got, w in ((g_recon, 2 * (r - a) / (B * A)), (g_mean, 0.5 * m / (B * L)), (g_std, -0.25 * (2 / s - 2 * s) / (B * L))):
            assert np.abs(got.cpu().numpy() - w).max() <= 2e-3 * np.abs(w).max()


def test_expand_and_perturb_kernels_against_fp64():
    from core.common import hip_ops

    rng = np.random.default_rng(2)
    for n, S, D, L, A in ((64, 10, 4, 32, 2), (1, 100, 4, 32, 2), (5, 1, 8, 7, 4), (3, 100, 5, 6, 3)):
        rows = n * S
        state = rng.uniform(-1, 1, (n, D + A)).astype(np.float32)
        noise = rng.normal(0, 1, (rows, L)).astype(np.float32)
        xdec, xp, xc = th.zeros(rows, D + L, device=DEV), th.zeros(rows, D + A, device=DEV), th.zeros(rows, D + A, device=DEV)
        st = _t(state)[:, :D] if S != 100 else _t(state[:, :D])  # a column block of wider rows, or contiguous (16-byte rows when D % 4 == 0)
        hip_ops.bcq_expand(st, S, _t(noise), None, xdec, xp, xc)
        rep = np.tile(state[:, :D], (S, 1))  # row r belongs to state r % n
        np.testing.assert_array_equal(xdec[:, :D].cpu().numpy(), rep)
        np.testing.assert_array_equal(xp[:, :D].cpu().numpy(), rep)
        np.testing.assert_array_equal(xc[:, :D].cpu().numpy(), rep)
        np.testing.assert_array_equal(xdec[:, D:].cpu().numpy(), np.clip(noise, -0.5, 0.5))
        assert float(xp[:, D:].abs().max()) == 0.0 and float(xc[:, D:].abs().max()) == 0.0
        # perturbation: rows clamped at both ends and exactly on the bounds
        a_vae = np.tanh(rng.normal(0, 2, (rows, A))).astype(np.float32)
        p = np.tanh(rng.normal(0, 2, (rows, A))).astype(np.float32)
        a_vae[0], p[0] = 1.0, 1.0      # beyond +1
        a_vae[-1], p[-1] = -1.0, -1.0  # beyond -1
        if rows > 2:
            a_vae[1], p[1] = 1.0, 0.0  # exactly +1: the gradient passes (closed interval)
            a_vae[2], p[2] = -1.0, 0.0  # ... and exactly -1
        xp[:, D:].copy_(_t(a_vae))
        hip_ops.bcq_perturb_fwd(xp[:, D:], _t(p), 0.05, xc[:, D:])
        x64 = a_vae.astype(np.float64) + np.float64(np.float32(0.05)) * p
        np.testing.assert_allclose(xc[:, D:].cpu().numpy(), np.clip(x64, -1, 1), rtol=1e-4, atol=2e-5)
        assert float(xc[:, D:].abs().max()) <= 1.0
        g = rng.normal(0, 1, (rows, D + A)).astype(np.float32)
        g_p = th.zeros(rows, A, device=DEV)
        hip_ops.bcq_perturb_bwd(_t(g)[:, D:], xp[:, D:], _t(p), 0.05, g_p)
        x32 = a_vae + p * np.float32(0.05)
        want = np.where((x32 >= -1) & (x32 <= 1), g[:, D:].astype(np.float64) * np.float64(np.float32(0.05)), 0.0)
        got = g_p.cpu().numpy()
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max()
        assert (got[0] == 0).all() and (got[-1] == 0).all()
        if rows > 2:
            assert (got[1] != 0).all() and (got[2] != 0).all()
            np.testing.assert_allclose(got[1:3], want[1:3], rtol=2e-6, atol=0)


@pytest.mark.parametrize("n_q", [1, 2])
@pytest.mark.parametrize("S", [1, 10, 100])
def test_target_and_select_kernels_against_fp64(n_q, S):
    from core.common import hip_ops

    rng = np.random.default_rng(10 * n_q + S)
    n, A, gamma = 64, 2, 0.99
    rows = n * S
    q = np.round(rng.normal(-3, 2, (n_q, rows, 1)), 1).astype(np.float32)  # rounded: plenty of ties
    rew, done = rng.uniform(-8, 0, (n, 1)).astype(np.float32), (rng.uniform(size=(n, 1)) < 0.3).astype(np.float32)
    qmin = q.astype(np.float64).min(0)[:, 0]
    for reference_grouping in (True, False):
        target, mq = th.zeros(n, 1, device=DEV), th.zeros(n, device=DEV)
        hip_ops.bcq_target(_t(q), n, S, reference_grouping, _t(rew), _t(done), gamma, target, mq)
        best = qmin.reshape(n, S).max(1) if reference_grouping else qmin.reshape(S, n).max(0)
        np.testing.assert_array_equal(mq.cpu().numpy(), best.astype(np.float32))
        want = rew[:, 0].astype(np.float64) + (1 - done[:, 0]) * np.float64(np.float32(gamma)) * best
        np.testing.assert_allclose(target[:, 0].cpu().numpy(), want, rtol=2e-6, atol=1e-7)
    if S > 1:
        assert not np.array_equal(qmin.reshape(n, S).max(1), qmin.reshape(S, n).max(0))  # the two groupings are different things
    # selection: first maximum wins, as argmax
    cand = rng.uniform(-1, 1, (rows, 4 + A)).astype(np.float32)
    idx, act = th.zeros(n, dtype=th.int64, device=DEV), th.zeros(n, A, device=DEV)
    hip_ops.bcq_select(_t(q[0, :, 0]), _t(cand)[:, 4:], n, S, idx, act)
    want_s = q[0, :, 0].reshape(S, n).argmax(0)  # numpy's argmax returns the first maximum
    np.testing.assert_array_equal(idx.cpu().numpy(), want_s * n + np.arange(n))
    np.testing.assert_array_equal(act.cpu().numpy(), cand[want_s * n + np.arange(n), 4:])


def test_drawn_noise_is_seeded_advances_and_is_standard_normal():
    from core.common import hip_ops

    n, S, D, L = 4096, 10, 4, 32
    state = th.zeros(n, D, device=DEV)
    outs = []
    for seed in (7, 7, 8):
        ctl = hip_ops.new_rng_ctl(seed, DEV)
        xdec = th.zeros(n * S, D + L, device=DEV)
        hip_ops.bcq_expand(state, S, None, ctl, xdec, clip=100.0)  # a clip nothing reaches: the raw draw
        first = xdec[:, D:].clone()
        assert int(ctl[1]) == n * S * L // 2 and int(ctl[2]) == 0  # offset advanced by the pairs drawn, ticket reset
        hip_ops.bcq_expand(state, S, None, ctl, xdec, clip=100.0)
        assert not th.equal(first, xdec[:, D:]) and int(ctl[1]) == n * S * L
        outs.append(first)
    assert th.equal(outs[0], outs[1]) and not th.equal(outs[0], outs[2])
    z = outs[0].double()
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1.0) < 5e-3
    ctl = hip_ops.new_rng_ctl(7, DEV)
    xdec = th.zeros(n * S, D + L, device=DEV)
    hip_ops.bcq_expand(state, S, None, ctl, xdec)
    assert float(xdec[:, D:].abs().max()) <= 0.5 and th.equal(xdec[:, D:], outs[0].clamp(-0.5, 0.5))
    # the latent launch: drawn eps is stored, z = mean + std * eps with it, the stream advances
    B = 32768
    params, state = th.zeros(B, 2 * L, device=DEV), th.zeros(B, D, device=DEV)
    ctl = hip_ops.new_rng_ctl(3, DEV)
    x, std, eps = th.zeros(B, D + L, device=DEV), th.zeros(B, L, device=DEV), th.zeros(B, L, device=DEV)
    hip_ops.bcq_latent_fwd(params, state[:B], None, ctl, x, std, eps)
    assert th.equal(x[:, D:], eps) and float(std.min()) == 1.0 and int(ctl[1]) == B * L // 2
    assert abs(float(eps.double().mean())) < 5e-3 and abs(float(eps.double().std()) - 1.0) < 5e-3
    eps2 = th.zeros(B, L, device=DEV)
    hip_ops.bcq_latent_fwd(params, state[:B], None, ctl, x, std, eps2)
    assert not th.equal(eps, eps2)


# ------------------------------------------------------------------------------------ predict
@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
def test_predict_against_the_reference(golden, path, monkeypatch):
    g, gp = golden("bcq_train_kat_small.npz"), golden("bcq_predict_kat.npz")
    model, _ = _teacher_forced(g, "small", path, monkeypatch, check=False)
    lab = f"bcq_predict_{path}"
    obs, draw = gp["obs"], th.as_tensor(gp["draw"])
    pol = model.policy
    pol.debug_capture = True
    chosen_q, actions = [], []
    for i in range(len(obs)):
        pol.predict_noise_queue = [draw]
        action, _ = model.predict(obs[i:i + 1], deterministic=bool(i % 2))  # `deterministic` is ignored, as in the reference
        assert action.shape == (1, 2) and not pol.predict_noise_queue
        q1 = pol.last_predict["q1"].cpu().numpy().reshape(-1)
        assert q1.shape == (100,)
        chosen_q.append(q1.max())
        actions.append(action[0])
    want_max = gp["q1"].max(1)
    err = q_err(np.array(chosen_q), want_max, lab)
    print(f"{lab}: chosen q1 vs the reference's maximum {err:.2e}")
    assert err < 1e-5
    top = np.sort(gp["q1"].astype(np.float64), axis=1)
    clear = (top[:, -1] - top[:, -2]) > 4 * strict_bound(lab) * np.abs(top[:, -1])
    assert (~clear).mean() <= 0.15
    np.testing.assert_allclose(np.array(actions)[clear], gp["action"][clear], rtol=1e-4, atol=2e-5)
    # n = 3: [3, A], row i = the n = 1 result for observation i with the same noise rows (candidate row r belongs to observation r % 3)
    gen = th.Generator().manual_seed(11)
    draw3 = th.randn(300, draw.shape[1], generator=gen)
    pol.predict_noise_queue = [draw3]
    a3, _ = model.predict(obs[:3])
    assert a3.shape == (3, 2)
    for i in range(3):
        pol.predict_noise_queue = [draw3[i::3].contiguous()]
        a1, _ = model.predict(obs[i:i + 1])
        np.testing.assert_allclose(a3[i], a1[0], rtol=1e-4, atol=2e-5)
    # without a queued draw the device stream serves: seeded, inside the action bounds
    a, _ = model.predict(obs[:5])
    assert a.shape == (5, 2) and np.isfinite(a).all()


# ------------------------------------------------------------------------------------ hipGraph replay
def _digest(model):
    pol = model.policy
    parts = [pol.vae_arena.flat, pol.pert_arena.flat, pol.critic_arena.flat, pol.vae_target_arena.flat, pol.pert_target_arena.flat,
             pol.critic_target_arena.flat]
    for o in (model.actor.vae_optimizer, model.actor.perturbation_optimizer, model.critic.optimizer):
        parts += [o.exp_avg, o.exp_avg_sq, o.ctl[:1].float()]
    parts += [model.replay_buffer.sampler_stream.float(), model._rng_ctl[:2].float()]
    return [p.detach().clone() for p in parts]


def test_graph_replay_equals_eager():
    from core.bcq import BCQ

    outs = []
    for graph in (False, True):
        model = BCQ("MlpPolicy", _env(), dataset=_synthetic_dataset(), seed=3, batch_size=64, policy_kwargs=dict(critic_net_arch=[64, 64]))
        model.enable_graph_capture(graph)
        model.learn(8)
        th.cuda.synchronize()
        st = model.graph_status()
        assert model._n_updates == 8 and model.num_timesteps == 8
        if graph:
            assert st["active"] and st["replays"] > 0 and st["error"] is None and st["graphs"] == 2, st
            assert set(st["abi_launches_per_iteration"]) == {0, 1}
        else:
            assert st["replays"] == 0
        outs.append(_digest(model))
    for a, b in zip(*outs):
        assert th.equal(a, b)
    # a queued draw keeps the iteration eager
    model.noise_queue = [th.zeros(64, 32)]
    assert not model._graph_eligible(model._noop_callback())
    model.noise_queue = []
    assert model._graph_eligible(model._noop_callback())


# ------------------------------------------------------------------------------------ path selection
def test_path_selection(monkeypatch):
    from core.bcq import BCQ
    from core.common import hip_ops

    calls = {}
    for name in ("bcq_latent_fwd", "bcq_vae_loss", "bcq_latent_bwd", "bcq_expand", "bcq_perturb_fwd", "bcq_perturb_bwd", "bcq_target",
                 "bcq_select", "twin_q_loss", "neg_mean_loss"):
        orig = getattr(hip_ops, name)

        def wrapped(*a, _o=orig, _n=name, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _o(*a, **k)

        monkeypatch.setattr(hip_ops, name, wrapped)
    pk = dict(critic_net_arch=[32, 32])
    model = BCQ("MlpPolicy", _env(), dataset=_synthetic_dataset(), seed=0, batch_size=32, policy_kwargs=pk)
    assert model.fused_learner
    model.train(gradient_steps=2, batch_size=32)  # one actor step
    assert calls == dict(bcq_latent_fwd=2, bcq_vae_loss=2, bcq_latent_bwd=2, bcq_expand=3, bcq_perturb_fwd=3, bcq_perturb_bwd=1, bcq_target=2,
                         twin_q_loss=2, neg_mean_loss=1), calls
    model.predict(np.zeros((1, 4), np.float32))
    assert calls["bcq_select"] == 1 and calls["bcq_expand"] == 4
    calls.clear()
    model.fused_learner = False
    model.train(gradient_steps=2, batch_size=32)
    model.predict(np.zeros((1, 4), np.float32))
    assert not any(k.startswith("bcq_") for k in calls), calls
    # n_critics 1 and 3 and a latent width the kernels decline take the torch statements
    for extra in (dict(n_critics=1), dict(n_critics=3),
                  dict(actor_net_arch=dict(vae_latent_dim=300, vae_hidden_dim=64, perturbation_hidden_dim=64, max_perturbation=0.05))):
        calls.clear()
        m = BCQ("MlpPolicy", _env(), dataset=_synthetic_dataset(), seed=0, batch_size=32, policy_kwargs=dict(pk, **extra))
        assert not m.fused_learner and m.policy.fast is None
        with pytest.raises(ValueError, match="no kernel path"):
            m.fused_learner = True
        n_q = len(m.critic.q_networks)
        assert n_q == extra.get("n_critics", 2)
        if n_q == 3:  # the target is the min over ALL N target critics: push the third one's output far down
            with th.no_grad():
                m.critic_target.q_networks[2][-1].bias.fill_(-1000.0)
        m.debug_capture = True
        m.train(gradient_steps=2, batch_size=32)
        t = m.last_train_tensors
        assert len(t["current_q"]) == n_q and t["actor_loss"] is not None
        for v in (t["critic_loss"], t["vae_loss"], t["actor_loss"], t["target_q"]):
            assert bool(th.isfinite(v).all())
        if n_q == 3:
            alive = m._static_batch.dones[:, 0] == 0
            assert bool((t["target_q"][alive, 0] < -500).all())
        assert not any(k.startswith("bcq_") for k in calls), calls
        assert m.actor.vae_optimizer.step_count == 2 and m.actor.perturbation_optimizer.step_count == 1


# ------------------------------------------------------------------------------------ dataset forms
def test_dataset_forms(tmp_path):
    from core.bcq import BCQ
    from core.sac import SAC

    sac = SAC("MlpPolicy", _env(8), seed=0, batch_size=32, buffer_size=8 * 16, policy_kwargs=dict(net_arch=[32, 32]))
    sac.learn(8 * 10)
    src = sac.replay_buffer
    assert src.n_envs == 8 and src.size() == 10
    pkl = str(tmp_path / "data.pkl")
    sac.save_replay_buffer(pkl)
    npz = str(tmp_path / "data.npz")
    fields = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")
    np.savez(npz, pos=np.int64(src.pos), full=np.uint8(src.full), **{k: getattr(src, k).cpu().numpy() for k in fields})
    pk = dict(critic_net_arch=[32, 32])
    for dataset in (src, pkl, npz):
        m = BCQ("MlpPolicy", _env(), dataset=dataset, seed=0, batch_size=32, policy_kwargs=pk)
        rb = m.replay_buffer
        assert m.n_envs == 1 and rb.n_envs == 8 and rb.size() == 10 and rb.pos == src.pos and rb.full == src.full
        assert rb.buffer_size == src.buffer_size and (dataset is not src or rb is src)
        for k in fields:
            assert th.equal(getattr(rb, k), getattr(src, k)), k
        m.learn(3)
        assert m._n_updates == 3 and m.fused_learner
    # all rows valid when pos / full are absent
    np.savez(npz, **{k: getattr(src, k).cpu().numpy() for k in fields})
    m = BCQ("MlpPolicy", _env(), dataset=npz, seed=0, batch_size=32, policy_kwargs=pk)
    assert m.replay_buffer.size() == src.buffer_size and m.replay_buffer.full
    # refusals
    with pytest.raises(ValueError, match="the model does not support multiple envs"):
        BCQ("MlpPolicy", _env(8), dataset=src)
    from core.common.buffers import ReplayBuffer

    with pytest.raises(ValueError, match="Loaded dataset is empty"):
        BCQ("MlpPolicy", _env(), dataset=ReplayBuffer(64, *_spaces(), device=DEV, n_envs=1))
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, observations=np.zeros((4, 1, 4)))
    with pytest.raises(ValueError, match="Dataset loading failed. Error type: ValueError, Message: .*missing arrays"):
        BCQ("MlpPolicy", _env(), dataset=bad)
    with pytest.raises(FileNotFoundError):
        BCQ("MlpPolicy", _env(), dataset=str(tmp_path / "nothing.pkl"))


# ------------------------------------------------------------------------------------ learn(), callbacks, checkpoints
class _Dumps:
    def __init__(self):
        self.rows = []

    def write(self, vals, excluded, step):
        self.rows.append((step, dict(vals)))


def _small_model(**kw):
    from core.bcq import BCQ

    kw.setdefault("policy_kwargs", dict(critic_net_arch=[32, 32]))
    return BCQ("MlpPolicy", _env(), dataset=_synthetic_dataset(), seed=1, batch_size=32, **kw)


def test_learn_counters_logs_callback_and_warmup():
    from core.common.callbacks import BaseCallback
    from core.common.logger import Logger

    model = _small_model()
    dumps = _Dumps()
    model.set_logger(Logger(output_formats=[dumps]))
    assert model.learn(8, log_interval=4) is model
    assert model.num_timesteps == 8 and model._n_updates == 8 and [s for s, _ in dumps.rows] == [4, 8]
    want = {"time/fps", "time/time_elapsed", "time/total_timesteps", "dataset/size", "training/bc_warmup_steps", "training/conservative_weight",
            "train/n_updates", "train/actor_loss", "train/critic_loss", "train/vae_loss", "train/learning_rate"}
    for step, row in dumps.rows:
        assert set(row) == want, (step, sorted(row))
        assert row["dataset/size"] == 512 and row["training/bc_warmup_steps"] == 0 and row["training/conservative_weight"] == 0.0
        assert row["train/n_updates"] == step and row["time/total_timesteps"] == step and row["train/learning_rate"] == 3e-4
        assert all(np.isfinite(float(row[k])) for k in ("train/actor_loss", "train/critic_loss", "train/vae_loss"))
    with pytest.warns(UserWarning, match="do not collect rollouts"):
        assert model.collect_rollouts(model.env, None, None, model.replay_buffer) is None

    class Stop(BaseCallback):
        def _on_step(self):
            return self.n_calls < 3

    stopped = _small_model()
    stopped.learn(8, callback=Stop())
    assert stopped.num_timesteps == 3 and stopped._n_updates == 3
    # gradient_steps > 1: counters and the running sums
    multi = _small_model(gradient_steps=3)
    multi.learn(2)
    assert multi.num_timesteps == 2 and multi._n_updates == 6 and multi.actor.perturbation_optimizer.step_count == 3
    # behavior_cloning_warmup is accepted and changes nothing (the reference's methods are `pass`)
    outs = []
    for warm in (0, 5):
        m = _small_model(behavior_cloning_warmup=warm)
        m.learn(4)
        assert m.behavior_cloning_warmup == warm and m.n_eval_episodes == 10 and m.conservative_weight == 0.0
        outs.append([p.detach().clone() for p in m.policy.parameters()])
    for a, b in zip(*outs):
        assert th.equal(a, b)


def test_checkpoint_round_trip_continues_identically(tmp_path):
    import zipfile

    from core.bcq import BCQ

    model = _small_model()
    model.learn(5)
    path = str(tmp_path / "bcq_ckpt")
    model.save(path)
    with zipfile.ZipFile(path + ".zip") as z:
        names = set(z.namelist())
    assert {"data", "policy.pth", "actor.vae_optimizer.pth", "actor.perturbation_optimizer.pth", "critic.optimizer.pth"} <= names
    sd = model.actor.vae_optimizer.state_dict()
    assert sd["param_groups"][0]["params"] == list(range(14)) and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    clone = BCQ.load(path, env=_env(), dataset=_synthetic_dataset())
    assert clone._n_updates == 5 and clone.num_timesteps == 5 and clone.actor_delay == 2 and clone.faithful_quirks and clone.fused_learner
    assert list(clone.policy.state_dict()) == list(model.policy.state_dict())
    for a, b in zip(model.policy.state_dict().values(), clone.policy.state_dict().values()):
        assert th.equal(a, b)
    for name in ("vae_optimizer", "perturbation_optimizer"):
        o, c = getattr(model.actor, name), getattr(clone.actor, name)
        assert o.step_count == c.step_count and th.equal(o.exp_avg, c.exp_avg) and th.equal(o.exp_avg_sq, c.exp_avg_sq)
    assert model.critic.optimizer.step_count == clone.critic.optimizer.step_count == 5
    outs = []
    for m in (model, clone):  # the same sampler stream and device noise stream from here on: identical updates
        m.set_random_seed(7)
        m.replay_buffer.seed_sampler(99)
        m.train(gradient_steps=3, batch_size=32)
        outs.append([p.detach().clone() for p in m.policy.parameters()])
    for a, b in zip(*outs):
        assert th.equal(a, b)
    # a path dataset is stored and read again by load() without dataset=
    pkl = str(tmp_path / "data.pkl")
    model.save_replay_buffer(pkl)
    m2 = BCQ("MlpPolicy", _env(), dataset=pkl, seed=1, batch_size=32, policy_kwargs=dict(critic_net_arch=[32, 32]))
    m2.save(path + "2")
    again = BCQ.load(path + "2", env=_env())
    assert again.dataset == pkl and again.replay_buffer.size() == 512


# ------------------------------------------------------------------------------------ it learns the behaviour it was given
def test_bcq_learns_the_behaviour_policy():
    """A check of sign and wiring errors that needs no claim about rewards: actions = clip(tanh(obs K) + N(0, 0.05)); after
    learn(1000) at the class defaults predict() is within 0.2 (mean absolute error) of tanh(obs K). The unmodified reference reaches
    0.087 / 0.084 / 0.080 (CPU, seeds 0, 1, 2), an untrained policy 0.42-0.44, uniform-random actions 0.64."""
    from core.bcq import BCQ
    from core.common.buffers import ReplayBuffer

    rng = np.random.default_rng(0)
    rows = 20_000
    K = rng.normal(0, 0.8, (4, 2))
    obs = rng.uniform(-1, 1, (rows, 4))
    act = np.clip(np.tanh(obs @ K) + rng.normal(0, 0.05, (rows, 2)), -1, 1)
    nobs = np.clip(obs + rng.normal(0, 0.05, (rows, 4)), -1, 1)
    rb = ReplayBuffer(rows, *_spaces(), device=DEV, n_envs=1)
    f = lambda a, *sh: th.as_tensor(a.astype(np.float32)).reshape(*sh)  # noqa: E731
    rb.observations.copy_(f(obs, rows, 1, 4)), rb.next_observations.copy_(f(nobs, rows, 1, 4)), rb.actions.copy_(f(act, rows, 1, 2))
    rb.rewards.copy_(f(rng.uniform(-8, 0, rows), rows, 1)), rb.dones.copy_(f((rng.uniform(size=rows) < 0.05).astype(np.float64), rows, 1))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    model = BCQ("MlpPolicy", _env(), dataset=rb, seed=0)
    assert model.fused_learner and model.batch_size == 256
    test_obs = rng.uniform(-1, 1, (200, 4)).astype(np.float32)

    def score():
        pred = np.concatenate([model.policy.scale_action(model.predict(test_obs[i:i + 1])[0]) for i in range(len(test_obs))])
        return float(np.abs(pred - np.tanh(test_obs @ K)).mean())

    before = score()
    model.learn(1000)
    after = score()
    print(f"behaviour cloning error: untrained {before:.3f}, after learn(1000) {after:.3f}")
    assert model._n_updates == 1000
    assert after < 0.2, f"mean |predict - tanh(obs K)| = {after:.3f} after learn(1000) (untrained {before:.3f}; the reference reaches 0.080-0.087)"
