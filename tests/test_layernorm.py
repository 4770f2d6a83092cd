"""LayerNorm / dropout critics on the MI355X (csrc/cstr_layernorm.hip): the two row-owning kernels against the torch statement in float64
on the CPU, the dropout stream, and SAC's / TD3's first gradient step and graph replay with such critics.

The bar, per output tensor: max |kernel - fp64| <= 4 x max |float32 ATen on the CPU - fp64| (equal where ATen's figure is 0).
Measured worst ratios (profiles/layernorm_gpu_tests.txt): bwd dbeta 1.88, bwd dgamma 1.53, bwd gz 1.76, fwd rstd 3.23, fwd xhat 2.26, fwd y 2.57, step critic_loss 3.92, step grad W/b 3.28, step grad gamma/beta 2.46, step q 1.67, step target_q 1.39.
"""
import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

from _sentinel_bufs import DEV, Bufs

pytestmark = pytest.mark.gpu

RELU, TANH = 1, 2
# (G, M, K, N): one row, one tile | row tail | fewer columns than waves x 16, column tail inside the only tile | column tail across waves,
# odd G | TD3's layer | the cap | SAC's layer with a shared 2-D input | a row of identical pre-activations, strided x
SHAPES = [(1, 1, 6, 16), (2, 17, 6, 64), (2, 16, 12, 20), (3, 48, 64, 300), (2, 32, 400, 300), (2, 16, 256, 512), (1, 33, 256, 256), (2, 16, 8, 64)]
CASES = [(s, p, RELU) for s in SHAPES for p in (0.0, 0.1)] + [((3, 48, 64, 300), 0.1, TANH)]


def within(name, kernel, ref64, aten32):
    """the 4 x rule, measured against the reference"""
    ek = float((kernel.detach().cpu().double() - ref64).abs().max())
    ea = float((aten32.double() - ref64).abs().max())
    print(f"{name}: kernel {ek:.3e} aten {ea:.3e}")
    assert ek <= 4.0 * ea, f"{name}: kernel error {ek:.3e} above 4 x ATen's {ea:.3e}"


def act_fn(v, act):
    return th.relu(v) if act == RELU else th.tanh(v)


def layer_from_z(z, gamma, beta, keep, p, act):
    """the statement behind the Linear, in the dtype of its operands: (y, xhat, rstd, z)"""
    n = z.shape[-1]
    d = z * keep / (1.0 - p)
    y = act_fn(th.stack([F.layer_norm(d[g], (n,), gamma[g], beta[g], eps=1e-5) for g in range(z.shape[0])]), act)
    return y, F.layer_norm(d, (n,), eps=1e-5), 1.0 / th.sqrt(d.var(-1, unbiased=False) + 1e-5), z


def layer(x, w, b, gamma, beta, keep, p, act):
    z = th.stack([F.linear(x[g] if x.dim() == 3 else x, w[g], b[g]) for g in range(w.shape[0])])
    return layer_from_z(z, gamma, beta, keep, p, act)


def operands(shape, p, seed=0):
    G, M, K, N = shape
    gen = th.Generator().manual_seed(seed + 7 * N + M)
    r = lambda *s: th.randn(*s, generator=gen)  # noqa: E731
    shared = shape == (1, 33, 256, 256)
    wide = r(M, K + 3) if shared else r(G, M, K + 3)
    if shape == (2, 16, 8, 64):
        wide[0, 3] = 0.0  # with a constant bias: a row of identical pre-activations
    x = wide[..., :K] if shape == (2, 16, 8, 64) else wide[..., :K].contiguous()
    w, b = r(G, N, K) / np.sqrt(K), r(G, N) * 0.1
    if shape == (2, 16, 8, 64):
        b[0] = 0.5
    gamma, beta = 1.0 + 0.1 * r(G, N), 0.1 * r(G, N)
    u = th.rand(G, M, N, generator=gen)
    keep = (u >= np.float32(p)).float() if p > 0 else th.ones(G, M, N)
    return x, w, b, gamma, beta, u, keep


@pytest.mark.parametrize("shape,p,act", CASES)
def test_forward(shape, p, act):
    from core.common import hip_ops

    G, M, K, N = shape
    x, w, b, gamma, beta, u, keep = operands(shape, p)
    ref = layer(*(t.double() for t in (x, w, b, gamma, beta, keep)), p, act)
    aten = layer(x, w, b, gamma, beta, keep, p, act)
    bufs = Bufs()
    out = (bufs.new("y", G, M, N), bufs.new("xhat", G, M, N), bufs.new("rstd", G, M))
    xd = x.to(DEV) if x.is_contiguous() else x._base.to(DEV)[..., :K]  # the strided case keeps its row stride K + 3
    args = [t.to(DEV) for t in (w, b, gamma, beta)]
    for _ in range(2):
        hip_ops.linear_ln_act_fwd(xd, *args, act, p, u_in=u.to(DEV) if p > 0 else None, out=out)
    bufs.check(written=("y", "xhat", "rstd"))
    for name, k, r64, a32 in zip(("y", "xhat", "rstd"), out, ref, aten):
        within(f"fwd {name}", k, r64, a32)
    if shape == (2, 16, 8, 64) and p == 0:
        assert abs(float(out[2][0, 3]) - 1e-5 ** -0.5) <= 1e-3  # variance 0: rstd = 1 / sqrt(eps)


def backward_ref(z, gamma, beta, keep, p, act, w_next, gz_next):
    z, gamma, beta = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    layer_from_z(z, gamma, beta, keep, p, act)[0].backward(th.bmm(gz_next, w_next))
    return z.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("shape,p,act", CASES)
@pytest.mark.parametrize("head", [False, True])
def test_backward(shape, p, act, head):
    from core.common import hip_ops

    G, M, K, N = shape  # K: the consumer's width (1 with `head`, the scalar Q head)
    Nn = 1 if head else K
    x, w, b, gamma, beta, u, keep = operands(shape, p)
    gen = th.Generator().manual_seed(N + Nn)
    w_next, gz_next = th.randn(G, Nn, N, generator=gen) / np.sqrt(N), th.randn(G, M, Nn, generator=gen) / M
    z32 = layer(*(t.double() for t in (x, w, b, gamma, beta, keep)), p, act)[3].float()  # both evaluations start from the same float32 pre-activations
    ref = backward_ref(z32.double(), gamma.double(), beta.double(), keep.double(), p, act, w_next.double(), gz_next.double())
    aten = backward_ref(z32, gamma, beta, keep, p, act, w_next, gz_next)
    y64, xhat64, rstd64, _ = layer_from_z(z32.double(), gamma.double(), beta.double(), keep.double(), p, act)
    bufs = Bufs()
    gz, dg, db = bufs.new("gz", G, M, N), bufs.new("dgamma", G, N), bufs.new("dbeta", G, N)
    n_parts = G * ((M + 15) // 16) * 2 * N
    parts_flat = th.full((n_parts + 64,), -6.0e23, dtype=th.float64, device=DEV)
    for _ in range(2):  # y, xhat, rstd are data: the fp64 forward rounded to float32, so no ReLU mask can flip
        hip_ops.ln_linear_bwd_input(gz_next.to(DEV), w_next.to(DEV), y64.float().to(DEV), xhat64.float().to(DEV), rstd64.float().to(DEV),
                                    gamma.to(DEV), act, p, u_in=u.to(DEV) if p > 0 else None, parts=parts_flat[:n_parts], dgamma=dg, dbeta=db,
                                    out=gz)
    bufs.check(written=("gz", "dgamma", "dbeta"))
    assert bool((parts_flat[n_parts:] == -6.0e23).all()) and not bool((parts_flat[:n_parts] == -6.0e23).any())
    for name, k, r64, a32 in zip(("gz", "dgamma", "dbeta"), (gz, dg, db), ref, aten):
        within(f"bwd {name}", k, r64, a32)


def test_dropout_stream():
    """the stream == the uniforms cstr_ln_dropout_uniform_f32 writes for it, forward and backward; consecutive passes differ"""
    from core import _native as nv
    from core.common import hip_ops

    shape, p = (2, 17, 12, 300), 0.1
    G, M, K, N = shape
    x, w, b, gamma, beta, _, _ = (t.to(DEV) for t in operands(shape, p))
    ctl = th.zeros(nv.RNG_CTL_WORDS, dtype=th.int64, device=DEV)
    ctl[0], ctl[1] = 1234, 5
    word = th.zeros(1, dtype=th.int64, device=DEV)
    u = hip_ops.ln_dropout_uniform(ctl, G, M, N, layer=1)
    a = hip_ops.linear_ln_act_fwd(x, w, b, gamma, beta, RELU, p, rng_ctl=ctl, advance=True, pass_out=word, layer=1)
    c = hip_ops.linear_ln_act_fwd(x, w, b, gamma, beta, RELU, p, u_in=u, layer=1)
    assert all(th.equal(s, t) for s, t in zip(a, c)) and int(word) == 5 and ctl.tolist()[:3] == [1234, 6, 0]
    gz_next, w_next = th.randn(G, M, 1, device=DEV), th.randn(G, 1, N, device=DEV)
    g1 = hip_ops.ln_linear_bwd_input(gz_next, w_next, *a, gamma, RELU, p, rng_ctl=ctl, pass_ctr=word, layer=1)
    g2 = hip_ops.ln_linear_bwd_input(gz_next, w_next, *a, gamma, RELU, p, u_in=u, layer=1)
    assert th.equal(g1, g2) and th.equal(hip_ops.ln_dropout_uniform(ctl, G, M, N, layer=1, pass_ctr=word), u)
    u2 = hip_ops.ln_dropout_uniform(ctl, G, M, N, layer=1)  # the next pass
    assert not th.equal(u2 >= p, u >= p) and bool(((u >= 0) & (u < 1)).all())
    kept, n = float((u >= p).float().mean()), G * M * N
    assert abs(kept - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)


def make_model(algo, n_critics=2, p=0.0, seed=1, **kw):
    from core import SAC, TD3
    from core.common.vec_env import CSTRVecEnv

    cls = SAC if algo == "sac" else TD3
    return cls("MlpPolicy", CSTRVecEnv(32, device=DEV), seed=seed, batch_size=32, buffer_size=32 * 16, learning_starts=64, device=DEV,
               policy_kwargs=dict(net_arch=[64, 64], n_critics=n_critics, layer_norm=True, dropout_rate=p), **kw)


def first_step(algo, n_critics):
    """(model, the batch, CPU copies of critic and target from before the step) of the kernel path's first gradient step at p = 0"""
    import copy

    model = make_model(algo, n_critics)
    assert model.fused_learner and type(model._fast_critic).__name__ == "FastLnCritic" and model._chain_for(32) is None
    model.learn(32 * 3)  # fills the buffer; training starts behind it
    th.cuda.synchronize()
    before = [copy.deepcopy(m).cpu() for m in (model.critic, model.critic_target)]
    seen, sample = {}, model._sample
    model._sample = lambda *a, **k: seen.setdefault("batch", sample(*a, **k))
    if algo == "sac":  # (x_pi, log_prob, x_next, next_log_prob) of the 2B-row actor pass
        pair = model._fast_actor.action_log_prob_pair
        model._fast_actor.action_log_prob_pair = lambda *a, **k: seen.setdefault("pair", pair(*a, **k))
    model.debug_capture = True
    model.policy.set_training_mode(True)
    model._train_device_only(1, 32)
    th.cuda.synchronize()
    return model, seen, before


@pytest.mark.parametrize("n_critics", [2, 3])
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_first_gradient_step(algo, n_critics):
    """against fp64 autograd of the same modules: Q values, critic loss (at the step's own target; the target itself: next test) and
    every critic gradient, d gamma / d beta included"""
    import copy

    model, seen, (critic32, _) = first_step(algo, n_critics)
    rd = seen["batch"][2]
    critic64, cap = copy.deepcopy(critic32).double(), model.last_train_tensors
    obs, act = rd.observations.detach().cpu(), rd.actions.detach().cpu()
    target_k, scale = cap["target_q"].cpu(), 0.5 if algo == "sac" else 1.0

    def step(critic, dt):
        qs = critic(obs.to(dt), act.to(dt))
        loss = scale * sum(F.mse_loss(q, target_k.to(dt)) for q in qs)
        loss.backward()
        return qs, loss, [p.grad for p in critic.parameters()]

    qs64, loss64, grads64 = step(critic64, th.float64)
    qs32, loss32, grads32 = step(critic32, th.float32)
    # no float32 path within the bar can flip a ReLU mask: the smallest |LN output * gamma + beta| of the reference against the row's scale
    pre, x = [], th.cat([obs, act], 1).double()
    with th.no_grad():
        for q in critic64.q_networks:
            h = x
            for m in q:
                h = m(h)
                if isinstance(m, th.nn.LayerNorm):
                    pre.append(float((h.abs().min(-1).values / h.abs().max(-1).values).min()))
    assert min(pre) > 64 * 2.0 ** -24
    for i in range(n_critics):
        within(f"step q{i}", cap["current_q"][i], qs64[i].detach(), qs32[i].detach())
    within("step critic_loss", cap["critic_loss"].reshape(()), loss64.detach(), loss32.detach())
    for (name, p), g64, g32 in zip(model.critic.named_parameters(), grads64, grads32):
        within(f"step grad {name.split('.', 1)[1]}", p.grad, g64, g32)


@pytest.mark.parametrize("n_critics", [2, 3])
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_td_target_and_soft_update_of_first_step(algo, n_critics):
    """the target critics' pass: the TD target (SAC: with the entropy term) against fp64 of the same modules at the kernel path's own
    next actions and log-probs; then every target parameter, LayerNorm's included, against the soft update's statement"""
    import copy

    model, seen, (_, t32) = first_step(algo, n_critics)
    (pb, _, rd), cap, t64 = seen["batch"], model.last_train_tensors, copy.deepcopy(t32).double()
    x_next, rew, done = pb.x_next.detach().cpu(), rd.rewards.cpu(), rd.dones.cpu()
    ent = float(cap["ent_coef"]) * seen["pair"][3].detach().cpu().reshape(-1, 1).double() if algo == "sac" else 0.0

    def target(critic, dt):
        q = th.cat([q(x_next.to(dt)) for q in critic.q_networks], 1).min(1, keepdim=True).values
        return rew.to(dt) + (1 - done.to(dt)) * model.gamma * (q - (ent.to(dt) if algo == "sac" else 0.0))

    with th.no_grad():
        within("step target_q", cap["target_q"], target(t64, th.float64), target(t32, th.float32))
    # TD3 updates its targets with the delayed policy step only (learn() above has run a train() call of its own)
    tau = model.tau if algo == "sac" or (model._n_updates + 1) % model.policy_delay == 0 else 0.0
    for (k, before), after, src in zip(t32.named_parameters(), model.critic_target.parameters(), model.critic.parameters()):
        want = (1 - tau) * before.double() + tau * src.detach().cpu().double()
        assert float((after.detach().cpu().double() - want).abs().max()) <= 2.0 ** -22 * max(1.0, float(want.abs().max())), k


@pytest.mark.parametrize("n_critics,unroll", [(2, 1), (1, 4)])
def test_replay_equals_eager(n_critics, unroll):
    """20 iterations with gradient_steps = 4 and p = 0.01: replayed from a hipGraph (1 and 4 iterations per graph; two critics, and one on
    a G = 1 stack) == eager, bit for bit; finite losses; the targets' LayerNorm parameters have moved"""
    runs = []
    for graph in (False, True):
        m = make_model("sac", n_critics, p=0.01, gradient_steps=4)
        if graph:
            m.enable_graph_capture(True, unroll=unroll)
        m.learn(32 * (2 + 20))
        th.cuda.synchronize()
        if graph:
            st = m.graph_status()
            assert st["replays"] > 0 and st["error"] is None
        runs.append(m)
    eager, replayed = runs
    for a, b in zip(eager.policy.parameters(), replayed.policy.parameters()):
        assert th.equal(a, b)
    assert all(bool(th.isfinite(v).all()) for v in eager._loss_sums.values()) and eager._n_updates == 80
    assert int(eager._fast_critic.rng_ctl[1]) == 3 * 80  # three critic passes per gradient step, each with a draw of its own
    for q in eager.critic_target.q_networks:
        assert not th.equal(q[2].weight, th.ones_like(q[2].weight)) and not th.equal(q[2].bias, th.zeros_like(q[2].bias))


def test_refusals(monkeypatch):
    import core
    from core.common import distributed as dist_util
    from core.common.vec_env import CSTRVecEnv

    env = lambda **k: CSTRVecEnv(4, device=DEV, **k)  # noqa: E731
    keys = dict(layer_norm=True, dropout_rate=0.01)
    kw = lambda: dict(policy_kwargs=dict(keys), device=DEV)  # noqa: E731  (a constructor may add keys of its own to the dict)
    with pytest.raises(ValueError, match="gSDE"):
        core.SAC("MlpPolicy", env(), use_sde=True, **kw())
    for cls in (core.SAC, core.TD3):
        with pytest.raises(ValueError, match="goal face"):
            cls("MultiInputPolicy", env(goal_conditioned=True, goal_range=(0.1, 0.4)), replay_buffer_class=core.HerReplayBuffer, **kw())
    with pytest.raises(ValueError, match="dropout_rate"):
        core.SAC("MlpPolicy", env(), policy_kwargs=dict(layer_norm=True, dropout_rate=1.0), device=DEV)
    dataset = core.SAC("MlpPolicy", env(), device=DEV).replay_buffer
    for name in ("BCQ", "TD3BC", "CQL", "IQL"):  # the offline classes look at their dataset first
        with pytest.raises(ValueError, match="layer_norm / dropout_rate"):
            getattr(core, name)("MlpPolicy", CSTRVecEnv(1, device=DEV), dataset=dataset, **kw())
    with pytest.raises(ValueError, match="layer_norm / dropout_rate"):
        core.ARS("MlpPolicy", env(), **kw())
    for name in ("MADDPG", "IDDPG"):
        with pytest.raises(ValueError, match="layer_norm / dropout_rate"):
            getattr(core, name)(2, "MlpPolicy", env(), [[0, 1], [2, 3]], [[0], [1]], learning_rate_list=[1e-3, 1e-3], **kw())
    torch_path = core.SAC("MlpPolicy", env(), policy_kwargs=dict(dropout_rate=0.1), device=DEV)  # dropout without LayerNorm
    assert not torch_path.fused_learner and torch_path._chain_for(32) is None
    monkeypatch.setattr(dist_util, "rank_world", lambda: (0, 2))
    for cls in (core.SAC, core.TD3):
        with pytest.raises(ValueError, match="data-parallel"):
            cls("MlpPolicy", env(), **kw())
