"""CPU-side checks of TD3+BC: the two cstr_td3bc_* entry points are exported and reject bad arguments on the host (nothing is
dereferenced or launched), `from core import TD3BC` resolves with the documented constructor, the policy has TD3Policy's state_dict
and seeded initial weights, the refusals that need no device, and the reference statements of tests/_td3bc_reference.py: the explicit
gradients against fp64 autograd, the comparator against the mistakes a wrong implementation makes, the normalisation statistics and
the folded first layer."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch as th

import _td3bc_reference as ref
from core import _native as nv

i64, f32 = C.c_int64, C.c_float
null = C.c_void_p(None)
P = lambda a: C.c_void_p(a)  # noqa: E731
Q, PI, ACT, GQ, LOUT, LSUM, AUX = 0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000, 0x5000100, 0x5000200
BAD, UNSUP = -1, -2


def test_symbols_declared_and_exported():
    lib = nv.lib()
    names = [s for s in nv.SYMBOLS if s.startswith("cstr_td3bc_")]
    assert sorted(names) == ["cstr_td3bc_act_bwd_rows_f32", "cstr_td3bc_actor_loss_f32"]
    assert all(hasattr(lib, n) for n in names)
    assert (nv.TD3BC_MAX_BATCH, nv.TD3BC_MAX_ACT) == (16384, 8)


def test_actor_loss_rejects_bad_arguments_on_the_host():
    lib = nv.lib()

    def loss(q=Q, pi=PI, act=ACT, gq=GQ, lout=LOUT, lsum=LSUM, aux=AUX, alpha=2.5, batch=256, a=2, ldpi=6, ldact=6):
        return lib.cstr_td3bc_actor_loss_f32(P(q), P(pi), i64(ldpi), P(act), i64(ldact), f32(alpha), P(gq), P(lout), P(lsum), P(aux), i64(batch),
                                             C.c_int(a), null)

    assert loss(q=None) == BAD and loss(pi=None) == BAD and loss(act=None) == BAD and loss(gq=None) == BAD
    assert loss(batch=0) == BAD and loss(batch=-3) == BAD and loss(batch=nv.TD3BC_MAX_BATCH + 1) == UNSUP
    assert loss(a=0) == BAD and loss(a=-1) == BAD and loss(a=nv.TD3BC_MAX_ACT + 1, ldpi=16, ldact=16) == UNSUP
    assert loss(ldpi=1) == BAD and loss(ldact=1) == BAD
    for k in ("q", "pi", "act", "gq", "lout", "lsum", "aux"):  # rows off a 4-byte boundary
        base = dict(q=Q, pi=PI, act=ACT, gq=GQ, lout=LOUT, lsum=LSUM, aux=AUX)[k]
        assert loss(**{k: base + 2}) == BAD, k
    assert loss(alpha=-0.5) == BAD and loss(alpha=float("nan")) == BAD
    # outputs over inputs
    assert loss(gq=Q) == BAD and loss(gq=Q + 4 * 255) == BAD and loss(gq=PI + 4 * 100) == BAD and loss(gq=ACT) == BAD
    assert loss(lout=Q + 8) == BAD and loss(lsum=PI) == BAD and loss(aux=ACT + 4 * (255 * 6 + 1)) == BAD
    # outputs over each other
    assert loss(lout=GQ + 4) == BAD and loss(lsum=LOUT) == BAD and loss(aux=LOUT - 8) == BAD and loss(aux=GQ + 4 * 255) == BAD
    assert loss(aux=LSUM - 4) == BAD


def test_act_bwd_rows_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    GY, Y, A, GZ = 0x1000000, 0x2000000, 0x3000000, 0x4000000

    def bwd(gy=GY, y=Y, act=A, gz=GZ, m=256, n=2, ldg=6, ldy=6, lda=6, kind=2, coef=0.004):
        return lib.cstr_td3bc_act_bwd_rows_f32(P(gy), i64(ldg), P(y), i64(ldy), P(act), i64(lda), f32(coef), C.c_int(kind), P(gz), i64(m), i64(n),
                                               null)

    assert bwd(gy=None) == BAD and bwd(y=None) == BAD and bwd(act=None) == BAD and bwd(gz=None) == BAD
    assert bwd(y=None, kind=0) == BAD  # the cloning term needs y whatever the activation
    assert bwd(m=0) == BAD and bwd(n=0) == BAD and bwd(m=-1) == BAD
    assert bwd(ldg=1) == BAD and bwd(ldy=1) == BAD and bwd(lda=1) == BAD
    assert bwd(gy=GY + 1) == BAD and bwd(y=Y + 2) == BAD and bwd(act=A + 3) == BAD and bwd(gz=GZ + 2) == BAD
    assert bwd(kind=3) == UNSUP and bwd(kind=-1) == UNSUP and bwd(m=1 << 31) == UNSUP
    assert bwd(gz=GY) == BAD and bwd(gz=Y + 4 * 6 * 255) == BAD and bwd(gz=A + 8) == BAD and bwd(gz=GY - 4 * 511) == BAD


def test_hip_ops_wrappers_refuse_cpu_tensors():
    from core.common import hip_ops

    z = th.zeros
    with pytest.raises(ValueError, match="device"):
        hip_ops.td3bc_actor_loss(z(8, 1), z(8, 2), z(8, 2), 2.5, z(8, 1))
    with pytest.raises(ValueError, match="device|No CPU fallback"):
        hip_ops.td3bc_act_bwd_rows(z(8, 2), z(8, 2), z(8, 2), 0.1, 2, z(8, 2))
    assert hip_ops.td3bc_supported(256, 2) and hip_ops.td3bc_supported(16384, 8)
    assert not hip_ops.td3bc_supported(16385, 2) and not hip_ops.td3bc_supported(256, 9) and not hip_ops.td3bc_supported(0, 2)


def test_from_core_import_td3bc_and_signature():
    import core
    from core import TD3BC
    from core.common.offline_policy_algorithm import OfflineAlgorithm
    from core.td3bc import TD3BC as T2

    assert TD3BC is T2 and "TD3BC" in core.__all__ and issubclass(TD3BC, OfflineAlgorithm)
    assert TD3BC.policy_aliases["MlpPolicy"].__name__ == "TD3BCPolicy" and list(TD3BC.policy_aliases) == ["MlpPolicy"]
    sig = inspect.signature(TD3BC.__init__)
    got = [(k, p.default) for k, p in sig.parameters.items() if k not in ("self", "policy", "env")][:13]
    assert got == [("learning_rate", 1e-3), ("dataset", None), ("buffer_size", 1_000_000), ("batch_size", 256), ("tau", 0.005), ("gamma", 0.99),
                   ("gradient_steps", 1), ("policy_delay", 2), ("target_policy_noise", 0.2), ("target_noise_clip", 0.5), ("alpha", 2.5),
                   ("normalize_states", True), ("behavior_cloning_warmup", 0)]
    rest = dict((k, p.default) for k, p in sig.parameters.items())
    assert rest["n_eval_episodes"] == 10 and rest["policy_kwargs"] is None and rest["seed"] is None and rest["device"] == "auto"
    assert rest["_init_setup_model"] is True and "actor_delay" not in rest and "faithful_quirks" not in rest
    assert not TD3BC.goal_face_support and TD3BC.chain_type is None


def test_policy_keys_and_seeded_init_equal_td3policy():
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.td3.policies import TD3Policy
    from core.td3bc.policies import TD3BCPolicy

    pols = []
    for cls in (TD3BCPolicy, TD3Policy):
        set_random_seed(0)
        pols.append(cls(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 1e-3))
    a, b = (p.state_dict() for p in pols)
    assert list(a) == list(b) and len(a) == 36 and list(a)[0] == "actor.mu.0.weight" and list(a)[-1] == "critic_target.qf1.4.bias"
    assert all(th.equal(a[k], b[k]) for k in a)
    assert pols[0].actor_arch == [400, 300] and isinstance(pols[0], TD3Policy)
    # the policy normalises what it is asked to act on, and refuses to act without its statistics
    pol = pols[0]
    obs = th.linspace(-1, 1, 12).reshape(3, 4)
    raw = pol._predict(obs)
    pol.normalize_states, pol.obs_norm = True, (th.tensor([0.1, -0.2, 0.3, 0.0]), th.tensor([0.5, 2.0, 1.0, 0.25]))
    assert th.equal(pol._predict(obs), pol.actor((obs - pol.obs_norm[0]) / pol.obs_norm[1])) and not th.equal(pol._predict(obs), raw)
    pol.obs_norm = None
    with pytest.raises(RuntimeError, match="statistics are missing"):
        pol._predict(obs)


def test_refusals_that_need_no_device(tmp_path):
    from core import TD3BC

    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'int'>"):
        TD3BC("MlpPolicy", None, dataset=5)
    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'NoneType'>"):
        TD3BC("MlpPolicy", None)
    with pytest.raises(FileNotFoundError, match="Dataset file not found"):
        TD3BC("MlpPolicy", None, dataset=str(tmp_path / "missing.pkl"))
    with pytest.raises(ValueError, match="does not support gSDE"):
        TD3BC("MlpPolicy", None, dataset=5, policy_kwargs=dict(use_sde=True))
    with pytest.raises(ValueError, match="alpha must be a non-negative number"):
        TD3BC("MlpPolicy", None, dataset=5, alpha=-1.0)
    with pytest.raises(ValueError, match="alpha must be a non-negative number"):
        TD3BC("MlpPolicy", None, dataset=5, alpha=float("nan"))
    np.savez(str(tmp_path / "d.npz"), observations=np.zeros((4, 1, 4)))
    with pytest.raises(ValueError, match="needs `env`"):
        TD3BC("MlpPolicy", None, dataset=str(tmp_path / "d.npz"))


# ---- the reference statements ------------------------------------------------------------------------------------------------------
def _case(sign: str, B: int = 37, A: int = 2, seed: int = 0):
    """z, actions, a frozen linear critic (c, e) whose q = tanh(z) . c + e is all negative / all positive / mixed"""
    rng = np.random.default_rng(seed)
    z, a, c = rng.normal(0, 0.8, (B, A)), rng.uniform(-1, 1, (B, A)), rng.normal(0, 0.7, A)
    e = rng.normal(0, 1.0, B) + dict(negative=-6.0, positive=6.0, mixed=0.0)[sign]
    q = np.tanh(z) @ c + e
    assert dict(negative=(q < 0).all(), positive=(q > 0).all(), mixed=(q < 0).any() and (q > 0).any())[sign]
    return z, a, c, e


@pytest.mark.parametrize("sign", ["negative", "positive", "mixed"])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_explicit_gradients_equal_fp64_autograd(sign, A):
    z, a, c, e = _case(sign, A=A)
    s = ref.last_layer_step(z, a, c, e, 2.5)
    np.testing.assert_allclose(s["gz"], s["gz_autograd"], rtol=1e-12, atol=1e-15)
    assert ref.same_step(dict(s, gz=s["gz_autograd"]), s, rtol=1e-11)
    # the loss-level statement and its gq / g_pi
    pi = np.tanh(z)
    q = pi @ c + e
    L = ref.actor_loss_f64(q, pi, a, 2.5)
    assert abs(L["loss"] - s["loss"]) < 1e-13 * max(1.0, abs(s["loss"])) and abs(L["lam"] - s["lam"]) < 1e-13 * s["lam"]
    qt, pt = th.tensor(q, requires_grad=True), th.tensor(pi, requires_grad=True)
    lam = 2.5 / qt.abs().mean().detach()
    (-lam * qt.mean() + ((pt - th.tensor(a)) ** 2).mean()).backward()
    np.testing.assert_allclose(L["gq"], qt.grad.numpy(), rtol=1e-13)
    np.testing.assert_allclose(L["g_pi"], pt.grad.numpy(), rtol=1e-13, atol=1e-18)
    # the chain the kernels compute: gz = (gq c + g_pi) * (1 - pi^2)
    np.testing.assert_allclose((L["gq"][:, None] * c[None, :] + L["g_pi"]) * (1 - pi * pi), s["gz"], rtol=1e-12, atol=1e-16)
    # and the float32 NumPy statement of the backward rows is that chain
    gy = (L["gq"][:, None] * c[None, :]).astype(np.float32)
    got = ref.act_bwd_rows_f32(gy, pi.astype(np.float32), a.astype(np.float32), 2.0 / (z.shape[0] * A), 2)
    np.testing.assert_allclose(got, s["gz"], rtol=2e-5, atol=1e-8)


@pytest.mark.parametrize("sign", ["negative", "mixed"])
@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_comparator_rejects_the_mistakes(sign, variant):
    z, a, c, e = _case(sign, A=2, seed=3)
    want = ref.last_layer_step(z, a, c, e, 2.5)
    assert ref.same_step(ref.last_layer_step(z, a, c, e, 2.5), want)
    wrong = ref.last_layer_step(z, a, c, e, 2.5, variant=variant)
    assert not ref.same_step(wrong, want, rtol=1e-6), variant
    if variant == "lam_not_detached" and sign == "negative":
        # one-signed q: -lam * mean(q) = alpha * mean(q) / mean(-q) = -alpha... a constant, its gradient is exactly the cloning term's
        pi = np.tanh(z)
        bc_only = 2.0 * (pi - a) / pi.size * (1 - pi * pi)
        np.testing.assert_allclose(wrong["gz"], bc_only, rtol=1e-9, atol=1e-16)
        assert abs(wrong["loss"] - want["loss"]) < 1e-12  # the value alone does not show it: the gradient does
        assert np.abs(want["gz"] - bc_only).max() > 1e-3 * np.abs(want["gz"]).max()
    if variant == "mean_in_lam" and sign == "negative":
        assert wrong["lam"] < 0 < want["lam"]


def test_coef_zero_statement_adds_nothing():
    rng = np.random.default_rng(1)
    gy, y, a = (rng.normal(0, 1, (9, 3)).astype(np.float32) for _ in range(3))
    gy[0, 0] = -0.0
    y = np.tanh(y)
    out = ref.act_bwd_rows_f32(gy, y, a, 0.0, 2)
    assert np.array_equal(out.view(np.uint32), (gy * (np.float32(1) - y * y)).view(np.uint32))


def test_normalisation_statistics_against_numpy_float64():
    from core.td3bc.td3bc import STD_EPS, dataset_statistics

    rng = np.random.default_rng(2)
    obs = (rng.normal(0, 1, (1000, 4)) * np.array([0.3, 2.0, 1e-4, 0.0]) + np.array([0.5, -3.0, 7.0, 0.25])).astype(np.float32)
    mean, std = dataset_statistics(th.as_tensor(obs))
    m64, s64 = ref.statistics_f64(obs)
    assert STD_EPS == 1e-3 and mean.dtype == th.float32 and std.dtype == th.float32
    assert np.array_equal(mean.numpy(), m64.astype(np.float32)) or np.abs(mean.numpy() - m64).max() <= np.spacing(np.abs(m64).astype(np.float32)).max()
    np.testing.assert_allclose(std.numpy(), obs.astype(np.float64).std(axis=0, ddof=0) + 1e-3, rtol=1e-6)
    np.testing.assert_allclose(std.numpy(), s64, rtol=1e-6)
    assert std.numpy()[3] == np.float32(1e-3)  # a constant column: the epsilon alone
    assert abs(float(np.std(obs[:, 0].astype(np.float64), ddof=1)) - float(s64[0] - 1e-3)) > 1e-5  # ddof matters at this size


def test_folded_first_layer_against_the_unfolded_network_fp64():
    from core.common.evaluation import _fold_obs_norm

    rng = np.random.default_rng(4)
    lin = th.nn.Linear(4, 64)
    mean, std = rng.normal(0, 0.5, 4).astype(np.float32), rng.uniform(0.05, 2.0, 4).astype(np.float32)
    obs = rng.uniform(-1, 1, (200, 4))
    w, b = lin.weight.detach().numpy().astype(np.float64), lin.bias.detach().numpy().astype(np.float64)
    want = ref.normalize_f64(obs, mean, std) @ w.T + b
    fw, fb = ref.fold_first_layer_f64(w, b, mean, std)
    np.testing.assert_allclose(obs @ fw.T + fb, want, rtol=1e-12, atol=1e-13)
    before = (lin.weight.detach().clone(), lin.bias.detach().clone())
    folded = _fold_obs_norm(lin, (th.as_tensor(mean), th.as_tensor(std)))
    assert th.equal(lin.weight, before[0]) and th.equal(lin.bias, before[1])  # the model's parameters are untouched
    assert folded.weight.dtype == th.float32 and (folded.in_features, folded.out_features) == (4, 64)
    got = obs @ folded.weight.numpy().astype(np.float64).T + folded.bias.numpy().astype(np.float64)
    # float32 storage of W' and b': one rounding each, |x| <= 1
    bound = (np.abs(fw).sum(axis=1) + np.abs(fb)) * 2.0 ** -24 * 1.01
    assert (np.abs(got - want) <= bound[None, :]).all()
    with pytest.raises(RuntimeError, match="statistics are missing"):
        _fold_obs_norm(lin, None)
