"""CPU-side checks of A2C: the two cstr_a2c entry points are exported and reject bad arguments on the host (nothing is dereferenced or
launched), `from core import A2C` resolves, the constructor rewrites `policy_kwargs` as the reference does (core/a2c/a2c.py:123-127),
gSDE is refused, the seeded initial policy weights match the fixture written by the unmodified reference
(tests/golden/a2c_train_kat_small.npz, tools/refharness/gen_golden.py --only a2c), and the NumPy float32 statement of the RMSprop step
that csrc/cstr_a2c.hip follows (kept here, imported by tests/test_a2c.py) is compared with torch.optim.RMSprop on the CPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

from core import _native as nv

i64, f32, f64 = C.c_int64, C.c_float, C.c_double
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
A2C_SYMBOLS = ("cstr_a2c_loss_f32", "cstr_rmsprop_f32")


def P(k: int) -> C.c_void_p:
    """the k-th of a set of fake, well separated, 256-byte-aligned device addresses (never dereferenced)"""
    return C.c_void_p(0x1000000 * (k + 1))


def off(p: C.c_void_p, nbytes: int) -> C.c_void_p:
    return C.c_void_p(p.value + nbytes)


def rmsprop_numpy(param, grad, square_avg, lr, alpha, eps, coef=np.float32(1.0)):
    """torch.optim.RMSprop's step (momentum 0, not centred, no weight decay) with every operation rounded to float32, in the order
    of include/cstr_rl_hip.h: g' = g * coef; sq = sq * alpha + ((1 - alpha) * g') * g'; param += (-lr * g') / (sqrt(sq) + eps).
    Returns (param, clipped grad, square_avg); lr / alpha / eps are Python floats, coef a float32."""
    assert param.dtype == grad.dtype == square_avg.dtype == np.float32
    g = grad * np.float32(coef)
    sq = square_avg * np.float32(alpha) + (np.float32(1.0 - alpha) * g) * g
    avg = np.sqrt(sq) + np.float32(eps)
    return param + (np.float32(-lr) * g) / avg, g, sq


def test_a2c_symbols_declared_and_exported():
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in A2C_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive
    assert C.sizeof(nv.A2cLoss) == 13 * 8 + 4 * 4  # twelve pointers and a row count / stride, four 32-bit fields


def loss_args(**kw):
    d = dict(mean=P(0), ldm=2, log_std=P(1), actions=P(2), values=P(3), adv=P(4), returns=P(5), batch=20, act_dim=2, normalize_advantage=0,
             ent_coef=0.0, vf_coef=0.5, g_mean=P(6), g_value=P(7), g_log_std=P(8), scalars_out=P(9), log_prob_out=null)
    d.update(kw)
    p = nv.A2cLoss()
    for k, v in d.items():
        setattr(p, k, v.value if isinstance(v, C.c_void_p) else v)
    return p


def test_loss_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    loss = lambda ws=P(10), **kw: lib.cstr_a2c_loss_f32(C.byref(loss_args(**kw)), ws, null)  # noqa: E731
    assert lib.cstr_a2c_loss_f32(null, P(10), null) == BAD and loss(ws=null) == BAD
    for name in ("mean", "log_std", "actions", "values", "adv", "returns", "g_mean", "g_value", "g_log_std"):
        assert loss(**{name: null}) == BAD, name
    assert loss(batch=0) == BAD and loss(batch=-3) == BAD and loss(act_dim=0) == BAD and loss(ldm=1) == BAD
    assert loss(act_dim=3, ldm=3) == UNSUP and loss(act_dim=8, ldm=8) == UNSUP and loss(batch=(1 << 30) + 1) == UNSUP
    assert loss(mean=off(P(0), 4)) == BAD and loss(act_dim=4, ldm=6) == BAD and loss(act_dim=4, ldm=4, g_mean=off(P(6), 8)) == BAD  # misaligned rows
    assert loss(ws=off(P(10), 4)) == BAD and loss(values=off(P(3), 2)) == BAD
    assert loss(g_mean=P(0)) == BAD and loss(g_value=P(3)) == BAD and loss(g_log_std=P(1)) == BAD  # an output over its input
    assert loss(scalars_out=P(6)) == BAD and loss(log_prob_out=P(7)) == BAD and loss(ws=P(7)) == BAD  # two outputs over each other


def test_rmsprop_rejects_bad_arguments_on_the_host():
    lib = nv.lib()

    def step(param=P(0), grad=P(1), sq=P(2), lr=P(3), alpha=0.99, eps=1e-5, mx=0.5, ws=P(4), out=null, n=1000):
        return lib.cstr_rmsprop_f32(param, grad, sq, lr, f64(alpha), f64(eps), f32(mx), ws, out, i64(n), null)

    assert step(param=null) == BAD and step(grad=null) == BAD and step(sq=null) == BAD and step(lr=null) == BAD
    assert step(n=0) == BAD and step(n=-1) == BAD
    assert step(mx=0.5, ws=null) == BAD                       # the clip needs the workspace ...
    assert step(mx=0.0, ws=null, param=null) == BAD           # ... the unclipped step does not, but still validates the rest
    assert step(mx=float("nan")) == BAD and step(alpha=float("nan")) == BAD and step(eps=-1.0) == BAD
    assert step(param=off(P(0), 4)) == BAD and step(grad=off(P(1), 8)) == BAD and step(sq=off(P(2), 4)) == BAD  # float4 accesses
    assert step(ws=off(P(4), 4)) == BAD and step(lr=off(P(3), 4)) == BAD and step(out=off(P(5), 2)) == BAD
    assert step(grad=P(0)) == BAD and step(sq=P(0)) == BAD and step(sq=P(1)) == BAD  # param / grad / square_avg overlapping
    assert step(grad=off(P(0), 4000 - 16)) == BAD                                  # the last 16 bytes of param
    assert step(ws=P(0)) == BAD and step(out=P(1)) == BAD and step(out=P(4)) == BAD and step(lr=P(2)) == BAD


def test_hip_ops_wrappers_refuse_cpu_tensors():
    import torch as th

    from core.common import hip_ops

    z = th.zeros(8)
    with pytest.raises(ValueError, match="No CPU fallback|device"):
        hip_ops.rmsprop(z, z.clone(), z.clone(), th.zeros(1, dtype=th.float64))
    with pytest.raises(ValueError, match="device"):
        hip_ops.a2c_loss(th.zeros(4, 2), th.zeros(2), th.zeros(4, 2), z[:4], z[:4], z[:4], False, 0.0, 0.5, th.zeros(4, 2), z[:4], th.zeros(2),
                         th.zeros(nv.PPO_WS_WORDS, dtype=th.int64))
    assert hip_ops.A2C_SCALARS == ("policy_loss", "value_loss", "entropy_loss", "loss")


def test_from_core_import_a2c():
    import core
    from core import A2C
    from core.a2c import A2C as A2, MlpPolicy
    from core.common.on_policy_algorithm import OnPolicyAlgorithm
    from core.common.policies import ActorCriticPolicy
    from core.ppo import PPO

    assert A2C is A2 and "A2C" in core.__all__ and issubclass(A2C, OnPolicyAlgorithm) and MlpPolicy is ActorCriticPolicy
    assert A2C.policy_aliases["MlpPolicy"] is ActorCriticPolicy
    assert A2C.flat_rmsprop and not PPO.flat_rmsprop and not OnPolicyAlgorithm.flat_rmsprop  # only A2C asks for the flat RMSprop
    sig = inspect.signature(A2C.__init__).parameters
    want = dict(learning_rate=7e-4, n_steps=5, gamma=0.99, gae_lambda=1.0, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, rms_prop_eps=1e-5,
                use_rms_prop=True, use_sde=False, sde_sample_freq=-1, rollout_buffer_class=None, rollout_buffer_kwargs=None,
                normalize_advantage=False, stats_window_size=100, tensorboard_log=None, policy_kwargs=None, verbose=0, seed=None,
                device="auto", _init_setup_model=True)
    assert {k: sig[k].default for k in want} == want and list(sig)[1:3] == ["policy", "env"]
    learn = inspect.signature(A2C.learn).parameters
    assert learn["log_interval"].default == 100 and learn["tb_log_name"].default == "A2C"


def make_policy(seed=0, **kw):
    import torch as th

    from core.a2c import MlpPolicy
    from core.common.spaces import Box

    one = np.ones(4, np.float32)
    th.manual_seed(seed)
    return MlpPolicy(Box(-one, one), Box(-one[:2], one[:2]), lambda _: 7e-4, **kw)


def test_constructor_rewrites_policy_kwargs_as_the_reference_does():
    import torch as th

    from core.a2c import A2C

    pk = A2C._rewrite_policy_kwargs({"net_arch": [32, 32]}, True, 1e-5)
    assert pk == {"net_arch": [32, 32], "optimizer_class": th.optim.RMSprop, "optimizer_kwargs": dict(alpha=0.99, eps=1e-5, weight_decay=0)}
    assert A2C._rewrite_policy_kwargs({}, True, 3e-4)["optimizer_kwargs"]["eps"] == 3e-4
    assert A2C._rewrite_policy_kwargs({}, False, 1e-5) == {}                                   # use_rms_prop=False: nothing is written
    own = {"optimizer_class": th.optim.SGD}
    assert A2C._rewrite_policy_kwargs(dict(own), True, 1e-5) == own                             # the caller's optimiser class wins
    pol = make_policy(**A2C._rewrite_policy_kwargs({}, True, 1e-5))
    assert pol.optimizer_class is th.optim.RMSprop and pol.optimizer_kwargs == dict(alpha=0.99, eps=1e-5, weight_decay=0)
    adam = make_policy(**A2C._rewrite_policy_kwargs({}, False, 1e-5))
    assert adam.optimizer_class is th.optim.Adam and adam.optimizer_kwargs == {"eps": 1e-5}   # Adam keeps the policy's eps (policies.py:470-472)
    with pytest.raises(ValueError, match="does not support gSDE"):
        A2C("MlpPolicy", None, use_sde=True)


def test_optimizer_routing_on_the_host():
    """make_optimizer's decision is a pure function of (class, kwargs, flag); FlatRMSprop itself needs a device."""
    import torch as th

    from core.common import arena

    assert inspect.signature(arena.make_optimizer).parameters["flat_rmsprop"].default is False
    sig = inspect.signature(arena.FlatRMSprop.step).parameters
    assert [sig[k].default for k in ("max_norm", "workspace", "norm_out")] == [None, None, None]
    for name in ("param_groups", "defaults"):
        assert name in inspect.getsource(arena.FlatRMSprop.__init__)
    for name in ("zero_grad", "sync_lr", "step", "step_count", "state_dict", "load_state_dict"):
        assert hasattr(arena.FlatRMSprop, name), name
    assert th.optim.RMSprop is not None


def test_seeded_initial_weights_match_the_fixture(golden):
    g = golden("a2c_train_kat_small.npz")
    assert (int(g["n_envs"]), int(g["n_steps"]), [int(w) for w in g["net_arch"]], float(g["ent_coef"]), float(g["learning_rate"])) == \
        (4, 5, [32, 32], 0.01, 3e-3)
    pol = make_policy(seed=int(g["seed"]), net_arch=[int(w) for w in g["net_arch"]])
    sd = pol.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_dict_keys"]]
    for k, v in sd.items():
        want = g[f"before/policy/{k}"]
        assert tuple(v.shape) == want.shape, k
        if k == "log_std" or k.endswith(".bias"):
            np.testing.assert_array_equal(v.numpy(), want, err_msg=k)
        else:  # orthogonal_: QR through LAPACK, whose last bits may depend on the host CPU
            np.testing.assert_allclose(v.numpy(), want, rtol=0, atol=1e-6, err_msg=k)


def test_fixtures_hold_what_the_gpu_tests_rely_on(golden):
    g = golden("a2c_train_kat_small.npz")
    assert int(g["iterations"]) == 2 and str(g["optimizer"]) == "RMSprop"
    for k in range(2):
        assert float(g[f"it{k}/grad_norm"]) > float(g["max_grad_norm"]) == 0.5      # the clip is engaged in both steps
        assert int(g[f"it{k}/timeouts"].sum()) >= 1                                 # a truncation inside each rollout
        assert sorted(g[f"it{k}/permutation"].tolist()) == list(range(20))
        assert int(g[f"it{k}/optimizer_steps"]) == k + 1 == int(g[f"it{k}/n_updates"])
    assert float(np.abs(g["it0/opt/square_avg/log_std"]).max()) > 0                # the second step meets a non-zero square_avg
    v = golden("a2c_train_kat_variants.npz")
    assert str(v["adam/optimizer"]) == "Adam" and float(v["noclip/max_grad_norm"]) == 1e6
    assert all(0.5 < float(v[f"noclip/it{k}/grad_norm"]) < 1e6 for k in range(2))
    d = golden("a2c_train_kat_default.npz")
    assert (int(d["n_envs"]), int(d["n_steps"]), float(d["learning_rate"]), float(d["ent_coef"])) == (8, 5, 7e-4, 0.0)
    import os

    from conftest import GOLDEN

    for name in ("small", "variants", "default"):
        assert os.path.getsize(os.path.join(GOLDEN, f"a2c_train_kat_{name}.npz")) < 100 * 1024


def test_numpy_rmsprop_statement_against_torch_on_the_cpu():
    """Three steps on 1e5 elements, gradients spanning 1e-8 .. 1. The float32 statement above is not bit-equal to ATen's CPU kernels,
    which contract differently; on the CPU of the development machine, torch 2.10, it was measured within 2.4e-7 relative on
    square_avg and 6e-8 absolute on weights of magnitude up to 1.5. Twice those figures are asserted."""
    import torch as th

    n, lr, alpha, eps = 100_000, 7e-4, 0.99, 1e-5
    rng = np.random.default_rng(0)
    w0 = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    grads = [(10.0 ** rng.uniform(-8, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(3)]
    p = th.nn.Parameter(th.tensor(w0))
    opt = th.optim.RMSprop([p], lr=lr, alpha=alpha, eps=eps, weight_decay=0)
    w, sq = w0.copy(), np.zeros(n, np.float32)
    for g in grads:
        p.grad = th.tensor(g)
        opt.step()
        w, _, sq = rmsprop_numpy(w, g, sq, lr, alpha, eps)
        want_sq = opt.state[p]["square_avg"].numpy()
        rel = float(np.max(np.abs(sq - want_sq) / want_sq))
        dw = float(np.max(np.abs(w - p.detach().numpy())))
        print(f"RMSprop NumPy vs ATen: square_avg rel {rel:.3g}, weights abs {dw:.3g}")
        assert rel <= 2 * 2.4e-7 and dw <= 2 * 6e-8
    assert float(np.abs(w - w0).max()) > 1e-3  # the steps moved the weights
