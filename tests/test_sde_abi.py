"""CPU-side checks of gSDE: the kernels' C ABI (cstr_sde_*_f32) is exported and rejects bad arguments on the host before anything is
dereferenced or launched; TD3 / MADDPG still refuse use_sde; a gSDE SACPolicy has the reference's parameters, state-dict keys and
construction draws."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from core import _native as nv

SDE_SYMBOLS = ("cstr_sde_draw_f32", "cstr_sde_head_fwd_f32", "cstr_sde_head_bwd_f32", "cstr_sde_param_grad_f32")
F = 0x1000  # never dereferenced: the argument checks fail first
p = C.c_void_p


def _draw(lib, log_std=F, cols=2, L=64, A=2, n=1, z=F, mats=F, z_keep=1):
    return lib.cstr_sde_draw_f32(p(log_std), C.c_int(cols), C.c_int(L), C.c_int(A), C.c_int(0), C.c_int64(n), p(None), p(z),
                                 C.c_int64(z_keep), p(mats), p(None), p(None))


def _fwd(lib, h=F, B=64, L=64, A=2, w=F, b=F, std=F, action=F, ldh=None):
    return lib.cstr_sde_head_fwd_f32(p(h), C.c_int64(L if ldh is None else ldh), C.c_int64(B), C.c_int(L), C.c_int(A), p(w), p(b),
                                     C.c_float(2.0), p(None), C.c_int64(0), p(std), p(action), C.c_int64(A), p(None), p(None), p(None))


def _bwd(lib, ga=F, gl=F, action=F, aux=F, h=F, B=64, L=64, A=2, w=F, std=F, below=1, mats=None, mat_stride=0):
    return lib.cstr_sde_head_bwd_f32(p(ga), C.c_int64(A), p(gl), p(action), C.c_int64(A), p(aux), p(h), C.c_int64(L), C.c_int64(B), C.c_int(L),
                                     C.c_int(A), p(w), C.c_float(2.0), p(mats), C.c_int64(mat_stride), p(std), C.c_int(below), p(F), p(F), p(F),
                                     p(F), p(None))


def _fwd_mats(lib, mat_stride, L=64, A=2):
    return lib.cstr_sde_head_fwd_f32(p(F), C.c_int64(L), C.c_int64(64), C.c_int(L), C.c_int(A), p(F), p(F), C.c_float(2.0), p(F),
                                     C.c_int64(mat_stride), p(F), p(F), C.c_int64(A), p(None), p(None), p(None))


def _grad(lib, h=F, B=64, L=64, A=2, gp=F, gx=F, gv=F, std=F, ls=F, cols=2):
    return lib.cstr_sde_param_grad_f32(p(h), C.c_int64(L), C.c_int64(B), C.c_int(L), C.c_int(A), p(gp), p(gx), p(gv), p(None), p(std), p(ls),
                                       C.c_int(cols), C.c_int(0), p(F), p(F), p(F), p(None))


def test_sde_symbols_are_exported():
    lib = nv.lib()
    for name in SDE_SYMBOLS:
        assert hasattr(lib, name) and name in nv.SYMBOLS
    assert lib.cstr_abi_version() == 5


def test_sde_kernels_reject_bad_arguments_on_the_host():
    lib = nv.lib()
    # NULL operands
    assert _draw(lib, log_std=None) == -1 and _draw(lib, z=None) == -1 and _draw(lib, mats=None) == -1
    assert _fwd(lib, h=None) == -1 and _fwd(lib, w=None) == -1 and _fwd(lib, b=None) == -1 and _fwd(lib, std=None) == -1
    assert _fwd(lib, action=None) == -1
    assert _bwd(lib, ga=None, gl=None) == -1 and _bwd(lib, action=None) == -1 and _bwd(lib, aux=None) == -1 and _bwd(lib, h=None) == -1
    assert _grad(lib, h=None) == -1 and _grad(lib, gp=None) == -1 and _grad(lib, gv=None) == -1 and _grad(lib, ls=None) == -1
    # batch / matrix count 0, non-positive widths
    assert _draw(lib, n=0) == -1 and _fwd(lib, B=0) == -1 and _bwd(lib, B=0) == -1 and _grad(lib, B=0) == -1
    assert _draw(lib, L=0) == -1 and _fwd(lib, A=0) == -1 and _grad(lib, L=-4) == -1
    # L / A out of range: unsupported
    assert _draw(lib, L=nv.SDE_MAX_LATENT + 1) == -2 and _fwd(lib, L=nv.SDE_MAX_LATENT + 1) == -2
    assert _draw(lib, A=nv.MAX_HEAD_ACT + 1, cols=1) == -2 and _bwd(lib, A=nv.MAX_HEAD_ACT + 1) == -2
    assert _grad(lib, A=nv.MAX_HEAD_ACT + 1, cols=1) == -2 and _draw(lib, n=nv.SDE_MAX_MATS + 1) == -2
    # log_std columns other than A or 1, a row stride below the width, an unknown activation
    assert _draw(lib, cols=3) == -1 and _grad(lib, cols=3) == -1
    assert _fwd(lib, ldh=32) == -1 and _bwd(lib, below=7) == -1
    # per-row matrices closer together than one matrix, in the forward and the backward alike; z kept for more matrices than drawn
    assert _fwd_mats(lib, 64 * 2 - 1) == -1 and _bwd(lib, mats=F, mat_stride=64 * 2 - 1) == -1 and _bwd(lib, mats=F, mat_stride=-1) == -1
    assert _draw(lib, n=2, z_keep=3) == -1 and _draw(lib, z_keep=-1) == -1


def test_algorithms_without_sde_support_refuse_gsde():
    """TD3 / DDPG / MADDPG pass sde_support=False (as in the reference) and have no use_sde argument; OffPolicyAlgorithm itself refuses
    use_sde=True without sde support before anything else is set up."""
    from core.common.off_policy_algorithm import OffPolicyAlgorithm

    class NoSde(OffPolicyAlgorithm):
        pass

    with pytest.raises(ValueError, match="does not support gSDE"):
        NoSde(object, None, 1e-3, use_sde=True, sde_support=False)


def test_sac_accepts_gsde_arguments():
    import inspect

    from core.sac import SAC
    from core.sac.policies import SACPolicy

    sig = inspect.signature(SAC.__init__).parameters
    assert all(k in sig for k in ("use_sde", "sde_sample_freq", "use_sde_at_warmup"))
    sig = inspect.signature(SACPolicy.__init__).parameters
    assert all(k in sig for k in ("use_sde", "log_std_init", "full_std", "use_expln", "clip_mean"))


def _spaces():
    from core.common.spaces import Box

    return Box(-1, 1, (4,), np.float32), Box(-1, 1, (2,), np.float32)


@pytest.mark.parametrize("kw", [dict(), dict(full_std=False, use_expln=True, clip_mean=0.0, log_std_init=-2.0)])
def test_gsde_policy_construction_matches_the_reference_order(kw):
    """Parameters and keys of the reference's gSDE actor, and its generator use: the mean Linear's init, then TWO standard-normal
    draws ([L, A], then [1, L, A]) before the critics are built -- so the critics' initial weights are those of a generator that
    made exactly these draws."""
    from torch import nn

    from core.common.torch_layers import create_mlp
    from core.sac.policies import SACPolicy

    obs, act = _spaces()
    th.manual_seed(3)
    pol = SACPolicy(obs, act, lambda _: 3e-4, net_arch=[32, 32], use_sde=True, **kw)
    a = pol.actor
    clipped = kw.get("clip_mean", 2.0) > 0  # mu = Sequential(Linear, Hardtanh), else the Linear itself
    mu_keys = ["mu.0.weight", "mu.0.bias"] if clipped else ["mu.weight", "mu.bias"]
    assert list(a.state_dict()) == ["log_std", "latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias"] + mu_keys
    cols = 1 if kw.get("full_std") is False else 2
    assert tuple(a.log_std.shape) == (32, cols) and bool((a.log_std == kw.get("log_std_init", -3.0)).all())
    assert isinstance(a.mu, nn.Sequential) == clipped
    th.manual_seed(3)
    latent = nn.Sequential(*create_mlp(4, -1, [32, 32], nn.ReLU))
    mu = nn.Linear(32, 2)
    z1, z2 = th.empty(32, 2).normal_(), th.empty(1, 32, 2).normal_()
    critic = pol.make_critic()  # built from the generator state right after the two draws
    for x, y in ((latent[0].weight, a.latent_pi[0].weight), (mu.weight, a.mu_linear.weight), (mu.bias, a.mu_linear.bias)):
        assert th.equal(x, y)
    d = a.action_dist
    std = d.get_std(a.log_std).detach()
    assert th.equal(d.exploration_mat.detach(), z1 * std) and th.equal(d.exploration_matrices.detach(), z2 * std)
    for k, v in critic.state_dict().items():
        assert th.equal(v, pol.critic.state_dict()[k]), k


def test_gsde_policy_reference_statements_on_cpu():
    """The ATen statements (distributions.py:541-617) on the construction matrices: one row uses exploration_mat, deterministic the mean."""
    from core.sac.policies import SACPolicy

    obs, act = _spaces()
    th.manual_seed(0)
    pol = SACPolicy(obs, act, lambda _: 3e-4, net_arch=[16, 16], use_sde=True)
    a = pol.actor
    x = th.rand(3, 4) * 2 - 1
    h = a.latent_pi(x)
    mean = a.mu(h)
    out = a(x[:1])
    assert th.allclose(out, th.tanh(mean[:1] + h[:1] @ a.action_dist.exploration_mat))
    assert th.allclose(a(x, deterministic=True), th.tanh(mean))
    act_, lp = a.action_log_prob(x)
    assert act_.shape == (3, 2) and lp.shape == (3,) and bool(th.isfinite(lp).all())


@pytest.mark.parametrize("tag", ["small", "variants"])
def test_gsde_policy_initial_weights_match_the_reference(golden, tag):
    """Built on the CPU generator after torch.manual_seed(0) (what SAC(seed=0) does before building its policy), the gSDE policy's
    actor, critics and the two construction draws equal the reference's (tests/golden/sac_sde_train_kat_*.npz) bit for bit."""
    from core.sac.policies import SACPolicy

    g = golden(f"sac_sde_train_kat_{tag}.npz")
    kw = dict(use_expln=True, full_std=False, clip_mean=0.0) if tag == "variants" else {}
    obs, act = _spaces()
    th.manual_seed(0)
    pol = SACPolicy(obs, act, lambda _: 3e-4, net_arch=[64, 64], use_sde=True, **kw)
    for nm in ("actor", "critic", "critic_target"):
        sd = getattr(pol, nm).state_dict()
        assert sorted(f"before/{nm}/{k}" for k in sd) == sorted(k for k in g.files if k.startswith(f"before/{nm}/"))
        for k, v in sd.items():
            np.testing.assert_array_equal(v.numpy(), g[f"before/{nm}/{k}"], err_msg=f"{nm}/{k}")
    z1, z2 = pol.actor.action_dist._host_z
    np.testing.assert_array_equal(z1.numpy(), g["init/z_mat"])
    np.testing.assert_array_equal(z2.numpy(), g["init/z_mats"])
