"""LayerNorm / dropout critics, host side: the entry points and their support table, the refusals that need no device, the unchanged
plain construction, and the torch-statement path of a layer_norm critic against fp64 autograd. CPU only."""
import numpy as np
import pytest
import torch as th
from torch import nn


def test_symbols_and_support_table():
    from core import _native as nv
    from core.common import hip_ops

    lib = nv.lib()
    assert lib.cstr_abi_version() == 5
    for sym in ("cstr_ln_supported", "cstr_linear_ln_act_fwd_f32", "cstr_ln_linear_bwd_input_f32", "cstr_ln_dropout_uniform_f32"):
        assert sym in nv.SYMBOLS and hasattr(lib, sym)
    ok = hip_ops.ln_supported
    assert ok(256, 512, 0.01, 1) and not ok(256, 513, 0.01, 1) and not ok(256, 256, 1.0, 1) and ok(1, 16, 0.0, 2)
    assert not ok(0, 16) and not ok(6, 16, -0.1) and not ok(6, 16, 0.0, 0)


@pytest.mark.parametrize("name", ["DDPG", "TQC", "PPO", "A2C", "TRPO", "DQN", "QRDQN"])
def test_other_classes_refuse_the_keys(name):
    """before anything else of the constructor (the offline classes, ARS, MADDPG and IDDPG need a dataset or an env first: test_refusals of tests/test_layernorm.py)"""
    import core

    with pytest.raises(ValueError, match="layer_norm / dropout_rate"):
        getattr(core, name)("MlpPolicy", None, policy_kwargs=dict(layer_norm=True, dropout_rate=0.01))


def test_plain_construction_unchanged(golden):
    """create_mlp's default output, and the seeded initial weights with and without the new modules (they draw no random numbers)"""
    from core.common.spaces import Box
    from core.common.torch_layers import create_mlp
    from core.sac.policies import SACPolicy

    assert [type(m) for m in create_mlp(6, 1, [8, 8])] == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear]
    assert [type(m) for m in create_mlp(6, 1, [8], nn.Tanh, layer_norm=True, dropout_rate=0.1)] == [nn.Linear, nn.Dropout, nn.LayerNorm, nn.Tanh, nn.Linear]
    g = golden("policy_init_kat.npz")
    build = lambda **kw: (th.manual_seed(0), SACPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4, **kw))[1]  # noqa: E731
    plain, normed = build(), build(layer_norm=True, dropout_rate=0.01)
    for nm in ("actor", "critic", "critic_target"):
        for k, v in getattr(plain, nm).state_dict().items():
            np.testing.assert_array_equal(v.numpy().reshape(-1)[:16], g[f"sac0/{nm}/{k}#head"], err_msg=f"{nm}/{k}")
            assert v.numpy().astype(np.float64).sum() == float(g[f"sac0/{nm}/{k}#sum"])
    linears = lambda pol: [m for nm in ("actor", "critic", "critic_target") for m in getattr(pol, nm).modules() if isinstance(m, nn.Linear)]  # noqa: E731
    for a, b in zip(linears(plain), linears(normed), strict=True):  # the same draws in the same order
        assert th.equal(a.weight, b.weight) and th.equal(a.bias, b.bias)
    assert [type(m) for m in normed.critic.qf0][:4] == [nn.Linear, nn.Dropout, nn.LayerNorm, nn.ReLU]
    assert {"qf0.2.weight", "qf0.2.bias", "qf1.6.weight"} <= set(normed.critic.state_dict()) and not any(
        isinstance(m, (nn.LayerNorm, nn.Dropout)) for m in normed.actor.modules())


def test_torch_statement_path_matches_fp64_autograd():
    """ContinuousCritic(layer_norm=True) at p = 0: forward and every parameter gradient against the same modules in float64"""
    import copy

    from core.common.policies import ContinuousCritic
    from core.common.spaces import Box
    from core.common.torch_layers import FlattenExtractor

    th.manual_seed(3)
    c32 = ContinuousCritic(Box(-1, 1, (4,)), Box(-1, 1, (2,)), [32, 32], FlattenExtractor(4), 4, n_critics=2, layer_norm=True)
    c64 = copy.deepcopy(c32).double()
    obs, act = th.randn(16, 4), th.randn(16, 2)
    q32, q64 = c32(obs, act), c64(obs.double(), act.double())
    sum(q.pow(2).mean() for q in q32).backward()
    sum(q.pow(2).mean() for q in q64).backward()
    for a, b in zip(q32, q64):
        assert float((a.double() - b).abs().max()) <= 1e-5
    for (k, a), b in zip(c32.named_parameters(), c64.parameters()):
        assert float((a.grad.double() - b.grad).abs().max()) <= 1e-5 * max(1.0, float(b.grad.abs().max())), k
