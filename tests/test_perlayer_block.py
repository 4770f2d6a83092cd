"""GPU checks of the host side of the per-layer fused gradient steps (core/common/fused.py, `PerLayerTwinCritic`): which ABI entry points
a train() call issues and in which order, for every configuration that takes this path; that `_chain_for` follows the replay buffer's
normaliser; that the block re-makes its buffers when the batch size changes.

Every decision checked here is host logic (the kernels' own shapes have their fp64 tests), so the shapes are tests/test_chain_block.py's:
4 envs, widths (32, 16), batch 48, a ring filled by 20 vec-steps of uniform actions.

tests/golden/perlayer_block_launches.json holds the expected sequences. `record_case` below produced them on the commit BEFORE the block
existed (b9dd4c9: the four hand-written `_gradient_step_fused` bodies), so the test pins the refactor to its parent, launch for launch."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [32, 16]
B = 48
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perlayer_block_launches.json")


def _warm(model, n_envs=4):
    model.learn(n_envs * 20)  # uniform actions only (learning_starts is never reached): fills the ring
    return model


def _off_policy(cls, batch=B, **kw):
    from core.common.vec_env import CSTRVecEnv

    pk = dict(net_arch=WIDTHS, **kw.pop("policy_kwargs", {}))
    return _warm(cls("MlpPolicy", CSTRVecEnv(4), seed=3, batch_size=batch, buffer_size=4 * 32, learning_starts=10**9, policy_kwargs=pk, **kw))


def _multi_agent(cls):
    from core.common.vec_env import CSTRVecEnv

    n = 2  # the 2-agent split of the CSTR env (as tests/test_chain_block.py)
    return _warm(cls(n, "MlpPolicy", CSTRVecEnv(4), [[0, 1], [2, 3]], [[0], [1]], learning_rate_list=[1e-3] * n, seed=3, batch_size=B,
                     buffer_size=4 * 32, learning_starts=10**9, policy_kwargs=dict(net_arch=[WIDTHS] * n)))


def _sac(**kw):
    from core.sac import SAC

    return _off_policy(SAC, **kw)


def _sac_normalized():
    from core.common.vec_env import CSTRVecEnv, VecNormalize

    model = _sac()
    model.replay_buffer.normalizer = VecNormalize(CSTRVecEnv(4))  # what _setup_learn does with a VecNormalize'd env: the non-packed branch
    return model


def _td3(**kw):
    from core.td3 import TD3

    return _off_policy(TD3, **kw)


def _ddpg():
    from core.td3.td3 import DDPG

    return _off_policy(DDPG)


def _maddpg():
    from core.maddpg import MADDPG

    return _multi_agent(MADDPG)


def _iddpg():
    from core.iddpg.iddpg import IDDPG

    return _multi_agent(IDDPG)


def _bcq():
    from test_bcq import _env, _synthetic_dataset  # built as tests/test_bcq.py builds it

    from core.bcq import BCQ

    return BCQ("MlpPolicy", _env(), dataset=_synthetic_dataset(), seed=0, batch_size=32, policy_kwargs=dict(critic_net_arch=[32, 32]))


# case -> (module flags switched off, builder, train() calls recorded: two where a delayed policy step exists, batch size)
CASES = {
    "sac_twin": ((), _sac, 1, B),
    "sac_no_loss_root": (("USE_LOSS_ROOT",), _sac, 1, B),
    "sac_no_twin_pair": (("USE_TWIN_PAIR",), _sac, 1, B),
    "sac_n_critics_1": ((), lambda: _sac(policy_kwargs=dict(n_critics=1)), 1, B),
    "sac_n_critics_3": ((), lambda: _sac(policy_kwargs=dict(n_critics=3)), 1, B),
    "sac_vecnormalize": ((), _sac_normalized, 1, B),
    "td3_twin": ((), _td3, 2, B),
    "td3_n_critics_3": ((), lambda: _td3(policy_kwargs=dict(n_critics=3)), 2, B),
    "ddpg": ((), _ddpg, 2, B),
    "maddpg": ((), _maddpg, 2, B),
    "iddpg": ((), _iddpg, 2, B),
    "bcq": ((), _bcq, 2, 32),
}


def record_case(name, monkeypatch) -> list:
    """The ABI entry points (the `what` of hip_ops.check) of each recorded train(gradient_steps=1) call of case `name`, per-layer path."""
    from core.common import chain, fused, hip_ops

    flags_off, build, n_calls, batch = CASES[name]
    monkeypatch.setattr(chain, "USE_CHAIN", False)
    for flag in flags_off:
        monkeypatch.setattr(fused, flag, False)
    model = build()
    log = []
    orig = hip_ops.check

    def check(status, what):
        log.append(what)
        return orig(status, what)

    monkeypatch.setattr(hip_ops, "check", check)
    calls = []
    for _ in range(n_calls):
        del log[:]
        model.train(gradient_steps=1, batch_size=batch)
        calls.append(list(log))
    monkeypatch.setattr(hip_ops, "check", orig)
    return calls


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence(name, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = record_case(name, monkeypatch)
    for k, (g, w) in enumerate(zip(got, want)):
        print(f"{name} train() call {k}: {len(g)} entry points, expected {len(w)}")
        assert g == w, f"{name}, train() call {k}: first difference at launch {next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))}"
    assert len(got) == len(want)


def _count_steps(monkeypatch, cls):
    calls = []
    orig = cls.step

    def step(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    monkeypatch.setattr(cls, "step", step)
    return calls


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_chain_for_follows_the_normalizer(algo, monkeypatch):
    """learn(); set_env(VecNormalize(...)); learn() sets replay_buffer.normalizer on a model whose chain step is already cached: train()
    must fall back to the per-layer path (the chain samples packed batches, which do not go through VecNormalize) and come back to the
    chain when the normaliser is gone."""
    from core.common import chain
    from core.common.vec_env import CSTRVecEnv, VecNormalize

    model, cls = (_sac(), chain.SacChain) if algo == "sac" else (_td3(), chain.Td3Chain)
    steps = _count_steps(monkeypatch, cls)
    model.train(gradient_steps=1, batch_size=B)
    assert len(steps) == 1
    model.replay_buffer.normalizer = VecNormalize(CSTRVecEnv(4))  # as _setup_learn would
    model.train(gradient_steps=1, batch_size=B)
    assert len(steps) == 1 and model._chain_for(B) is None
    model.replay_buffer.normalizer = None
    model.train(gradient_steps=1, batch_size=B)
    assert len(steps) == 2


@pytest.mark.parametrize("build", [_sac, _td3, _maddpg], ids=["sac", "td3", "maddpg"])
def test_block_buffers_follow_the_batch_size(build, monkeypatch):
    import torch as th

    from core.common import chain

    monkeypatch.setattr(chain, "USE_CHAIN", False)
    model = build()
    blocks = model._critic_blocks if hasattr(model, "_critic_blocks") else [model._critic_block]
    for batch in (48, 16):
        model.train(gradient_steps=2, batch_size=batch)
        for blk in blocks:
            assert blk.gq.shape == (2, batch, 1) and (blk.g_logp is None or blk.g_logp.shape == (batch,))
    th.cuda.synchronize()
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
