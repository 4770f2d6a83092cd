"""GPU checks of the host side of the row-chain gradient steps (core/common/chain.py): which launches one step issues, in which order
and on how many networks / tiles / dW sets; the actor optimiser's step counter when its dW launch is not fused with Adam; the
validation of the Q networks' weights behind chain_net's raw pointers.

Shapes: 4 envs, widths (32, 16), batch 48 (the smallest multiple of 16 above the B > 32 threshold of the fused dW + Adam launch) and
batch 16 (below it: dW launch, then the optimiser's own launch)."""
import inspect

import pytest
import torch as th

pytestmark = pytest.mark.gpu

LAUNCHES = ("sac_actor_chain_fwd", "sac_actor_chain_bwd", "q_chain_fwd", "q_chain_bwd", "linear_bwd_weight_sets", "linear_bwd_weight_adam_sets",
            "chain_sum_parts")
WIDTHS = [32, 16]


def _record(monkeypatch, log):
    """Recording shims around the hip_ops entry points of the chain steps: (name, networks, tiles, dW sets, optimisers) per call."""
    from core.common import hip_ops

    def shim(name, orig):
        sig = inspect.signature(orig)

        def call(*a, **k):
            arg = sig.bind(*a, **k).arguments
            nets = len(arg["nets"]) if "nets" in arg else arg.get("n_nets")
            log.append((name, nets, arg.get("tiles"), len(arg["sets"]) if "sets" in arg else None, len(arg["opts"]) if "opts" in arg else None))
            if name == "linear_bwd_weight_adam_sets":
                log.append(("opt_index", [st[4] for st in arg["sets"]]))
            return orig(*a, **k)

        return call

    for name in LAUNCHES:
        monkeypatch.setattr(hip_ops, name, shim(name, getattr(hip_ops, name)))


def _span(monkeypatch, cls, method, log):
    """Mark where `cls.method` begins and ends in the log."""
    orig = getattr(cls, method)

    def call(self, *a, **k):
        log.append(("enter", method))
        out = orig(self, *a, **k)
        log.append(("exit", method))
        return out

    monkeypatch.setattr(cls, method, call)


def _spans(log, method):
    """The launches of every call of `method`, one list per call (opt_index notes kept beside their launch)."""
    out, cur = [], None
    for rec in log:
        if rec == ("enter", method):
            cur = []
        elif rec == ("exit", method):
            out.append(cur)
            cur = None
        elif cur is not None and rec[0] not in ("enter", "exit"):
            cur.append(rec)
    return out


def _warm(model, n_envs=4):
    model.learn(n_envs * 20)  # uniform actions only (learning_starts is never reached): fills the ring
    return model


def _make(cls, B, **kw):
    from core.common.vec_env import CSTRVecEnv

    return _warm(cls("MlpPolicy", CSTRVecEnv(4), seed=3, batch_size=B, buffer_size=4 * 32, learning_starts=10**9,
                     policy_kwargs=dict(net_arch=WIDTHS), **kw))


def _dw(B, n_sets, n_opts=1):
    """The dW / db launch of `n_sets` Linears: with the Adam steps inside above batch 32, gradients only below."""
    if B > 32:
        return [("linear_bwd_weight_adam_sets", None, None, n_sets, n_opts), ("opt_index", [k for k in range(n_opts) for _ in range(n_sets // n_opts)])]
    return [("linear_bwd_weight_sets", None, None, n_sets, None)]


@pytest.mark.parametrize("B", [48, 16])
def test_sac_step_launch_sequence(B, monkeypatch):
    from core.common import chain
    from core.sac import SAC

    model = _make(SAC, B)
    c = model._chain_for(B)
    assert c is not None and c._head_params is not None
    t_act, t_q4, t_q2, t_qb, t_ab = chain.TILES  # widths (32, 16): every wanted tile count fits (hip_ops.chain_tiles_ok)
    log = []
    _record(monkeypatch, log)
    _span(monkeypatch, chain.SacChain, "step", log)
    model.train(gradient_steps=1, batch_size=B)
    (step,) = _spans(log, "step")
    assert step == ([("sac_actor_chain_fwd", None, t_act, None, None), ("q_chain_fwd", 4, t_q4, None, None), ("q_chain_bwd", 2, t_qb, None, None)]
                    + _dw(B, 6)
                    + [("q_chain_fwd", 2, t_q2, None, None), ("q_chain_bwd", 2, t_qb, None, None), ("sac_actor_chain_bwd", 2, t_ab, None, None)]
                    + _dw(B, 3))
    assert len([r for r in step if r[0] != "opt_index"]) == 8


@pytest.mark.parametrize("B", [48, 16])
def test_td3_step_launch_sequence(B, monkeypatch):
    from core.common import chain
    from core.td3 import TD3

    model = _make(TD3, B)
    assert model._chain_for(B) is not None and model.policy_delay == 2
    t_act, t_q4, t_q2, t_qb, t_ab = chain.TD3_TILES
    log = []
    _record(monkeypatch, log)
    _span(monkeypatch, chain.Td3Chain, "step", log)
    policy_steps = []
    for _ in range(2):
        before = model.actor.optimizer.step_count
        model.train(gradient_steps=1, batch_size=B)
        policy_steps.append(model.actor.optimizer.step_count - before)
    assert sorted(policy_steps) == [0, 1]
    critic = ([("sac_actor_chain_fwd", None, t_act, None, None), ("q_chain_fwd", 4, t_q4, None, None), ("q_chain_bwd", 2, t_qb, None, None)]
              + _dw(B, 6))
    policy = ([("sac_actor_chain_fwd", None, t_act, None, None), ("q_chain_fwd", 1, t_q2, None, None), ("q_chain_bwd", 1, t_qb, None, None),
               ("sac_actor_chain_bwd", 1, t_ab, None, None)] + _dw(B, 3))
    for step, with_policy in zip(_spans(log, "step"), policy_steps):
        assert step == (critic + policy if with_policy else critic)
        assert len([r for r in step if r[0] != "opt_index"]) == (9 if with_policy else 4)


@pytest.mark.parametrize("B", [48, 16])
def test_maddpg_critic_chain_launch_sequences(B, monkeypatch):
    """The 2-agent split of the CSTR env (as tests/test_learner_parity.py): an update without a policy step takes `critic_steps_all`, one
    with it `critic_step` and `actor_loss_grad` per agent."""
    from core.common import chain
    from core.common.vec_env import CSTRVecEnv
    from core.maddpg import MADDPG

    n = 2
    model = _warm(MADDPG(n, "MlpPolicy", CSTRVecEnv(4), [[0, 1], [2, 3]], [[0], [1]], learning_rate_list=[1e-3] * n, seed=3, batch_size=B,
                         buffer_size=4 * 32, learning_starts=10**9, policy_kwargs=dict(net_arch=[WIDTHS] * n)))
    assert model._chain_for(B) is not None and model.policy_delay == 2
    t_act, t_q4, t_q2, t_qb, t_ab = chain.TD3_TILES
    log = []
    _record(monkeypatch, log)
    for method in ("critic_step", "critic_steps_all", "actor_loss_grad"):
        _span(monkeypatch, chain.MaddpgCriticChain, method, log)
    for _ in range(2):
        model.train(gradient_steps=1, batch_size=B)
    bwd = ("q_chain_bwd", 2, t_qb, None, None)
    assert _spans(log, "critic_steps_all") == [[("q_chain_fwd", 4 * n, t_q4, None, None)] + [bwd] * n + _dw(B, 6 * n, n)]
    assert _spans(log, "critic_step") == [[("q_chain_fwd", 4, t_q4, None, None), bwd] + _dw(B, 6)] * n
    assert _spans(log, "actor_loss_grad") == [[("q_chain_fwd", 1, t_q2, None, None), ("q_chain_bwd", 1, t_qb, None, None),
                                               ("chain_sum_parts", None, None, None, None)]] * n


def test_sac_actor_step_counter_without_head_views():
    """Without the merged head's moment views the actor's dW / db launch is not fused with Adam and `optimizer.step()` advances the
    counter itself: the actor-loss root must not have advanced it already. After 3 steps the control word holds step 3 and the third
    powers of the betas (three float64 products: exact to a few 1e-16); advanced twice per step it would hold the sixth."""
    from core.sac import SAC

    B = 48
    model = _make(SAC, B)
    c = model._chain_for(B)
    assert c is not None
    c._head_params = None
    for _ in range(3):
        model.train(gradient_steps=1, batch_size=B)
    opt = model.actor.optimizer
    b1, b2 = opt.param_groups[0]["betas"]
    ctl = opt.ctl.cpu()
    pow1, pow2 = (float(v) for v in ctl.view(th.float64)[2:4])
    print(f"step {int(ctl[0])}, beta powers {pow1!r} {pow2!r}, wanted {b1 ** 3!r} {b2 ** 3!r}")
    assert int(ctl[0]) == 3
    assert abs(pow1 - b1 ** 3) <= 1e-12 * b1 ** 3 and abs(pow2 - b2 ** 3) <= 1e-12 * b2 ** 3


def test_chain_weight_validation(monkeypatch):
    """What chain_net passes as raw pointers is checked where the networks are bound: a bad operand raises before any launch."""
    from core.common import hip_ops
    from core.sac import SAC

    B = 48
    model = _make(SAC, B)
    c = model._chain_for(B)
    assert c is not None  # a block built from a healthy model validates clean
    blk = c.block
    W, H1, H2 = blk.W, blk.H1, blk.H2
    assert (W, H1, H2) == (6, 32, 16)
    nets = blk.crit + blk.targ
    hip_ops.chain_check_nets(nets, W, H1, H2)
    log = []
    _record(monkeypatch, log)
    (w1, b1), (w2, b2), (w3, b3) = (tuple(t.detach() for t in layer) for layer in nets[0])
    bad = {"a transposed (non-contiguous) w2 view": ((w1, b1), (th.empty(H1, H2, device=w2.device).t(), b2), (w3, b3)),
           "a float64 bias": ((w1, b1), (w2, b2.double()), (w3, b3)),
           "a w1 whose second dimension is not W": ((w1.new_zeros(H1, W + 1), b1), (w2, b2), (w3, b3))}
    for what, net in bad.items():
        with pytest.raises(ValueError):
            hip_ops.chain_check_nets([nets[1], net], W, H1, H2)
            print("accepted:", what)
    # ... and a step object is not built on such a network: the block's constructor raises, nothing has been launched
    from core.common import chain

    bias = model.critic_target.q_networks[1][2].bias
    bias.data = bias.data.double()
    with pytest.raises(ValueError):
        chain.SacChain(model, B)
    assert not log
