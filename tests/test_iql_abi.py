"""CPU-side checks of IQL: cstr_iql_loss_f32 is exported and rejects bad arguments on the host (nothing is dereferenced or launched),
`from core import IQL` resolves with the documented constructor, the policy is SAC's plus `value_net` (keys, seeded initial weights),
the refusals that need no device, and the reference statements of tests/_iql_reference.py: the explicit gradients against fp64
autograd, the float32 torch evaluation against the comparator's bars, the comparator against the twelve mistakes a wrong
implementation makes, and the expectile ordering on the reference alone."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch as th

import _iql_reference as ref
from core import _native as nv

i64, f32, ci = C.c_int64, C.c_float, C.c_int
null = C.c_void_p(None)
P = lambda a: C.c_void_p(a)  # noqa: E731
BAD, UNSUP = -1, -2
# never-dereferenced addresses, 1 MiB apart: inputs ...
INS = dict(qt1=0x1000000, qt2=0x1100000, v=0x1200000, v_next=0x1300000, q1=0x1400000, q2=0x1500000, params=0x1600000, act=0x1700000,
           rew=0x1800000, done=0x1900000)
# ... and outputs
OUTS = dict(g_v=0x2000000, gq1=0x2100000, gq2=0x2200000, g_params=0x2300000, loss_out=0x2400000, loss_sum=0x2400100, aux=0x2400200,
            target_out=0x2500000, adv_out=0x2600000, logp_out=0x2700000)


def _call(lib, batch=256, a=2, ldp=4, ldact=6, gamma=0.99, expectile=0.7, beta=3.0, m=100.0, **ptrs):
    p = dict(INS, **OUTS)
    p.update(ptrs)
    return lib.cstr_iql_loss_f32(P(p["qt1"]), P(p["qt2"]), P(p["v"]), P(p["v_next"]), P(p["q1"]), P(p["q2"]), P(p["params"]), i64(ldp),
                                 P(p["act"]), i64(ldact), P(p["rew"]), P(p["done"]), f32(gamma), f32(expectile), f32(beta), f32(m),
                                 P(p["g_v"]), P(p["gq1"]), P(p["gq2"]), P(p["g_params"]), P(p["loss_out"]), P(p["loss_sum"]), P(p["aux"]),
                                 P(p["target_out"]), P(p["adv_out"]), P(p["logp_out"]), i64(batch), ci(a), null)


def test_symbol_declared_and_exported():
    lib = nv.lib()
    assert [s for s in nv.SYMBOLS if s.startswith("cstr_iql_")] == ["cstr_iql_loss_f32"] and hasattr(lib, "cstr_iql_loss_f32")
    assert nv.IQL_MAX_BATCH == nv.MAX_SAMPLE_BATCH == 16384 and lib.cstr_abi_version() == 5
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/cstr_rl_hip.h").read()
    assert "int cstr_iql_loss_f32(" in header and "#define CSTR_IQL_MAX_BATCH CSTR_MAX_SAMPLE_BATCH" in header


def test_loss_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    call = lambda **kw: _call(lib, **kw)  # noqa: E731
    for k in INS:  # every input is required
        assert call(**{k: None}) == BAD, k
    assert call(batch=0) == BAD and call(batch=-3) == BAD and call(a=0) == BAD and call(a=-1) == BAD
    assert call(ldp=3) == BAD and call(ldact=1) == BAD and call(a=4, ldp=7, ldact=8) == BAD and call(a=4, ldp=8, ldact=3) == BAD
    assert call(gq1=None) == BAD and call(gq2=None) == BAD  # the critic's gradients are one group
    for bad in (0.0, 1.0, -0.2, 1.5, float("nan")):
        assert call(expectile=bad) == BAD, bad
    assert call(beta=-0.1) == BAD and call(beta=float("nan")) == BAD
    assert call(m=0.0) == BAD and call(m=-1.0) == BAD and call(m=float("nan")) == BAD
    assert call(batch=nv.IQL_MAX_BATCH + 1) == UNSUP and call(a=nv.MAX_HEAD_ACT + 1, ldp=16, ldact=16) == UNSUP
    for k, base in dict(INS, **OUTS).items():  # off a 4-byte boundary
        assert call(**{k: base + 2}) == BAD, k
    # outputs over inputs ...
    assert call(g_v=INS["qt1"]) == BAD and call(g_v=INS["v"] + 4 * 255) == BAD and call(gq1=INS["q1"]) == BAD and call(gq2=INS["q2"] - 4 * 255) == BAD
    assert call(g_params=INS["params"] + 4 * (255 * 4 + 3)) == BAD and call(g_params=INS["act"] - 4 * (256 * 4 - 1)) == BAD
    assert call(target_out=INS["act"] + 4 * (255 * 6 + 1)) == BAD and call(adv_out=INS["rew"]) == BAD and call(logp_out=INS["done"]) == BAD
    assert call(loss_out=INS["v_next"]) == BAD and call(loss_sum=INS["qt2"] + 4 * 255) == BAD and call(aux=INS["rew"] - 4 * 5) == BAD
    # ... and over each other
    assert call(gq2=OUTS["gq1"]) == BAD and call(g_v=OUTS["g_params"] + 4 * (256 * 4 - 1)) == BAD and call(loss_sum=OUTS["loss_out"] + 8) == BAD
    assert call(aux=OUTS["loss_sum"] + 8) == BAD and call(target_out=OUTS["adv_out"] - 4 * 255) == BAD and call(logp_out=OUTS["g_v"]) == BAD


def test_hip_ops_wrapper_refuses_cpu_tensors():
    from core.common import hip_ops

    z = th.zeros
    ok = lambda: [z(8), z(8), z(8), z(8), z(8), z(8), z(8, 4), z(8, 2), z(8), z(8)]  # noqa: E731
    with pytest.raises(ValueError, match="device"):
        hip_ops.iql_loss(*ok(), 0.99, 0.7, 3.0, 100.0)
    assert hip_ops.iql_supported(256, 2) and hip_ops.iql_supported(16384, 4) and hip_ops.iql_supported(1, 1)
    assert not hip_ops.iql_supported(16385, 2) and not hip_ops.iql_supported(256, 5) and not hip_ops.iql_supported(0, 2)


def test_from_core_import_iql_and_signature():
    import core
    from core import IQL
    from core.common.offline_policy_algorithm import OfflineAlgorithm
    from core.iql import IQL as I2
    from core.iql.policies import IQLPolicy
    from core.sac.policies import SACPolicy

    assert IQL is I2 and "IQL" in core.__all__ and issubclass(IQL, OfflineAlgorithm)
    assert IQL.policy_aliases == {"MlpPolicy": IQLPolicy} and issubclass(IQLPolicy, SACPolicy)
    sig = inspect.signature(IQL.__init__)
    got = [(k, p.default) for k, p in sig.parameters.items() if k not in ("self", "policy", "env")]
    assert got == [("learning_rate", 3e-4), ("dataset", None), ("buffer_size", 1_000_000), ("batch_size", 256), ("tau", 0.005), ("gamma", 0.99),
                   ("gradient_steps", 1), ("target_update_interval", 1), ("expectile", 0.7), ("beta", 3.0), ("exp_adv_max", 100.0),
                   ("behavior_cloning_warmup", 0), ("n_eval_episodes", 10), ("policy_kwargs", None), ("stats_window_size", 100),
                   ("tensorboard_log", None), ("verbose", 0), ("device", "auto"), ("seed", None), ("_init_setup_model", True)]
    assert not IQL.goal_face_support and IQL.chain_type is None


def test_policy_keys_and_seeded_init_equal_sacpolicy():
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.iql.policies import IQLPolicy
    from core.sac.policies import SACPolicy

    pols = []
    for cls in (IQLPolicy, SACPolicy):
        set_random_seed(0)
        pols.append(cls(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4))
    a, b = (p.state_dict() for p in pols)
    assert list(a)[:len(b)] == list(b) and all(th.equal(a[k], b[k]) for k in b)  # SAC's modules first, with SAC's draws
    assert list(a)[len(b):] == [f"value_net.v_net.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    assert a["value_net.v_net.0.weight"].shape == (256, 4) and a["value_net.v_net.4.weight"].shape == (1, 256)
    assert isinstance(pols[0].value_net.v_net[1], th.nn.ReLU)
    # value_net draws AFTER the target critic: constructing it does not move the draws in front of it (above), and it is not a copy
    assert not th.equal(a["value_net.v_net.2.weight"], a["critic.qf0.2.weight"])


def test_refusals_that_need_no_device(tmp_path):
    from core import IQL

    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'int'>"):
        IQL("MlpPolicy", None, dataset=5)
    with pytest.raises(FileNotFoundError, match="Dataset file not found"):
        IQL("MlpPolicy", None, dataset=str(tmp_path / "missing.pkl"))
    with pytest.raises(ValueError, match="does not support gSDE"):
        IQL("MlpPolicy", None, dataset=5, policy_kwargs=dict(use_sde=True))
    for bad in (0.0, 1.0, -0.5, 1.2, float("nan")):
        with pytest.raises(ValueError, match=r"expectile must lie inside \(0, 1\)"):
            IQL("MlpPolicy", None, dataset=5, expectile=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="beta must be a non-negative number"):
            IQL("MlpPolicy", None, dataset=5, beta=bad)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="exp_adv_max must be a positive number"):
            IQL("MlpPolicy", None, dataset=5, exp_adv_max=bad)
    np.savez(str(tmp_path / "d.npz"), observations=np.zeros((4, 1, 4)))
    with pytest.raises(ValueError, match="needs `env`"):
        IQL("MlpPolicy", None, dataset=str(tmp_path / "d.npz"))


# ---- the reference statements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", [(12, 2), (1, 1), (7, 3), (5, 4)])
def test_explicit_gradients_equal_fp64_autograd(B, A):
    case = ref.small_case(B=B, A=A, seed=B)
    for tau_e, beta in ((0.7, 3.0), (0.5, 0.0), (0.9, 10.0)):
        case.update(expectile=tau_e, beta=beta)
        auto, expl = ref.step_f64(case), ref.step_f64(case, explicit=True)
        assert ref.same_step(expl, auto, rtol=1e-12), (tau_e, beta)
        np.testing.assert_allclose(expl["aux"], auto["aux"], rtol=1e-12, atol=1e-15)
        assert np.array_equal(expl["clipped"], auto["clipped"])
        if beta == 0.0:
            assert (expl["w"] == 1.0).all()


def test_small_case_covers_what_the_mistakes_touch():
    case = ref.small_case()
    want = ref.step_f64(case, explicit=True)
    B = want["u"].shape[0]
    assert (want["u"] < 0).sum() >= 3 and (want["u"] > 0).sum() >= 3  # mixed-sign u
    assert want["clipped"].sum() >= 2 and (~want["clipped"]).sum() >= B // 4
    assert abs(case["act"][0, 0]) == 1.0 and case["params"][1, 2] < -20 and case["params"][2, 2] > 2
    assert (want["g_params"][1:3, 2:] == 0).all() and np.isfinite(want["logp"]).all()


def test_float32_torch_statement_passes_the_bars():
    """float32 against fp64 at the project's convention on itself: a float32 evaluation is within 4 x its own distance by construction;
    what this pins is that the comparator and the floors run on real shapes and that the distance is small against each output's scale
    away from |a| = 1 (the statement is well conditioned there), so a bar of 4 x that distance is a tight one."""
    rng = np.random.default_rng(3)
    B, A = 257, 2
    f = lambda *s: rng.normal(-3, 1, s).astype(np.float32)  # noqa: E731
    qt1, qt2 = f(B), f(B)
    v = (np.minimum(qt1, qt2) + rng.normal(0, 1, B)).astype(np.float32)
    params = np.concatenate([rng.normal(0, 0.5, (B, A)), rng.normal(-1, 0.7, (B, A))], axis=1).astype(np.float32)
    act = np.tanh(rng.normal(0, 0.8, (B, A))).astype(np.float32)
    args = (qt1, qt2, v, f(B), f(B), f(B), params, act, rng.uniform(-8, 0, B).astype(np.float32),
            (rng.uniform(size=B) < 0.2).astype(np.float32), 0.99, 0.7, 3.0, 100.0)
    want, got, fl = ref.loss_f64(*args), ref.loss_torch(*args, dtype=th.float32), ref.floors(*args)
    for k in ("u", "g_v", "y", "gq1", "gq2", "w", "logp", "g_params", "losses", "aux"):
        assert ref.close(got[k], want[k], got[k], floor=fl[k]) <= 1.0
        assert np.abs(got[k] - want[k]).max() <= 2e-5 * np.abs(want[k]).max(), k
        assert (fl[k] <= 1e-4 * np.maximum(np.abs(want[k]), np.abs(want[k]).max() * 1e-2)).all(), k  # the floors stay small
    assert np.array_equal(got["clipped"], want["clipped"])


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_comparator_rejects_the_mistakes(variant):
    case = ref.small_case()
    want = ref.step_f64(case)
    assert ref.same_step(ref.step_f64(case), want) and ref.same_step(ref.step_f64(case, explicit=True), want)
    assert not ref.same_step(ref.step_f64(case, variant=variant), want, rtol=1e-6), variant


def test_expectile_ordering_on_the_reference():
    """The reference alone, ORDER_ARGS = 300 steps at (32, 32) / batch 64 / lr 3e-3 / seed 0 on `ordering_dataset` (actions uniform whatever
    the state, reward -4 + 3 a_0, so Q(s, .) spreads over a state's dataset actions): the mean of V over the first 2048 dataset
    observations is -3.237 after expectile 0.5 and -2.512 after expectile 0.9. On BCQ's synthetic dataset, whose reward does not depend on
    the action, the same runs give -3.258 and -3.155: no gap to speak of, which is why this dataset exists. tests/test_iql.py asserts the
    same inequality on the device path."""
    data = ref.ordering_dataset()
    vals = {t: ref.dataset_value(ref.train_reference(data, t, **ref.ORDER_ARGS), data) for t in (0.5, 0.9)}
    print(f"reference: mean V after expectile 0.5: {vals[0.5]:.3f}, after 0.9: {vals[0.9]:.3f}")
    assert vals[0.9] > vals[0.5] + 0.2, vals


def test_float32_torch_statement_at_an_untrained_critic():
    """Why tests/test_iql.py's teacher-forced runs start from critics and a V whose output bias is the dataset's mean reward (CQL's tests
    do the same, tests/test_cql_abi.py). RefIQL in float32 against float64, class defaults, batch 256, two steps from the SEEDED INITIAL
    WEIGHTS: untrained networks give Q and V = 0 +- 0.1, and tests/_parity_helpers.py q_err's per-element bar |dq| <= 5e-5 max(|q|, 1e-3)
    then asks for 5e-8 of a sum of 256 terms of size 0.1. Measured here (seeds 0 and 1), second step, per-element |dq| / max(|q|, 1e-3):
    seeded start Q 8.8e-5, 1.4e-4, 1.2e-4, 2.3e-6, V 1.9e-5 and 1.8e-5 -- the float32 torch statement itself is beyond the 5e-5 of the
    hand-written path; output biases at the mean reward: 4e-8 to 8e-8 everywhere. Asserted with a margin for another machine's float32
    sums: the seeded start beyond 5e-5 for at least one critic, the biased start below a quarter of the tightest bar (1.25e-5)."""
    import copy

    rows, B = 2048, 256
    strict = {False: [], True: []}
    for seed in (0, 1):
        for biased in (False, True):
            pol = ref.make_policy(seed)
            rng = np.random.default_rng(3)
            obs = rng.uniform(-1, 1, (rows, 4)).astype(np.float32)
            nobs = np.clip(obs + rng.normal(0, 0.05, obs.shape), -1, 1).astype(np.float32)
            act, rew = rng.uniform(-1, 1, (rows, 2)).astype(np.float32), rng.uniform(-8, 0, rows).astype(np.float32)
            done = (rng.uniform(size=rows) < 0.1).astype(np.float32)
            if biased:
                with th.no_grad():
                    for critic in (pol.critic, pol.critic_target):
                        for qnet in critic.q_networks:
                            qnet[-1].bias.fill_(float(rew.mean()))
                    pol.value_net.v_net[-1].bias.fill_(float(rew.mean()))
            r64 = ref.RefIQL(copy.deepcopy(pol).double(), 3e-4, 0.99, 0.005, 0.7, 3.0, 100.0)
            r32 = ref.RefIQL(copy.deepcopy(pol).float(), 3e-4, 0.99, 0.005, 0.7, 3.0, 100.0, dtype=th.float32)
            for _ in range(2):
                idx = rng.integers(0, rows, B)
                args = (obs[idx], act[idx], nobs[idx], rew[idx], done[idx])
                want, got = r64.step(*args), r32.step(*args)
            for g, w_ in ((got["q"][0], want["q"][0]), (got["q"][1], want["q"][1]), (got["v"], want["v"])):
                strict[biased].append(float((np.abs(g - w_) / np.maximum(np.abs(w_), 1e-3)).max()))
    print("float32 torch statement, per-element |d| / max(|.|, 1e-3) of q1, q2, v at the second step: seeded start "
          + ", ".join(f"{v:.2e}" for v in strict[False]) + "; output biases at the mean reward " + ", ".join(f"{v:.2e}" for v in strict[True]))
    assert max(strict[False]) > 5e-5 and max(strict[True]) < 1.25e-5, strict
