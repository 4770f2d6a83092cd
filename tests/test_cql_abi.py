"""CPU-side checks of CQL: the two cstr_cql_* entry points are exported and reject bad arguments on the host (nothing is dereferenced
or launched), `from core import CQL` resolves with the documented constructor, the policy is SAC's (keys, seeded initial weights), the
refusals that need no device, and the reference statements of tests/_cql_reference.py: the explicit gradients against fp64 autograd in
both importance modes, the float32 torch evaluation against the comparator's bars, the comparator against the mistakes a wrong
implementation makes, the Philox restatement against the array restatement of tests/_rowkernel_reference.py, and the conservative
effect on the reference alone."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch as th

import _cql_reference as ref
from core import _native as nv

i64, f32, ci = C.c_int64, C.c_float, C.c_int
null = C.c_void_p(None)
P = lambda a: C.c_void_p(a)  # noqa: E731
BAD, UNSUP = -1, -2
OBS, PC, PN, U, EPS, RNG, X, CORR = 0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000, 0x6000000, 0x7000000, 0x9000000


def test_symbols_declared_and_exported():
    lib = nv.lib()
    names = [s for s in nv.SYMBOLS if s.startswith("cstr_cql_")]
    assert sorted(names) == ["cstr_cql_candidates_f32", "cstr_cql_q_loss_f32"]
    assert all(hasattr(lib, n) for n in names)
    assert (nv.CQL_MAX_ACTIONS, nv.CQL_TAG) == (21, ref.CQL_TAG) and 3 * nv.CQL_MAX_ACTIONS + 1 == 64
    assert lib.cstr_abi_version() == 5


def test_candidates_rejects_bad_arguments_on_the_host():
    lib = nv.lib()

    def cand(obs=OBS, pc=PC, pn=PN, u=U, eps=EPS, rng=None, x=X, corr=CORR, batch=256, n=10, d=4, a=2, ldo=6, ldp=4, ldx=6):
        return lib.cstr_cql_candidates_f32(P(obs), i64(ldo), P(pc), P(pn), i64(ldp), i64(batch), ci(n), ci(d), ci(a), P(u), P(eps), P(rng),
                                           f32(-1.3862944), P(x), i64(ldx), P(corr), null)

    assert cand(obs=None) == BAD and cand(pc=None) == BAD and cand(pn=None) == BAD and cand(x=None) == BAD
    assert cand(batch=0) == BAD and cand(batch=-1) == BAD and cand(n=0) == BAD and cand(d=0) == BAD and cand(a=0) == BAD and cand(a=-2) == BAD
    assert cand(ldo=3) == BAD and cand(ldp=3) == BAD and cand(ldx=5) == BAD
    # exactly one noise source
    assert cand(rng=RNG) == BAD and cand(u=None, eps=None) == BAD and cand(u=None) == BAD and cand(eps=None) == BAD
    assert cand(u=None, rng=RNG) == BAD and cand(eps=None, rng=RNG) == BAD
    for k, base in dict(obs=OBS, pc=PC, pn=PN, u=U, eps=EPS, x=X, corr=CORR).items():  # rows off a 4-byte boundary
        assert cand(**{k: base + 2}) == BAD, k
    assert cand(u=None, eps=None, rng=RNG + 4) == BAD
    assert cand(a=nv.MAX_HEAD_ACT + 1, ldp=16, ldx=16) == UNSUP and cand(n=nv.CQL_MAX_ACTIONS + 1) == UNSUP
    assert cand(batch=nv.BCQ_MAX_ROWS // 30 + 1) == UNSUP
    # outputs over inputs and over each other
    assert cand(x=OBS) == BAD and cand(x=OBS + 4 * (255 * 6 + 3)) == BAD and cand(x=PC + 8) == BAD and cand(x=PN) == BAD
    assert cand(x=U + 4 * 100) == BAD and cand(x=EPS + 4 * (256 * 20 * 2 - 1)) == BAD and cand(corr=OBS) == BAD and cand(corr=EPS) == BAD
    assert cand(u=None, eps=None, rng=RNG, corr=RNG + 8) == BAD and cand(u=None, eps=None, rng=RNG, x=RNG - 4 * 6) == BAD
    assert cand(corr=X + 4 * 100) == BAD and cand(corr=X + 4 * (7680 * 6 - 1)) == BAD and cand(x=CORR - 4 * (7680 * 6 - 1)) == BAD


def test_q_loss_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    Q, Q1T, Q2T, NLP, REW, DONE, EC, TOUT, GQ, LOUT, LSUM, AUX = (0x1000000, 0x2000000, 0x2100000, 0x2200000, 0x2300000, 0x2400000, 0x2500000,
                                                                   0x3000000, 0x4000000, 0x5000000, 0x5000100, 0x5000200)
    rows = 31 * 256

    def loss(q=Q, corr=CORR, wd=0, q1t=Q1T, q2t=Q2T, nlp=NLP, rew=REW, done=DONE, ec=EC, gamma=0.99, w=5.0, temp=1.0, tout=TOUT, gq=GQ, lout=LOUT,
             lsum=LSUM, aux=AUX, batch=256, n=10, stride=rows):
        return lib.cstr_cql_q_loss_f32(P(q), i64(stride), P(corr), ci(wd), P(q1t), P(q2t), P(nlp), P(rew), P(done), P(ec), f32(gamma), f32(w),
                                       f32(temp), P(tout), P(gq), P(lout), P(lsum), P(aux), i64(batch), ci(n), null)

    for k in ("q", "q1t", "q2t", "rew", "done", "gq"):
        assert loss(**{k: None}) == BAD, k
    assert loss(batch=0) == BAD and loss(batch=-2) == BAD and loss(n=0) == BAD and loss(n=-1) == BAD
    assert loss(wd=2) == BAD and loss(wd=-1) == BAD and loss(corr=None) == BAD and loss(ec=None) == BAD
    assert loss(w=-0.1) == BAD and loss(w=float("nan")) == BAD and loss(temp=0.0) == BAD and loss(temp=-1.0) == BAD
    assert loss(temp=float("nan")) == BAD and loss(gamma=float("nan")) == BAD
    assert loss(stride=rows - 1) == BAD
    assert loss(n=nv.CQL_MAX_ACTIONS + 1, stride=67 * 256) == UNSUP and loss(batch=nv.MAX_SAMPLE_BATCH + 1, stride=31 * 16385) == UNSUP
    for k, base in dict(q=Q, corr=CORR, q1t=Q1T, q2t=Q2T, nlp=NLP, rew=REW, done=DONE, ec=EC, tout=TOUT, gq=GQ, lout=LOUT, lsum=LSUM,
                        aux=AUX).items():
        assert loss(**{k: base + 1}) == BAD, k
    # outputs over inputs, outputs over each other
    assert loss(gq=Q) == BAD and loss(gq=Q + 4 * (2 * rows - 1)) == BAD and loss(tout=Q1T) == BAD and loss(tout=CORR + 4 * 7679) == BAD
    assert loss(aux=REW + 4 * 255) == BAD and loss(lout=EC) == BAD and loss(lsum=DONE) == BAD and loss(gq=NLP - 4 * (2 * rows - 1)) == BAD
    assert loss(tout=GQ + 4 * (2 * rows - 1)) == BAD and loss(lout=GQ) == BAD and loss(lsum=LOUT) == BAD and loss(aux=LSUM - 12) == BAD
    assert loss(aux=TOUT + 4 * 255) == BAD


def test_hip_ops_wrappers_refuse_cpu_tensors():
    from core.common import hip_ops

    z = th.zeros
    with pytest.raises(ValueError, match="device"):
        hip_ops.cql_candidates(z(8, 4), z(8, 4), z(8, 4), 2, z(48, 6), z(8, 6), u=z(8, 2, 2), eps=z(8, 4, 2))
    with pytest.raises(ValueError, match="device"):
        hip_ops.cql_q_loss(z(2, 56, 1), z(8, 6), False, z(8), z(8), None, z(8), z(8), None, 0.99, 5.0, 1.0, z(8), z(2, 56, 1))
    with pytest.raises(ValueError, match="exactly one noise source"):
        hip_ops.cql_candidates(z(8, 4), z(8, 4), z(8, 4), 2, z(48, 6), z(8, 6))
    assert hip_ops.cql_supported(10, 2) and hip_ops.cql_supported(21, 4) and hip_ops.cql_supported(1, 1)
    assert not hip_ops.cql_supported(22, 2) and not hip_ops.cql_supported(10, 5) and not hip_ops.cql_supported(0, 2)
    assert hip_ops.cql_log_unif(2) == float(np.float32(2) * np.log(np.float32(0.5))) and hip_ops.cql_log_unif(3) == float(np.float32(3) * np.log(np.float32(0.5)))


def test_from_core_import_cql_and_signature():
    import core
    from core import CQL
    from core.common.offline_policy_algorithm import OfflineAlgorithm
    from core.cql import CQL as C2
    from core.sac import SAC
    from core.sac.policies import SACPolicy

    assert CQL is C2 and "CQL" in core.__all__ and issubclass(CQL, OfflineAlgorithm) and issubclass(CQL, SAC)
    assert CQL.policy_aliases == {"MlpPolicy": SACPolicy}
    sig = inspect.signature(CQL.__init__)
    got = [(k, p.default) for k, p in sig.parameters.items() if k not in ("self", "policy", "env")][:17]
    assert got == [("learning_rate", 3e-4), ("dataset", None), ("buffer_size", 1_000_000), ("batch_size", 256), ("tau", 0.005), ("gamma", 0.99),
                   ("gradient_steps", 1), ("ent_coef", "auto"), ("target_update_interval", 1), ("target_entropy", "auto"),
                   ("conservative_weight", 5.0), ("cql_n_actions", 10), ("cql_temp", 1.0), ("cql_importance_sample", True),
                   ("backup_entropy", False), ("behavior_cloning_warmup", 0), ("n_eval_episodes", 10)]
    rest = dict((k, p.default) for k, p in sig.parameters.items())
    assert rest["policy_kwargs"] is None and rest["seed"] is None and rest["device"] == "auto" and rest["_init_setup_model"] is True
    assert "learning_starts" not in rest and "train_freq" not in rest and "use_sde" not in rest
    assert not CQL.goal_face_support and CQL.chain_type is None
    assert "0.5 x the published" in inspect.getmodule(CQL).__doc__


def test_policy_keys_and_seeded_init_equal_sacpolicy():
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.cql.policies import CQLPolicy, MlpPolicy
    from core.sac.policies import SACPolicy

    pols = []
    for cls in (CQLPolicy, SACPolicy):
        set_random_seed(0)
        pols.append(cls(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4))
    a, b = (p.state_dict() for p in pols)
    assert MlpPolicy is SACPolicy and list(a) == list(b) and list(a)[0] == "actor.latent_pi.0.weight" and list(a)[-1] == "critic_target.qf1.4.bias"
    assert all(th.equal(a[k], b[k]) for k in a) and pols[0].net_arch == [256, 256]


def test_refusals_that_need_no_device(tmp_path):
    from core import CQL

    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'int'>"):
        CQL("MlpPolicy", None, dataset=5)
    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'NoneType'>"):
        CQL("MlpPolicy", None)
    with pytest.raises(FileNotFoundError, match="Dataset file not found"):
        CQL("MlpPolicy", None, dataset=str(tmp_path / "missing.pkl"))
    with pytest.raises(ValueError, match="does not support gSDE"):
        CQL("MlpPolicy", None, dataset=5, policy_kwargs=dict(use_sde=True))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="conservative_weight must be a non-negative number"):
            CQL("MlpPolicy", None, dataset=5, conservative_weight=bad)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="cql_temp must be a positive number"):
            CQL("MlpPolicy", None, dataset=5, cql_temp=bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="cql_n_actions must be a positive integer"):
            CQL("MlpPolicy", None, dataset=5, cql_n_actions=bad)
    np.savez(str(tmp_path / "d.npz"), observations=np.zeros((4, 1, 4)))
    with pytest.raises(ValueError, match="needs `env`"):
        CQL("MlpPolicy", None, dataset=str(tmp_path / "d.npz"))


# ---- the reference statements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("importance", [True, False])
@pytest.mark.parametrize("B,N,A", [(5, 3, 2), (1, 1, 1), (7, 4, 3)])
def test_explicit_gradients_equal_fp64_autograd(importance, B, N, A):
    case = ref.small_case(B=B, N=N, A=A, importance=importance, seed=B)
    for backup in (False, True):
        case["backup_entropy"] = backup
        auto, expl = ref.critic_step(case), ref.critic_step(case, explicit=True)
        assert ref.same_step(expl, auto, rtol=1e-12), (importance, backup)
        # and q_loss_torch (autograd w.r.t. q) against q_loss_f64 (term by term) on the same q
        rng = np.random.default_rng(B)
        q = rng.normal(-2, 1.5, (2, (1 + 3 * N) * B))
        corr = rng.normal(-1, 1, (B, 3 * N)) if importance else None
        args = (q, corr, not importance, case["q1_t"], case["q2_t"], case["next_logp"] if backup else None, case["rew"], case["done"], 0.3, 0.99,
                5.0, 0.7)
        a, b = ref.q_loss_f64(*args), ref.q_loss_torch(*args)
        assert abs(a["loss"] - b["loss"]) < 1e-12 * abs(b["loss"])
        for k in ("target", "aux", "lse", "gq"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("importance", [True, False])
def test_float32_torch_statement_passes_the_bars(importance):
    """float32 against fp64 at the project's convention on itself: a float32 evaluation is within 4 x its own distance by construction;
    what this pins is that the comparator runs on real shapes in both modes and that the distance is small against each output's scale
    (the statement is well conditioned at these sizes), so a bar of 4 x that distance is a tight one."""
    rng = np.random.default_rng(3)
    B, N = 65, 10
    q = rng.normal(-2, 1.5, (2, (1 + 3 * N) * B)).astype(np.float32)
    corr = rng.normal(-1, 1, (B, 3 * N)).astype(np.float32) if importance else None
    f = lambda *s: rng.normal(-3, 1, s).astype(np.float32)  # noqa: E731
    args = (q, corr, not importance, f(B), f(B), None, f(B), (rng.uniform(size=B) < 0.2).astype(np.float32), None, 0.99, 5.0, 1.0)
    want, got = ref.q_loss_f64(*args), ref.q_loss_torch(*args, dtype=th.float32)
    for k in ("target", "lse", "gq", "aux"):
        assert ref.close(got[k], want[k], got[k]) <= 1.0
        assert np.abs(got[k] - want[k]).max() <= 1e-5 * np.abs(want[k]).max(), k
    assert abs(got["loss"] - want["loss"]) < 16 * np.spacing(np.float32(abs(want["loss"])))


# (the two mistakes about the corrections exist only where the corrections do)
@pytest.mark.parametrize("importance,variant", [(imp, v) for imp in (True, False) for v in ref.VARIANTS
                                                if imp or v not in ("corr_added", "unif_sign")])
def test_comparator_rejects_the_mistakes(importance, variant):
    case = ref.small_case(importance=importance)
    want = ref.critic_step(case)
    assert ref.same_step(ref.critic_step(case), want) and ref.same_step(ref.critic_step(case, explicit=True), want)
    assert not ref.same_step(ref.critic_step(case, variant=variant), want, rtol=1e-6), variant


def test_candidates_layout_and_mode():
    rng = np.random.default_rng(0)
    B, N, D, A = 3, 2, 4, 2
    obs, pc, pn = rng.normal(size=(B, D)), rng.normal(size=(B, 2 * A)), rng.normal(size=(B, 2 * A))
    u, eps = rng.uniform(-1, 1, (B, N, A)), np.zeros((B, 2 * N, A))
    x, corr = ref.candidates(obs, pc, pn, u, eps)
    assert x.shape == (B * 3 * N, D + A) and corr.shape == (B, 3 * N)
    xr = x.reshape(B, 3 * N, D + A)
    assert np.array_equal(xr[:, :, :D], np.repeat(obs[:, None], 3 * N, 1)) and np.array_equal(xr[:, :N, D:], u)
    np.testing.assert_allclose(xr[:, N:2 * N, D:], np.repeat(np.tanh(pc[:, None, :A]), N, 1))  # eps = 0: the mode
    np.testing.assert_allclose(xr[:, 2 * N:, D:], np.repeat(np.tanh(pn[:, None, :A]), N, 1))
    np.testing.assert_allclose(corr[:, :N], A * np.log(0.5))
    # raw log_std beyond both clamp bounds
    pc[:, A:] = [30.0, -40.0]
    _, c2 = ref.candidates(obs, pc, pn, u, rng.normal(size=(B, 2 * N, A)))
    assert np.isfinite(c2).all()


def test_philox_restatement_against_the_array_restatement():
    """counter word 2 = 0 is what tests/_rowkernel_reference.py's array Philox evaluates: CQL's sub 0 block on the integer
    restatement equals it word for word (a carry into counter word 1 and a seed above 2^32 included)."""
    import _rowkernel_reference as rk

    seed, base, N = rk.HI_SEED, 2 ** 32 - 3, 2
    a, b = rk._uniform_pairs(seed, base, 8, ref.CQL_TAG)
    for i in range(8):
        w = ref._block(seed, base, i // N, i % N, N, 0)
        assert (w[0] >> 8, w[1] >> 8) == (int(a[i]), int(b[i]))
    u = ref.cql_uniforms(seed, base, 4, N, 2)
    assert u.dtype == np.float32 and (u >= -1).all() and (u < 1).all() and len(np.unique(u)) == u.size
    e = ref.cql_normals(seed, base, 64, N, 3)
    assert e.shape == (64, 4, 3) and abs(e.mean()) < 0.15 and 0.8 < e.std() < 1.2
    # the pi(.|s) and pi(.|s') draws of one sample come from the two halves of one block; sub 1 + p separates the column pairs
    w = ref._block(seed, base, 1, 1, N, 1)
    assert np.allclose(e[1, 1, :2], ref._box_muller(w[0], w[1])) and np.allclose(e[1, N + 1, :2], ref._box_muller(w[2], w[3]))
    assert e[1, 1, 2] == ref._box_muller(*ref._block(seed, base, 1, 1, N, 2)[:2])[0]


# the reference alone, K = 200 steps at (32, 32) / batch 64 / N = 4 / lr 3e-3 / seed 0 on BCQ's synthetic dataset: the mean of
# lse - Q(s, a) over 512 dataset rows and both critics is 3.985 after w = 0 and -0.173 after w = 5 (an untrained policy: about 3.9, the
# importance corrections of a narrow initial policy). tests/test_cql.py asserts the inequality on the kernels with the same arguments.
GAP_ARGS = ref.GAP_ARGS


def test_conservative_effect_on_the_reference():
    data = ref.synthetic_dataset()
    gaps = {w: ref.dataset_gap(ref.train_reference(data, w, **GAP_ARGS), data, 4, 1.0, rows=512) for w in (0.0, 5.0)}
    print(f"reference: mean(lse - Q(s,a)) after w=0: {gaps[0.0]:.3f}, after w=5: {gaps[5.0]:.3f}")
    assert gaps[5.0] < gaps[0.0] - 2.0, gaps


def test_float32_torch_statement_misses_the_per_element_q_bar_at_an_untrained_critic():
    """Why tests/test_cql.py's teacher-forced runs start from critics whose output bias is the dataset's mean reward. The reference's own
    statements (RefCQL: plain torch, torch.optim.Adam, CPU ATen) in float32 against float64, class defaults, batch 256, N = 10, two steps
    from the SEEDED INITIAL WEIGHTS: an untrained critic gives Q = 0 +- 0.1, and tests/_parity_helpers.py q_err's per-element bar
    |dq| <= 5e-5 max(|q|, 1e-3) then asks for 5e-8 of a sum of 256 terms of size 0.1. Measured here (two seeds): at the second step the
    float32 statement is at 1.1e-4 and 1.3e-4 of max(|q|, 1e-3) -- beyond the 5e-5 of the hand-written path, the 6e-5 of rocBLAS and the 1e-4
    of ATen -- while relative to the batch's Q scale it is at 1e-6. With the output biases at the mean reward the same evaluation is at
    7e-8 per element. Asserted with a margin for another machine's float32 sums: unmodified start beyond 5e-5 on at least one seed
    and everywhere below 1e-5 of the batch scale; biased start below a quarter of the tightest bar (1.25e-5) per element."""
    import copy

    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.sac.policies import SACPolicy

    rows, B, N = 2048, 256, 10
    strict = {False: [], True: []}
    for seed in (0, 1):
        for biased in (False, True):
            set_random_seed(seed)
            pol = SACPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4)
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
            r64 = ref.RefCQL(copy.deepcopy(pol).double(), 3e-4, 0.99, 0.005, 5.0, N, 1.0)
            r32 = ref.RefCQL(copy.deepcopy(pol).float(), 3e-4, 0.99, 0.005, 5.0, N, 1.0, dtype=th.float32)
            for k in range(2):
                idx = rng.integers(0, rows, B)
                noise = [x.astype(np.float32) for x in (rng.normal(size=(B, 2)), rng.normal(size=(B, 2)), rng.uniform(-1, 1, (B, N, 2)),
                                                        rng.normal(size=(B, 2 * N, 2)))]
                args = (obs[idx], act[idx], nobs[idx], rew[idx], done[idx], *noise)
                want, got = r64.step(*args), r32.step(*args)
            for i in range(2):  # the second step's Q values: after one float32 Adam step
                w_, g = want["current_q"][i], got["current_q"][i].astype(np.float64)
                strict[biased].append(float((np.abs(g - w_) / np.maximum(np.abs(w_), 1e-3)).max()))
                assert np.abs(g - w_).max() <= 1e-5 * np.abs(w_).mean(), (seed, biased, i)
    print("float32 torch statement, per-element |dq| / max(|q|, 1e-3) at the second step: seeded start "
          + ", ".join(f"{v:.2e}" for v in strict[False]) + "; output biases at the mean reward " + ", ".join(f"{v:.2e}" for v in strict[True]))
    assert max(strict[False]) > 5e-5 and max(strict[True]) < 1.25e-5, strict
