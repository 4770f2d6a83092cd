"""CPU-side checks of the MultiCategorical head of PPO / A2C on the MultiDiscrete valve face: the two cstr_multicategorical entry
points are exported and reject bad arguments on the host (nothing is dereferenced or launched); the MultiDiscrete space and
as_multi_discrete; the env face's level values and constructor refusals; PPO and A2C admit the space, SAC, TD3 and DQN refuse it with
the reference's assertion wording; ActorCriticPolicy on MultiDiscrete([K0, K1]) has the reference's state_dict keys and seeded initial
weights and no log_std (tests/golden/ppo_mcat_*.npz, a2c_mcat_*.npz, written by the unmodified reference:
tools/refharness/gen_golden.py gen_ppo_multidiscrete / gen_a2c_multidiscrete); MultiDiscrete([2, 2]) builds the multi-categorical
form although its four logits are a square; MultiCategoricalDistribution against torch's Categorical per split; and the fp64
restatement of the loss that tests/test_multicategorical.py holds the kernel to against the reference's own recorded scalars -- the
yardstick is checked before the GPU run."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import _mcat_helpers as mh
import test_categorical_abi as tca
from _parity_helpers import check_init
from core import _native as nv

i64 = C.c_int64
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
P, off = tca.P, tca.off
MCAT_SYMBOLS = ("cstr_multicategorical_act_f32", "cstr_multicategorical_loss_f32")


def test_symbols_declared_and_exported():
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in MCAT_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive
    assert C.sizeof(nv.MultiCategoricalLoss) == C.sizeof(nv.CategoricalLoss) == 8 * 8 + 8 + 4 * 4 + 2 * 8 + 2 * 4 + 5 * 8
    assert nv.MCAT_MAX_LEVELS == 32


def act(z=P(0), ldz=8, n=8, k0=3, k1=5, det=0, a_in=null, u=P(1), rng=null, af=P(2), a_out=null, valve=P(3), logp=P(4), u_out=null):
    return nv.lib().cstr_multicategorical_act_f32(z, i64(ldz), i64(n), k0, k1, det, a_in, u, rng, af, a_out, valve, logp, u_out, null)


def test_act_rejects_bad_arguments_on_the_host():
    # every call below fails a host-side check: none reaches a launch (the pointers are fake)
    assert act(z=null) == BAD and act(af=null) == BAD and act(n=0) == BAD and act(k0=0) == BAD and act(k1=-1) == BAD and act(ldz=7) == BAD
    assert act(k0=1) == UNSUP and act(k1=1) == UNSUP and act(k0=33, ldz=64) == UNSUP and act(k1=33, ldz=64) == UNSUP
    assert act(n=(1 << 30) + 1) == UNSUP
    assert act(u=null) == BAD                                                    # no source
    assert act(det=1) == BAD and act(a_in=P(5)) == BAD and act(rng=P(5)) == BAD  # two sources
    assert act(u=null, a_in=P(5), rng=P(6)) == BAD
    assert act(u=null, det=1, u_out=P(7)) == BAD                                 # no uniforms to keep
    assert act(af=off(P(0), 16)) == BAD and act(logp=P(0)) == BAD                # an output inside the logits
    assert act(valve=P(2)) == BAD and act(a_out=P(4)) == BAD                     # two outputs over each other
    assert act(u_out=P(1)) == BAD                                                # the kept uniforms on the given ones
    assert act(z=off(P(0), 2)) == BAD and act(valve=off(P(3), 4)) == BAD and act(a_out=off(P(6), 4)) == BAD and act(af=off(P(2), 4)) == BAD
    assert act(u=off(P(1), 4)) == BAD and act(u_out=off(P(7), 4)) == BAD         # rows of pairs are 8-byte aligned
    assert act(u=null, rng=off(P(5), 4)) == BAD and act(u=null, a_in=off(P(5), 4)) == BAD


def loss_args(**kw):
    d = dict(logits=P(0), ldz=8, actions=P(1), values=P(2), old_values=null, old_log_prob=P(3), adv=P(4), returns=P(5), batch=12, levels0=3,
             levels1=5, objective=0, normalize_advantage=1, clip_range=0.2, clip_range_vf=-1.0, ent_coef=0.0, vf_coef=0.5, g_logits=P(6),
             g_value=P(7), scalars_out=P(8), scalars_sum=null, log_prob_out=null)
    d.update(kw)
    p = nv.MultiCategoricalLoss()
    for k, v in d.items():
        setattr(p, k, v.value if isinstance(v, C.c_void_p) else v)
    return p


def test_loss_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    loss = lambda ws=P(9), **kw: lib.cstr_multicategorical_loss_f32(C.byref(loss_args(**kw)), ws, null)  # noqa: E731
    # every call below fails a host-side check: none reaches a launch (the pointers are fake)
    assert lib.cstr_multicategorical_loss_f32(null, P(9), null) == BAD and loss(ws=null) == BAD
    for name in ("logits", "actions", "values", "adv", "returns", "g_logits", "g_value", "old_log_prob"):
        assert loss(**{name: null}) == BAD, name
    assert loss(batch=0) == BAD and loss(levels0=0) == BAD and loss(levels1=0) == BAD and loss(ldz=7) == BAD
    assert loss(objective=2) == BAD and loss(objective=-1) == BAD
    assert loss(clip_range_vf=0.2) == BAD                                      # value clipping needs old_values
    assert loss(objective=1, old_log_prob=null, g_value=P(2)) == BAD          # A2C needs no old log-probs: held to the next checks
    assert loss(objective=1, old_log_prob=null, clip_range_vf=0.2, levels0=33, ldz=64) == UNSUP  # ... nor a value clip
    assert loss(clip_range=float("nan")) == BAD
    assert loss(levels0=1) == UNSUP and loss(levels1=1) == UNSUP and loss(levels0=33, ldz=64) == UNSUP and loss(levels1=33, ldz=64) == UNSUP
    assert loss(batch=(1 << 30) + 1) == UNSUP
    assert loss(ws=off(P(9), 4)) == BAD and loss(logits=off(P(0), 2)) == BAD and loss(g_value=off(P(7), 1)) == BAD
    assert loss(actions=off(P(1), 4)) == BAD                                   # the pair rows are 8-byte aligned
    assert loss(g_logits=P(0)) == BAD and loss(g_logits=off(P(0), 64)) == BAD  # the gradient on / inside the logits
    assert loss(g_value=P(2)) == BAD and loss(scalars_out=P(4)) == BAD and loss(log_prob_out=P(3)) == BAD and loss(ws=P(6)) == BAD
    assert loss(scalars_sum=P(8)) == BAD and loss(log_prob_out=P(7)) == BAD
    assert loss(g_value=off(P(1), 8 * 11)) == BAD  # inside the last of the [batch][2] action rows


def test_wrappers_know_the_face():
    from core.common import hip_ops

    assert hip_ops.multicategorical_supported(4, (2, 2)) and hip_ops.multicategorical_supported(8, (32, 2))
    assert not hip_ops.multicategorical_supported(4, (1, 5)) and not hip_ops.multicategorical_supported(4, (33, 5))
    assert not hip_ops.multicategorical_supported(4, (3, 5, 2)) and not hip_ops.multicategorical_supported(6, (3, 5))
    assert hip_ops.rollout_supported(4, 2)  # the pair row is the Gaussian head's width: add and gather are reused


def test_multi_discrete_space():
    from core.common.spaces import Box, Discrete, MultiDiscrete, as_box, as_discrete, as_multi_discrete, get_action_dim

    s = MultiDiscrete([3, 5])
    assert s.shape == (2,) and s.dtype == np.int64 and s.nvec.dtype == np.int64 and s.nvec.tolist() == [3, 5]
    assert repr(s) == "MultiDiscrete([3 5])" and s == MultiDiscrete((3, 5)) and s != MultiDiscrete([5, 3]) and s != MultiDiscrete([3, 5, 2])
    assert s != Discrete(15) and s != Box(-1, 1, (2,)) and Discrete(15) != s
    assert s.contains(np.array([2, 4])) and s.contains([0, 0]) and not s.contains(np.array([3, 0])) and not s.contains(np.array([0, 5]))
    assert not s.contains(np.array([-1, 0])) and not s.contains(np.array([1.0, 2.0])) and not s.contains(np.array([1, 2, 0])) and not s.contains(1)
    s.seed(0)
    draws = np.stack([s.sample() for _ in range(200)])
    assert draws.dtype == np.int64 and draws.shape == (200, 2) and all(s.contains(d) for d in draws)
    assert set(draws[:, 0]) == {0, 1, 2} and set(draws[:, 1]) == {0, 1, 2, 3, 4}
    batch = s.sample_batch(7)
    assert batch.shape == (7, 2) and batch.dtype == np.int64
    s.seed(0)
    assert np.array_equal(np.stack([s.sample() for _ in range(200)]), draws)  # the space's own generator
    for bad in ([], [[2, 2]], [3, 0], 4):
        with pytest.raises(ValueError):
            MultiDiscrete(bad)
    assert get_action_dim(s) == 2 and get_action_dim(MultiDiscrete([4, 4, 4])) == 3 and get_action_dim(Discrete(9)) == 1
    assert as_discrete(s) is None and as_multi_discrete(s) is s and as_multi_discrete(Discrete(9)) is None and as_multi_discrete(Box(-1, 1, (2,))) is None
    duck = type("GymMultiDiscrete", (), {"nvec": np.array([3, 5]), "shape": (2,), "dtype": np.dtype(np.int64)})()
    assert as_multi_discrete(duck) == s and as_discrete(duck) is None
    assert as_multi_discrete(type("Grid", (), {"nvec": np.array([[3, 5]])})()) is None  # a 1-D nvec only
    assert as_discrete(Discrete(4)) == Discrete(4) and as_box(Box(-1, 1, (2,))) == Box(-1, 1, (2,))  # what they returned before
    with pytest.raises(ValueError, match="Unsupported space"):
        as_box(s)


def test_env_face_refusals_and_level_values(monkeypatch):
    """the constructor's refusals come before the device is touched; the level values against the NumPy float32 statement"""
    from core.common.vec_env import CSTRVecEnv
    from core.common.vec_env import cstr_vec_env as ve

    for kw, msg in ((dict(twin=True, obs_dim=8), "twin=False"), (dict(discrete_actions=3), "discrete_actions"),
                    (dict(goal_conditioned=True), "goal_conditioned")):
        with pytest.raises(ValueError, match=msg):
            CSTRVecEnv(2, multi_discrete_actions=(3, 5), device="cpu", **kw)
    for bad in (1, 33, (3,), (3, 5, 2), (1, 5), (3, 33), (3.0, 5), (True, 5)):
        with pytest.raises(ValueError, match="multi_discrete_actions must be"):
            CSTRVecEnv(2, multi_discrete_actions=bad, device="cpu")
    assert ve.MAX_MULTI_VALVE_LEVELS == nv.MCAT_MAX_LEVELS == 32 and ve.MAX_VALVE_LEVELS == 16  # the joint face keeps its bound
    nvec = (2, 32)
    pairs = np.array([[0, 0], [1, 31], [0, 17], [1, 5]], np.int64)
    got = ve.decode_valve_levels(pairs, nvec)
    want = np.stack([np.float32(-1) + (2 * pairs[:, 0]).astype(np.float32) / np.float32(1),
                     np.float32(-1) + (2 * pairs[:, 1]).astype(np.float32) / np.float32(31)], axis=-1)
    assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes() == mh.valves_np(pairs, nvec).tobytes()
    assert got[0].tolist() == [-1.0, -1.0] and got[1].tolist() == [1.0, 1.0]
    assert np.array_equal(ve.valve_levels(32), np.float32(-1) + (2 * np.arange(32)).astype(np.float32) / np.float32(31))


class _MultiEnv:
    num_envs = 2

    def __init__(self, nvec=(3, 5)):
        from core.common.spaces import Box, MultiDiscrete

        self.observation_space, self.action_space = Box(-1, 1, (4,)), MultiDiscrete(list(nvec))

    def reset(self):
        return np.zeros((2, 4), np.float32)

    def step(self, actions):
        raise NotImplementedError


def test_who_admits_a_multi_discrete_action_space(monkeypatch):
    """the constructors' action-space check (no device is touched: the model is not set up)"""
    from core.a2c import A2C
    from core.common import base_class
    from core.common.spaces import MultiDiscrete
    from core.dqn import DQN
    from core.ppo import PPO
    from core.sac import SAC
    from core.td3 import TD3

    monkeypatch.setattr(base_class, "get_device", lambda device: th.device("cpu"))
    for cls in (PPO, A2C):
        model = cls("MlpPolicy", _MultiEnv(), _init_setup_model=False)  # "Unsupported space" before this head existed
        assert model.action_space == MultiDiscrete([3, 5]) and model.n_envs == 2
    for cls in (SAC, TD3):  # the reference's assertion, not as_box's "Unsupported space"
        with pytest.raises(AssertionError, match=r"The algorithm only supports .* as action spaces but MultiDiscrete\(\[3 5\]\) was provided"):
            cls("MlpPolicy", _MultiEnv(), _init_setup_model=False)
    with pytest.raises(AssertionError, match=r"only supports .*Discrete.* but MultiDiscrete\(\[3 5\]\) was provided"):
        DQN("MlpPolicy", _MultiEnv())
    assert tca._DiscreteEnv().action_space != _MultiEnv().action_space
    for cls in (SAC, TD3):  # the joint face's refusal is what it was
        with pytest.raises(AssertionError, match="only supports"):
            cls("MlpPolicy", tca._DiscreteEnv(), _init_setup_model=False)


@pytest.mark.parametrize("name,algo", [("ppo_mcat_train_kat_small.npz", "PPO"), ("ppo_mcat_train_kat_default.npz", "PPO"),
                                       ("a2c_mcat_train_kat_small.npz", "A2C")])
def test_policy_keys_and_seeded_initial_weights(golden, name, algo):
    import core
    from core.common.spaces import Box, MultiDiscrete

    g = golden(name)
    nvec = [int(k) for k in g["nvec"]]
    cls = getattr(core, algo)
    kw = dict(net_arch=[int(w) for w in g["net_arch"]])
    if algo == "A2C":
        kw.update(cls._rewrite_policy_kwargs({}, True, 1e-5))
    threads = th.get_num_threads()
    th.set_num_threads(1)  # the fixture's run: LAPACK's QR of a 64 x 64 matrix rounds differently when it is threaded
    try:
        th.manual_seed(int(g["seed"]))  # set_random_seed(seed) of the fixture's run
        pol = cls.policy_aliases["MlpPolicy"](Box(-1, 1, (4,)), MultiDiscrete(nvec), lambda _: float(g["learning_rate"]), **kw)
    finally:
        th.set_num_threads(threads)
    keys = [str(k) for k in g["state_dict_keys"]]
    assert list(pol.state_dict()) == keys and len(keys) == 12 and not hasattr(pol, "log_std") and "log_std" not in keys
    assert pol.action_net.out_features == sum(nvec) and pol.action_net.in_features == int(g["net_arch"][-1])
    assert pol.multi_discrete and not pol.discrete and tuple(pol.state_dict()["action_net.weight"].shape) == (sum(nvec), int(g["net_arch"][-1]))
    check_init(type("M", (), {"policy": pol})(), g, ["policy"])
    obs = th.as_tensor(g["init_obs"])
    n = len(obs)
    with th.no_grad():
        a, v, lp = pol(obs)
        a_det, _, _ = pol(obs, deterministic=True)
        v2, lp2, ent = pol.evaluate_actions(obs, a.float())  # the buffer's [n, 2] float rows
        dist = pol.get_distribution(obs)
    assert a.dtype == th.int64 and tuple(a.shape) == (n, 2) and tuple(v.shape) == (n, 1) and tuple(lp.shape) == (n,)
    assert th.equal(lp, lp2) and th.equal(v, v2) and tuple(ent.shape) == (n,) and th.equal(dist.mode(), a_det)
    pairs, state = pol.predict(g["init_obs"], deterministic=True)
    assert state is None and pairs.dtype == np.int64 and pairs.shape == (n, 2) and np.array_equal(pairs, a_det.numpy())
    one, _ = pol.predict(g["init_obs"][0], deterministic=True)
    assert one.shape == (2,) and one.dtype == np.int64 and np.array_equal(one, pairs[0])


def test_four_logits_of_two_valves_are_not_a_joint_face():
    """MultiDiscrete([2, 2]) and Discrete(4) both have four logits: the form follows the space, never the width"""
    from core.common.fused import FastActorCritic
    from core.common.policies import ActorCriticPolicy
    from core.common.spaces import Box, Discrete, MultiDiscrete

    multi = ActorCriticPolicy(Box(-1, 1, (4,)), MultiDiscrete([2, 2]), lambda _: 3e-4)
    joint = ActorCriticPolicy(Box(-1, 1, (4,)), Discrete(4), lambda _: 3e-4)
    assert multi.action_net.out_features == joint.action_net.out_features == 4 and FastActorCritic.face_levels(4) == 2
    assert multi.multi_discrete and not multi.discrete and joint.discrete and not joint.multi_discrete
    fm, fj = FastActorCritic(multi), FastActorCritic(joint)
    assert fm.multi_discrete and not fm.discrete and fm.nvec == (2, 2) and fm.act_dim == 2 and not hasattr(fm, "levels")
    assert fj.discrete and not fj.multi_discrete and fj.levels == 2 and fj.act_dim == 1
    assert type(multi.action_dist).__name__ == "MultiCategoricalDistribution" and type(joint.action_dist).__name__ == "CategoricalDistribution"


def test_multi_categorical_distribution_against_torch():
    from core.common.distributions import MultiCategoricalDistribution

    th.manual_seed(3)
    logits = th.randn(7, 8) * 2
    d = MultiCategoricalDistribution([3, 5])
    net = d.proba_distribution_net(latent_dim=6)
    assert isinstance(net, th.nn.Linear) and (net.in_features, net.out_features) == (6, 8)
    refs = [th.distributions.Categorical(logits=logits[:, :3]), th.distributions.Categorical(logits=logits[:, 3:])]
    assert d.proba_distribution(logits) is d
    a = th.stack([th.arange(7) % 3, th.arange(7) % 5], dim=1)
    assert th.equal(d.log_prob(a), th.stack([refs[0].log_prob(a[:, 0]), refs[1].log_prob(a[:, 1])], dim=1).sum(dim=1))
    assert th.equal(d.log_prob(a.float()), d.log_prob(a))  # the buffer's float rows: Categorical.log_prob takes value.long()
    assert th.equal(d.entropy(), th.stack([refs[0].entropy(), refs[1].entropy()], dim=1).sum(dim=1))
    mode = th.stack([th.argmax(refs[0].probs, dim=1), th.argmax(refs[1].probs, dim=1)], dim=1)
    assert th.equal(d.mode(), mode) and th.equal(d.get_actions(deterministic=True), mode)
    s = d.sample()
    assert s.dtype == th.int64 and tuple(s.shape) == (7, 2) and int(s.min()) >= 0 and int(s[:, 0].max()) < 3 and int(s[:, 1].max()) < 5
    d.action_queue.append(a)  # the teacher-forcing hook
    assert th.equal(d.get_actions(), a) and not d.action_queue
    assert th.equal(d.actions_from_params(logits, deterministic=True), mode)
    acts, lp = d.log_prob_from_params(logits)
    assert th.equal(lp, refs[0].log_prob(acts[:, 0]) + refs[1].log_prob(acts[:, 1]))


def minibatch_case(g, pre, rpre, rows):
    obs = tca.flat(g[f"{rpre}rollout/observations"])[rows]
    z = tca.mlp_f64(g, pre, "policy_net", "action_net", obs)
    values = tca.mlp_f64(g, pre, "value_net", "value_net", obs).reshape(-1)
    f = lambda name: tca.flat(g[f"{rpre}rollout/{name}"]).reshape(-1)[rows]  # noqa: E731
    return dict(z=z, a=tca.flat(g[f"{rpre}rollout/actions"])[rows].astype(np.int64), old_lp=f("log_probs"), values=values,
                old_values=f("values"), adv=f("advantages"), returns=f("returns"))


@pytest.mark.parametrize("name", ["small", "default"])
def test_fp64_restatement_reproduces_the_reference_ppo(golden, name):
    """the first minibatch of the fixture (the `before` weights, rows permutations[0][:batch]): scalars, values and log-probs of the
    f32 reference within 1e-5 of the fp64 statement tests/test_multicategorical.py applies to the kernel"""
    g = golden(f"ppo_mcat_train_kat_{name}.npz")
    nvec = tuple(int(k) for k in g["nvec"])
    assert g["rollout/actions"].shape == (int(g["n_steps"]), int(g["n_envs"]), 2) and g["rollout/actions"].dtype == np.float32
    assert (g["rollout/actions"] >= 0).all() and (g["rollout/actions"].reshape(-1, 2).max(axis=0) < np.array(nvec)).all()
    rows = g["permutations"][0][:int(g["batch_size"])]
    c = minibatch_case(g, "before", "", rows)
    scal, _, _, lp, _ = mh.loss_torch(c, nvec, 0, th.float64, True, float(g["ent_coef"]), float(g["vf_coef"]), clip_range=float(g["clip_range"]))
    want = g["mb0/scalars"].astype(np.float64)
    assert np.abs(c["values"] - g["mb0/values"].reshape(-1)).max() <= 1e-5 * max(np.abs(g["mb0/values"]).mean(), 1e-3) * 10
    assert np.abs(lp - g["mb0/log_prob"]).max() <= 1e-5 * np.abs(g["mb0/log_prob"]).mean()
    for k in range(5):
        assert abs(scal[k] - want[k]) <= 1e-5 * max(abs(want[k]), 1.0), (k, scal[k], want[k])
    assert scal[5] == want[5]
    # the rollout's own log-probs are the log-probs of the stored pairs under the `before` weights: ratio 1 in the first minibatch
    assert abs(want[4]) < 1e-6 and want[5] == 0.0


def test_fp64_restatement_reproduces_the_reference_a2c(golden):
    g = golden("a2c_mcat_train_kat_small.npz")
    nvec = tuple(int(k) for k in g["nvec"])
    for it in range(int(g["iterations"])):
        pre = "before" if it == 0 else f"it{it - 1}/after"
        rows = g[f"it{it}/permutation"]
        c = minibatch_case(g, pre, f"it{it}/", rows)
        scal, _, _, lp, _ = mh.loss_torch(c, nvec, 1, th.float64, False, float(g["ent_coef"]), float(g["vf_coef"]))
        want = g[f"it{it}/scalars"].astype(np.float64)
        assert np.abs(lp - g[f"it{it}/log_prob"]).max() <= 1e-5 * np.abs(g[f"it{it}/log_prob"]).mean()
        for k in range(4):
            assert abs(scal[k] - want[k]) <= 1e-5 * max(abs(want[k]), 1.0), (it, k, scal[k], want[k])
        assert g[f"it{it}/rollout/actions"].shape == (int(g["n_steps"]), int(g["n_envs"]), 2) and g[f"it{it}/rollout/actions"].dtype == np.float32


def test_predict_fixture_is_consistent(golden):
    g = golden("ppo_mcat_predict_kat.npz")
    nvec = tuple(int(k) for k in g["nvec"])
    z = tca.mlp_f64({f"before/{k}": g[k] for k in g.files}, "before", "policy_net", "action_net", g["obs"])
    assert g["deterministic"].dtype == np.int64 and g["deterministic"].shape == (16, 2) and np.abs(z - g["logits"]).max() < 1e-5
    for v, (z64, z32) in enumerate(zip(mh.split(z, nvec), mh.split(g["logits"], nvec))):
        assert np.array_equal(z64.argmax(axis=1), g["deterministic"][:, v])
        top = np.sort(z32, axis=1)
        assert ((top[:, -1] - top[:, -2]) > 1e-4 * np.abs(g["logits"]).max()).all()  # every row, per valve: the tests leave out none


# ---- the arguments the four loss structs share: one table of bad values through all four entry points ------------------------------
SHARED = dict(values=P(2), adv=P(4), returns=P(5), g_value=P(7), scalars_out=P(8), log_prob_out=null, batch=12, normalize_advantage=1,
              ent_coef=0.0, vf_coef=0.5)
PPO_ONLY = dict(old_values=null, old_log_prob=P(3), clip_range=0.2, clip_range_vf=-1.0, scalars_sum=null)
GAUSSIAN = dict(mean=P(0), ldm=2, log_std=P(10), actions=P(1), act_dim=2, g_mean=P(6), g_log_std=P(11))
LOSS_ENTRY_POINTS = {
    "ppo": ("cstr_ppo_loss_f32", nv.PpoLoss, dict(SHARED, **PPO_ONLY, **GAUSSIAN)),
    "a2c": ("cstr_a2c_loss_f32", nv.A2cLoss, dict(SHARED, **GAUSSIAN)),
    "categorical": ("cstr_categorical_loss_f32", nv.CategoricalLoss,
                    dict(SHARED, **PPO_ONLY, logits=P(0), ldz=16, actions=P(1), n_actions=9, levels=3, objective=0, g_logits=P(6))),
    "multicategorical": ("cstr_multicategorical_loss_f32", nv.MultiCategoricalLoss,
                         dict(SHARED, **PPO_ONLY, logits=P(0), ldz=8, actions=P(1), levels0=3, levels1=5, objective=0, g_logits=P(6))),
}


@pytest.mark.parametrize("entry", list(LOSS_ENTRY_POINTS))
def test_loss_entry_points_agree_on_bad_shared_arguments(entry):
    """every call fails a host-side check: none reaches a launch (the pointers are fake)"""
    symbol, struct, base = LOSS_ENTRY_POINTS[entry]
    fn = getattr(nv.lib(), symbol)

    def loss(ws=P(9), **kw):
        p = struct()
        for k, v in dict(base, **kw).items():
            setattr(p, k, v.value if isinstance(v, C.c_void_p) else v)
        return fn(C.byref(p), ws, null)

    assert loss(ws=null) == BAD
    for name in ("values", "adv", "returns", "g_value"):  # each shared required pointer
        assert loss(**{name: null}) == BAD, name
    assert loss(ws=off(P(9), 4)) == BAD                   # the workspace holds 8-byte words
    assert loss(g_value=P(2)) == BAD                      # g_value over values
    assert loss(scalars_out=P(4)) == BAD                  # scalars_out over adv
    assert loss(log_prob_out=P(7)) == BAD                 # log_prob_out over g_value
    assert loss(ws=P(7)) == BAD and loss(ws=P(8)) == BAD  # the workspace over an output
    assert loss(batch=(1 << 30) + 1) == UNSUP
    if "scalars_sum" in base:
        assert loss(scalars_sum=P(8)) == BAD              # scalars_sum over scalars_out
        assert loss(old_log_prob=null) == BAD             # the PPO objective reads it
