"""CPU-side checks of the Categorical head of PPO / A2C: the two cstr_categorical entry points are exported and reject bad arguments
on the host (nothing is dereferenced or launched), the rollout add / gather argument checks take act_dim 1, PPO and A2C admit a
Discrete action space (SAC and TD3 still refuse it), ActorCriticPolicy on a Discrete space has the reference's state_dict keys and
seeded initial weights and no log_std (tests/golden/ppo_cat_*.npz, a2c_cat_*.npz, written by the unmodified reference:
tools/refharness/gen_golden.py gen_ppo_discrete / gen_a2c_discrete), CategoricalDistribution against torch's Categorical, and the
fp64 restatement of the loss that tests/test_categorical.py holds the kernel to against the reference's own recorded scalars -- the
yardstick is checked before the GPU run."""
import ctypes as C
import re

import numpy as np
import pytest
import torch as th

import test_categorical as tc
from core import _native as nv

i64 = C.c_int64
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
CAT_SYMBOLS = ("cstr_categorical_act_f32", "cstr_categorical_loss_f32")


def P(k: int) -> C.c_void_p:
    """the k-th of a set of fake, well separated, 256-byte-aligned device addresses (never dereferenced)"""
    return C.c_void_p(0x1000000 * (k + 1))


def off(p: C.c_void_p, nbytes: int) -> C.c_void_p:
    return C.c_void_p(p.value + nbytes)


def test_symbols_declared_and_exported():
    import os

    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in CAT_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cstr_rl_hip.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|void|const char \*)\s*(cstr_\w+)\(", header, flags=re.M)))
    assert sorted(nv.SYMBOLS) == declared
    assert C.sizeof(nv.CategoricalLoss) == 8 * 8 + 8 + 4 * 4 + 2 * 8 + 2 * 4 + 5 * 8


def act(z=P(0), ldz=9, n=8, m=9, k=3, det=0, a_in=null, u=P(1), rng=null, idx=P(2), index=null, valve=P(3), logp=P(4), u_out=null):
    return nv.lib().cstr_categorical_act_f32(z, i64(ldz), i64(n), m, k, det, a_in, u, rng, idx, index, valve, logp, u_out, null)


def test_act_rejects_bad_arguments_on_the_host():
    # every call below fails a host-side check: none reaches a launch (the pointers are fake)
    assert act(z=null) == BAD and act(idx=null) == BAD and act(n=0) == BAD and act(m=0) == BAD and act(ldz=8) == BAD
    assert act(k=1, m=1, ldz=1) == UNSUP and act(k=17, m=289, ldz=289) == UNSUP and act(m=10, ldz=10) == UNSUP
    assert act(n=(1 << 30) + 1) == UNSUP
    assert act(u=null) == BAD                                                    # no source
    assert act(det=1) == BAD and act(a_in=P(5)) == BAD and act(rng=P(5)) == BAD  # two sources
    assert act(u=null, a_in=P(5), rng=P(6)) == BAD
    assert act(u=null, det=1, u_out=P(7)) == BAD                                 # no uniform to keep
    assert act(idx=off(P(0), 16)) == BAD and act(logp=P(0)) == BAD               # an output inside the logits
    assert act(valve=P(2)) == BAD and act(index=P(4)) == BAD                     # two outputs over each other
    assert act(u_out=P(1)) == BAD                                                # the kept uniforms on the given ones
    assert act(z=off(P(0), 2)) == BAD and act(valve=off(P(3), 4)) == BAD and act(index=off(P(6), 4)) == BAD
    assert act(u=null, rng=off(P(5), 4)) == BAD and act(u=null, a_in=off(P(5), 4)) == BAD


def loss_args(**kw):
    d = dict(logits=P(0), ldz=9, actions=P(1), values=P(2), old_values=null, old_log_prob=P(3), adv=P(4), returns=P(5), batch=12, n_actions=9,
             levels=3, objective=0, normalize_advantage=1, clip_range=0.2, clip_range_vf=-1.0, ent_coef=0.0, vf_coef=0.5, g_logits=P(6),
             g_value=P(7), scalars_out=P(8), scalars_sum=null, log_prob_out=null)
    d.update(kw)
    p = nv.CategoricalLoss()
    for k, v in d.items():
        setattr(p, k, v.value if isinstance(v, C.c_void_p) else v)
    return p


def test_loss_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    loss = lambda ws=P(9), **kw: lib.cstr_categorical_loss_f32(C.byref(loss_args(**kw)), ws, null)  # noqa: E731
    # every call below fails a host-side check: none reaches a launch (the pointers are fake)
    assert lib.cstr_categorical_loss_f32(null, P(9), null) == BAD and loss(ws=null) == BAD
    for name in ("logits", "actions", "values", "adv", "returns", "g_logits", "g_value", "old_log_prob"):
        assert loss(**{name: null}) == BAD, name
    assert loss(batch=0) == BAD and loss(n_actions=0) == BAD and loss(ldz=8) == BAD
    assert loss(objective=2) == BAD and loss(objective=-1) == BAD
    assert loss(clip_range_vf=0.2) == BAD                                      # value clipping needs old_values
    assert loss(objective=1, old_log_prob=null, g_value=P(2)) == BAD          # A2C needs no old log-probs: held to the next checks
    assert loss(objective=1, old_log_prob=null, clip_range_vf=0.2, levels=17, n_actions=289, ldz=289) == UNSUP  # ... nor a value clip
    assert loss(clip_range=float("nan")) == BAD
    assert loss(levels=1, n_actions=1, ldz=1) == UNSUP and loss(levels=17, n_actions=289, ldz=289) == UNSUP and loss(n_actions=8) == UNSUP
    assert loss(batch=(1 << 30) + 1) == UNSUP
    assert loss(ws=off(P(9), 4)) == BAD and loss(logits=off(P(0), 2)) == BAD and loss(g_value=off(P(7), 1)) == BAD
    assert loss(g_logits=P(0)) == BAD and loss(g_logits=off(P(0), 64)) == BAD  # the gradient on / inside the logits
    assert loss(g_value=P(2)) == BAD and loss(scalars_out=P(4)) == BAD and loss(log_prob_out=P(3)) == BAD and loss(ws=P(6)) == BAD
    assert loss(scalars_sum=P(8)) == BAD and loss(log_prob_out=P(7)) == BAD


def test_rollout_entry_points_take_the_index_row():
    """act_dim 1 passes the width check of add and gather and is held to the next checks (a misaligned row, an overlap: BADARG where
    act_dim 3 answers UNSUPPORTED before them); no call reaches a launch"""
    from test_ppo_abi import rollout

    lib = nv.lib()
    f32 = C.c_float

    def add(rb, act=P(10), obs=P(9)):
        return lib.cstr_rollout_add_f32(C.byref(rb), P(8), obs, act, P(11), P(12), P(13), P(14), null, null, f32(0.99), null, null, null, null, null)

    def gather(rb, act=P(10), idx=P(8)):
        return lib.cstr_ppo_gather_f32(C.byref(rb), idx, i64(12), P(9), act, P(11), P(12), P(13), P(14), null)

    for d in (4, 8):
        assert add(rollout(a=1, d=d), act=off(P(10), 2)) == BAD and gather(rollout(a=1, d=d), act=off(P(10), 2)) == BAD
        assert add(rollout(a=3, d=d), act=off(P(10), 2)) == UNSUP and gather(rollout(a=3, d=d), act=off(P(10), 2)) == UNSUP
    assert add(rollout(a=1), act=P(1)) == BAD and gather(rollout(a=1), act=P(1)) == BAD  # the row inside the buffer's action field
    assert add(rollout(a=1), obs=off(P(9), 8)) == BAD and gather(rollout(a=1), idx=off(P(8), 4)) == BAD
    assert add(rollout(a=3)) == UNSUP and gather(rollout(a=3)) == UNSUP and add(rollout(a=1, d=6)) == UNSUP
    from core.common import hip_ops

    assert hip_ops.rollout_supported(4, 1) and hip_ops.rollout_supported(8, 1) and not hip_ops.rollout_supported(4, 3)
    assert not hip_ops.ppo_supported(4, 3) and not hip_ops.ppo_supported(6, 2) and not hip_ops.ppo_supported(4, 1)  # the Gaussian head's
    assert hip_ops.categorical_supported(4, 25, 5) and not hip_ops.categorical_supported(4, 24, 5) and not hip_ops.categorical_supported(4, 289, 17)


class _DiscreteEnv:
    num_envs = 2

    def __init__(self, n=9):
        from core.common.spaces import Box, Discrete

        self.observation_space, self.action_space = Box(-1, 1, (4,)), Discrete(n)

    def reset(self):
        return np.zeros((2, 4), np.float32)

    def step(self, actions):
        raise NotImplementedError


def test_ppo_and_a2c_admit_a_discrete_action_space(monkeypatch):
    """the constructors' action-space check (no device is touched: the model is not set up)"""
    from core.a2c import A2C
    from core.common import base_class
    from core.common.spaces import Discrete
    from core.ppo import PPO
    from core.sac import SAC
    from core.td3 import TD3

    monkeypatch.setattr(base_class, "get_device", lambda device: th.device("cpu"))
    for cls in (PPO, A2C):
        model = cls("MlpPolicy", _DiscreteEnv(), _init_setup_model=False)  # "only supports" before this head existed
        assert model.action_space == Discrete(9) and model.n_envs == 2
    for cls in (SAC, TD3):
        with pytest.raises(AssertionError, match="only supports"):
            cls("MlpPolicy", _DiscreteEnv(), _init_setup_model=False)


@pytest.mark.parametrize("name,algo", [("ppo_cat_train_kat_small.npz", "PPO"), ("ppo_cat_train_kat_default.npz", "PPO"),
                                       ("a2c_cat_train_kat_small.npz", "A2C")])
def test_policy_keys_and_seeded_initial_weights(golden, name, algo):
    import core
    from core.common.spaces import Box, Discrete, get_action_dim

    g = golden(name)
    K = int(g["levels"])
    assert get_action_dim(Discrete(9)) == 1 and get_action_dim(Discrete(K * K)) == 1 and get_action_dim(Box(-1, 1, (2,))) == 2
    cls = getattr(core, algo)
    kw = dict(net_arch=[int(w) for w in g["net_arch"]])
    if algo == "A2C":
        kw.update(cls._rewrite_policy_kwargs({}, True, 1e-5))
    threads = th.get_num_threads()
    th.set_num_threads(1)  # the fixture's run: LAPACK's QR of a 64 x 64 matrix rounds differently when it is threaded
    try:
        th.manual_seed(int(g["seed"]))  # set_random_seed(seed) of the fixture's run
        pol = cls.policy_aliases["MlpPolicy"](Box(-1, 1, (4,)), Discrete(K * K), lambda _: float(g["learning_rate"]), **kw)
    finally:
        th.set_num_threads(threads)
    keys = [str(k) for k in g["state_dict_keys"]]
    assert list(pol.state_dict()) == keys and len(keys) == 12 and not hasattr(pol, "log_std") and "log_std" not in keys
    assert pol.action_net.out_features == K * K and pol.action_net.in_features == int(g["net_arch"][-1]) and pol.discrete
    tc.check_init(type("M", (), {"policy": pol})(), g, ["policy"])
    obs = th.as_tensor(g["init_obs"])
    with th.no_grad():
        a, v, lp = pol(obs)
        a_det, _, _ = pol(obs, deterministic=True)
        v2, lp2, ent = pol.evaluate_actions(obs, a.float().reshape(-1, 1))  # the buffer's [n, 1] float rows
    assert a.dtype == th.int64 and tuple(a.shape) == (len(obs),) and tuple(v.shape) == (len(obs), 1) and tuple(lp.shape) == (len(obs),)
    assert th.equal(lp, lp2) and th.equal(v, v2) and tuple(ent.shape) == (len(obs),)
    idx, state = pol.predict(g["init_obs"], deterministic=True)
    assert state is None and idx.dtype == np.int64 and idx.shape == (len(obs),) and np.array_equal(idx, a_det.numpy())
    one, _ = pol.predict(g["init_obs"][0], deterministic=True)
    assert one.shape == () and int(one) == int(idx[0])


def test_categorical_distribution_against_torch():
    from core.common.distributions import CategoricalDistribution

    th.manual_seed(3)
    logits = th.randn(7, 9) * 2
    d = CategoricalDistribution(9)
    net = d.proba_distribution_net(latent_dim=5)
    assert isinstance(net, th.nn.Linear) and (net.in_features, net.out_features) == (5, 9)
    ref = th.distributions.Categorical(logits=logits)
    assert d.proba_distribution(logits) is d
    a = th.arange(7) % 9
    assert th.equal(d.log_prob(a), ref.log_prob(a)) and th.equal(d.entropy(), ref.entropy())
    assert th.equal(d.mode(), th.argmax(ref.probs, dim=1)) and th.equal(d.get_actions(deterministic=True), d.mode())
    s = d.sample()
    assert s.dtype == th.int64 and tuple(s.shape) == (7,) and int(s.min()) >= 0 and int(s.max()) < 9
    d.action_queue.append(a)  # the teacher-forcing hook
    assert th.equal(d.get_actions(), a) and not d.action_queue
    assert th.equal(d.actions_from_params(logits, deterministic=True), d.mode())
    acts, lp = d.log_prob_from_params(logits)
    assert th.equal(lp, ref.log_prob(acts))


def mlp_f64(g, pre, net, head, x):
    h = np.asarray(x, np.float64)
    for i in (0, 2):
        h = np.tanh(h @ g[f"{pre}/policy/mlp_extractor.{net}.{i}.weight"].astype(np.float64).T + g[f"{pre}/policy/mlp_extractor.{net}.{i}.bias"])
    return h @ g[f"{pre}/policy/{head}.weight"].astype(np.float64).T + g[f"{pre}/policy/{head}.bias"]


def flat(a):
    """RolloutBuffer.swap_and_flatten: [T, N, ...] -> [N * T, ...]"""
    a = a if a.ndim > 2 else a[..., None]
    return a.swapaxes(0, 1).reshape(a.shape[0] * a.shape[1], *a.shape[2:])


def minibatch_case(g, pre, rpre, rows):
    obs = flat(g[f"{rpre}rollout/observations"])[rows]
    z = mlp_f64(g, pre, "policy_net", "action_net", obs)
    values = mlp_f64(g, pre, "value_net", "value_net", obs).reshape(-1)
    f = lambda name: flat(g[f"{rpre}rollout/{name}"]).reshape(-1)[rows]  # noqa: E731
    return dict(z=z, a=f("actions").astype(np.int64), old_lp=f("log_probs"), values=values, old_values=f("values"), adv=f("advantages"),
                returns=f("returns"))


@pytest.mark.parametrize("name", ["small", "default"])
def test_fp64_restatement_reproduces_the_reference_ppo(golden, name):
    """the first minibatch of the fixture (the `before` weights, rows permutations[0][:batch]): scalars, values and log-probs of the
    f32 reference within 1e-5 of the fp64 statement tests/test_categorical.py applies to the kernel"""
    g = golden(f"ppo_cat_train_kat_{name}.npz")
    rows = g["permutations"][0][:int(g["batch_size"])]
    c = minibatch_case(g, "before", "", rows)
    scal, _, _, lp, _ = tc.loss_torch(c, 0, th.float64, True, float(g["ent_coef"]), float(g["vf_coef"]), clip_range=float(g["clip_range"]))
    want = g["mb0/scalars"].astype(np.float64)
    assert np.abs(c["values"] - g["mb0/values"].reshape(-1)).max() <= 1e-5 * max(np.abs(g["mb0/values"]).mean(), 1e-3) * 10
    assert np.abs(lp - g["mb0/log_prob"]).max() <= 1e-5 * np.abs(g["mb0/log_prob"]).mean()
    for k in range(5):
        assert abs(scal[k] - want[k]) <= 1e-5 * max(abs(want[k]), 1.0), (k, scal[k], want[k])
    assert scal[5] == want[5]
    # the rollout's own log-probs are the log-probs of the stored indices under the `before` weights: ratio 1 in the first minibatch
    assert abs(want[4]) < 1e-6 and want[5] == 0.0


def test_fp64_restatement_reproduces_the_reference_a2c(golden):
    g = golden("a2c_cat_train_kat_small.npz")
    for it in range(int(g["iterations"])):
        pre = "before" if it == 0 else f"it{it - 1}/after"
        rows = g[f"it{it}/permutation"]
        c = minibatch_case(g, pre, f"it{it}/", rows)
        scal, _, _, lp, _ = tc.loss_torch(c, 1, th.float64, False, float(g["ent_coef"]), float(g["vf_coef"]))
        want = g[f"it{it}/scalars"].astype(np.float64)
        assert np.abs(lp - g[f"it{it}/log_prob"]).max() <= 1e-5 * np.abs(g[f"it{it}/log_prob"]).mean()
        for k in range(4):
            assert abs(scal[k] - want[k]) <= 1e-5 * max(abs(want[k]), 1.0), (it, k, scal[k], want[k])
        assert g[f"it{it}/rollout/actions"].shape == (int(g["n_steps"]), int(g["n_envs"]), 1) and g[f"it{it}/rollout/actions"].dtype == np.float32


def test_predict_fixture_is_consistent(golden):
    g = golden("ppo_cat_predict_kat.npz")
    z = mlp_f64({f"before/{k}": g[k] for k in g.files}, "before", "policy_net", "action_net", g["obs"])
    assert g["deterministic"].dtype == np.int64 and g["deterministic"].shape == (16,) and np.array_equal(z.argmax(axis=1), g["deterministic"])
    top = np.sort(g["logits"], axis=1)
    assert ((top[:, -1] - top[:, -2]) > 1e-4 * np.abs(g["logits"]).max()).all() and np.abs(z - g["logits"]).max() < 1e-5
