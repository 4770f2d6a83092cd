"""CPU-side checks of PPO: the six cstr_ppo entry points are exported and reject bad arguments on the host (nothing is dereferenced
or launched), `from core import PPO` resolves, ActorCriticPolicy built on the CPU has the reference's state_dict keys and shapes and its
seeded initial weights (tests/golden/ppo_train_kat_small.npz, written by the unmodified reference: tools/refharness/gen_golden.py
gen_ppo), the constructor's assertions and warning fire, gSDE is refused, the minibatch permutation stream is the reference's, and a
NumPy statement of GAE reproduces the fixture bit for bit (the expression order csrc/cstr_ppo.hip follows)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from core import _native as nv

i64, f32, f64 = C.c_int64, C.c_float, C.c_double
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
PPO_SYMBOLS = ("cstr_diag_gaussian_act_f32", "cstr_rollout_add_f32", "cstr_gae_f32", "cstr_ppo_gather_f32", "cstr_ppo_loss_f32",
               "cstr_grad_clip_f32")


def P(k: int) -> C.c_void_p:
    """the k-th of a set of fake, well separated, 256-byte-aligned device addresses (never dereferenced)"""
    return C.c_void_p(0x1000000 * (k + 1))


def gae_numpy(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda):
    """compute_returns_and_advantage (reference core/common/buffers.py:423-438) on float32 arrays [T, N] with Python-float gamma /
    gae_lambda: NumPy rounds gamma and the double product gamma * gae_lambda to float32 when they meet a float32 array (NEP 50)."""
    T = rewards.shape[0]
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(T)):
        if step == T - 1:
            next_non_terminal = 1.0 - dones.astype(np.float32)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    return advantages, advantages + values


def rollout(obs=P(0), act=P(1), rew=P(2), es=P(3), val=P(4), lp=P(5), adv=P(6), ret=P(7), rows=8, n=4, d=4, a=2):
    return nv.Rollout(obs.value, act.value, rew.value, es.value, val.value, lp.value, adv.value, ret.value, rows, n, d, a)


def test_ppo_symbols_declared_and_exported():
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in PPO_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive
    assert (nv.ROLLOUT_CTL_WORDS, nv.PPO_WS_WORDS, nv.PPO_MAX_BLOCKS) == (4, 1024, 64)


def test_head_rejects_bad_arguments_on_the_host():
    lib = nv.lib()

    def head(mean=P(0), log_std=P(1), eps=P(2), rng=null, low=P(3), high=P(4), det=0, action=P(5), env=P(6), logp=P(7), eps_out=null, n=64, a=2):
        return lib.cstr_diag_gaussian_act_f32(mean, log_std, eps, rng, low, high, det, action, env, logp, eps_out, i64(n), a, null)

    assert head(mean=null) == BAD and head(log_std=null) == BAD and head(action=null) == BAD
    assert head(n=0) == BAD and head(a=0) == BAD
    assert head(eps=null) == BAD and head(rng=P(8)) == BAD      # no noise source / two of them
    assert head(low=null) == BAD                                 # one bound without the other
    assert head(a=3) == UNSUP and head(a=8) == UNSUP
    assert head(mean=C.c_void_p(P(0).value + 4)) == BAD and head(a=4, action=C.c_void_p(P(5).value + 8)) == BAD  # misaligned rows
    assert head(action=P(0)) == BAD and head(env=P(2)) == BAD and head(logp=P(5)) == BAD                       # overlapping in / out rows
    assert head(env=C.c_void_p(P(5).value + 64)) == BAD          # two outputs over each other


def test_rollout_entry_points_reject_bad_arguments_on_the_host():
    lib = nv.lib()

    def add(rb=None, ctl=P(8), obs=P(9), act=P(10), rew=P(11), es=P(12), val=P(13), lp=P(14), tout=null, tv=null, done=null, er=null, el=null,
            st=null):
        rb = rollout() if rb is None else rb
        return lib.cstr_rollout_add_f32(C.byref(rb), ctl, obs, act, rew, es, val, lp, tout, tv, f32(0.99), done, er, el, st, null)

    assert lib.cstr_rollout_add_f32(null, P(8), P(9), P(10), P(11), P(12), P(13), P(14), null, null, f32(0.99), null, null, null, null, null) == BAD
    assert add(ctl=null) == BAD and add(obs=null) == BAD and add(lp=null) == BAD
    assert add(rb=rollout(rows=0)) == BAD and add(rb=rollout(n=0)) == BAD and add(rb=rollout(ret=null)) == BAD
    assert add(rb=rollout(a=3)) == UNSUP and add(rb=rollout(d=6)) == UNSUP
    assert add(tout=P(15)) == BAD                                # a timeout flag without terminal values
    assert add(er=P(15), el=P(16), st=P(17)) == BAD              # episode statistics need `done`
    assert add(obs=C.c_void_p(P(9).value + 8)) == BAD            # misaligned observation rows
    assert add(obs=P(0)) == BAD and add(val=P(4)) == BAD         # an input row inside the buffer it is copied into
    assert add(done=P(12)) == BAD                                # done over the episode starts it replaces

    def gae(rew=P(0), val=P(1), es=P(2), last=P(3), dones=P(4), adv=P(5), ret=P(6), t=8, n=4):
        return lib.cstr_gae_f32(rew, val, es, last, dones, f64(0.99), f64(0.95), adv, ret, i64(t), i64(n), null)

    assert gae(rew=null) == BAD and gae(adv=null) == BAD and gae(last=null) == BAD and gae(t=0) == BAD and gae(n=0) == BAD
    assert gae(adv=P(0)) == BAD and gae(ret=P(5)) == BAD and gae(val=C.c_void_p(P(1).value + 2)) == BAD
    assert gae(t=1 << 20, n=1 << 20) == UNSUP

    def gather(rb=None, idx=P(8), b=12, obs=P(9), act=P(10), ov=P(11), olp=P(12), adv=P(13), ret=P(14)):
        rb = rollout() if rb is None else rb
        return lib.cstr_ppo_gather_f32(C.byref(rb), idx, i64(b), obs, act, ov, olp, adv, ret, null)

    assert gather(idx=null) == BAD and gather(obs=null) == BAD and gather(ret=null) == BAD and gather(b=0) == BAD
    assert gather(rb=rollout(a=3)) == UNSUP
    assert gather(obs=P(0)) == BAD and gather(adv=P(12)) == BAD and gather(idx=C.c_void_p(P(8).value + 4)) == BAD


def loss_args(**kw):
    d = dict(mean=P(0), ldm=2, log_std=P(1), actions=P(2), values=P(3), old_values=P(4), old_log_prob=P(5), adv=P(6), returns=P(7), batch=12,
             act_dim=2, normalize_advantage=1, clip_range=0.2, clip_range_vf=-1.0, ent_coef=0.0, vf_coef=0.5, g_mean=P(8), g_value=P(9),
             g_log_std=P(10), scalars_out=P(11), scalars_sum=null, log_prob_out=null)
    d.update(kw)
    p = nv.PpoLoss()
    for k, v in d.items():
        setattr(p, k, v.value if isinstance(v, C.c_void_p) else v)
    return p


def test_loss_and_clip_reject_bad_arguments_on_the_host():
    lib = nv.lib()
    loss = lambda ws=P(12), **kw: lib.cstr_ppo_loss_f32(C.byref(loss_args(**kw)), ws, null)  # noqa: E731
    assert lib.cstr_ppo_loss_f32(null, P(12), null) == BAD and loss(ws=null) == BAD
    for name in ("mean", "log_std", "actions", "values", "old_log_prob", "adv", "returns", "g_mean", "g_value", "g_log_std"):
        assert loss(**{name: null}) == BAD, name
    assert loss(batch=0) == BAD and loss(act_dim=0) == BAD and loss(ldm=1) == BAD and loss(clip_range=-0.1) == BAD
    assert loss(act_dim=3, ldm=3) == UNSUP
    assert loss(clip_range_vf=0.2, old_values=null) == BAD          # value clipping needs the old values
    assert loss(mean=C.c_void_p(P(0).value + 4)) == BAD and loss(act_dim=4, ldm=6) == BAD  # misaligned rows
    assert loss(g_mean=P(0)) == BAD and loss(g_value=P(3)) == BAD and loss(scalars_out=P(8)) == BAD and loss(ws=P(9)) == BAD

    clip = lambda grad=P(0), n=1000, mx=0.5, ws=P(1), out=null: lib.cstr_grad_clip_f32(grad, i64(n), f32(mx), ws, out, null)  # noqa: E731
    assert clip(grad=null) == BAD and clip(ws=null) == BAD and clip(n=0) == BAD and clip(mx=-1.0) == BAD and clip(mx=float("nan")) == BAD
    assert clip(ws=P(0)) == BAD and clip(out=P(0)) == BAD and clip(ws=C.c_void_p(P(1).value + 4)) == BAD


def test_hip_ops_wrappers_refuse_cpu_tensors():
    import torch as th

    from core.common import hip_ops

    with pytest.raises(ValueError, match="No CPU fallback|device"):
        hip_ops.grad_clip(th.zeros(8), 0.5, th.zeros(nv.PPO_WS_WORDS, dtype=th.int64))
    with pytest.raises(ValueError, match="obs_dim"):
        hip_ops.DeviceRollout(8, 4, 5, 2, "cpu")
    assert hip_ops.ppo_supported(4, 2) and hip_ops.ppo_supported(8, 4) and not hip_ops.ppo_supported(4, 3) and not hip_ops.ppo_supported(6, 2)


def test_from_core_import_ppo():
    import core
    from core import PPO
    from core.ppo import PPO as P2, MlpPolicy
    from core.common.on_policy_algorithm import OnPolicyAlgorithm
    from core.common.policies import ActorCriticPolicy

    assert PPO is P2 and "PPO" in core.__all__ and issubclass(PPO, OnPolicyAlgorithm) and MlpPolicy is ActorCriticPolicy
    assert PPO.policy_aliases["MlpPolicy"] is ActorCriticPolicy
    for name in ("_setup_model", "collect_rollouts", "learn", "_dump_logs", "_get_torch_save_params"):
        assert name in vars(OnPolicyAlgorithm), name
    assert "clip_range" not in OnPolicyAlgorithm.__init__.__code__.co_varnames  # nothing PPO-specific in the base class


def make_policy(seed=0, **kw):
    import torch as th

    from core.common.spaces import Box
    from core.ppo import MlpPolicy

    one = np.ones(4, np.float32)
    th.manual_seed(seed)
    return MlpPolicy(Box(-one, one), Box(-one[:2], one[:2]), lambda _: 3e-4, **kw)


def test_policy_keys_shapes_and_seeded_initial_weights(golden):
    import torch as th

    g = golden("ppo_train_kat_small.npz")
    pol = make_policy(seed=int(g["seed"]), net_arch=[int(w) for w in g["net_arch"]])
    sd = pol.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_dict_keys"]]
    assert list(sd.keys())[0] == "log_std" and "mlp_extractor.policy_net.2.bias" in sd and "mlp_extractor.value_net.0.weight" in sd
    for k, v in sd.items():
        want = g[f"before/policy/{k}"]
        assert tuple(v.shape) == want.shape, k
        if k == "log_std" or k.endswith(".bias"):
            np.testing.assert_array_equal(v.numpy(), want, err_msg=k)
        else:  # orthogonal_: QR through LAPACK, whose last bits may depend on the host CPU
            np.testing.assert_allclose(v.numpy(), want, rtol=0, atol=1e-6, err_msg=k)
    assert pol.optimizer_kwargs == {"eps": 1e-5} and pol.optimizer_class is th.optim.Adam
    # class defaults: [64, 64] each, Tanh; dict form; ReLU; log_std_init
    d = make_policy()
    assert d.net_arch == dict(pi=[64, 64], vf=[64, 64]) and isinstance(d.mlp_extractor.policy_net[1], th.nn.Tanh)
    e = make_policy(net_arch=dict(pi=[32], vf=[16, 8]), activation_fn=th.nn.ReLU, log_std_init=-0.5, ortho_init=False)
    assert e.action_net.in_features == 32 and e.value_net.in_features == 8 and isinstance(e.mlp_extractor.value_net[1], th.nn.ReLU)
    assert np.allclose(e.log_std.detach().numpy(), -0.5)
    # gains: sqrt(2) for the trunks, 0.01 for the action head, 1 for the value head (rows of an orthogonal matrix times the gain)
    w = d.mlp_extractor.policy_net[2].weight.detach().double()
    assert th.allclose(w @ w.t(), 2 * th.eye(64, dtype=th.float64), atol=1e-5)
    wa, wv = d.action_net.weight.detach().double(), d.value_net.weight.detach().double()
    assert th.allclose(wa @ wa.t(), 1e-4 * th.eye(2, dtype=th.float64), atol=1e-9) and abs(float(wv @ wv.t()) - 1) < 1e-5


def test_policy_torch_statements_on_the_cpu():
    import torch as th

    pol = make_policy(seed=3)
    obs = th.randn(5, 4)
    pol.action_dist.eps_queue.append(th.full((5, 2), 0.5))
    actions, values, log_prob = pol(obs)
    dist = pol.get_distribution(obs)
    assert th.allclose(actions, dist.mode() + 0.5 * pol.log_std.exp()) and values.shape == (5, 1) and log_prob.shape == (5,)
    v2, lp2, ent = pol.evaluate_actions(obs, actions)
    assert th.allclose(v2, values) and th.allclose(lp2, log_prob) and th.allclose(v2, pol.predict_values(obs)) and ent.shape == (5,)
    det, _, _ = pol(obs, deterministic=True)
    assert th.equal(det, dist.mode())


def test_constructor_assertions_warning_and_refusals():
    import torch as th

    from core.common.torch_layers import FlattenExtractor
    from core.ppo import PPO

    with pytest.raises(AssertionError, match="`batch_size` must be greater than 1"):
        PPO._check_batch_arguments(1, 8, 4, True)
    with pytest.raises(AssertionError, match="`n_steps \\* n_envs` must be greater than 1"):
        PPO._check_batch_arguments(2, 1, 1, True)
    PPO._check_batch_arguments(1, 1, 1, False)
    with pytest.warns(UserWarning, match="truncated mini-batch of size 8"):
        PPO._check_batch_arguments(12, 8, 4, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        PPO._check_batch_arguments(16, 8, 4, True)
    with pytest.raises(ValueError, match="does not support gSDE"):
        PPO("MlpPolicy", None, use_sde=True)
    with pytest.raises(ValueError, match="does not support gSDE"):
        make_policy(use_sde=True)

    class OtherExtractor(FlattenExtractor):
        pass

    with pytest.raises(NotImplementedError, match="FlattenExtractor"):
        make_policy(features_extractor_class=OtherExtractor)
    with pytest.raises(AssertionError, match="squash_output"):
        make_policy(squash_output=True)
    import inspect

    sig = inspect.signature(PPO.__init__).parameters
    want = dict(learning_rate=3e-4, n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2, clip_range_vf=None,
                normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, use_sde=False, sde_sample_freq=-1,
                rollout_buffer_class=None, rollout_buffer_kwargs=None, target_kl=None, stats_window_size=100, tensorboard_log=None,
                policy_kwargs=None, verbose=0, seed=None, device="auto", _init_setup_model=True)
    assert {k: sig[k].default for k in want} == want and list(sig)[1:3] == ["policy", "env"]
    assert th.optim.Adam is not None


def test_permutation_stream_is_the_reference_s(golden):
    """The reference's minibatch order for seed 7 and 4 envs is RandomState(10)'s (the last env's seeded reset reseeds the global
    stream with seed + n_envs - 1), and the fixture recorded it; tests/test_ppo.py checks that learn() consumes exactly this stream."""
    g = golden("ppo_train_kat_small.npz")
    assert (int(g["seed"]), int(g["n_envs"])) == (7, 4)
    rs = np.random.RandomState(int(g["seed"]) + int(g["n_envs"]) - 1)
    want = np.random.RandomState(10)
    for e in range(int(g["n_epochs"])):
        perm = rs.permutation(32)
        np.testing.assert_array_equal(perm, want.permutation(32))
        np.testing.assert_array_equal(perm, g["permutations"][e])
    from core.common.on_policy_algorithm import OnPolicyAlgorithm

    class Holder:  # the hook learn() reaches through the seeded reset of the model's own envs
        rollout_buffer = type("B", (), {"permutation_rng": None})()

    OnPolicyAlgorithm._numpy_reseeded(Holder, 10)
    np.testing.assert_array_equal(Holder.rollout_buffer.permutation_rng.permutation(32), g["permutations"][0])


@pytest.mark.parametrize("name", ["ppo_train_kat_small.npz", "ppo_train_kat_vfclip.npz", "ppo_train_kat_default.npz"])
def test_numpy_gae_reproduces_the_fixture_bit_for_bit(golden, name):
    g = golden(name)
    gamma, lam = float(g["gamma"]), float(g["gae_lambda"])
    adv, ret = gae_numpy(g["rollout/rewards"], g["rollout/values"], g["rollout/episode_starts"], g["last_values"], g["dones"], gamma, lam)
    np.testing.assert_array_equal(adv, g["rollout/advantages"])
    np.testing.assert_array_equal(ret, g["rollout/returns"])
    assert g["rollout/advantages"].dtype == np.float32 and int(g["n_truncations"]) >= 2
