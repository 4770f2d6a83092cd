"""CPU checks of TQC: the fp64 restatement of tests/_tqc_reference.py against itself (autograd on torch.sort against the closed-form
gradient, the G = Nq = 1 case, the effect of truncation, ties), the policy's modules and keys, the class's refusals that need no
device, and the two entry points' argument checks on the host (nothing is dereferenced or launched)."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import _tqc_reference as ref

CASES = [(1, 1, 0), (2, 25, 2), (2, 25, 0), (2, 25, 24), (5, 25, 2), (3, 13, 1), (16, 16, 3), (2, 32, 1), (5, 13, 1)]


@pytest.mark.parametrize("G,Nq,k", CASES)
@pytest.mark.parametrize("mode", ["random", "done", "ties", "edges"])
def test_autograd_and_the_closed_form_agree(G, Nq, k, mode):
    inp = ref.loss_inputs(7, G, Nq, seed=G * 100 + Nq + k, scale=1.0, mode=mode)
    out = ref.critic_loss(inp["z"], inp["z_next"], inp["next_logp"], inp["rew"], inp["done"], inp["alpha"], inp["gamma"], k)
    assert out["y"].shape == (7, ref.n_keep(G, Nq, k)) and out["gz"].shape == (G, 7, Nq)
    np.testing.assert_allclose(out["gz"], out["gz_closed"], rtol=1e-12, atol=1e-15)
    assert (np.diff(out["y"], axis=1) >= 0).all()
    if mode == "edges":  # delta in {0, -1, +1} exactly: Huber is 0 or 0.5, its derivative 0 or +-1
        d = out["y"][:, None, None, :] - inp["z"].astype(np.float64).transpose(1, 0, 2)[:, :, :, None]
        assert set(np.unique(d)) <= {-1.0, 0.0, 1.0}


def test_one_critic_one_atom_is_half_the_huber_loss():
    rng = np.random.default_rng(0)
    B = 33
    z, zn = rng.normal(0, 2, (1, B, 1)).astype(np.float32), rng.normal(0, 2, (1, B, 1)).astype(np.float32)
    lp, rew, done = rng.normal(-1, 1, B).astype(np.float32), rng.uniform(-8, 0, B).astype(np.float32), (rng.uniform(size=B) < 0.3).astype(np.float32)
    out = ref.critic_loss(z, zn, lp, rew, done, 0.2, 0.99, 0)
    y = rew.astype(np.float64) + (1 - done.astype(np.float64)) * 0.99 * (zn.reshape(B).astype(np.float64) - 0.2 * lp.astype(np.float64))
    np.testing.assert_allclose(out["y"].reshape(B), y, rtol=1e-15)
    d = y - z.reshape(B).astype(np.float64)
    huber = np.where(np.abs(d) <= 1, 0.5 * d * d, np.abs(d) - 0.5)
    assert abs(out["loss"] - 0.5 * huber.mean()) <= 1e-14 * abs(out["loss"])  # tau_0 = 0.5: |0.5 - 1[.]| = 0.5 either way


def test_truncation_lowers_the_target_mean():
    inp = ref.loss_inputs(64, 2, 25, seed=4)
    args = (inp["z"], inp["z_next"], inp["next_logp"], inp["rew"], inp["done"], inp["alpha"], inp["gamma"])
    cut, full = ref.critic_loss(*args, 2), ref.critic_loss(*args, 0)
    assert cut["target_mean"] <= full["target_mean"] and cut["y"].shape[1] == 46 and full["y"].shape[1] == 50
    np.testing.assert_array_equal(cut["y"], full["y"][:, :46])  # the smallest 46 of the same sorted row


@pytest.mark.parametrize("G,Nq,k", [(2, 25, 2), (5, 13, 1), (16, 16, 3)])
def test_duplicated_critics_keep_exactly_n_keep(G, Nq, k):
    inp = ref.loss_inputs(5, G, Nq, seed=9, mode="ties")
    assert all(np.array_equal(inp["z_next"][0], inp["z_next"][g]) for g in range(G))  # every atom tied at least G-fold
    out = ref.critic_loss(inp["z"], inp["z_next"], inp["next_logp"], inp["rew"], inp["done"], inp["alpha"], inp["gamma"], k)
    assert out["y"].shape == (5, G * Nq - k * G) and np.isfinite(out["gz"]).all()
    # the kept multiset is the sorted row's head, whatever order ties come in
    pooled = np.sort(inp["z_next"].astype(np.float64).transpose(1, 0, 2).reshape(5, -1), axis=1)[:, :G * Nq - k * G]
    col = lambda a: a.astype(np.float64).reshape(-1, 1)  # noqa: E731
    want = col(inp["rew"]) + (1 - col(inp["done"])) * inp["gamma"] * (pooled - inp["alpha"] * col(inp["next_logp"]))
    np.testing.assert_array_equal(out["y"], want)


def test_actor_and_alpha_restatements():
    inp = ref.loss_inputs(9, 3, 13, seed=2)
    out = ref.actor_loss(inp["z_pi"], inp["logp"], inp["alpha"])
    np.testing.assert_allclose(out["gz_pi"], -1.0 / (9 * 39), rtol=1e-12)
    np.testing.assert_allclose(out["g_logp"], inp["alpha"] / 9, rtol=1e-12)
    zm = inp["z_pi"].astype(np.float64).transpose(1, 0, 2).reshape(9, -1).mean(axis=1)
    np.testing.assert_allclose(out["z_pi_mean"], zm, rtol=1e-12)
    assert abs(out["loss"] - (inp["alpha"] * inp["logp"].astype(np.float64) - zm).mean()) < 1e-12
    ap = ref.alpha_part(-0.8, inp["logp"], -2.0)
    m = (inp["logp"].astype(np.float64) - 2.0).mean()
    assert abs(ap["grad"] + m) < 1e-12 and abs(ap["loss"] - 0.8 * m) < 1e-12 and abs(ap["ent_coef"] - np.exp(-0.8)) < 1e-15


def test_policy_modules_keys_and_seeded_actor():
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.sac.policies import SACPolicy
    from core.tqc.policies import MlpPolicy, QuantileCritic, TQCPolicy

    assert MlpPolicy is TQCPolicy and issubclass(TQCPolicy, SACPolicy)
    p = ref.make_policy(seed=3, arch=(32, 32))
    assert isinstance(p.critic, QuantileCritic) and p.critic.n_quantiles == 25 and len(p.critic.q_networks) == 2
    assert p.critic.quantiles_nets is p.critic.q_networks and p.critic.q_networks[1] is p.critic.qf1
    keys = list(p.state_dict())
    assert "critic.qf0.0.weight" in keys and "critic.qf1.4.bias" in keys and "critic_target.qf0.0.weight" in keys and "actor.mu.weight" in keys
    assert tuple(p.critic.qf0[4].weight.shape) == (25, 32)
    z = p.critic(th.zeros(5, 4), th.zeros(5, 2))
    assert tuple(z.shape) == (5, 2, 25)
    assert all(th.equal(a, b) for a, b in zip(p.critic.parameters(), p.critic_target.parameters()))
    # SACPolicy's construction order: the same seed gives SAC's actor
    set_random_seed(3)
    sac = SACPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4, net_arch=[32, 32])
    assert all(th.equal(a, b) for a, b in zip(sac.actor.parameters(), p.actor.parameters()))
    q = ref.make_policy(seed=3, arch=(32, 32), n_quantiles=7, n_critics=3)
    assert tuple(q.critic(th.zeros(5, 4), th.zeros(5, 2)).shape) == (5, 3, 7) and "critic.qf2.4.bias" in q.state_dict()
    for bad in (dict(n_quantiles=0), dict(n_critics=0), dict(use_sde=True)):
        with pytest.raises(ValueError):
            ref.make_policy(arch=(32, 32), **bad)


def test_import_and_refusals_without_a_device():
    import core
    from core import TQC
    from core.sac import SAC
    from core.tqc import TQC as T2

    assert TQC is T2 and "TQC" in core.__all__ and issubclass(TQC, SAC)
    assert TQC.policy_aliases.keys() == {"MlpPolicy"} and TQC.chain_type is None and not TQC.goal_face_support
    for kw, msg in ((dict(use_sde=True), "gSDE"), (dict(policy_kwargs=dict(use_sde=True)), "gSDE"),
                    (dict(policy_kwargs=dict(n_quantiles=0)), "n_quantiles"), (dict(top_quantiles_to_drop_per_net=-1), "negative"),
                    (dict(top_quantiles_to_drop_per_net=25), "drops every atom"), (dict(top_quantiles_to_drop_per_net=3, policy_kwargs=dict(n_quantiles=3)), "drops every atom")):
        with pytest.raises(ValueError, match=msg):
            TQC("MlpPolicy", None, **kw)


def test_entry_points_check_their_arguments_on_the_host():
    from core import _native as nv

    lib = nv.lib()
    null, fake, odd = C.c_void_p(None), C.c_void_p(0x1000), C.c_void_p(0x1002)
    i64, dbl = C.c_int64, C.c_double
    assert {"cstr_tqc_supported", "cstr_tqc_critic_loss_f32", "cstr_tqc_actor_loss_f32"} <= set(nv.SYMBOLS)
    sup = lambda g, n, k: bool(lib.cstr_tqc_supported(g, n, k))  # noqa: E731
    assert sup(1, 1, 0) and sup(2, 25, 2) and sup(16, 16, 3) and sup(16, 16, 15) and sup(1, 256, 255)
    assert not sup(0, 25, 0) and not sup(17, 1, 0) and not sup(2, 129, 0) and not sup(1, 257, 0) and not sup(2, 25, 25) and not sup(2, 25, -1) and not sup(2, 0, 0)
    P = [C.c_void_p(0x10000 * (i + 1)) for i in range(12)]  # disjoint fake buffers, 64 KiB apart

    def critic(z=P[0], zn=P[1], lp=P[2], rew=P[3], done=P[4], ec=P[5], gamma=0.99, g=2, nq=25, k=2, gz=P[6], lo=null, ls=null, tg=null, mo=null, ms=null,
               ws=P[7], alpha=None, batch=8):
        return lib.cstr_tqc_critic_loss_f32(z, zn, lp, rew, done, ec, dbl(gamma), g, nq, k, gz, lo, ls, tg, mo, ms, ws, alpha, i64(batch), null)

    for kw in (dict(z=null), dict(zn=null), dict(lp=null), dict(rew=null), dict(done=null), dict(gz=null), dict(ws=null), dict(ec=null), dict(batch=0),
               dict(g=0), dict(nq=0), dict(k=-1), dict(k=25), dict(gamma=-0.1), dict(gamma=float("nan")), dict(z=odd), dict(gz=odd),
               dict(ws=C.c_void_p(0x80004)), dict(gz=P[0]), dict(tg=P[1]), dict(lo=P[3]), dict(lo=P[6]), dict(mo=C.c_void_p(0x70004), lo=P[6]),
               dict(ws=C.c_void_p(0x70000 + 4 * 8 * 50 - 8))):
        assert critic(**kw) == -1, kw
    for kw in (dict(g=17, nq=1, k=0), dict(g=2, nq=129, k=0), dict(batch=16385)):
        assert critic(**kw) == -2, kw
    part = nv.AlphaPart(0x100000, None, -2.0, 0x110000, 0x120000, None, None, None)  # log_alpha without logp_pi
    assert critic(ec=null, alpha=C.byref(part)) == -1
    part = nv.AlphaPart(0x100000, 0x130000, -2.0, 0x110000, 0x10000, None, None, None)  # ent_coef_out on z
    assert critic(ec=null, alpha=C.byref(part)) == -1

    def actor(z=P[0], lp=P[1], ec=P[2], g=2, nq=25, gz=P[3], glp=P[4], lo=null, ls=null, zm=null, batch=8):
        return lib.cstr_tqc_actor_loss_f32(z, lp, ec, g, nq, gz, glp, lo, ls, zm, i64(batch), null)

    for kw in (dict(z=null), dict(lp=null), dict(ec=null), dict(gz=null), dict(glp=null), dict(batch=0), dict(g=0), dict(nq=0), dict(z=odd), dict(glp=odd),
               dict(gz=P[0]), dict(glp=P[1]), dict(lo=P[2]), dict(zm=P[4]), dict(lo=P[5], ls=P[5])):
        assert actor(**kw) == -1, kw
    for kw in (dict(g=17, nq=1), dict(g=2, nq=129), dict(batch=16385)):
        assert actor(**kw) == -2, kw
