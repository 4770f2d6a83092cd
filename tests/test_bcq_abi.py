"""CPU-side checks of BCQ: the cstr_bcq_* entry points reject bad arguments on the host (nothing is dereferenced or launched), `from
core import BCQ` resolves, BCQPolicy built on the CPU has the reference's state_dict keys in the reference's order and bit-equal seeded
initial weights (tests/golden/bcq_train_kat_{small,default}.npz, written by the unmodified reference: tools/refharness/gen_golden.py
gen_bcq), the actor_net_arch assertions carry the reference's messages, and the dataset argument / .npz reader checks run on host
logic only."""
import ctypes as C
import os

import numpy as np
import pytest

from _parity_helpers import check_init
from core import _native as nv

i64, f32 = C.c_int64, C.c_float
null, fake, fake2, fake3 = C.c_void_p(None), C.c_void_p(0x10000), C.c_void_p(0x2000000), C.c_void_p(0x4000000)
BAD, UNSUP = -1, -2


def test_bcq_symbols_declared_and_exported():
    lib = nv.lib()
    names = [s for s in nv.SYMBOLS if s.startswith("cstr_bcq_")]
    assert sorted(names) == sorted(f"cstr_bcq_{n}_f32" for n in ("latent_fwd", "vae_loss", "latent_bwd", "expand", "perturb_fwd", "perturb_bwd",
                                                                  "target", "select"))
    assert all(hasattr(lib, n) for n in names)
    assert (nv.BCQ_MAX_LATENT, nv.BCQ_MAX_ACT, nv.BCQ_MAX_SAMPLES) == (256, 64, 4096)


def test_latent_entry_points_reject_bad_arguments_on_the_host():
    lib = nv.lib()

    def fwd(params=fake, obs=fake2, eps=fake3, rng=null, xdec=C.c_void_p(0x6000000), std=C.c_void_p(0x8000000), eps_out=null, batch=64, d=4, lat=32,
            ldp=64, ldo=4, ldx=36):
        return lib.cstr_bcq_latent_fwd_f32(params, i64(ldp), obs, i64(ldo), eps, rng, xdec, i64(ldx), std, eps_out, i64(batch), d, lat, null)

    assert fwd(params=null) == BAD and fwd(obs=null) == BAD and fwd(xdec=null) == BAD and fwd(std=null) == BAD
    assert fwd(batch=0) == BAD and fwd(lat=0) == BAD and fwd(d=0) == BAD
    assert fwd(eps=null) == BAD                      # no noise source
    assert fwd(rng=fake3) == BAD                     # two noise sources
    assert fwd(eps=null, rng=fake3) == BAD           # drawn noise must be kept for the backward
    assert fwd(ldp=63) == BAD and fwd(ldx=35) == BAD and fwd(ldo=3) == BAD
    assert fwd(lat=257, ldp=514, ldx=261) == UNSUP   # latent beyond the supported width
    assert fwd(xdec=fake) == BAD                     # decoder input rows overlap the head output
    assert fwd(std=fake) == BAD
    big = C.c_void_p(0x8000000)
    assert fwd(xdec=big) == BAD and fwd(eps_out=big) == BAD and fwd(eps_out=C.c_void_p(0x6000000)) == BAD  # outputs over each other
    assert fwd(xdec=fake3) == BAD and fwd(std=fake3) == BAD                                               # ... and over the noise read

    def loss(recon=fake, act=fake2, params=fake3, std=C.c_void_p(0x6000000), batch=64, a=2, lat=32, g_recon=C.c_void_p(0x8000000), g_mean=null,
             g_std=null, out=null):
        return lib.cstr_bcq_vae_loss_f32(recon, i64(a), act, i64(a), params, i64(2 * lat), std, i64(batch), a, lat, g_recon, g_mean, g_std, out,
                                         null, null)

    assert loss(recon=null) == BAD and loss(act=null) == BAD and loss(params=null) == BAD and loss(std=null) == BAD
    assert loss(batch=0) == BAD and loss(a=0) == BAD and loss(lat=0) == BAD
    assert loss(g_recon=null) == BAD                 # nothing to write
    assert loss(a=65) == UNSUP and loss(lat=300) == UNSUP
    assert loss(g_recon=fake) == BAD                 # gradient over its own input
    assert loss(g_std=C.c_void_p(0x6000000)) == BAD
    assert loss(g_mean=C.c_void_p(0x8000000)) == BAD and loss(g_mean=C.c_void_p(0xA000000), g_std=C.c_void_p(0xA000000)) == BAD
    assert loss(out=C.c_void_p(0x8000000)) == BAD  # the scalar inside a gradient

    def bwd(g_z=fake, gm=null, gs=null, params=fake2, std=fake3, eps=C.c_void_p(0x6000000), g_params=C.c_void_p(0x8000000), batch=64, lat=32, ldg=36):
        return lib.cstr_bcq_latent_bwd_f32(g_z, i64(ldg), gm, gs, params, i64(2 * lat), std, eps, g_params, i64(batch), lat, null)

    assert bwd(params=null) == BAD and bwd(std=null) == BAD and bwd(eps=null) == BAD and bwd(g_params=null) == BAD
    assert bwd(g_z=null) == BAD                      # no gradient source at all
    assert bwd(batch=0) == BAD and bwd(ldg=31) == BAD
    assert bwd(lat=257) == UNSUP
    assert bwd(g_params=fake2) == BAD and bwd(g_params=fake) == BAD


def test_candidate_entry_points_reject_bad_arguments_on_the_host():
    lib = nv.lib()

    def expand(state=fake, n=64, s=10, d=4, lat=32, noise=fake2, rng=null, clip=0.5, xdec=fake3, xa=null, xb=null, lds=4, ldx=36):
        return lib.cstr_bcq_expand_f32(state, i64(lds), i64(n), s, d, lat, noise, rng, f32(clip), xdec, i64(ldx), xa, i64(6), xb, i64(6), null)

    assert expand(state=null) == BAD and expand(xdec=null) == BAD and expand(n=0) == BAD
    assert expand(s=0) == BAD                        # S = 0
    assert expand(noise=null) == BAD and expand(rng=fake2) == BAD
    assert expand(clip=-1.0) == BAD and expand(lds=3) == BAD and expand(ldx=35) == BAD
    assert expand(lat=257, ldx=261) == UNSUP and expand(s=4097) == UNSUP
    assert expand(xdec=fake) == BAD                  # output rows over the states they are read from
    assert expand(xa=fake3) == BAD                   # two outputs over each other
    assert expand(xa=C.c_void_p(0x6000000), xb=C.c_void_p(0x6000000)) == BAD

    def pf(a_vae=fake, p=fake2, out=fake3, rows=640, a=2, ld=6):
        return lib.cstr_bcq_perturb_fwd_f32(a_vae, i64(ld), p, i64(a), f32(0.05), out, i64(ld), i64(rows), a, null)

    assert pf(a_vae=null) == BAD and pf(p=null) == BAD and pf(out=null) == BAD and pf(rows=0) == BAD and pf(a=0) == BAD
    assert pf(ld=1) == BAD and pf(a=65, ld=70) == UNSUP
    assert pf(out=fake) == BAD and pf(out=fake2) == BAD  # in place is not supported: input rows are re-read by the backward

    def pb(g=fake, a_vae=fake2, p=fake3, g_p=C.c_void_p(0x6000000), rows=64, a=2, ld=6):
        return lib.cstr_bcq_perturb_bwd_f32(g, i64(ld), a_vae, i64(ld), p, i64(a), f32(0.05), g_p, i64(rows), a, null)

    assert pb(g=null) == BAD and pb(a_vae=null) == BAD and pb(p=null) == BAD and pb(g_p=null) == BAD and pb(rows=0) == BAD
    assert pb(ld=1) == BAD and pb(a=65, ld=70) == UNSUP and pb(g_p=fake3) == BAD


def test_target_and_select_reject_bad_arguments_on_the_host():
    lib = nv.lib()

    def target(q=fake, stride=640, n_q=2, n=64, s=10, grouping=0, rew=fake2, done=fake2, out=fake3, max_q=null):
        return lib.cstr_bcq_target_f32(q, i64(stride), n_q, i64(n), s, grouping, rew, done, f32(0.99), out, max_q, null)

    assert target(q=null) == BAD and target(n=0) == BAD and target(s=0) == BAD and target(n_q=0) == BAD
    assert target(out=null) == BAD                   # no output
    assert target(rew=null) == BAD and target(done=null) == BAD
    assert target(grouping=2) == BAD and target(stride=639) == BAD
    assert target(n_q=17, stride=640) == UNSUP and target(s=4097) == UNSUP
    assert target(out=fake) == BAD                   # the target over the Q values it reduces
    assert target(n_q=1, stride=0, q=null) == BAD

    def select(q1=fake, cand=fake2, n=3, s=100, a=2, idx=null, out=fake3, ldc=6):
        return lib.cstr_bcq_select_f32(q1, cand, i64(ldc), i64(n), s, a, idx, out, null)

    assert select(q1=null) == BAD and select(cand=null) == BAD and select(out=null) == BAD
    assert select(n=0) == BAD and select(s=0) == BAD and select(a=0) == BAD and select(ldc=1) == BAD
    assert select(a=65, ldc=70) == UNSUP and select(s=5000) == UNSUP
    assert select(out=fake2) == BAD


def test_hip_ops_wrappers_refuse_cpu_tensors():
    import torch as th

    from core.common import hip_ops

    with pytest.raises(ValueError, match="No CPU fallback|device"):
        hip_ops.bcq_perturb_fwd(th.zeros(8, 2), th.zeros(8, 2), 0.05, th.zeros(8, 2))
    with pytest.raises(ValueError, match="exactly one noise source"):
        hip_ops.bcq_expand(th.zeros(4, 4), 10, None, None, th.zeros(40, 36))
    assert hip_ops.bcq_supported(32, 2, 100) and not hip_ops.bcq_supported(257, 2, 100) and not hip_ops.bcq_supported(32, 65, 10)


def test_from_core_import_bcq():
    import core
    from core import BCQ
    from core.bcq import BCQ as B2

    assert BCQ is B2 and "BCQ" in core.__all__
    assert BCQ.policy_aliases["MlpPolicy"].__name__ == "BCQPolicy"


@pytest.mark.parametrize("tag", ["small", "default"])
def test_policy_keys_and_seeded_init(golden, tag):
    from core.bcq.policies import BCQPolicy
    from core.common.spaces import Box
    from core.common.utils import set_random_seed

    g = golden(f"bcq_train_kat_{tag}.npz")
    set_random_seed(0)
    pk = dict(critic_net_arch=[64, 64]) if tag == "small" else {}
    pol = BCQPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4, **pk)
    assert list(pol.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    keys = list(pol.state_dict().keys())
    want_head = ["actor.vae.encoder.0.weight", "actor.vae.encoder.0.bias", "actor.vae.encoder.2.weight", "actor.vae.encoder.2.bias",
                 "actor.vae.mean.weight", "actor.vae.mean.bias", "actor.vae.log_std.weight", "actor.vae.log_std.bias", "actor.vae.decoder.0.weight"]
    assert keys[:9] == want_head and keys[-1] == "critic_target.qf1.4.bias"
    check_init(pol, g, ["actor", "actor_target", "critic", "critic_target"])
    n_vae = sum(p.numel() for p in BCQPolicy._vae_params(pol.actor))
    n_pert = sum(p.numel() for p in pol.actor.perturbation.parameters())
    n_crit = sum(p.numel() for p in pol.critic.parameters())
    assert [n_vae, n_pert, n_crit] == g["n_params"].tolist()
    if tag == "default":
        assert [n_vae, n_pert, n_crit] == [15426, 4738, 246802]
        assert pol.actor_arch == dict(vae_latent_dim=32, vae_hidden_dim=64, perturbation_hidden_dim=64, max_perturbation=0.05)
        assert pol.critic_arch == [400, 300] and len(pol.critic.q_networks) == 2


def test_actor_net_arch_assertions_carry_the_reference_messages():
    from core.bcq.policies import BCQPolicy
    from core.common.spaces import Box

    full = dict(vae_latent_dim=8, vae_hidden_dim=16, perturbation_hidden_dim=16, max_perturbation=0.05)
    mk = lambda arch: BCQPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4, actor_net_arch=arch, critic_net_arch=[16])  # noqa: E731
    with pytest.raises(AssertionError, match="Error: the net_arch can only contain be a list of ints or a dict"):
        mk([64, 64])
    for key in full:
        arch = {k: v for k, v in full.items() if k != key}
        with pytest.raises(AssertionError, match=f"Error: no key '{key}' was provided in net_arch for the actor network"):
            mk(arch)
    pol = mk(full)
    assert pol.actor.vae.latent_dim == 8 and pol.actor.perturbation.max_perturbation == 0.05
    import torch as th

    assert mk(full).activation_fn is th.nn.ReLU  # stored, never used


def test_dataset_argument_checks_are_host_logic(tmp_path):
    from core import BCQ

    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'int'>"):
        BCQ("MlpPolicy", None, dataset=5)
    with pytest.raises(ValueError, match=r"Dataset must be a path string or a ReplayBuffer instance, got <class 'NoneType'>"):
        BCQ("MlpPolicy", None)
    with pytest.raises(FileNotFoundError, match="Dataset file not found"):
        BCQ("MlpPolicy", None, dataset=str(tmp_path / "missing.pkl"))


def test_npz_reader_shape_checks(tmp_path):
    from core.common.offline_policy_algorithm import NPZ_FIELDS, read_npz_dataset

    rng = np.random.default_rng(0)
    R, N, D, A = 7, 3, 4, 2
    good = dict(observations=rng.uniform(-1, 1, (R, N, D)), next_observations=rng.uniform(-1, 1, (R, N, D)), actions=rng.uniform(-1, 1, (R, N, A)),
                rewards=rng.uniform(-8, 0, (R, N)), dones=np.zeros((R, N)), timeouts=np.zeros((R, N)))
    p = str(tmp_path / "d.npz")
    np.savez(p, **good)
    out = read_npz_dataset(p)
    assert out["pos"] == 0 and out["full"] is True and all(out[k].dtype == np.float32 for k in NPZ_FIELDS)
    np.testing.assert_array_equal(out["actions"], good["actions"].astype(np.float32))
    np.savez(p, pos=np.int64(5), full=np.uint8(0), **good)
    out = read_npz_dataset(p)
    assert out["pos"] == 5 and out["full"] is False
    np.savez(p, pos=np.int64(5), **good)
    assert read_npz_dataset(p)["full"] is False
    for drop in NPZ_FIELDS:
        np.savez(p, **{k: v for k, v in good.items() if k != drop})
        with pytest.raises(ValueError, match="missing arrays"):
            read_npz_dataset(p)
    for key, bad in (("observations", good["observations"][:, 0]), ("next_observations", good["next_observations"][:-1]),
                     ("actions", good["actions"][:, :2]), ("rewards", good["rewards"][:, :2]), ("dones", good["dones"][None]),
                     ("timeouts", good["timeouts"].T)):
        np.savez(p, **dict(good, **{key: bad}))
        with pytest.raises(ValueError, match=key if key != "next_observations" else "next_observations"):
            read_npz_dataset(p)
    np.savez(p, pos=np.int64(7), full=np.uint8(1), **good)
    with pytest.raises(ValueError, match="pos 7 outside"):
        read_npz_dataset(p)
    assert os.path.exists(p)
