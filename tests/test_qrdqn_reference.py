"""CPU checks of QR-DQN: the fp64 restatement of tests/_qrdqn_reference.py against itself (autograd against the closed-form gradient,
the Nq = 1 case, the greedy index's tie and NaN conventions, the folded head against the mean of the atoms), the policy's modules,
keys and seeded construction order, the class's defaults and refusals that need no device, and the entry points' argument checks on
the host (nothing is dereferenced or launched)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch as th

import _qrdqn_reference as ref

CASES = [(2, 1), (3, 8), (4, 64), (4, 65), (5, 200), (16, 25)]


@pytest.mark.parametrize("K,Nq", CASES)
@pytest.mark.parametrize("mode", ["random", "done", "edges", "ties"])
def test_autograd_and_the_closed_form_agree(K, Nq, mode):
    B, M = 5, K * K
    inp = ref.loss_inputs(B, K, Nq, seed=K * 100 + Nq, mode=mode)
    out = ref.loss_step(inp["z"], inp["z_next"], inp["valve"], inp["rew"], inp["done"], inp["gamma"], K)
    assert out["y"].shape == (B, Nq) and out["cur"].shape == (B, Nq) and out["gz"].shape == (B, Nq * M)
    np.testing.assert_allclose(out["gz"], out["gz_closed"], rtol=1e-12, atol=1e-15)
    dense = out["gz"].reshape(B, Nq, M)
    off = np.ones((B, Nq, M), bool)
    off[np.arange(B), :, inp["index"]] = False
    assert (dense[off] == 0).all()  # only the taken action's atoms carry a gradient
    np.testing.assert_array_equal(out["cur"], inp["z"].reshape(B, Nq, M)[np.arange(B), :, inp["index"]].astype(np.float64))
    if mode == "done":
        np.testing.assert_array_equal(out["y"], np.repeat(inp["rew"].astype(np.float64)[:, None], Nq, axis=1))
    if mode == "edges":  # delta in {0, -1, +1} exactly: Huber is 0 or 0.5, its derivative 0 or +-1
        assert set(np.unique(out["y"][:, None, :] - out["cur"][:, :, None])) <= {-1.0, 0.0, 1.0}
    if mode == "ties":  # actions 1 and M - 1 tie at the top: the first one wins
        assert (out["next_index"] == 1).all()


def test_one_atom_is_half_the_mean_huber_loss():
    rng = np.random.default_rng(0)
    B = 33
    cur, tgt = rng.normal(0, 2, (B, 1)), rng.normal(0, 2, (B, 1))
    d = (tgt - cur).reshape(B)
    huber = np.where(np.abs(d) <= 1, 0.5 * d * d, np.abs(d) - 0.5)
    got = ref.quantile_huber(cur, tgt)
    assert abs(got - 0.5 * huber.mean()) <= 1e-14 * abs(got)  # tau_0 = 0.5: |0.5 - 1[.]| = 0.5 either way


def test_the_loss_sums_over_the_current_quantile_and_averages_the_rest():
    rng = np.random.default_rng(1)
    B, Nq, Nt = 4, 7, 5
    cur, tgt = rng.normal(0, 2, (B, Nq)), rng.normal(0, 2, (B, Nt))
    total = 0.0
    for b in range(B):
        for i in range(Nq):
            for j in range(Nt):
                d = tgt[b, j] - cur[b, i]
                h = 0.5 * d * d if abs(d) <= 1 else abs(d) - 0.5
                total += abs((i + 0.5) / Nq - (1.0 if d < 0 else 0.0)) * h
    assert abs(ref.quantile_huber(cur, tgt) - total / (B * Nt)) <= 1e-13 * total
    from core.qrdqn.qrdqn import quantile_huber_loss

    mine = quantile_huber_loss(th.as_tensor(cur), th.as_tensor(tgt))
    assert abs(float(mine) - total / (B * Nt)) <= 1e-13 * total
    assert abs(float(quantile_huber_loss(th.as_tensor(cur), th.as_tensor(tgt), sum_over_quantiles=False)) - total / (B * Nt * Nq)) <= 1e-13 * total


def test_greedy_index_takes_the_first_maximum_and_a_nan_as_the_greatest():
    z = np.zeros((3, 2, 4), np.float32)
    z[0, :, 2] = z[0, :, 3] = 1.0
    z[1, 1, 1], z[1, :, 3] = np.nan, 9.0
    z[2, 0, 0], z[2, 1, 0] = 5.0, -5.0  # sums to 0 like every other action: index 0
    np.testing.assert_array_equal(ref.greedy_index(z), [2, 1, 0])


@pytest.mark.parametrize("K,Nq", [(3, 8), (5, 200), (16, 25)])
def test_folded_head_gives_the_mean_of_the_atoms(K, Nq):
    pol = ref.make_policy(K, seed=0, n_quantiles=Nq)
    net = pol.quantile_net.quantile_net.double()
    obs = th.as_tensor(np.random.default_rng(2).uniform(-1, 1, (64, 4)))
    with th.no_grad():
        h = net[:-1](obs)
        want = net(obs).view(64, Nq, K * K).mean(dim=1).numpy()
    w, b = ref.folded_head(net[-1].weight.detach().numpy(), net[-1].bias.detach().numpy(), Nq, K * K)
    np.testing.assert_allclose(h.numpy() @ w.T + b, want, rtol=0, atol=1e-15 * Nq)


def test_policy_modules_keys_and_seeded_trunk():
    from core.common.spaces import Box, Discrete
    from core.common.utils import set_random_seed
    from core.dqn.policies import DQNPolicy
    from core.qrdqn.policies import MlpPolicy, QRDQNPolicy, QuantileNetwork

    assert MlpPolicy is QRDQNPolicy and issubclass(QRDQNPolicy, DQNPolicy)
    sig = inspect.signature(QRDQNPolicy.__init__).parameters
    assert sig["n_quantiles"].default == 200 and sig["net_arch"].default is None
    p = ref.make_policy(3, seed=3)
    assert isinstance(p.quantile_net, QuantileNetwork) and p.quantile_net.n_quantiles == 200 and p.quantile_net.net_arch == [64, 64]
    want = [f"{n}.quantile_net.{l}.{t}" for n in ("quantile_net", "quantile_net_target") for l in (0, 2, 4) for t in ("weight", "bias")]
    assert sorted(p.state_dict()) == sorted(want)
    assert tuple(p.quantile_net.quantile_net[4].weight.shape) == (200 * 9, 64)
    assert all(th.equal(a, b) for a, b in zip(p.quantile_net.parameters(), p.quantile_net_target.parameters()))
    q = ref.make_policy(3, seed=3, arch=(32, 32), n_quantiles=8)
    obs = th.rand(5, 4) * 2 - 1
    z = q.quantile_net(obs)
    assert tuple(z.shape) == (5, 8, 9)
    np.testing.assert_array_equal(z.detach().numpy(), q.quantile_net.quantile_net(obs).detach().numpy().reshape(5, 8, 9))  # atom i of action a at i * M + a
    assert th.equal(q.quantile_net._predict(obs), z.mean(dim=1).argmax(dim=1))
    act, state = q.predict(obs.numpy(), deterministic=True)
    assert state is None and act.dtype == np.int64 and act.shape == (5,) and np.array_equal(act, z.mean(dim=1).argmax(dim=1).numpy())
    # construction order network, target, copy: the same seed gives DQNPolicy's first two Linear layers bit for bit
    set_random_seed(3)
    dqn = DQNPolicy(Box(-1, 1, (4,)), Discrete(9), lambda _: 1e-4)
    for l in (0, 2):
        assert th.equal(dqn.q_net.q_net[l].weight, p.quantile_net.quantile_net[l].weight) and th.equal(dqn.q_net.q_net[l].bias, p.quantile_net.quantile_net[l].bias)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="n_quantiles"):
            ref.make_policy(3, n_quantiles=bad)
    with pytest.raises(ValueError, match="Discrete"):
        QuantileNetwork(Box(-1, 1, (4,)), Box(-1, 1, (2,)), th.nn.Flatten(), 4)


def test_class_defaults_and_refusals_without_a_device():
    import core
    from core import QRDQN
    from core.dqn import DQN
    from core.qrdqn import QRDQN as Q2

    assert QRDQN is Q2 and "QRDQN" in core.__all__ and issubclass(QRDQN, DQN) and QRDQN.policy_aliases.keys() == {"MlpPolicy"}
    sig = {k: v.default for k, v in inspect.signature(QRDQN.__init__).parameters.items()}
    want = dict(learning_rate=5e-5, buffer_size=1_000_000, learning_starts=100, batch_size=32, tau=1.0, gamma=0.99, train_freq=4, gradient_steps=1,
                target_update_interval=10000, exploration_fraction=0.005, exploration_initial_eps=1.0, exploration_final_eps=0.01, max_grad_norm=None,
                faithful_quirks=True, policy_kwargs=None, optimize_memory_usage=False)
    assert {k: sig[k] for k in want} == want
    # no optimiser named: Adam (the policy's default class) with the paper's eps = 0.01 / batch_size; a named class is left alone
    assert QRDQN.default_policy_kwargs(None, 32) == dict(optimizer_kwargs=dict(eps=0.01 / 32))
    mine = dict(n_quantiles=8)
    assert QRDQN.default_policy_kwargs(mine, 64) == dict(n_quantiles=8, optimizer_kwargs=dict(eps=0.01 / 64)) and mine == dict(n_quantiles=8)
    named = dict(optimizer_class=th.optim.SGD, optimizer_kwargs=dict(momentum=0.5))
    assert QRDQN.default_policy_kwargs(named, 32) == named
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_quantiles"):
            QRDQN("MlpPolicy", None, policy_kwargs=dict(n_quantiles=bad))
    with pytest.raises(ValueError, match="n_quantiles=8"):  # an archive of 8 atoms against a model asked to have 16
        QRDQN._check_load_arguments(dict(n_quantiles=8), dict(policy_kwargs=dict(n_quantiles=16)))
    QRDQN._check_load_arguments(dict(n_quantiles=8), dict(policy_kwargs=dict(n_quantiles=8)))
    QRDQN._check_load_arguments(dict(n_quantiles=200), dict())
    with pytest.raises(ValueError, match="n_quantiles=8"):  # an archive that contradicts itself
        QRDQN._check_archive(dict(n_quantiles=8, policy_kwargs=dict(n_quantiles=16)), None)
    with pytest.raises(ValueError, match="discrete_actions"):
        QRDQN._check_archive(dict(n_quantiles=8, policy_kwargs=dict(n_quantiles=8), discrete_actions=3), None)
    assert QRDQN._ctor_keys() == DQN._ctor_keys()  # every key is a constructor argument


def test_entry_points_check_their_arguments_on_the_host():
    from core import _native as nv

    lib = nv.lib()
    null, odd = C.c_void_p(None), C.c_void_p(0x10002)
    i64, dbl = C.c_int64, C.c_double
    assert {"cstr_qrdqn_supported", "cstr_qrdqn_fold_head_f32", "cstr_qrdqn_loss_f32"} <= set(nv.SYMBOLS) and nv.QRDQN_MAX_QUANTILES == 256
    sup = lambda m, k, n: bool(lib.cstr_qrdqn_supported(m, k, n))  # noqa: E731
    assert sup(4, 2, 1) and sup(9, 3, 8) and sup(25, 5, 200) and sup(256, 16, 256)
    assert not sup(4, 2, 0) and not sup(4, 2, 257) and not sup(1, 1, 8) and not sup(289, 17, 8) and not sup(10, 3, 8) and not sup(9, 3, -1)
    P = [C.c_void_p(0x1000000 * (i + 1)) for i in range(12)]  # disjoint fake buffers, 16 MiB apart

    def loss(z=P[0], ldz=72, zn=P[1], ldn=72, valve=P[2], rew=P[3], done=P[4], gamma=0.99, batch=8, m=9, k=3, nq=8, gz=P[5], lo=null, ls=null,
             cur=null, tgt=null, nxt=null, ws=P[6]):
        return lib.cstr_qrdqn_loss_f32(z, i64(ldz), zn, i64(ldn), valve, rew, done, dbl(gamma), i64(batch), m, k, nq, gz, lo, ls, cur, tgt, nxt, ws, null)

    for kw in (dict(z=null), dict(zn=null), dict(valve=null), dict(rew=null), dict(done=null), dict(gz=null), dict(ws=null), dict(batch=0), dict(m=0),
               dict(k=0), dict(nq=0), dict(gamma=-0.1), dict(gamma=float("nan")), dict(ldz=71), dict(ldn=71), dict(z=odd), dict(gz=odd),
               dict(valve=C.c_void_p(0x3000004)), dict(ws=C.c_void_p(0x7000004)), dict(nxt=C.c_void_p(0x8000004)), dict(gz=P[0]), dict(gz=P[1]),
               dict(tgt=P[1]), dict(cur=P[3]), dict(lo=P[5]), dict(lo=P[7], ls=P[7]), dict(nxt=P[6]),
               dict(ws=C.c_void_p(0x1000000 + 4 * (7 * 72 + 72) - 8))):  # ws on the last atoms of z
        assert loss(**kw) == -1, kw
    for kw in (dict(nq=257, ldz=257 * 9, ldn=257 * 9), dict(m=10), dict(k=17, m=289, ldz=8 * 289, ldn=8 * 289), dict(batch=16385)):
        assert loss(**kw) == -2, kw

    def fold(w=P[0], b=P[1], m=9, nq=8, h=64, wm=P[2], bm=P[3]):
        return lib.cstr_qrdqn_fold_head_f32(w, b, m, nq, i64(h), wm, bm, null)

    for kw in (dict(w=null), dict(b=null), dict(wm=null), dict(bm=null), dict(m=0), dict(nq=0), dict(h=0), dict(w=odd), dict(bm=odd), dict(wm=P[0]),
               dict(bm=P[1]), dict(bm=P[2]), dict(wm=C.c_void_p(0x1000000 + 4 * (72 * 64 - 1)))):
        assert fold(**kw) == -1, kw
    assert fold(m=1 << 20, h=1 << 12) == -2
