"""CPU-side checks of DQN: the three cstr_dqn entry points are exported and reject bad arguments on the host (nothing is dereferenced
or launched), `from core import DQN` resolves, the Discrete space, the discrete valve face v(.) and its inverse, the seeded initial
weights of DQNPolicy against the fixtures written by the unmodified reference (tests/golden/dqn_*.npz, tools/refharness/gen_golden.py
--only dqn), the exploration schedule and the legacy-stream draw order of the reference's learn(), and the fp64 restatements of
tests/_dqn_helpers.py against the reference's own Q values, targets and losses -- the yardstick is checked before the GPU run."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from _dqn_helpers import level_np, loss_f64, mlp_f64, pair_np, valve_np
from core import _native as nv

i64, f32 = C.c_int64, C.c_float
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
DQN_SYMBOLS = ("cstr_mt19937_rand_flag_f64", "cstr_dqn_act_f32", "cstr_dqn_loss_f32")


def P(k: int) -> C.c_void_p:
    """the k-th of a set of fake, well separated, 256-byte-aligned device addresses (never dereferenced)"""
    return C.c_void_p(0x1000000 * (k + 1))


def off(p: C.c_void_p, nbytes: int) -> C.c_void_p:
    return C.c_void_p(p.value + nbytes)


def test_dqn_symbols_declared_and_exported():
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in DQN_SYMBOLS)
    assert lib.cstr_abi_version() == 5  # additive


def test_rand_flag_rejects_bad_arguments_on_the_host():
    f = nv.lib().cstr_mt19937_rand_flag_f64
    assert f(null, P(1), P(2), null, null) == BAD and f(P(0), null, P(2), null, null) == BAD and f(P(0), P(1), null, null, null) == BAD
    assert f(P(0), off(P(1), 4), P(2), null, null) == BAD          # the threshold is a double
    assert f(P(0), P(1), off(P(2), 2), null, null) == BAD          # the flag an int32
    assert f(P(0), P(1), P(2), off(P(3), 4), null) == BAD          # the kept draw a double
    assert f(P(0), off(P(0), 8 * 100), P(2), null, null) == BAD    # the threshold inside the stream image
    assert f(P(0), P(1), P(1), null, null) == BAD                  # flag on the threshold


def act(q=P(0), ldq=9, n=8, m=9, k=3, mode=0, eps=null, flag=null, u=null, rng=null, valve=P(5), index=null):
    return nv.lib().cstr_dqn_act_f32(q, i64(ldq), i64(n), m, k, mode, eps, flag, u, rng, valve, index, null)


def test_act_rejects_bad_arguments_on_the_host():
    assert act(q=null) == BAD and act(valve=null) == BAD and act(n=0) == BAD and act(m=0) == BAD and act(ldq=8) == BAD
    assert act(mode=3) == BAD and act(mode=-1) == BAD
    assert act(mode=1, u=P(3)) == BAD and act(mode=2, u=P(3)) == BAD              # mode 1 needs the flag, mode 2 the rate
    assert act(mode=1, flag=P(2)) == BAD and act(mode=1, flag=P(2), u=P(3), rng=P(4)) == BAD  # exactly one source of uniforms
    assert act(m=10, ldq=10) == UNSUP and act(k=1, m=1, ldq=1) == UNSUP and act(k=17, m=289, ldq=289) == UNSUP
    assert act(n=(1 << 30) + 1) == UNSUP
    assert act(valve=off(P(5), 4)) == BAD and act(index=off(P(6), 4)) == BAD and act(q=off(P(0), 2)) == BAD
    assert act(mode=2, eps=off(P(1), 4), u=P(3)) == BAD and act(mode=2, eps=P(1), u=off(P(3), 4)) == BAD
    assert act(valve=off(P(0), 8)) == BAD                                            # the valve rows inside q
    assert act(index=P(5)) == BAD                                                    # index on the valve rows
    assert act(mode=2, eps=P(1), u=P(5)) == BAD                                      # the uniforms are the output


def loss(q=P(0), ldq=9, nq=P(1), ldn=9, valve=P(2), rew=P(3), done=P(4), gamma=0.99, b=32, m=9, k=3, g=P(5), out=P(6), acc=null, cur=null,
         tgt=null, ws=P(9)):
    return nv.lib().cstr_dqn_loss_f32(q, i64(ldq), nq, i64(ldn), valve, rew, done, f32(gamma), i64(b), m, k, g, out, acc, cur, tgt, ws, null)


def test_loss_rejects_bad_arguments_on_the_host():
    for name in ("q", "nq", "valve", "rew", "done", "g", "out", "ws"):
        assert loss(**{name: null}) == BAD, name
    assert loss(b=0) == BAD and loss(m=0) == BAD and loss(ldq=8) == BAD and loss(ldn=8) == BAD and loss(gamma=float("nan")) == BAD
    assert loss(m=8, ldq=9) == UNSUP and loss(k=17, m=289, ldq=289, ldn=289) == UNSUP and loss(k=1, m=1) == UNSUP
    assert loss(b=(1 << 30) + 1) == UNSUP
    assert loss(valve=off(P(2), 4)) == BAD and loss(ws=off(P(9), 4)) == BAD and loss(q=off(P(0), 2)) == BAD and loss(out=off(P(6), 2)) == BAD
    assert loss(g=P(0)) == BAD and loss(g=off(P(1), 64)) == BAD                      # the gradient on q / inside next_q
    assert loss(out=off(P(5), 16)) == BAD and loss(cur=P(3)) == BAD and loss(tgt=P(4)) == BAD and loss(acc=P(6)) == BAD
    assert loss(cur=P(7), tgt=P(7)) == BAD and loss(ws=P(5)) == BAD


def test_core_exports_dqn():
    import core
    from core import DQN
    from core.common.off_policy_algorithm import OffPolicyAlgorithm
    from core.dqn import DQN as D2, DQNPolicy, MlpPolicy

    assert DQN is D2 and "DQN" in core.__all__ and issubclass(DQN, OffPolicyAlgorithm) and MlpPolicy is DQNPolicy
    assert set(DQN.policy_aliases) == {"MlpPolicy"}


def test_discrete_space():
    from core.common.spaces import Box, Discrete, as_discrete

    d = Discrete(9, seed=5)
    assert d.n == 9 and d.start == 0 and d.shape == () and d.dtype == np.int64 and repr(d) == "Discrete(9)"
    s = [d.sample() for _ in range(200)]
    assert all(isinstance(x, np.int64) and 0 <= x < 9 for x in s) and len(set(int(x) for x in s)) == 9
    assert np.array_equal(Discrete(9, seed=5).sample_batch(200), np.array(s))        # one call = the sequential draws
    assert d.contains(0) and d.contains(np.int64(8)) and not d.contains(9) and not d.contains(-1) and not d.contains(1.0)
    assert not d.contains(np.array([1])) and not d.contains(True)
    assert d == Discrete(9) and d != Discrete(8) and d != Discrete(9, start=1) and d != Box(-1, 1, (2,))
    e = Discrete(3, start=2, seed=0)
    assert repr(e) == "Discrete(3, start=2)" and set(int(x) for x in e.sample_batch(100)) == {2, 3, 4} and e.contains(4) and not e.contains(1)
    with pytest.raises(ValueError):
        Discrete(0)

    class Duck:
        n, start = 4, 0

    assert as_discrete(Duck()) == Discrete(4) and as_discrete(Box(-1, 1, (2,))) is None and as_discrete(d) is d


def test_valve_face_round_trips_and_matches_the_float32_statement():
    from core.common.vec_env.cstr_vec_env import decode_valve_index, encode_valve_pair, valve_levels

    for K in range(2, 17):
        v = valve_levels(K)
        want = np.array([np.float32(-1) + np.float32(2 * q) / np.float32(K - 1) for q in range(K)], np.float32)
        assert v.dtype == np.float32 and v.tobytes() == want.tobytes() and v.tobytes() == valve_np(np.arange(K), K).tobytes()
        assert v[0] == -1 and v[-1] == 1 and np.all(np.diff(v) > 0)
        assert np.array_equal(level_np(v, K), np.arange(K))
        a = np.arange(K * K)
        pairs = decode_valve_index(a, K)
        assert pairs.shape == (K * K, 2) and pairs.tobytes() == pair_np(a, K).tobytes()
        assert np.array_equal(pairs[:, 0], v[a // K]) and np.array_equal(pairs[:, 1], v[a % K])
        assert np.array_equal(encode_valve_pair(pairs, K), a)
        assert np.array_equal(encode_valve_pair(decode_valve_index(a.reshape(K, K), K), K), a.reshape(K, K))


@pytest.mark.parametrize("name,K,arch", [("dqn_train_kat_small.npz", 3, [64, 64]), ("dqn_train_kat_default.npz", 5, None)])
def test_policy_keys_and_seeded_initial_weights(golden, name, K, arch):
    from core.common.spaces import Box, Discrete
    from core.dqn import DQNPolicy

    g = golden(name)
    th.manual_seed(0)  # set_random_seed(0) of the fixture's run
    pol = DQNPolicy(Box(-1, 1, (4,)), Discrete(K * K), lambda _: 1e-4, **({} if arch is None else dict(net_arch=arch)))
    keys = sorted(pol.state_dict())
    assert keys == sorted(f"{n}.q_net.{i}.{p}" for n in ("q_net", "q_net_target") for i in (0, 2, 4) for p in ("weight", "bias"))
    assert pol.net_arch == [64, 64] and pol.q_net.q_net[4].out_features == K * K and isinstance(pol.q_net.q_net[1], th.nn.ReLU)
    for nm in ("q_net", "q_net_target"):
        for k, v in getattr(pol, nm).state_dict().items():
            np.testing.assert_array_equal(v.numpy(), g[f"before/{nm}/{k}"], err_msg=f"{nm}/{k}")


def test_exploration_schedule_of_the_reference_run(golden):
    from core.common.utils import get_linear_fn

    g = golden("dqn_explore_kat.npz")
    n, total, ls = int(g["n_envs"]), int(g["total_timesteps"]), int(g["learning_starts"])
    sched = get_linear_fn(float(g["exploration_initial_eps"]), float(g["exploration_final_eps"]), float(g["exploration_fraction"]))
    # a step at num_timesteps t uses the rate the previous step's _on_step set: schedule(1 - t / total); warm-up steps draw nothing
    steps = [t for t in range(0, total, n) if t >= ls]
    want = [sched(1.0 - float(t) / float(total)) for t in steps]
    assert len(want) == len(g["exploration_rate"]) and want == g["exploration_rate"].tolist()  # float64, bit for bit
    assert sched(1.0 - float(int(g["num_timesteps"])) / float(total)) == float(g["final_exploration_rate"])


def test_draw_order_of_the_reference_run(golden):
    """rand() per post-warm-up vec-step, two randint per gradient step, on one legacy stream"""
    g = golden("dqn_explore_kat.npz")
    n, B, tf, ls, total = (int(g[k]) for k in ("n_envs", "batch_size", "train_freq", "learning_starts", "total_timesteps"))
    rs = np.random.RandomState()
    rs.set_state(("MT19937", g["mt_key0"], int(g["mt_pos0"])))
    flags, draws, bis, eis = [], [], [], []
    t, rates, rows = 0, list(g["exploration_rate"]), 0
    while t < total:
        for _ in range(tf):
            if t >= ls:
                r = rs.random_sample()
                draws.append(r)
                flags.append(r < rates[len(flags)])
            t += n
            rows += 1
        if t > ls:
            bis.append(rs.randint(0, rows, size=B))
            eis.append(rs.randint(0, n, size=(B,)))
    assert draws == g["rand"].tolist() and np.array_equal(np.array(flags, np.uint8), g["explored"])
    assert np.array_equal(np.stack(bis), g["batch_inds"]) and np.array_equal(np.stack(eis), g["env_indices"])
    assert [int(h) for h in g["batch_high"]] == [tf * (i + 1) for i in range(len(bis))]
    st = rs.get_state()
    assert np.array_equal(st[1], g["mt_key_final"]) and int(st[2]) == int(g["mt_pos_final"])
    assert g["explored"].any() and not g["explored"].all()


@pytest.mark.parametrize("name", ["dqn_train_kat_small.npz", "dqn_train_kat_default.npz"])
def test_fp64_restatement_reproduces_the_reference(golden, name):
    """current_q / target_q / loss of every step from the fixture's weights, at 1e-5 of the batch's Q scale (the f32 reference against
    fp64): the weights before step k are `before` (k = 0) or `after/step{k-1}`"""
    g = golden(name)
    gamma, n_steps, K = float(g["hyper"][0]), int(g["hyper"][5]), int(g["hyper"][6])
    for k in range(n_steps):
        pre = "before" if k == 0 else f"after/step{k - 1}"
        q = mlp_f64(g, f"{pre}/q_net", g[f"step{k}/batch_observations"])
        nq = mlp_f64(g, f"{pre}/q_net_target", g[f"step{k}/batch_next_observations"])
        cur, target, loss, _ = loss_f64(q, nq, g[f"step{k}/batch_index"], g[f"step{k}/batch_rewards"], g[f"step{k}/batch_dones"], gamma)
        wc, wt = g[f"step{k}/current_q"].reshape(-1).astype(np.float64), g[f"step{k}/target_q"].reshape(-1).astype(np.float64)
        scale = max(np.abs(wt).mean(), np.abs(wc).mean())
        assert np.abs(cur - wc).max() <= 1e-5 * scale and np.abs(target - wt).max() <= 1e-5 * scale, (k, scale)
        assert abs(loss - float(g[f"step{k}/loss"])) <= 1e-5 * max(abs(loss), 1.0)
        assert int(g[f"step{k}/n_updates"]) == k + 1 and int(g[f"step{k}/optimizer_step"]) == k + 1
    upd = int(g["hyper"][7])
    for k in range(n_steps):  # the target net changes exactly at the update
        prev = "before" if k == 0 else f"after/step{k - 1}"
        same = all(np.array_equal(g[f"{prev}/q_net_target/q_net.{i}.weight"], g[f"after/step{k}/q_net_target/q_net.{i}.weight"]) for i in (0, 2, 4))
        assert same == (k != upd)
        if k == upd:
            assert all(np.array_equal(g[f"after/step{k}/q_net/q_net.{i}.weight"], g[f"after/step{k}/q_net_target/q_net.{i}.weight"]) for i in (0, 2, 4))
    assert {"train/learning_rate", "train/loss", "train/n_updates"} <= set(g["logged_keys"].tolist())


def test_predict_fixture_is_consistent(golden):
    g = golden("dqn_predict_kat.npz")
    q = mlp_f64(g, "before/q_net", g["obs"])
    assert np.array_equal(q.argmax(axis=1), g["actions"]) and g["actions"].dtype == np.int64 and len(g["obs"]) == int(g["kept"]) >= 32
    top = np.sort(q, axis=1)
    assert ((top[:, -1] - top[:, -2]) >= 0.9e-3 * np.abs(q).mean()).all()
