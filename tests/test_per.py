"""GPU checks of prioritized experience replay (csrc/cstr_per.hip, PrioritizedReplayBuffer, DQN on it) against the float64 NumPy
statements of tests/_per_reference.py. The shapes are the smallest at which the radix-64 tree can go wrong: (3, 5) one level above the
leaves, (5, 13) C = 65: two levels and a row that straddles a 64-boundary, (65, 64) C = 4160 > 64^2: three levels."""
import pickle

import numpy as np
import pytest
import torch as th

from _dqn_helpers import loss_f64, pair_np, ulps
from _per_reference import children_sums, update_f64, weights_f64
from test_dqn import dev, loss_case, make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (5, 13), (65, 64)]


def make_buffer(rows, n, seed=0, **kw):
    """a partly filled ring of random fields; leaf priorities in [1e-3, 10], zero runs at the front, the unfilled tail zero"""
    from core.common.buffers import PrioritizedReplayBuffer
    from core.common.spaces import Box

    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)  # noqa: E731
    flag = lambda: (rng.uniform(size=(rows, n)) < 0.3).astype(np.float32)  # noqa: E731
    filled = rows - 1
    rb = PrioritizedReplayBuffer.from_arrays(Box(-1, 1, (4,)), Box(-1, 1, (2,)), DEV, f(rows, n, 4), f(rows, n, 4), f(rows, n, 2), f(rows, n),
                                             flag(), flag(), pos=filled, full=False, **kw)
    leaves = rng.uniform(1e-3, 10.0, rows * n)
    leaves[filled * n:] = 0.0
    leaves[[0, 1]] = 0.0
    leaves[3:3 + min(n, 70)] = 0.0
    rb._load_priorities(leaves, 10.0)
    return rb, leaves


def check_nodes(rb):
    """every internal node is the float64 sum of its children as read back"""
    lv = [t.cpu().numpy() for t in rb.tree_levels]
    for child, parent in zip(lv[:-1], lv[1:]):
        np.testing.assert_allclose(parent, children_sums(child), rtol=1e-13, atol=0)
    return lv


@pytest.mark.parametrize("B", [1, 32, 67])
@pytest.mark.parametrize("rows,n", SHAPES)
def test_sample(rows, n, B):
    rb, leaves = make_buffer(rows, n, seed=rows + B)
    rb.set_beta(0.7)
    u = np.random.default_rng(B).uniform(size=B).astype(np.float32)
    u[0], u[-1] = 0.0, 1.0 - 2.0 ** -24  # B = 1: the largest float32 below 1
    total = float(rb.tree.root)
    s1, s2 = rb.sample_into(rb.alloc_batch(B), u=dev(u)), rb.sample_into(rb.alloc_batch(B), u=dev(u))
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(s1, s2))  # two runs, identical bytes
    i = s1.leaf_indices.cpu().numpy()
    cum = np.cumsum(leaves)
    mass, tol = (np.arange(B) + u.astype(np.float64)) * total / B, 1e-12 * total
    assert (leaves[i] > 0).all()
    assert (np.where(i > 0, cum[i - 1], 0.0) - tol <= mass).all() and (mass <= cum[i] + tol).all()
    r, e = i // n, i % n
    ring = {k: getattr(rb, k).cpu().numpy() for k in rb._FIELDS}
    want = (ring["observations"][r, e], ring["actions"][r, e], ring["next_observations"][r, e],
            (ring["dones"] * (1 - ring["timeouts"]))[r, e, None], ring["rewards"][r, e, None])
    assert all(got.cpu().numpy().tobytes() == w.tobytes() for got, w in zip(s1[:5], want))  # the slot's fields, bit for bit
    np.testing.assert_allclose(s1.weights.cpu().numpy()[:, 0], weights_f64(leaves[i], total, (rows - 1) * n, 0.7), rtol=1e-6)
    drawn = rb.sample(B)  # the buffer's own Philox stream: the offset advances by B, no zero leaf comes back
    assert (leaves[drawn.leaf_indices.cpu().numpy()] > 0).all() and int(rb.tree.ctl[2]) == B


@pytest.mark.parametrize("rows,n", SHAPES)
def test_update_add_and_rebuild(rows, n):
    from core.common import hip_ops

    rb, leaves = make_buffer(rows, n, seed=7, alpha=0.6, min_priority=1e-3)
    rng = np.random.default_rng(1)
    last = (rows - 1) * n - 1                 # the last filled slot: only position 11 names it
    idx = rng.integers(0, last, 40)
    idx[[5, 17, 39]] = idx[2]                 # one leaf four times: position 39 wins
    idx[30] = idx[9]
    idx[11] = last
    td = rng.uniform(0.0, 20.0, 40).astype(np.float32) * rng.choice([-1, 1], 40)
    td[9] = np.nan                            # a duplicate that loses to position 30
    td[11] = np.nan                           # the NaN entry: holds max_priority^alpha
    rb.update_priorities(dev(idx, th.int64), dev(td))
    want, want_max = update_f64(leaves, 10.0, idx, td, 0.6, 1e-3)
    got = rb.priorities.cpu().numpy().reshape(-1)
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
    assert abs(got[last] / 10.0 ** 0.6 - 1) <= 1e-15 and want[idx[9]] == want[idx[30]] != 10.0 ** 0.6
    assert rb.max_priority == want_max and want_max > 10.0   # exact
    before = [t.copy() for t in check_nodes(rb)]
    # the add behind a ring write that wraps pos from rows - 1 to 0
    rb._adds = rows - 1
    rb.ring.ctl.copy_(th.tensor([rows - 1, 0, 0, rows - 1]))
    z = lambda *s: th.zeros(*s, device=DEV)  # noqa: E731
    rb.add(z(n, 4), z(n, 4), z(n, 2), z(n), z(n), None)
    assert rb.ring.ctl.tolist()[:2] == [0, 1]
    after = check_nodes(rb)
    np.testing.assert_allclose(after[0][(rows - 1) * n:], want_max ** 0.6, rtol=1e-15)
    assert np.array_equal(after[0][:(rows - 1) * n], before[0][:(rows - 1) * n])
    for t in rb.tree_levels[1:]:              # the tree is a pure function of its leaves: a rebuild gives the same bits back
        t.zero_()
    hip_ops.per_rebuild(rb.tree)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after, check_nodes(rb)))


@pytest.mark.parametrize("B", [1, 65, 257])
def test_weighted_loss(B):
    from core.common import hip_ops as ops

    K, M = 3, 9
    q, nq, index, rew, done = loss_case(B, K, 5 * B)

    def run(w):
        g, out, cur, tgt, tda = th.full((B, M), 5.0, device=DEV), th.zeros(1, device=DEV), *(th.zeros(B, device=DEV) for _ in range(3))
        per = {} if w is None else dict(weights=dev(w), td_abs_out=tda)
        ops.dqn_loss(dev(q), dev(nq), dev(pair_np(index, K)), dev(rew), dev(done), 0.99, K, g, out, ops.new_ppo_workspace(DEV), cur_q_out=cur,
                     target_out=tgt, **per)
        return [t.cpu().numpy() for t in (g, out, cur, tgt, tda)]

    plain, ones = run(None), run(np.ones(B, np.float32))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain[:4], ones[:4]))  # w = 1: cstr_dqn_loss_f32's bytes
    w = np.random.default_rng(B).uniform(0.05, 1.0, B).astype(np.float32)
    g, loss, cur, tgt, tda = run(w)
    wc, wt, _, wg = loss_f64(q, nq, index, rew, done, 0.99)
    z = np.abs(wc - wt)
    wl = float((w * np.where(z < 1.0, 0.5 * z * z, z - 0.5)).mean())
    assert ulps(tgt, wt).max() <= 2 and ulps(cur, wc).max() <= 2 and ulps(g, wg * w[:, None].astype(np.float64)).max() <= 2
    assert ulps(tda, z).max() <= 2 and abs(float(loss[0]) - wl) <= 1e-5 * max(abs(wl), 1.0)


def per_model(**kw):
    from core.common.buffers import PrioritizedReplayBuffer

    return make_model(3, n_envs=8, seed=5, batch_size=16, buffer_size=64 * 8, learning_starts=16, replay_buffer_class=PrioritizedReplayBuffer,
                      policy_kwargs=dict(net_arch=[32, 32]), **kw)


def test_dqn_fused_against_torch_statements():
    """three teacher-forced gradient steps; the bars are those test_teacher_forced_train_matches_the_reference applies to the same
    quantities (1e-5 on losses over the target scale); priorities are (|td| + 1e-6)^0.6 of values held to that bar"""
    u = [th.rand(16, generator=th.Generator().manual_seed(k)) for k in range(3)]
    caps = []
    for fused in (True, False):
        model = per_model()
        model.learn(8 * 8)
        model.fused_learner, model.debug_capture, model.per_uniform_queue = fused, True, [t.clone() for t in u]
        del model.train_capture[:]
        for _ in range(3):
            model.train(gradient_steps=1, batch_size=16)
        caps.append((model.train_capture, model.replay_buffer.priorities.cpu().numpy()))
        assert not model.per_uniform_queue and {"train/per_beta", "train/per_weight_mean", "train/per_max_priority"} <= set(model.logger.name_to_value)
    (a, pa), (b, pb) = caps
    scale = max(float(y["target_q"].abs().mean()) for y in b)
    for x, y in zip(a, b):
        assert th.equal(x["leaf_indices"], y["leaf_indices"])
        assert abs(float(x["loss"]) - float(y["loss"])) <= 1e-5 * scale
        np.testing.assert_allclose(x["weights"].cpu().numpy(), y["weights"].cpu().numpy(), rtol=1e-5)
    # a priority is (|current - target| + min_priority)^alpha: both Q values are held to 1e-5 * scale, so |td| to twice that
    assert np.abs(pa ** (1 / 0.6) - pb ** (1 / 0.6)).max() <= 2e-5 * scale


def test_dqn_graph_replay_pickle_and_refusal():
    from core.common.buffers import PrioritizedReplayBuffer
    from core.common.vec_env import CSTRVecEnv
    from core.qrdqn import QRDQN
    from test_dqn import snapshot

    def run(graph):
        model = per_model(train_freq=4, target_update_interval=2 * 4 * 8, exploration_fraction=0.5)
        if graph:
            model.enable_graph_capture(True, unroll=1)
        model.learn(8 * 4 * 30)
        th.cuda.synchronize()
        rb = model.replay_buffer
        return model, dict(snapshot(model), tree=rb.tree.node.cpu().numpy(), per_ctl=rb.tree.ctl.cpu().numpy(), beta=rb._beta_dev.cpu().numpy())

    _, a = run(False)
    model, b = run(True)
    st = model.graph_status()
    assert st["active"] and st["error"] is None and st["replays"] > 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    rb = model.replay_buffer
    back = pickle.loads(pickle.dumps(rb))
    assert th.equal(back.priorities, rb.priorities) and th.equal(back.tree.root, rb.tree.root) and back.max_priority == rb.max_priority
    with pytest.raises(NotImplementedError):
        QRDQN("MlpPolicy", CSTRVecEnv(4, discrete_actions=3, device=DEV), device=DEV, replay_buffer_class=PrioritizedReplayBuffer)


def test_skew():
    """the descent follows the mass: equal priorities reach every leaf, one dominant leaf takes its share"""
    rb, _ = make_buffer(2, 64, seed=3)
    rb._adds = 128
    rb.ring.ctl.copy_(th.tensor([0, 1, 0, 128]))
    u = th.rand(4, 1024, generator=th.Generator().manual_seed(0)).to(DEV)
    for heavy in (False, True):
        leaves = np.zeros(128)
        leaves[:64] = 1.0
        if heavy:
            leaves[37] = 1000.0 * 63.0
        rb._load_priorities(leaves, 1.0)
        hits = th.cat([rb.sample_into(rb.alloc_batch(1024), u=u[k]).leaf_indices for k in range(4)]).cpu().numpy()
        counts = np.bincount(hits, minlength=128)
        assert counts[64:].sum() == 0 and ((counts[37] >= 0.99 * 4096) if heavy else (counts[:64] > 0).all())
