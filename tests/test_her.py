"""GPU tests of HER (csrc/cstr_her.hip, core/her, the goal face of CSTRVecEnv).

  * cstr_her_add_f32 against the NumPy restatement of tests/_her_reference.py step by step (bookkeeping, ring rows, goals, control words,
    the sampler's summaries), sentinels, relaunch;
  * cstr_her_sample_f32 against `np.random.RandomState` itself through the restatement: indices, goal rows, the five outputs and the
    final MT19937 image bit for bit, for the three strategies, B in {1, 10, 256}, nb_virtual in {0, int(0.8 B)}, streams at position 0,
    at 620 (a twist inside the draws) and with a cached Gaussian; the bound cases of the array-form randint; forced mode; the empty buffer;
  * the fixture of the unmodified reference (tests/golden/her_buffer_kat.npz) replayed through the device buffer;
  * cstr_goal_vec_step_f32 against cstr_vec_step_f32 + cstr_reset_draw_f32 (everything but the reward bit-identical), the reward against
    the NumPy statement with per-env targets, the NaN path, the Philox target redraw against its counter contract.
The restatement itself is held to the reference's fixture in tests/test_her_abi.py. Virtual rewards are compared bit for bit: the
library is built with contraction off and IEEE division."""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch as th

from _dqn_helpers import philox4x32_10
from _her_reference import GOAL_TAG, HerNp, goal_of_target, goal_reward, mt_image, scripted_adds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "her_buffer_kat.npz")
SENTINEL = -777.0


@pytest.fixture(scope="module")
def ops():
    from core import _native as nv
    from core.common import hip_ops

    nv.lib()
    assert th.cuda.is_available()
    return hip_ops


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(GOLDEN))


def dev(x, dtype=None):
    t = th.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def make_buffer(rows, n_envs, n_sampled_goal=4, strategy="future", seed=None, goal_range=None):
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    env = CSTRVecEnv(n_envs, device=DEV, goal_conditioned=True, goal_range=goal_range)
    rb = HerReplayBuffer(rows * n_envs, env.observation_space, env.action_space, env, device=DEV, n_envs=n_envs, n_sampled_goal=n_sampled_goal,
                         goal_selection_strategy=strategy)
    if seed is not None:
        rb.seed_sampler(seed)
    return env, rb


def assert_state_equal(rb, h, where):
    assert np.array_equal(rb.ep_start, h.ep_start), where
    assert np.array_equal(rb.ep_length, h.ep_length), where
    assert np.array_equal(rb._current_ep_start, h.cur), where
    r = rb.ring
    for got, want in ((r.observations, h.observation), (r.next_observations, h.next_observation), (rb.her.desired_goal, h.desired_goal),
                      (r.actions, h.actions), (r.rewards, h.rewards), (r.dones, h.dones), (r.timeouts, h.timeouts)):
        assert np.array_equal(got.cpu().numpy(), want), where
    assert r.ctl.tolist() == [h.pos, int(h.full), 0, h.adds], where
    valid = h.ep_length > 0  # the sampler's summaries
    assert np.array_equal(rb.her.row_valid.cpu().numpy(), valid.sum(axis=1)), where
    bits = rb.her.valid_bits.cpu().numpy().view(np.uint64)
    got = ((bits[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(h.rows, -1)[:, :h.n_envs].astype(bool)
    assert np.array_equal(got, valid), where


def lengths_for(rows, n_envs):
    base = [1, rows + 3, rows, 2, rows - 1, 3, 2 * rows + 1]
    return [base[i % len(base)] for i in range(n_envs)]


# ---- cstr_her_add_f32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_envs, rows", [(1, 4), (3, 4), (3, 7), (65, 7), (65, 12), (1, 12)])
def test_add_matches_the_restatement_step_by_step(ops, n_envs, rows):
    """Rings of 4, 7 and 12 rows through three wraps with uneven episode ends: episodes of 1 and 2 steps, as long as the ring, longer than
    the ring (and more than twice as long), ending on the last row, and a done on the row that starts an invalidation.
    The episode ends here are scripted per env (`scripted_adds`), not the env's: `max_steps` is one number for all envs, so the env
    cannot give episodes of 1, 2 and 2 * rows + 1 steps side by side. Uneven ends that do come from the env, through
    `set_state(obs, step_count)`, are in test_add_follows_env_steps_with_uneven_ends_from_set_state below."""
    _, rb = make_buffer(rows, n_envs)
    h = HerNp(rows, n_envs)
    # one env: every step an episode end (rows = 4: the last row, the invalidating row) or episodes longer than the ring (rows = 12)
    lengths = lengths_for(rows, n_envs) if n_envs > 1 else [1 if rows == 4 else rows + 3]
    seen = dict(last_row=False, done_on_invalidating_row=False, longer=any(v > rows for v in lengths))
    for t, (o, nx, a, r, d, to) in enumerate(scripted_adds(np.random.default_rng(rows * 100 + n_envs), n_envs, 3 * rows + 2, lengths)):
        seen["last_row"] |= bool(h.pos == rows - 1 and d.any())
        seen["done_on_invalidating_row"] |= bool(((h.ep_length[h.pos] > 0) & (d > 0)).any())
        h.add(o, nx, a, r, d, to)
        rb.add_device(dev(o), dev(nx), dev(a), dev(r), dev(d), dev(to))
        assert_state_equal(rb, h, (n_envs, rows, t))
    if n_envs > 1:
        assert all(seen.values()), seen
    elif rows == 4:
        assert seen["last_row"] and seen["done_on_invalidating_row"], seen
    else:
        assert seen["longer"], seen
    assert rb.pos == h.pos and rb.full == h.full


@pytest.mark.parametrize("n_envs, rows", [(1, 4), (3, 4), (65, 7), (3, 12)])
def test_add_follows_env_steps_with_uneven_ends_from_set_state(ops, n_envs, rows):
    """The env step feeding the add, step by step against the restatement: 6-step episodes whose first ends are staggered by
    `set_state(obs, step_count)` (env i starts at step i % 6, so every vec-step ends some envs and not others), targets redrawn per
    episode, rings of 4 rows (episodes longer than the ring), 7 and 12 rows through three wraps."""
    from core import _native as nv

    max_steps = 6
    env, rb = make_buffer(rows, n_envs, goal_range=(0.10, 0.40))
    env.coef = nv.default_coef(0.20, 0.05, 0.45, max_steps)
    env.seed(9)
    env.reset()
    rng = np.random.default_rng(rows * 100 + n_envs)
    env.set_state(rng.uniform(-0.5, 0.5, (n_envs, 4)).astype(np.float32), (np.arange(n_envs) % max_steps).astype(np.int32))
    h = HerNp(rows, n_envs)
    ends = []
    for t in range(3 * rows + 2):
        prev = env.flat.clone()
        act = dev(rng.uniform(-1, 1, (n_envs, 2)).astype(np.float32))
        _, rew, done, tout, nxt = env.step_device(act)
        rb.add_device(prev, nxt, act, rew, done, tout)
        o, nx, a, r, d, to = (x.cpu().numpy() for x in (prev, nxt, act, rew, done, tout))
        assert np.array_equal(o[:, 0], o[:, 4]) and np.array_equal(nx[:, 0], nx[:, 4]) and np.array_equal(o[:, 1], nx[:, 1])
        h.add(o, nx, a, r, d, to)
        assert_state_equal(rb, h, (n_envs, rows, t))
        ends.append(d > 0)
    ends = np.asarray(ends)
    assert ends.any(axis=0).all()  # every env finished an episode
    if n_envs > 1:
        assert (ends.any(axis=1) & ~ends.all(axis=1)).any() and len({int(np.argmax(e)) for e in ends.T}) > 1  # uneven ends
    assert (h.ep_length > 0).any() and rb.pos == h.pos and rb.full == h.full


@pytest.mark.parametrize("nsg, ratio, nbv10, nbv256", [(0, 0.0, 0, 0), (1, 0.5, 5, 128), (4, 0.8, 8, 204)])
def test_buffer_her_ratio_and_nb_virtual(ops, nsg, ratio, nbv10, nbv256):
    """`HerReplayBuffer.her_ratio` (her_replay_buffer.py:90) and the number of virtual samples the host passes to the sampler (:218)."""
    _, rb = make_buffer(4, 2, n_sampled_goal=nsg)
    assert rb.n_sampled_goal == nsg and rb.her_ratio == 1 - (1.0 / (nsg + 1)) and abs(rb.her_ratio - ratio) < 1e-12
    assert rb.nb_virtual(10) == nbv10 and rb.nb_virtual(256) == nbv256 and rb.nb_virtual(1) == 0


def test_add_leaves_sentinels_alone_and_relaunches_identically(ops):
    """Every array of the ring and of the side state sits between sentinel pads; two launches from equal state write equal bits."""
    from core import _native as nv

    rows, n, pad = 7, 65, 64
    words = (n + 63) // 64

    def padded(numel, dtype, fill):
        full = th.full((numel + 2 * pad,), fill, dtype=dtype, device=DEV)
        return full, full[pad:pad + numel]

    def build():
        spec = dict(obs=(rows * n * 4, th.float32), next_obs=(rows * n * 4, th.float32), act=(rows * n * 2, th.float32), rew=(rows * n, th.float32),
                    done=(rows * n, th.float32), timeout=(rows * n, th.float32), goal=(rows * n, th.float32), start=(rows * n, th.int32),
                    length=(rows * n, th.int32), cur=(n, th.int32), valid=(rows, th.int32), bits=(rows * words, th.int64))
        full, view = {}, {}
        for k, (numel, dt) in spec.items():
            full[k], view[k] = padded(numel, dt, SENTINEL if dt == th.float32 else -777)
            view[k].zero_()
        ring = type("R", (), {})()
        ring.c = nv.Ring(*(view[k].data_ptr() for k in ("obs", "next_obs", "act", "rew", "done", "timeout")), rows, n, 4, 2)
        ring.ctl, ring.n_envs, ring.rows = th.zeros(4, dtype=th.int64, device=DEV), n, rows
        her = type("H", (), {})()
        her.c = nv.Her(*(view[k].data_ptr() for k in ("goal", "start", "length", "cur", "valid", "bits")))
        return full, view, ring, her

    runs = []
    for _ in range(2):
        full, view, ring, her = build()
        h = HerNp(rows, n)
        for o, nx, a, r, d, to in scripted_adds(np.random.default_rng(5), n, 2 * rows + 3, lengths_for(rows, n)):
            h.add(o, nx, a, r, d, to)
            ops.her_add(ring, her, dev(o), dev(nx), dev(a), dev(r), dev(d), dev(to))
        th.cuda.synchronize()
        for k, t in full.items():
            body = view[k].numel()
            assert bool((t[:pad] == (SENTINEL if t.dtype == th.float32 else -777)).all()), k
            assert bool((t[pad + body:] == (SENTINEL if t.dtype == th.float32 else -777)).all()), k
        assert np.array_equal(view["length"].cpu().numpy().reshape(rows, n), h.ep_length)
        assert np.array_equal(view["start"].cpu().numpy().reshape(rows, n), h.ep_start)
        runs.append({k: v.clone() for k, v in view.items()})
    assert all(th.equal(runs[0][k], runs[1][k]) for k in runs[0])


# ---- cstr_her_sample_f32 ---------------------------------------------------------------------------------------------------------------
def upload(rb, h):
    """device buffer <- the restatement's state (the summaries are rebuilt from ep_length)"""
    r = rb.ring
    for t, a in ((r.observations, h.observation), (r.next_observations, h.next_observation), (rb.her.desired_goal, h.desired_goal),
                 (r.actions, h.actions), (r.rewards, h.rewards), (r.dones, h.dones), (r.timeouts, h.timeouts)):
        t.copy_(dev(a))
    rb.her.ep_start.copy_(dev(h.ep_start, th.int32))
    rb.her.ep_length.copy_(dev(h.ep_length, th.int32))
    rb.her.cur_ep_start.copy_(dev(h.cur, th.int32))
    rb.her.rebuild_summaries()
    rb._adds = h.adds
    r.ctl.copy_(th.tensor([h.pos, int(h.full), 0, h.adds], dtype=th.int64))


def filled(rows, n_envs, lengths, seed=0, steps=None):
    h = HerNp(rows, n_envs)
    for args in scripted_adds(np.random.default_rng(seed), n_envs, steps or 2 * rows + 1, lengths):
        h.add(*args)
    return h


def stream_at(kind, seed=11):
    rs = np.random.RandomState(seed)
    if kind == "gauss":
        rs.normal()  # leaves a cached deviate behind: has_gauss = 1
        assert rs.get_state()[3] == 1
    else:
        st = list(rs.get_state())
        st[2] = int(kind)
        rs.set_state(tuple(st))
    return rs


def check_sample(rb, h, rs, B, forced=None):
    """one launch against the restatement on the same stream: indices, goal rows, the five outputs, the stream image"""
    rb._stream = dev(mt_image(rs).view(np.int32))
    want = h.sample(rs, B, forced=forced)
    f = None if forced is None else tuple(dev(np.asarray(x, np.int64)) for x in forced)
    out, bi, ei, gi = rb.sample_with_indices(B, forced=f)
    assert np.array_equal(bi.cpu().numpy(), want["row"]) and np.array_equal(ei.cpu().numpy(), want["env"])
    assert np.array_equal(gi.cpu().numpy(), want["goal_row"])
    for got, k in ((out.observations, "obs"), (out.next_observations, "next"), (out.actions, "act"), (out.dones, "done"), (out.rewards, "rew")):
        assert np.array_equal(got.cpu().numpy(), want[k]), k
    assert np.array_equal(rb._stream.cpu().numpy().view(np.uint32), mt_image(rs))
    nbv = int(h.her_ratio * B)
    if nbv:  # virtual rewards = the float32 statement on (next achieved, new goal), virtual goals = achieved goals of the ring
        o, n = out.observations.cpu().numpy(), out.next_observations.cpu().numpy()
        assert np.array_equal(out.rewards.cpu().numpy()[B - nbv:, 0], goal_reward(n[B - nbv:, 0], n[B - nbv:, 1]))
        assert np.array_equal(o[:, 1], n[:, 1]) and np.array_equal(o[:, 0], o[:, 4]) and np.array_equal(n[:, 0], n[:, 4])
    return want


@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
@pytest.mark.parametrize("B", [1, 10, 256])
def test_sample_matches_numpy_randomstate(ops, strategy, B):
    rows, n = 12, 65
    h = filled(rows, n, lengths_for(rows, n), seed=3, steps=3 * rows + 2)
    for nsg in (0, 4):
        _, rb = make_buffer(rows, n, n_sampled_goal=nsg, strategy=strategy)
        upload(rb, h)
        h.strategy, h.her_ratio = strategy, rb.her_ratio
        assert rb.nb_virtual(B) == (0 if nsg == 0 else int(0.8 * B))
        for kind in (0, 620, "gauss"):
            check_sample(rb, h, stream_at(kind), B)
            check_sample(rb, h, stream_at(kind, seed=5), B)


@pytest.mark.parametrize("case", ["no_draw", "power_of_two", "mixed", "one_valid", "one_env_per_row", "single_env"])
def test_sample_bound_cases(ops, case):
    """`high - low == 1` takes no draw (episodes of one step); a power-of-two span never rejects; mixed widths in one batch; a mask that
    leaves one valid transition (randint(0, 1): no draw); one valid env per row; a single env."""
    rows, n = 8, 5
    lengths = dict(no_draw=[1] * n, power_of_two=[2, 4, 2, 4, 2], mixed=[1, 2, 3, 5, 8], one_valid=[3, 4, 2, 5, 8], one_env_per_row=[1, 2, 4, 2, 1],
                   single_env=[3])[case]
    if case == "single_env":
        n = 1
    h = filled(rows, n, lengths, seed=9, steps=rows if case == "power_of_two" else (2 * rows if case == "one_env_per_row" else 2 * rows + 1))
    if case == "power_of_two":
        assert set(np.unique(h.ep_length)) == {2, 4}  # every `episode` span is a power of two
    if case == "one_valid":
        r, e = np.argwhere(h.ep_length > 0)[7]
        keep = np.zeros_like(h.ep_length, bool)
        keep[r, e] = True
        h.ep_length[~keep] = 0
    if case == "one_env_per_row":
        keep = np.zeros_like(h.ep_length, bool)
        for r in range(rows):
            e = np.flatnonzero(h.ep_length[r] > 0)
            keep[r, e[r % len(e)]] = True
        h.ep_length[~keep] = 0
        assert ((h.ep_length > 0).sum(axis=1) == 1).all()
    for strategy in ("future", "final", "episode"):
        _, rb = make_buffer(rows, n, strategy=strategy)
        upload(rb, h)
        h.strategy, h.her_ratio = strategy, rb.her_ratio
        for B in (10, 256):
            rs = stream_at(0)
            before = mt_image(rs).copy()
            want = check_sample(rb, h, rs, B)
            if case == "no_draw" and strategy != "final":
                assert np.array_equal(want["goal_idx"], np.zeros(int(0.8 * B), np.int64))
            if case == "one_valid":
                assert len(set(zip(want["row"], want["env"]))) == 1
                if strategy == "final":
                    assert np.array_equal(mt_image(rs), before)  # randint(0, 1) and `final` draw nothing at all


def test_sample_forced_pairs_and_goals(ops):
    rows, n, B = 12, 65, 10
    h = filled(rows, n, lengths_for(rows, n), seed=3, steps=3 * rows + 2)
    _, rb = make_buffer(rows, n)
    upload(rb, h)
    valid = np.argwhere(h.ep_length > 0)
    pick = valid[np.random.default_rng(0).integers(0, len(valid), B)]
    goal_rows = (h.ep_start[pick[:, 0], pick[:, 1]] + h.ep_length[pick[:, 0], pick[:, 1]] - 1) % rows
    rs = stream_at(0)
    before = mt_image(rs).copy()
    want = check_sample(rb, h, rs, B, forced=(pick[:, 0], pick[:, 1], goal_rows))
    assert np.array_equal(mt_image(rs), before)  # nothing was drawn
    assert np.array_equal(want["row"], np.concatenate([pick[8:, 0], pick[:8, 0]]))
    check_sample(rb, h, stream_at(620), B, forced=(pick[:, 0], pick[:, 1]))  # pairs given, goals drawn from the stream


def test_sample_relaunch_is_identical(ops):
    rows, n, B = 7, 65, 256
    h = filled(rows, n, lengths_for(rows, n), seed=4)
    _, rb = make_buffer(rows, n, seed=21)
    upload(rb, h)
    a = rb.sample_into(rb.alloc_batch(B))
    s1 = rb.sampler_stream.clone()
    rb.seed_sampler(21)
    b = rb.sample_into(rb.alloc_batch(B))
    assert all(th.equal(x, y) for x, y in zip(a, b)) and th.equal(s1, rb.sampler_stream)


def test_empty_buffer_raises_the_reference_error(ops):
    _, rb = make_buffer(4, 3, seed=1)
    stream = rb.sampler_stream.clone()
    with pytest.raises(RuntimeError, match="Unable to sample before the end of the first episode"):
        rb.sample(10)
    assert th.equal(stream, rb.sampler_stream) and not rb.has_valid_transition()
    one = np.ones((3, 6), np.float32)
    rb.add_device(dev(one), dev(one), dev(np.zeros((3, 2), np.float32)), dev(np.zeros(3, np.float32)), dev(np.zeros(3, np.float32)),
                  dev(np.zeros(3, np.float32)))
    with pytest.raises(RuntimeError, match="Unable to sample"):  # a transition, but no finished episode
        rb.sample(10)


# ---- the reference's fixture through the device buffer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["r4a", "r4b", "r12a", "r12b"])
def test_fixture_adds_samples_and_truncation(ops, kat, tag):
    R, N, T, pos, full = (int(v) for v in kat[f"{tag}/meta"])
    env, rb = make_buffer(R, N)
    for t in range(T):
        rb.add_device(*(dev(kat[f"{tag}/{k}"][t]) for k in ("obs", "next", "act", "rew", "done", "timeout")))
        assert np.array_equal(rb.ep_start, kat[f"{tag}/ep_start"][t]) and np.array_equal(rb.ep_length, kat[f"{tag}/ep_length"][t]), t
        assert np.array_equal(rb._current_ep_start, kat[f"{tag}/cur"][t]), t
    assert (rb.pos, int(rb.full)) == (pos, full)
    from core.her.goal_selection_strategy import KEY_TO_GOAL_STRATEGY

    for key in sorted(k[:-len("/flat_idx")] for k in kat if k.startswith(tag + "/") and k.endswith("/flat_idx")):
        _, strategy, nsg, B = key.split("/")
        rb.goal_selection_strategy, rb.n_sampled_goal, rb.her_ratio = KEY_TO_GOAL_STRATEGY[strategy], int(nsg), 1 - (1.0 / (int(nsg) + 1))
        rb.seed_sampler(1000 + int(B) + int(nsg))
        out, bi, ei, gi = rb.sample_with_indices(int(B))
        nbv = rb.nb_virtual(int(B))
        flat = kat[key + "/flat_idx"]  # draw order: virtual first
        assert np.array_equal(bi.cpu().numpy() * N + ei.cpu().numpy(), np.concatenate([flat[nbv:], flat[:nbv]])), key
        for got, k in ((out.observations, "obs"), (out.next_observations, "next"), (out.actions, "act"), (out.dones, "done"), (out.rewards, "rew")):
            assert np.array_equal(got.cpu().numpy(), kat[f"{key}/{k}"]), (key, k)
        image = rb.sampler_stream.cpu().numpy().view(np.uint32)
        assert np.array_equal(image[:624], kat[key + "/mt_key"]) and image[624:626].tolist() == kat[key + "/mt_pos"].tolist(), key
        d = rb.as_dict_samples(out)
        assert d.observations["observation"].shape == (int(B), 4) and d.observations["desired_goal"].data_ptr() == out.observations.data_ptr() + 4
    # pickle without the env, then truncate_last_trajectory (her_replay_buffer.py:101-133, :386-408)
    clone = pickle.loads(pickle.dumps(rb))
    assert clone.env is None and np.array_equal(clone.ep_length, rb.ep_length) and clone.ring.ctl.tolist() == rb.ring.ctl.tolist()
    assert th.equal(clone.her.valid_bits, rb.her.valid_bits) and th.equal(clone.her.row_valid, rb.her.row_valid)
    with pytest.raises(AssertionError, match="You must initialize HerReplayBuffer with a VecEnv"):
        clone.sample(4)
    clone.set_env(env)
    with pytest.raises(ValueError, match="already initialized"):
        clone.set_env(env)
    keep = pickle.loads(pickle.dumps(rb))  # "without truncation": the state stays what it was
    assert np.array_equal(keep._current_ep_start, rb._current_ep_start) and th.equal(keep.dones, rb.dones)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        clone.truncate_last_trajectory()
    assert len(w) == int(kat[f"{tag}/trunc/warned"][0])
    assert np.array_equal(clone.ep_length, kat[f"{tag}/trunc/ep_length"]) and np.array_equal(clone._current_ep_start, kat[f"{tag}/trunc/cur"])
    assert np.array_equal(clone.dones.cpu().numpy(), kat[f"{tag}/trunc/dones"]) and np.array_equal(clone.timeouts.cpu().numpy(), kat[f"{tag}/trunc/timeouts"])
    assert np.array_equal(clone.her.row_valid.cpu().numpy(), (kat[f"{tag}/trunc/ep_length"] > 0).sum(axis=1))


def test_host_add_equals_device_add(ops):
    """`add()` with the reference's dicts and `add_device()` with flat rows leave equal buffers."""
    from core.common.vec_env.cstr_vec_env import goal_rows_to_dict

    rows, n = 7, 3
    _, a = make_buffer(rows, n)
    _, b = make_buffer(rows, n)
    for o, nx, act, r, d, to in scripted_adds(np.random.default_rng(2), n, 2 * rows, [2, 7, 10]):
        a.add_device(dev(o), dev(nx), dev(act), dev(r), dev(d), dev(to))
        b.add(goal_rows_to_dict(o), goal_rows_to_dict(nx), act, r, d.astype(bool), [{"TimeLimit.truncated": bool(x)} for x in to])
    for k in ("ep_start", "ep_length", "_current_ep_start"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    for x, y in ((a.ring.observations, b.ring.observations), (a.ring.next_observations, b.ring.next_observations), (a.her.desired_goal, b.her.desired_goal),
                 (a.actions, b.actions), (a.rewards, b.rewards), (a.dones, b.dones), (a.timeouts, b.timeouts), (a.ring.ctl, b.ring.ctl)):
        assert th.equal(x, y)


def test_refusals(ops, monkeypatch):
    from core.common import distributed as dist_util
    from core.common.buffers import ReplayBuffer
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    goal = CSTRVecEnv(2, device=DEV, goal_conditioned=True)
    box = CSTRVecEnv(2, device=DEV)
    with pytest.raises(ValueError, match="goal face"):
        HerReplayBuffer(8, goal.observation_space, goal.action_space, box, device=DEV, n_envs=2)
    with pytest.raises(ValueError, match="goal face"):
        HerReplayBuffer(8, box.observation_space, box.action_space, goal, device=DEV, n_envs=2)
    with pytest.raises(ValueError, match="copy_info_dict"):
        HerReplayBuffer(8, goal.observation_space, goal.action_space, goal, device=DEV, n_envs=2, copy_info_dict=True)
    for kw in (dict(twin=True, obs_dim=8), dict(obs_dim=8), dict(discrete_actions=3)):
        with pytest.raises(ValueError, match="goal_conditioned"):
            CSTRVecEnv(2, device=DEV, goal_conditioned=True, **kw)
    with pytest.raises(ValueError, match="goal_range"):
        CSTRVecEnv(2, device=DEV, goal_range=(0.1, 0.4))
    with pytest.raises(ValueError, match="goal_range"):
        CSTRVecEnv(2, device=DEV, goal_conditioned=True, goal_range=(0.1, 0.6))
    with pytest.raises(ValueError, match="goal face"):
        box.compute_reward(np.zeros(1), np.zeros(1), None)
    import core
    from core.common.vec_env import VecNormalize

    her = dict(replay_buffer_class=HerReplayBuffer, device=DEV)
    for name in ("SAC", "TD3", "DDPG"):  # the reference's wording for a Dict space (base_class.py:210)
        with pytest.raises(ValueError, match="You must use `MultiInputPolicy` when working with dict observation space, not MlpPolicy"):
            getattr(core, name)("MlpPolicy", goal, **her)
        with pytest.raises(ValueError, match="HerReplayBuffer needs the goal face"):
            getattr(core, name)("MlpPolicy", box, **her)
        with pytest.raises(ValueError, match="needs replay_buffer_class=HerReplayBuffer"):
            getattr(core, name)("MultiInputPolicy", goal, device=DEV)
        with pytest.raises(ValueError, match="MultiInputPolicy needs a Dict observation space"):
            getattr(core, name)("MultiInputPolicy", box, device=DEV)
    for name in ("DQN", "PPO", "A2C"):  # HER is built for SAC, TD3 and DDPG
        with pytest.raises(ValueError, match="does not support a Dict observation space"):
            getattr(core, name)("MlpPolicy", goal, device=DEV)
    with pytest.raises(ValueError, match="MultiInputPolicy unknown"):
        core.DQN("MultiInputPolicy", goal, device=DEV)
    for name in ("MADDPG", "IDDPG"):  # the splits are read after the base class has seen the env
        with pytest.raises(ValueError, match="does not support a Dict observation space"):
            getattr(core, name)(2, "MlpPolicy", goal, [[0, 1], [2, 3]], [[0], [1]], learning_rate_list=[1e-3, 1e-3], device=DEV)
    with pytest.raises(ValueError, match="does not support a Dict observation space"):
        core.BCQ("MlpPolicy", CSTRVecEnv(1, device=DEV, goal_conditioned=True),
                 dataset=ReplayBuffer(64, box.observation_space, box.action_space, device=DEV, n_envs=1), device=DEV)
    with monkeypatch.context() as m:  # a rank of a two-process job: the goal face does not run data-parallel
        m.setattr(dist_util, "rank_world", lambda: (0, 2))
        with pytest.raises(ValueError, match="data-parallel"):
            core.SAC("MultiInputPolicy", goal, **her)
    with pytest.raises(ValueError, match="gSDE"):
        core.SAC("MultiInputPolicy", goal, use_sde=True, **her)
    with pytest.raises(ValueError, match="VecNormalize is not built for the goal face"):
        core.SAC("MultiInputPolicy", VecNormalize(goal), **her)
    model = core.SAC("MultiInputPolicy", goal, train_freq=(1, "episode"), buffer_size=64, policy_kwargs=dict(net_arch=[16, 16]), **her)
    with pytest.raises((ValueError, AssertionError)):  # episodic collection: one env in the reference, device steps only here
        model.learn(8)


# ---- the env step on the goal face ------------------------------------------------------------------------------------------------------
def goal_env_pair(n, goal_range=None, seed=5, integrator="euler"):
    """a goal-face env and a Box-face env in the same state: same seeds, observations and step counters (some about to time out)"""
    from core.common.vec_env import CSTRVecEnv

    g = CSTRVecEnv(n, device=DEV, goal_conditioned=True, goal_range=goal_range, goal_seed=77, seed_offset=3, integrator=integrator)
    b = CSTRVecEnv(n, device=DEV, seed_offset=3, integrator=integrator)
    for e in (g, b):
        e.seed(seed)
        e.reset()
    rng = np.random.default_rng(n)
    steps = rng.integers(396, 400, n).astype(np.int32)
    obs = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    g.set_state(obs, steps)
    b.set_state(obs, steps)
    return g, b, rng


@pytest.mark.parametrize("n, integrator", [(1, "euler"), (130, "euler"), (130, "rk4")])
def test_goal_step_changes_the_reward_and_nothing_else(ops, n, integrator):
    g, b, rng = goal_env_pair(n, integrator=integrator)
    targets = rng.uniform(0.05, 0.45, n).astype(np.float32)
    assert g.set_targets(targets) and not g.set_targets(np.full(n, 0.5, np.float32))
    for t in range(5):
        act = rng.uniform(-1.2, 1.2, (n, 2)).astype(np.float32)
        flat, rew, done, tout, nxt = (x.clone() for x in g.step_device(dev(act)))
        obs_b, _, done_b, tout_b, nxt_b = (x.clone() for x in b.step_device(dev(act)))
        assert th.equal(flat[:, 2:], obs_b) and th.equal(nxt[:, 2:], nxt_b) and th.equal(done, done_b) and th.equal(tout, tout_b), t
        assert th.equal(g.obs, b.obs) and th.equal(g.step_count, b.step_count) and th.equal(g.pcg_state, b.pcg_state), t
        f, x = flat.cpu().numpy(), nxt.cpu().numpy()
        dg = goal_of_target(targets)
        assert np.array_equal(f[:, 0], f[:, 4]) and np.array_equal(x[:, 0], x[:, 4])            # achieved_goal = observation[2]
        assert np.array_equal(f[:, 1], dg) and np.array_equal(x[:, 1], dg)                          # desired_goal = the env's own target
        assert np.array_equal(rew.cpu().numpy(), goal_reward(x[:, 0], dg)), t                     # per-env targets, bit for bit
        assert np.array_equal(rew.cpu().numpy(), g.compute_reward(x[:, 0:1], x[:, 1:2], None))
        assert np.array_equal(g.targets.cpu().numpy(), targets) and g.episode is None           # goal_range=None: targets stay
    assert g.step_count.max().item() < 6  # every env went through an auto-reset


def test_goal_step_nan_action(ops):
    g, b, rng = goal_env_pair(70)
    act = rng.uniform(-1, 1, (70, 2)).astype(np.float32)
    act[[0, 33, 69], [0, 1, 0]] = np.nan
    before = g.flat.clone()
    flat, rew, done, tout, nxt = g.step_device(dev(act))
    obs_b, rew_b, done_b, _, nxt_b = b.step_device(dev(act))
    bad = [0, 33, 69]
    assert rew[bad].tolist() == [-10.0] * 3 and done[bad].tolist() == [1.0] * 3 and tout[bad].tolist() == [1.0] * 3
    assert th.equal(nxt[bad], before[bad])  # old state
    assert th.equal(flat[:, 2:], obs_b) and th.equal(nxt[:, 2:], nxt_b) and th.equal(done, done_b)


def test_goal_range_redraw_follows_the_philox_contract(ops):
    """counter (seed_offset + env index [64 bit], episode ordinal, tag), key = goal_seed; u = (word 0 >> 8) * 2^-24; target = lo + (hi - lo) u
    in float32 -- element by element; at reset() and at auto-resets; the env's PCG64 reset stream is what it is on the Box face."""
    n, lo, hi = 130, 0.10, 0.40
    g, b, rng = goal_env_pair(n, goal_range=(lo, hi))

    def contract(ordinal):
        c = np.zeros((n, 4), np.uint32)
        c[:, 0], c[:, 2], c[:, 3] = 3 + np.arange(n), ordinal, GOAL_TAG
        u = (philox4x32_10(c, np.array([77, 0], np.uint64))[:, 0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        return np.float32(lo) + (np.float32(hi) - np.float32(lo)) * u

    targets = contract(np.zeros(n, np.uint32))  # drawn by reset()
    assert np.array_equal(g.targets.cpu().numpy(), targets) and g.episode.tolist() == [1] * n
    assert targets.min() >= np.float32(lo) and targets.max() <= np.float32(hi) and len(np.unique(targets)) > n // 2
    ordinal = np.ones(n, np.uint32)
    n_done = 0
    for t in range(5):
        act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        flat, rew, done, _, nxt = (x.clone() for x in g.step_device(dev(act)))
        obs_b = b.step_device(dev(act))[0]
        d = done.cpu().numpy() > 0
        assert np.array_equal(nxt.cpu().numpy()[:, 1], goal_of_target(targets))  # the terminal observation keeps the old goal
        assert np.array_equal(rew.cpu().numpy(), goal_reward(nxt.cpu().numpy()[:, 0], goal_of_target(targets)))
        targets = np.where(d, contract(ordinal), targets).astype(np.float32)
        ordinal = ordinal + d.astype(np.uint32)
        assert np.array_equal(g.targets.cpu().numpy(), targets) and np.array_equal(g.episode.cpu().numpy(), ordinal.astype(np.int32))
        assert np.array_equal(flat.cpu().numpy()[:, 1], goal_of_target(targets)) and th.equal(flat[:, 2:], obs_b) and th.equal(g.pcg_state, b.pcg_state)
        n_done += int(d.sum())
    assert n_done >= n  # every env went through an auto-reset


def test_goal_face_host_views(ops):
    from core.common.spaces import Dict
    from core.common.vec_env import CSTRVecEnv

    n = 4
    env = CSTRVecEnv(n, device=DEV, goal_conditioned=True)
    assert isinstance(env.observation_space, Dict) and list(env.observation_space.keys()) == ["achieved_goal", "desired_goal", "observation"]
    env.seed(1)
    obs = env.reset()
    assert {k: v.shape for k, v in obs.items()} == {"achieved_goal": (n, 1), "desired_goal": (n, 1), "observation": (n, 4)}
    assert np.array_equal(obs["achieved_goal"][:, 0], obs["observation"][:, 2]) and env.observation_space.contains({k: v[0] for k, v in obs.items()})
    assert np.array_equal(obs["desired_goal"][:, 0], goal_of_target(np.full(n, 0.20, np.float32)))
    box = CSTRVecEnv(n, device=DEV)
    box.seed(1)
    assert np.array_equal(box.reset(), obs["observation"])  # reset observations stay what they are on the Box face
    assert env.set_target(0.3) and not env.set_target(0.6)
    env.set_state(obs["observation"], np.array([399, 0, 399, 5], np.int32))
    o2, rew, done, infos = env.step(np.zeros((n, 2), np.float32))
    assert done.tolist() == [True, False, True, False] and rew.dtype == np.float32
    term = infos[0]["terminal_observation"]
    assert isinstance(term, dict) and term["observation"].shape == (4,) and term["achieved_goal"][0] == term["observation"][2]
    assert np.array_equal(o2["desired_goal"][:, 0], goal_of_target(np.full(n, 0.3, np.float32))) and "terminal_observation" not in infos[1]
    assert np.array_equal(env.env_method("compute_reward", term["achieved_goal"][None], term["desired_goal"][None], [{}], indices=[0])[0],
                          rew[:1])


# ---- the learners on the goal face ---------------------------------------------------------------------------------------------------
def her_model(algo, n_envs=4, max_steps=None, goal_range=None, **kw):
    import core
    from core import _native as nv
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    env = CSTRVecEnv(n_envs, device=DEV, goal_conditioned=True, goal_range=goal_range)
    if max_steps is not None:
        env.coef = nv.default_coef(0.20, 0.05, 0.45, max_steps)
    return getattr(core, algo)("MultiInputPolicy", env, seed=0, replay_buffer_class=HerReplayBuffer, device=DEV, **kw), env


def replay_fixture_adds(model, g):
    for t in range(g["adds_obs"].shape[0]):
        model.replay_buffer.add_device(*(dev(g[f"adds_{k}"][t]) for k in ("obs", "next", "act", "rew", "done", "timeout")))


def set_path(monkeypatch, fused_path):
    """True: the per-layer fused path; "rocblas": the same glue with the GEMMs left to rocBLAS; False: stock ATen (test_learner_parity.py)"""
    from core.common import chain, fused

    monkeypatch.setattr(chain, "USE_CHAIN", False)
    if fused_path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    return fused_path is not False, f"her_{'aten' if fused_path is False else 'rocblas' if fused_path == 'rocblas' else 'fused'}"


@pytest.mark.parametrize("fused_path", [True, "rocblas", False])
def test_sac_her_train_teacher_forced(golden, fused_path, monkeypatch):
    """Teacher-forced SAC.train() on the goal face against the unmodified reference (MultiInputPolicy + HerReplayBuffer): the ring is
    rebuilt from the recorded adds, the sampler reproduces the reference's relabelled batches bit for bit, Q values / targets / losses
    / weights within the bars of tests/_parity_helpers.py on the three code paths."""
    from _parity_helpers import check_init, check_weights, q_err, rel_err
    from core.common import legacy_rng

    use_fused, lab = set_path(monkeypatch, fused_path)
    g = golden("sac_her_train_kat_small.npz")
    gamma, tau, target_entropy, lr, B, n_steps = g["hyper"]
    B, n_steps = int(B), int(n_steps)
    model, _ = her_model("SAC", batch_size=B, buffer_size=64 * 4, policy_kwargs=dict(net_arch=[64, 64]))
    assert model.fused_learner, "K = 6 / K = 8 inputs run on the per-layer Linear kernels"
    model.fused_learner = use_fused
    assert (model.gamma, model.tau, model.target_entropy, model.lr_schedule(1)) == (gamma, tau, target_entropy, lr)
    mods = ["actor", "critic", "critic_target"]
    check_init(model, g, mods)
    replay_fixture_adds(model, g)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    model.debug_capture = True
    for k in range(n_steps):
        model.actor.action_dist.eps_queue = [th.as_tensor(g[f"step{k}/eps_pi"]), th.as_tensor(g[f"step{k}/eps_next"])]
        model.train(gradient_steps=1, batch_size=B)
        assert not model.actor.action_dist.eps_queue
        for name in ("observations", "actions", "next_observations", "dones", "rewards"):
            np.testing.assert_array_equal(getattr(model._static_batch, name).cpu().numpy(), g[f"step{k}/batch_{name}"], err_msg=f"step {k} {name}")
        t = model.last_train_tensors
        assert q_err(t["target_q"].cpu().numpy(), g[f"step{k}/target_q"], lab) < 1e-5
        assert q_err(t["current_q"][0].cpu().numpy(), g[f"step{k}/current_q1"], lab) < 1e-5
        assert q_err(t["current_q"][1].cpu().numpy(), g[f"step{k}/current_q2"], lab) < 1e-5
        lv = model.logger.name_to_value
        for key in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef"):
            assert rel_err(float(lv[f"train/{key}"]), float(g[f"step{k}/{key}"]), 1e-3) < 1e-5, (key, k)
    check_weights(model, g, "after", mods)
    assert abs(float(model.log_ent_coef.detach()) - float(g["after/log_ent_coef"][0])) < 1e-6 and model._n_updates == n_steps


@pytest.mark.parametrize("fused_path", [True, "rocblas", False])
def test_td3_her_train_teacher_forced(golden, fused_path, monkeypatch):
    from _parity_helpers import check_init, check_weights, q_err, rel_err
    from core.common import legacy_rng

    use_fused, lab = set_path(monkeypatch, fused_path)
    g = golden("td3_her_train_kat_small.npz")
    gamma, tau, tpn, tnc, delay, lr, B, n_steps = g["hyper"]
    B, n_steps = int(B), int(n_steps)
    model, _ = her_model("TD3", batch_size=B, buffer_size=64 * 4, policy_kwargs=dict(net_arch=[48, 32]))
    assert model.fused_learner
    model.fused_learner = use_fused
    assert (model.gamma, model.tau, model.target_policy_noise, model.target_noise_clip, model.policy_delay, model.lr_schedule(1)) == (gamma, tau, tpn, tnc, int(delay), lr)
    mods = ["actor", "actor_target", "critic", "critic_target"]
    check_init(model, g, mods)
    replay_fixture_adds(model, g)
    legacy_rng.seed(int(g["np_seed"]), model.device)
    model.debug_capture = True
    for k in range(n_steps):
        model.noise_queue = [th.as_tensor(g[f"step{k}/noise_raw"])]
        model.train(gradient_steps=1, batch_size=B)
        for name in ("observations", "actions", "next_observations", "dones", "rewards"):
            np.testing.assert_array_equal(getattr(model._static_batch, name).cpu().numpy(), g[f"step{k}/batch_{name}"], err_msg=f"step {k} {name}")
        t = model.last_train_tensors
        assert q_err(t["target_q"].cpu().numpy(), g[f"step{k}/target_q"], lab) < 1e-5
        assert q_err(t["current_q"][0].cpu().numpy(), g[f"step{k}/current_q1"], lab) < 1e-5
        assert q_err(t["current_q"][1].cpu().numpy(), g[f"step{k}/current_q2"], lab) < 1e-5
        lv = model.logger.name_to_value
        assert rel_err(float(lv["train/critic_loss"]), float(g[f"step{k}/critic_loss"]), 1e-3) < 1e-5
        if f"step{k}/actor_loss" in g:
            assert rel_err(float(lv["train/actor_loss"]), float(g[f"step{k}/actor_loss"]), 1e-3) < 1e-5
    check_weights(model, g, "after", mods)
    assert model.critic.optimizer.step_count == n_steps and model.actor.optimizer.step_count == n_steps // int(delay)


def test_device_rollout_equals_the_host_add_path(ops):
    """A warm-up rollout on the device (uniform actions from the action space's generator, cstr_goal_vec_step_f32, cstr_her_add_f32, no
    host synchronisation) leaves the buffer equal to HerReplayBuffer.add() fed the transitions of a twin env stepped through the
    host face: episodes of 7 steps, targets redrawn per episode, a 16-row ring through a wrap; episode statistics as Monitor's."""
    from core import _native as nv
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    n, steps = 5, 30
    model, env = her_model("SAC", n_envs=n, max_steps=7, goal_range=(0.10, 0.40), buffer_size=16 * n, learning_starts=10 ** 6,
                           policy_kwargs=dict(net_arch=[16, 16]))
    model.learn(n * steps)
    rb = model.replay_buffer
    assert model.num_timesteps == n * steps and rb._adds == steps and model._n_updates == 0
    twin = CSTRVecEnv(n, device=DEV, goal_conditioned=True, goal_range=(0.10, 0.40))
    twin.coef = nv.default_coef(0.20, 0.05, 0.45, 7)
    host = HerReplayBuffer(16 * n, twin.observation_space, twin.action_space, twin, device=DEV, n_envs=n)
    twin.seed(0)
    obs = twin.reset()
    ret, returns, lengths = np.zeros(n), [], []
    first = steps - 16
    # the 16-row ring holds the last 16 vec-steps only: the whole action stream comes from an equally seeded model with a 64-row ring
    model2, _ = her_model("SAC", n_envs=n, max_steps=7, goal_range=(0.10, 0.40), buffer_size=64 * n, learning_starts=10 ** 6,
                          policy_kwargs=dict(net_arch=[16, 16]))
    model2.learn(n * steps)
    acts = model2.replay_buffer.actions.cpu().numpy()[:steps]
    assert np.array_equal(acts[first:], np.roll(rb.actions.cpu().numpy(), -rb.pos, axis=0))
    for t in range(steps):
        lo, hi = np.float32(-1), np.float32(1)
        nobs, r, d, infos = twin.step(lo + (np.float32(0.5) * (acts[t] + np.float32(1)) * (hi - lo)))  # unscale_action of the buffer action (:406)
        nxt = {k: v.copy() for k, v in nobs.items()}
        for i in np.nonzero(d)[0]:
            for k in nxt:
                nxt[k][i] = infos[i]["terminal_observation"][k]
        host.add(obs, nxt, acts[t], r, d, infos)
        ret += r
        for i in np.nonzero(d)[0]:
            returns.append(ret[i]), lengths.append(7)
            ret[i] = 0.0
        obs = nobs
    for k in ("ep_start", "ep_length", "_current_ep_start"):
        assert np.array_equal(getattr(rb, k), getattr(host, k)), k
    for x, y in ((rb.ring.observations, host.ring.observations), (rb.ring.next_observations, host.ring.next_observations),
                 (rb.her.desired_goal, host.her.desired_goal), (rb.actions, host.actions), (rb.rewards, host.rewards), (rb.dones, host.dones),
                 (rb.timeouts, host.timeouts), (rb.ring.ctl, host.ring.ctl), (rb.her.row_valid, host.her.row_valid), (rb.her.valid_bits, host.her.valid_bits)):
        assert th.equal(x, y)
    assert th.equal(env.flat, twin.flat) and th.equal(env.targets, twin.targets)
    n_ep, ret_sum, len_sum, _ = model._ep_stats.cpu().tolist()
    assert model._episode_num == n_ep == len(returns) == n * (steps // 7) and len_sum == sum(lengths)
    assert abs(ret_sum - float(np.sum(returns))) < 1e-4 * abs(ret_sum)


def test_predict_evaluate_save_load_and_replay_buffer_pickles(ops, tmp_path):
    import core
    from core.common.evaluation import evaluate_policy
    from core.common.noise import NormalActionNoise
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    n = 4
    model, env = her_model("TD3", n_envs=n, max_steps=6, buffer_size=16 * n, learning_starts=8 * n, batch_size=16,
                           policy_kwargs=dict(net_arch=[16, 16]), replay_buffer_kwargs=dict(n_sampled_goal=2, goal_selection_strategy="episode"),
                           action_noise=NormalActionNoise(np.zeros(2), 0.1 * np.ones(2)))
    model.learn(n * 14)  # 8 warm-up vec-steps, then 6 iterations with a gradient step and exploration noise from the legacy stream
    assert model._n_updates == 6 and type(model.action_noise).__name__ == "LegacyStreamNormalActionNoise"
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters()) and model._episode_num == n * 2
    ev = CSTRVecEnv(n, device=DEV, goal_conditioned=True)  # predictions and evaluation leave the training env alone
    ev.coef = env.coef
    obs = ev.reset()
    a_dict, _ = model.predict(obs, deterministic=True)
    a_flat, _ = model.predict(ev.flat.cpu().numpy(), deterministic=True)
    assert a_dict.shape == (n, 2) and np.array_equal(a_dict, a_flat) and np.abs(a_dict).max() <= 1.0
    assert model.predict({k: v[0] for k, v in obs.items()}, deterministic=True)[0].shape == (2,)
    ev.seed(3)
    mean, std = evaluate_policy(model, ev, n_eval_episodes=2 * n, warn=False)
    ev.seed(3)
    rets, lens = evaluate_policy(model, ev, n_eval_episodes=2 * n, return_episode_rewards=True, warn=False)
    assert np.isfinite(mean) and mean < 0.0 and lens == [6] * (2 * n) and abs(np.mean(rets) - mean) < 1e-4 * abs(mean)
    # the model: the Dict space and HER's arguments in the zip; load on the goal face, refused on the Box face
    path = str(tmp_path / "td3_her")
    model.save(path)
    env2 = CSTRVecEnv(n, device=DEV, goal_conditioned=True)
    loaded = core.TD3.load(path, env=env2, device=DEV)
    assert isinstance(loaded.replay_buffer, HerReplayBuffer) and loaded.replay_buffer.n_sampled_goal == 2
    assert loaded.replay_buffer.strategy_key == "episode" and loaded.goal_space == env2.observation_space
    for (k, v), (k2, v2) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert k == k2 and th.equal(v, v2), k
    assert np.array_equal(loaded.predict(obs, deterministic=True)[0], a_dict)
    with pytest.raises(ValueError, match="goal face"):
        core.TD3.load(path, env=CSTRVecEnv(n, device=DEV), device=DEV)
    with pytest.raises(ValueError, match="Observation spaces do not match"):
        loaded.set_env(CSTRVecEnv(n, device=DEV))
    # the replay buffer: without truncation the state stays; with it, the reference's warning and bookkeeping (her_replay_buffer.py:386-408)
    model.learn(n * 3, reset_num_timesteps=False)  # leave an episode unfinished
    rb = model.replay_buffer
    assert (rb._current_ep_start != rb.pos).any()
    pkl = str(tmp_path / "rb.pkl")
    model.save_replay_buffer(pkl)
    loaded.load_replay_buffer(pkl, truncate_last_traj=False)
    kept = loaded.replay_buffer
    assert kept.env is env2 and np.array_equal(kept.ep_length, rb.ep_length) and th.equal(kept.dones, rb.dones) and kept.pos == rb.pos
    want = pickle.loads(pickle.dumps(rb))
    with pytest.warns(UserWarning, match="The last trajectory in the replay buffer will be truncated"):
        want.truncate_last_trajectory()
    with pytest.warns(UserWarning, match="The last trajectory in the replay buffer will be truncated"):
        loaded.load_replay_buffer(pkl, truncate_last_traj=True)
    cut = loaded.replay_buffer
    assert np.array_equal(cut.ep_length, want.ep_length) and th.equal(cut.dones, want.dones) and th.equal(cut.timeouts, want.timeouts)
    assert (cut._current_ep_start == cut.pos).all() and int((cut.ep_length > 0).sum()) > int((rb.ep_length > 0).sum())
    cut.sample(8)
    with pytest.raises(ValueError, match="HerReplayBuffer belongs to a model of the goal face"):
        core.TD3("MlpPolicy", CSTRVecEnv(n, device=DEV), device=DEV).load_replay_buffer(pkl)


def test_training_refuses_to_start_before_the_first_episode_ends(ops):
    model, _ = her_model("SAC", n_envs=2, buffer_size=64, learning_starts=4, batch_size=8, policy_kwargs=dict(net_arch=[16, 16]))
    with pytest.raises(RuntimeError, match="Unable to sample before the end of the first episode"):
        model.learn(2 * 8)  # 400-step episodes: nothing can be relabelled yet (her_replay_buffer.py:197-201), checked once


def test_sac_her_learns_setpoint_tracking(ops):
    """SAC + HER (future, 4 goals) on goal_range=(0.10, 0.40), sized like the other learning runs: the mean evaluation reward over a
    fixed set of targets ends above the untrained policy's. The run is eager (graph replay is not built for the goal face), so its
    length is its iteration count: about 6 s for 4000 iterations on an MI355X, whatever the number of envs, hence 64 of them. At the
    class defaults the evaluation reward starts to move after about 3000 updates (unchanged at 2560, up by about 25 at 3560)."""
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv

    n = 64
    model, env = her_model("SAC", n_envs=n, goal_range=(0.10, 0.40), buffer_size=n * 1024, learning_starts=n * 410)  # 400-step episodes
    ev = CSTRVecEnv(16, device=DEV, goal_conditioned=True)
    ev.coef = env.coef
    targets = np.linspace(0.10, 0.40, 16).astype(np.float32)

    def evaluate():  # evaluate_policy resets the env: targets are set after its reset through a reset hook of the test
        orig = ev.reset_device

        def reset_then_targets():
            out = orig()
            ev.set_targets(targets)
            return out

        ev.reset_device = reset_then_targets
        try:
            ev.seed(123)
            return evaluate_policy(model, ev, n_eval_episodes=16, warn=False)[0]
        finally:
            ev.reset_device = orig

    before = evaluate()
    model.learn(n * 4000)
    after = evaluate()
    print(f"SAC + HER mean evaluation reward over 16 fixed targets: untrained {before:.2f}, trained {after:.2f}")
    assert model._n_updates == 4000 - 410 and after > before, (before, after)
