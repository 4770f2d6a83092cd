"""The n-step sampler on an MI355X: every slot of a small ring against the float64 statement (tests/_nstep_reference.py), the index
stream against the one-step sampler's, and n_steps through the algorithm classes (eager, and replayed from a hipGraph)."""
import copy
import functools

import numpy as np
import pytest
import torch as th

from _nstep_reference import nstep_reference, valid_pairs

pytestmark = pytest.mark.gpu
GAMMA, ROWS, ENVS = 0.9, 8, 3
FIELDS = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


def make_ring(ops, d, a, pos, full, pending):
    """random contents; done at (2, 0), done + timeout at (5, 1), done at (6, 1) right behind it, done at the wrap row (7, 2).
    Rows that the state leaves unwritten hold NaN rewards: a window that runs into them shows."""
    rng = np.random.default_rng(d * 10 + a)
    f = dict(observations=rng.standard_normal((ROWS, ENVS, d)), next_observations=rng.standard_normal((ROWS, ENVS, d)),
             actions=rng.standard_normal((ROWS, ENVS, a)), rewards=rng.standard_normal((ROWS, ENVS)), dones=np.zeros((ROWS, ENVS)),
             timeouts=np.zeros((ROWS, ENVS)))
    for r, e in ((2, 0), (5, 1), (6, 1), (7, 2)):
        f["dones"][r, e] = 1.0
    f["timeouts"][5, 1] = 1.0
    f = {k: v.astype(np.float32) for k, v in f.items()}
    if not full:
        f["rewards"][pos + pending:] = np.nan
    ring = ops.DeviceRing(ROWS, ENVS, d, a, "cuda")
    for k in FIELDS:
        getattr(ring, k).copy_(th.from_numpy(f[k]))
    ring.ctl.copy_(th.tensor([pos, full, 0, pos + ROWS * full]))
    return ring, f


def packed_out(batch, d, a):
    z = lambda *s: th.full(s, 7.0, device="cuda")  # noqa: E731
    return dict(x_data=z(batch, d + a), x_next=z(batch, d + a), x_pi=z(batch, d + a), done=z(batch, 1), rew=z(batch, 1), disc=z(batch, 1),
                fold=z(batch, 1), bi=th.zeros(batch, dtype=th.int64, device="cuda"), ei=th.zeros(batch, dtype=th.int64, device="cuda"))


def gather(ops, ring, idx, n_steps, o, **kw):
    ops.replay_gather_nstep_packed(ring, idx, idx.shape[1], n_steps, GAMMA, o["x_data"], o["x_next"], o["x_pi"], o["done"], o["rew"], o["disc"],
                                   o["fold"], o["bi"], o["ei"], **kw)


@pytest.mark.parametrize("d,a,states", [(4, 2, ((5, 0, 0), (3, 1, 0), (0, 1, 0), (4, 1, 1), (1, 0, 0))), (8, 4, ((3, 1, 0),))])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 5, 16])
def test_every_slot_of_a_small_ring(ops, n_steps, d, a, states):
    for pos, full, pending in states:
        ring, f = make_ring(ops, d, a, pos, full, pending)
        row, env = valid_pairs(ROWS, ENVS, pos, bool(full), bool(pending))
        B = len(row)
        idx = th.from_numpy(np.stack([row, env]).astype(np.int32)).cuda()
        o, rng_ctl = packed_out(B, d, a), th.zeros(16, dtype=th.int64, device="cuda")
        gather(ops, ring, idx, n_steps, o, advance_ring=bool(pending), rng_advance=(rng_ctl, 5))
        ref = nstep_reference(f, row, env, n_steps, GAMMA, pos, bool(full), bool(pending))
        got = {k: v.cpu().numpy() for k, v in o.items()}
        tag = f"n={n_steps} state={(pos, full, pending)} layout={(d, a)}"
        np.testing.assert_array_equal(got["x_data"], np.concatenate([ref["observations"], ref["actions"]], axis=1), err_msg=tag)
        np.testing.assert_array_equal(got["x_next"][:, :d], ref["next_observations"], err_msg=tag)
        np.testing.assert_array_equal(got["x_pi"][:, :d], ref["observations"], err_msg=tag)
        assert (got["x_next"][:, d:] == 7.0).all() and (got["x_pi"][:, d:] == 7.0).all(), tag  # the actor head's columns stay
        np.testing.assert_array_equal(got["done"][:, 0], ref["dones"].astype(np.float32), err_msg=tag)
        np.testing.assert_array_equal(got["bi"], row, err_msg=tag)
        np.testing.assert_array_equal(got["ei"], env, err_msg=tag)
        np.testing.assert_array_equal(got["disc"][:, 0], (GAMMA ** ref["m"]).astype(np.float32), err_msg=tag)
        err_r = np.abs(got["rew"][:, 0].astype(np.float64) - ref["rewards"])
        err_f = np.abs(got["fold"][:, 0].astype(np.float64) - ref["fold"])
        print(f"NSTEP {tag}: B={B} m in [{ref['m'].min()}, {ref['m'].max()}] rewards err {err_r.max():.3g} fold err {err_f.max():.3g}")
        assert (err_r <= n_steps * 2.0 ** -23 * ref["reward_scale"]).all(), tag
        assert (err_f <= 2.0 ** -24).all(), tag
        if n_steps == 1:
            np.testing.assert_array_equal(got["fold"], got["done"], err_msg=tag)
        if not pending:
            assert ring.ctl.tolist() == [pos, full, 0, pos + ROWS * full], tag
            continue
        twin, rng2 = copy.copy(ring), th.zeros(16, dtype=th.int64, device="cuda")  # what cstr_replay_gather_packed_f32 does to the words
        twin.ctl = th.tensor([pos, full, 0, pos + ROWS * full], device="cuda")
        ops.replay_gather_packed(twin, idx, B, o["x_data"], o["x_next"], o["x_pi"], o["done"], o["rew"], advance_ring=True, rng_advance=(rng2, 5))
        assert ring.ctl.tolist() == twin.ctl.tolist() and rng_ctl.tolist() == rng2.tolist(), tag


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("pos,full", [(5, 0), (3, 1)])
def test_index_stream_is_the_one_step_samplers(ops, pos, full, packed):
    from core.common import legacy_rng

    B, d, a = 256, 4, 2
    ring, _ = make_ring(ops, d, a, pos, full, 0)
    e = lambda *s: th.empty(*s, device="cuda")  # noqa: E731

    def draw(n):
        """n = 0: the one-step sampler -> [mt_state, row_idx, env_idx, the three row fields, dones, rewards(, discounts, fold)]"""
        mt, bi, ei = legacy_rng.new_stream(11, "cuda"), th.empty(B, dtype=th.int64, device="cuda"), th.empty(B, dtype=th.int64, device="cuda")
        out = ([e(B, d + a) for _ in range(3)] if packed else [e(B, d), e(B, a), e(B, d)]) + [e(B, 1) for _ in range(4 if n else 2)]
        if n:
            (ops.replay_sample_nstep_packed if packed else ops.replay_sample_nstep)(ring, mt, B, n, GAMMA, *out, bi, ei)
        else:
            (ops.replay_sample_packed if packed else ops.replay_sample)(ring, mt, B, *out, bi, ei)
        # packed rows are (x_data, x_next, x_pi); the action columns of x_next / x_pi belong to the actor head
        return [mt, bi, ei] + ([out[0], out[1][:, :d], out[2][:, :d]] if packed else out[:3]) + out[3:]

    base, one, three = draw(0), draw(1), draw(3)
    assert all(th.equal(x, y) for x, y in zip(one, base)) and th.equal(one[9], one[6])  # n = 1: the one-step bits, fold == dones
    assert all(th.equal(x, y) for x, y in zip(three[:3], base[:3]))  # the same words consumed, the same indices
    o = packed_out(B, d, a)
    gather(ops, ring, th.stack(three[1:3]).int().contiguous(), 3, o)
    rows = [o["x_data"], o["x_next"][:, :d], o["x_pi"][:, :d]] if packed else [o["x_data"][:, :d], o["x_data"][:, d:], o["x_next"][:, :d]]
    assert all(th.equal(x, y) for x, y in zip(three[3:], rows + [o["done"], o["rew"], o["disc"], o["fold"]]))


def make_model(algo, monkeypatch, **kw):
    import core
    from core.common import chain
    from core.common.vec_env import CSTRVecEnv

    N = 8
    monkeypatch.setattr(chain, "USE_CHAIN", algo != "sac_perlayer")
    common = dict(seed=3, batch_size=32, buffer_size=N * 64, learning_starts=N * 20, device="cuda", policy_kwargs=dict(net_arch=[32, 32]))
    if algo == "dqn":
        return core.DQN("MlpPolicy", CSTRVecEnv(N, discrete_actions=3, device="cuda"), train_freq=1, **common, **kw), N
    return (core.TD3 if algo == "td3" else core.SAC)("MlpPolicy", CSTRVecEnv(N, device="cuda"), **common, **kw), N


def weights(model):
    th.cuda.synchronize()
    return th.cat([p.detach().reshape(-1) for p in model.policy.parameters()]).clone()


def mlp64(seq):
    """a float64 copy of a Sequential of Linear / ReLU layers, frozen at its present weights"""
    ws = [(m.weight.detach().double().clone(), m.bias.detach().double().clone()) if isinstance(m, th.nn.Linear) else None for m in seq]
    assert all(w is not None or isinstance(m, th.nn.ReLU) for w, m in zip(ws, seq))
    return lambda x: functools.reduce(lambda h, w: h.clamp_min(0.0) if w is None else h @ w[0].T + w[1], ws, x)


@pytest.mark.parametrize("algo", ["sac", "sac_perlayer", "td3", "dqn"])
def test_first_target_is_the_float64_n_step_statement(ops, algo, monkeypatch):
    """target_q of the first gradient step == rewards + (1 - dones) * discounts * next_q in float64, from the reference sample of the
    indices the step draws and the target networks as they stand before it, to 1e-5 of the batch's Q scale (README, "Parity")."""
    model, N = make_model(algo, monkeypatch, n_steps=3)
    model.learn(N * 20)  # 20 rows, no gradient step yet: windows meet the write head
    rb, B, d = model.replay_buffer, 32, 4
    assert model._n_updates == 0 and rb.n_steps == 3 and rb.gamma == model.gamma
    s, bi, ei = rb.alloc_batch(B), th.empty(B, dtype=th.int64, device="cuda"), th.empty(B, dtype=th.int64, device="cuda")
    ops.replay_sample_nstep(rb.ring, rb.sampler_stream.clone(), B, 3, model.gamma, *s[:3], s.dones, s.rewards, s.discounts, s.fold, bi, ei)
    ref = nstep_reference({k: getattr(rb, k).cpu().numpy() for k in FIELDS}, bi.cpu().numpy(), ei.cpu().numpy(), 3, model.gamma, rb.pos, rb.full, False)
    nets = [mlp64(q) for q in ([model.q_net_target.q_net] if algo == "dqn" else model.critic_target.q_networks)]
    model.debug_capture = True
    model.train(gradient_steps=1, batch_size=B)
    th.cuda.synchronize()
    if algo == "dqn":
        cap = model.train_capture[-1]
        assert th.equal(cap["batch_inds"], bi) and th.equal(cap["env_indices"], ei)
        next_q = nets[0](th.from_numpy(ref["next_observations"]).cuda().double()).max(dim=1).values
    else:
        cap, x_next = model.last_train_tensors, model._packed.x_next
        np.testing.assert_array_equal(x_next[:, :d].cpu().numpy(), ref["next_observations"])  # the step drew these indices
        next_q = th.stack([q(x_next.double())[:, 0] for q in nets]).min(dim=0).values
        if algo != "td3":
            next_q = next_q - cap["ent_coef"].double() * cap["next_log_prob"].double().reshape(-1)
    want = ref["rewards"] + (1.0 - ref["dones"]) * ref["discounts"] * next_q.cpu().numpy()
    err = np.abs(cap["target_q"].reshape(-1).cpu().numpy().astype(np.float64) - want)
    print(f"NSTEP target_q {algo}: m in [{ref['m'].min()}, {ref['m'].max()}] max err {err.max():.3g}, Q scale {np.abs(want).mean():.3g}")
    assert ref["m"].max() == 3 and (err <= 1e-5 * np.maximum(np.abs(want), np.abs(want).mean())).all()
    if algo == "dqn":  # a teacher-forced one-step batch carries no fold
        model.batch_queue.append((None,) * 5)
        with pytest.raises(ValueError, match="batch_queue"):
            model.train(gradient_steps=1, batch_size=B)


@pytest.mark.parametrize("algo", ["sac", "td3", "dqn"])
def test_one_step_is_unchanged(algo, monkeypatch):
    from core.common.buffers import NStepReplayBuffer

    runs = []
    for kw in ({}, dict(n_steps=1), dict(replay_buffer_class=NStepReplayBuffer, replay_buffer_kwargs=dict(n_steps=1))):
        model, N = make_model(algo, monkeypatch, **kw)
        model.learn(N * 25)
        assert model._n_updates == 5
        runs.append(weights(model))
    assert th.equal(runs[0], runs[1]) and th.equal(runs[0], runs[2])


@pytest.mark.parametrize("unroll", [1, 4])
def test_sac_three_steps_from_a_hipgraph_equals_eager(unroll, monkeypatch, tmp_path):
    res = []
    for use_graph in (False, True):
        model, N = make_model("sac", monkeypatch, n_steps=3)
        if use_graph:
            model.enable_graph_capture(True, unroll=unroll)
        model.learn(N * 28)
        if use_graph:
            st = model.graph_status()
            assert st["replays"] > 0 and st["error"] is None, st
        rb = model.replay_buffer
        res.append((weights(model), rb.sampler_stream.clone(), rb.ring.ctl.clone(), rb.rewards.clone()))
    assert model._n_updates == 8
    for i, (x, y) in enumerate(zip(*res)):
        assert th.equal(x, y), f"tensor {i} differs between the eager run and the replayed one"
    model.save(str(tmp_path / "m.zip"))  # a checkpoint carries n_steps
    again = type(model).load(str(tmp_path / "m.zip"), env=model.env, device="cuda")
    assert again.n_steps == 3 and type(again.replay_buffer) is type(model.replay_buffer) and again.replay_buffer.n_steps == 3
