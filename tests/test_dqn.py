"""GPU checks of DQN on the HIP path.

Kernels (csrc/cstr_dqn.hip) against the NumPy / fp64 restatements of tests/_dqn_helpers.py (checked on the CPU against the
reference-written fixtures by tests/test_dqn_abi.py): the legacy-stream draw (bit-exact against RandomState.random_sample, twist
included), the action selection (indices and valve pairs exact), the loss launch (targets, gathered Q values and gradients within
2 ulp of the f32-rounded fp64 value, the loss within 1e-5 * max(|want|, 1)). Then the class: teacher-forced train() against
tests/golden/dqn_train_kat_{small,default}.npz on the kernel path, with CSTR_FUSED_LINEAR=0 and on the torch-statement path, with
the bars of tests/_parity_helpers.py; predict; a seeded learn() against the reference's exploration rates, explore flags, sampled
indices and final MT19937 image; hipGraph replay against eager launches bit for bit; path selection, logger keys, callbacks,
save / load; and a wiring check on a synthetic one-step problem."""
import os

import numpy as np
import pytest
import torch as th

from _dqn_helpers import act_np, dqn_uniforms, loss_f32, loss_f64, pair_np, ulps
from _parity_helpers import check_init, check_weights, q_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = (2, 3, 5, 11, 16)  # M = 4, 9, 25, 121 (no multiple of 16 or 64), 256


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


# ---- cstr_mt19937_rand_flag_f64 -----------------------------------------------------------------------------------------------
def stream_image(key, pos):
    return dev(np.concatenate([np.asarray(key, np.uint32), np.array([pos, 0, 0, 0], np.uint32)]).view(np.int32), th.int32)


@pytest.mark.parametrize("pos", [0, 622, 623, 624])
def test_rand_flag_is_random_sample_bit_for_bit(ops, pos):
    rs = np.random.RandomState(1234)
    rs.random_sample(700)  # past the first twist: a stream in use
    key = rs.get_state()[1].copy()
    rs.set_state(("MT19937", key, pos))
    want = rs.random_sample()
    after = rs.get_state()
    draw, flag = th.zeros(1, dtype=th.float64, device=DEV), th.full((1,), 7, dtype=th.int32, device=DEV)
    for thr, expect in ((np.nextafter(want, 1.0), 1), (want, 0), (np.nextafter(want, 0.0), 0), (1.0, 1), (0.0, 0)):
        mt = stream_image(key, pos)
        ops.mt19937_rand_flag(mt, dev([thr], th.float64), flag, draw)
        assert float(draw) == want and int(flag) == expect, (thr, float(draw), want)  # draw < threshold, compared in f64
        got = mt.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:624], after[1]) and int(got[624]) == int(after[2]) and not got[625:].any()
    mt = stream_image(key, pos)  # two draws in a row stay on the stream
    rs.set_state(("MT19937", key, pos))
    for _ in range(3):
        ops.mt19937_rand_flag(mt, dev([0.5], th.float64), flag, draw)
        assert float(draw) == rs.random_sample()


# ---- cstr_dqn_act_f32 -----------------------------------------------------------------------------------------------------------
def act_case(n, K, seed):
    rng = np.random.default_rng(seed)
    M = K * K
    wide = rng.normal(size=(n, M + 3)).astype(np.float32)  # ldq > M: the kernel must not look at the three columns behind the row
    wide[:, M:] = 100.0
    q = wide[:, :M]
    for r in range(0, n, 3):  # ties: the first maximum wins
        c = np.sort(rng.choice(M, size=min(3, M), replace=False))
        q[r, c] = q[r].max() + 1.0
    return wide, q, rng


def run_act(ops, wide, K, mode, **kw):
    n, M = wide.shape[0], K * K
    valve, index = th.full((n, 2), 9.0, device=DEV), th.full((n,), -1, dtype=th.int64, device=DEV)
    ops.dqn_act(dev(wide)[:, :M], K, mode, valve, index, **kw)
    return valve.cpu().numpy(), index.cpu().numpy()


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1030])
def test_act_against_numpy(ops, n, K):
    wide, q, rng = act_case(n, K, 1000 * K + n)
    M = K * K
    eps = 0.375
    u = rng.uniform(size=(n, 2)).astype(np.float32)
    u[::4, 0] = np.float32(eps)                              # exactly at the rate: not below it, greedy
    u[1::4, 0] = np.nextafter(np.float32(eps), np.float32(0))  # just below: explores
    u[::5, 1] = np.nextafter(np.float32(1), np.float32(0))    # just below 1: the last index, never M
    u[2::7, 1] = 0.0
    valve, index = run_act(ops, wide, K, ops.DQN_GREEDY)
    assert np.array_equal(index, act_np(q, K, 0)) and valve.tobytes() == pair_np(index, K).tobytes()
    for flag in (0, 1):
        valve, index = run_act(ops, wide, K, ops.DQN_ALL_OR_NONE, flag=dev([flag], th.int32), u=dev(u))
        assert np.array_equal(index, act_np(q, K, 1, flag=flag, u=u)) and valve.tobytes() == pair_np(index, K).tobytes()
        assert index.min() >= 0 and index.max() < M
    valve, index = run_act(ops, wide, K, ops.DQN_PER_ROW, eps=dev([eps], th.float64), u=dev(u))
    want = act_np(q, K, 2, eps=eps, u=u)
    assert np.array_equal(index, want) and valve.tobytes() == pair_np(index, K).tobytes()
    assert np.array_equal(want[::4], act_np(q, K, 0)[::4])   # the rows exactly at the rate are the greedy ones


def test_act_draws_its_uniforms_from_philox(ops):
    n, K, seed = 1030, 5, 99
    wide, q, _ = act_case(n, K, 5)
    ctl = ops.new_rng_ctl(seed, DEV)
    eps = 0.5
    for call in range(2):
        u = dqn_uniforms(seed, call * n, n)
        valve, index = run_act(ops, wide, K, ops.DQN_PER_ROW, eps=dev([eps], th.float64), rng_ctl=ctl)
        assert np.array_equal(index, act_np(q, K, 2, eps=eps, u=u)) and valve.tobytes() == pair_np(index, K).tobytes()
        assert int(ctl[1]) == (call + 1) * n and int(ctl[2]) == 0  # the offset advanced by the row count, the ticket reset itself
        assert 0.4 < (u[:, 0] < eps).mean() < 0.6 and abs(u[:, 1].mean() - 0.5) < 0.05
    for call, flag in enumerate((1, 0)):
        _, index = run_act(ops, wide, K, ops.DQN_ALL_OR_NONE, flag=dev([flag], th.int32), rng_ctl=ctl)  # mode 1 draws whatever the flag says
        assert np.array_equal(index, act_np(q, K, 1, flag=flag, u=dqn_uniforms(seed, (2 + call) * n, n)))
    assert int(ctl[1]) == 4 * n
    _, index = run_act(ops, wide, K, ops.DQN_GREEDY)  # greedy neither needs nor moves a stream
    assert int(ctl[1]) == 4 * n
    with pytest.raises(Exception, match="code -1"):
        run_act(ops, wide, K, ops.DQN_PER_ROW, eps=dev([eps], th.float64))  # no source of uniforms


# ---- cstr_dqn_loss_f32 ------------------------------------------------------------------------------------------------------------
def loss_case(B, K, seed):
    """Inputs whose f32 evaluation has no cancellation: taken Q values <= 0, rewards and bootstrap terms >= 0, so that target = r +
    (c * max) and d = cur - target add magnitudes and the 2-ulp bar (two dependent roundings per output) applies. Rows of scale 0.2 land
    below the Huber threshold, rows of scale 3 above it; rows 0 .. 2 (when there) sit on it exactly: d = -1, +1 and -1 with done = 1."""
    rng = np.random.default_rng(seed)
    M = K * K
    s = np.where(rng.uniform(size=(B, 1)) < 0.5, 0.2, 3.0).astype(np.float32)
    q = (-np.abs(rng.normal(size=(B, M))) * s - 0.01).astype(np.float32)
    nq = ((np.abs(rng.normal(size=(B, M))) + 0.1) * s * 0.5).astype(np.float32)
    rew = (rng.uniform(0.1, 1.0, (B, 1)) * s).astype(np.float32).reshape(B)
    done = (rng.uniform(size=B) < 0.3).astype(np.float32)
    index = rng.integers(0, M, B)
    for r, (cur, rw) in enumerate(((-0.25, 0.75), (1.5, 0.5), (-0.5, 0.5))[:B]):
        q[r, index[r]], rew[r], done[r] = cur, rw, 1.0
    return q, nq, index, rew, done


def run_loss(ops, q, nq, index, rew, done, K, gamma=0.99, loss_sum=None, pad=0):
    B, M = q.shape
    qd, nqd = dev(np.pad(q, ((0, 0), (0, pad)))), dev(np.pad(nq, ((0, 0), (0, pad + 1))))
    g = th.full((B, M + pad), 5.0, device=DEV)
    out, cur, tgt = th.zeros(1, device=DEV), th.zeros(B, device=DEV), th.zeros(B, device=DEV)
    ops.dqn_loss(qd[:, :M], nqd[:, :M], dev(pair_np(index, K)), dev(rew), dev(done), gamma, K, g[:, :M], out, ops.new_ppo_workspace(DEV),
                 loss_sum=loss_sum, cur_q_out=cur, target_out=tgt)
    return g.cpu().numpy(), float(out), cur.cpu().numpy(), tgt.cpu().numpy()


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1030])
def test_loss_against_fp64(ops, B, K):
    q, nq, index, rew, done = loss_case(B, K, 77 * K + B)
    M = K * K
    wc, wt, wl, wg = loss_f64(q, nq, index, rew, done, 0.99)
    d = np.abs(wc - wt)
    if B >= 64:
        assert (d < 1).any() and (d > 1).any()
    assert (np.abs(wc - wt)[:min(B, 3)] == 1.0).all()
    acc = th.zeros(1, device=DEV)
    g, loss, cur, tgt = run_loss(ops, q, nq, index, rew, done, K, loss_sum=acc, pad=3)
    u_t, u_c, u_g = ulps(tgt, wt).max(), ulps(cur, wc).max(), ulps(g[:, :M], wg).max()
    print(f"ULP B={B} K={K}: target {u_t:.2f} current {u_c:.2f} gradient {u_g:.2f}; loss {loss:.9g} want {wl:.9g}")
    assert u_t <= 2 and u_c <= 2 and u_g <= 2
    assert (g[:, M:] == 5.0).all()                                    # nothing behind the row is written
    assert np.count_nonzero(g[:, :M]) == B                            # one entry per row ...
    assert np.array_equal(np.nonzero(g[:, :M])[1], index)             # ... at the taken index
    assert abs(loss - wl) <= 1e-5 * max(abs(wl), 1.0)
    g2, loss2, cur2, tgt2 = run_loss(ops, q, nq, index, rew, done, K, loss_sum=acc, pad=3)
    assert g.tobytes() == g2.tobytes() and loss == loss2 and cur.tobytes() == cur2.tobytes() and tgt.tobytes() == tgt2.tobytes()
    assert float(acc) == np.float32(loss) + np.float32(loss)          # loss_sum accumulates


@pytest.mark.parametrize("B,K", [(65, 3), (257, 5), (1030, 16)])
def test_loss_of_mixed_sign_inputs_is_the_f32_statement_bit_for_bit(ops, B, K):
    """Q values, rewards and bootstrap terms of both signs: target and d cancel, where an ulp bar against fp64 says nothing about f32
    arithmetic. The header fixes the operation order, so the float32 NumPy statement of it is what the kernel must give exactly."""
    rng = np.random.default_rng(B + K)
    M = K * K
    q, nq = (rng.normal(size=(B, M)) * 2).astype(np.float32), (rng.normal(size=(B, M)) * 2 - 2.5).astype(np.float32)
    rew, done = rng.uniform(-3, 3, B).astype(np.float32), (rng.uniform(size=B) < 0.3).astype(np.float32)
    index = rng.integers(0, M, B)
    wc, wt, wg = loss_f32(q, nq, index, rew, done, 0.99)
    assert (wt > 0).any() and (wt < 0).any() and (np.abs(wc - wt) < 1).any() and (np.abs(wc - wt) > 1).any()
    g, loss, cur, tgt = run_loss(ops, q, nq, index, rew, done, K, pad=3)
    assert tgt.tobytes() == wt.tobytes() and cur.tobytes() == wc.tobytes() and g[:, :M].tobytes() == wg.tobytes()
    wl = loss_f64(q, nq, index, rew, done, 0.99)[2]
    assert abs(loss - wl) <= 1e-5 * max(abs(wl), 1.0)


def test_loss_propagates_a_nan_of_the_next_q_values(ops):
    K, B = 3, 65
    q, nq, index, rew, done = loss_case(B, K, 3)
    nq[7, 4], done[7] = np.nan, 0.0
    nq[9, 0], done[9] = np.nan, 1.0   # (1 - done) * gamma = 0, and 0 * NaN is still NaN
    g, loss, cur, tgt = run_loss(ops, q, nq, index, rew, done, K)
    wc, wt, wl, wg = loss_f64(q, nq, index, rew, done, 0.99)
    assert np.isnan(tgt[[7, 9]]).all() and np.isnan(wt[[7, 9]]).all() and np.isnan(loss) and np.isnan(wl)
    assert np.isnan(g[[7, 9], index[[7, 9]]]).all() and np.isnan(g).sum() == 2
    ok = np.ones(B, bool)
    ok[[7, 9]] = False
    assert ulps(tgt[ok], wt[ok]).max() <= 2 and ulps(g[ok], wg[ok]).max() <= 2 and np.array_equal(cur, wc.astype(np.float32))


# ---- the class --------------------------------------------------------------------------------------------------------------------
def quiet(model):
    from core.common.logger import Logger

    model.set_logger(Logger(folder=None, output_formats=[]))
    return model


def make_model(K, n_envs=4, **kw):
    from core.common.vec_env import CSTRVecEnv
    from core.dqn import DQN

    return quiet(DQN("MlpPolicy", CSTRVecEnv(n_envs, discrete_actions=K, device=DEV), device=DEV, **kw))


def fixture_batch(g, k):
    return tuple(g[f"step{k}/batch_{f}"] for f in ("observations", "index", "next_observations", "rewards", "dones"))


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("name", ["dqn_train_kat_small.npz", "dqn_train_kat_default.npz"])
def test_teacher_forced_train_matches_the_reference(golden, monkeypatch, name, path):
    from core.common import fused

    g = golden(name)
    gamma, tau, max_norm, lr, B, n_steps, K, upd = (float(x) for x in g["hyper"])
    B, n_steps, K, upd = int(B), int(n_steps), int(K), int(upd)
    if path == "rocblas":  # the kernel path with every GEMM left to PyTorch-ROCm / rocBLAS (CSTR_FUSED_LINEAR=0)
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    kw = dict(policy_kwargs=dict(net_arch=[64, 64]), target_update_interval=1000) if "small" in name else {}
    model = make_model(K, seed=0, batch_size=B, buffer_size=256, max_grad_norm=max_norm, **kw)
    assert (model.gamma, model.tau, model.lr_schedule(1)) == (gamma, tau, lr)
    if path == "torch":
        model.fused_learner = False
    assert model.fused_learner == (path != "torch")
    check_init(model, g, ("q_net", "q_net_target"))
    model.debug_capture = True
    label = dict(fused="dqn", rocblas="dqn_rocblas", torch="dqn_aten")[path]
    clipped = False
    for k in range(n_steps):
        model.batch_queue.append(fixture_batch(g, k))
        model.train(gradient_steps=1, batch_size=B)
        cap = model.train_capture[-1]
        wc, wt = g[f"step{k}/current_q"].reshape(-1), g[f"step{k}/target_q"].reshape(-1)
        e_c, e_t = q_err(cap["current_q"].cpu().numpy(), wc, label), q_err(cap["target_q"].cpu().numpy(), wt, label)
        scale = float(np.abs(wt).mean())
        e_l = abs(float(cap["loss"]) - float(g[f"step{k}/loss"])) / scale
        e_n = rel_err(float(cap["grad_norm"]), float(g[f"step{k}/grad_norm"]))
        print(f"PARITY {name} {path} step {k}: current_q {e_c:.3g} target_q {e_t:.3g} loss {e_l:.3g} grad_norm {e_n:.3g}")
        assert e_c <= 1e-5 and e_t <= 1e-5 and e_l <= 1e-5 and e_n < 5e-5
        clipped |= float(g[f"step{k}/grad_norm"]) > max_norm
        assert abs(float(model.logger.name_to_value["train/loss"]) - float(g[f"step{k}/loss"])) <= 1e-5 * scale
        assert model.logger.name_to_value["train/n_updates"] == k + 1 == model._n_updates
        assert model.logger.name_to_value["train/learning_rate"] == float(g[f"step{k}/learning_rate"])
        assert model.policy.optimizer.step_count == int(g[f"step{k}/optimizer_step"]) == k + 1
        before = model.policy.target_arena.flat.clone()
        if k == upd:  # the class's own _on_step at the vec-step where _n_calls hits the period
            model._n_calls = model._target_period() - 1
            model._on_step()
        assert th.equal(before, model.policy.target_arena.flat) == (k != upd)  # the target net changes exactly at the update
        if k == upd:
            assert th.equal(model.policy.target_arena.flat, model.policy.arena.flat)
        check_weights(model, g, f"after/step{k}", ("q_net", "q_net_target"))
    assert clipped == bool(g["clip_engaged"]) and not model.batch_queue


def test_predict_matches_the_reference(golden):
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv

    g = golden("dqn_predict_kat.npz")
    K = int(g["levels"])
    model = make_model(K, n_envs=1, seed=3, policy_kwargs=dict(net_arch=[64, 64]))
    check_init(model, g, ("q_net",))
    obs, want = g["obs"], g["actions"]
    act, state = model.predict(obs, deterministic=True)
    assert state is None and act.dtype == np.int64 and act.shape == (len(obs),) and np.array_equal(act, want)  # no row left out
    for n in (1, 5):
        a, _ = model.predict(obs[:n], deterministic=True)
        assert a.shape == (n,) and np.array_equal(a, want[:n])
    one, _ = model.predict(obs[0], deterministic=True)
    assert isinstance(one, np.ndarray) and one.shape == () and one.dtype == np.int64 and int(one) == int(want[0])
    # the reference's rand() < exploration_rate: rate 0 never explores (and consumes one draw), rate 1 always does
    stream = model.replay_buffer.sampler_stream
    pos = int(stream[624])
    a, _ = model.predict(obs, deterministic=False)
    assert np.array_equal(a, want) and (int(stream[624]) - pos) % 624 == 2
    model.exploration_rate = 1.0
    a, _ = model.predict(obs, deterministic=False)
    assert a.shape == want.shape and a.dtype == np.int64 and not np.array_equal(a, want) and a.min() >= 0 and a.max() < K * K
    one, _ = model.predict(obs[0], deterministic=False)
    assert one.shape == () and 0 <= int(one) < K * K
    model.exploration_rate = 0.0
    mean, std = evaluate_policy(model, CSTRVecEnv(2, discrete_actions=K, device=DEV), n_eval_episodes=2, warn=False)
    assert np.isfinite(mean) and np.isfinite(std)


def test_seeded_learn_mirrors_the_reference_streams(golden):
    """exploration rate per step, explore flags, sampled indices and the final MT19937 image of a short seeded learn(): they depend on
    the streams and the ring position only, not on the (unpinned) warm-up / random action values"""
    from core.common.callbacks import BaseCallback

    g = golden("dqn_explore_kat.npz")
    n, K, B, ls = int(g["n_envs"]), int(g["levels"]), int(g["batch_size"]), int(g["learning_starts"])
    model = make_model(K, n_envs=n, seed=int(g["seed"]), batch_size=B, buffer_size=64 * n, learning_starts=ls, train_freq=int(g["train_freq"]),
                       target_update_interval=int(g["target_update_interval"]), exploration_fraction=float(g["exploration_fraction"]),
                       policy_kwargs=dict(net_arch=[64, 64]))
    model.debug_capture = True
    rates, flags = [], []

    class Rec(BaseCallback):
        def _on_step(self) -> bool:
            if self.model.num_timesteps - n >= ls:  # a post-warm-up step: the rate still is the one it ran with
                rates.append(float(self.model.exploration_rate))
                flags.append(int(self.model._flag))
            return True

    model.learn(int(g["total_timesteps"]), callback=Rec())
    assert rates == g["exploration_rate"].tolist() and np.array_equal(np.array(flags, np.uint8), g["explored"])
    assert model.exploration_rate == float(g["final_exploration_rate"])
    assert (model._n_updates, model._n_calls, model.num_timesteps) == (int(g["n_updates"]), int(g["n_calls"]), int(g["num_timesteps"]))
    bi = np.stack([c["batch_inds"].cpu().numpy() for c in model.train_capture])
    ei = np.stack([c["env_indices"].cpu().numpy() for c in model.train_capture])
    assert np.array_equal(bi, g["batch_inds"]) and np.array_equal(ei, g["env_indices"])
    img = model.replay_buffer.sampler_stream.cpu().numpy().view(np.uint32)
    assert np.array_equal(img[:624], g["mt_key_final"]) and int(img[624]) == int(g["mt_pos_final"])


def snapshot(model):
    pol, rb, env = model.policy, model.replay_buffer, model._denv
    opt = pol.optimizer
    t = dict(q=pol.arena.flat, target=pol.target_arena.flat, m=opt.exp_avg, v=opt.exp_avg_sq, adam=opt.ctl, obs=rb.observations,
             next_obs=rb.next_observations, act=rb.actions, rew=rb.rewards, done=rb.dones, timeout=rb.timeouts, ring=rb.ring.ctl,
             env_obs=env.obs, env_steps=env.step_count, pcg=env.pcg_state, mt=rb.sampler_stream, philox=model._rng_ctl)
    out = {k: v.detach().cpu().numpy().copy() for k, v in t.items()}
    lv = model.logger.name_to_value
    out["logged"] = np.array([float(lv["rollout/exploration_rate"]), float(lv["train/loss"]), float(lv["train/n_updates"]), model.exploration_rate,
                              model._n_calls, model._n_updates, model.num_timesteps])
    return out


@pytest.mark.parametrize("tf,period,faithful,unroll", [(4, 2, True, 1), (1, 3, False, 4), (4, 3, False, 1), (4, 2, True, 4)])
def test_graph_replay_is_eager_bit_for_bit(tf, period, faithful, unroll):
    """`period`: bodies between two target updates"""
    n, iters = 8, 40

    def run(graph):
        model = make_model(3, n_envs=n, seed=5, batch_size=16, buffer_size=64 * n, learning_starts=2 * n, train_freq=tf,
                           target_update_interval=period * tf * n, exploration_fraction=0.5, faithful_quirks=faithful,
                           policy_kwargs=dict(net_arch=[32, 32]))
        if graph:
            model.enable_graph_capture(True, unroll=unroll)
        model.learn(n * tf * iters)
        th.cuda.synchronize()
        return model, snapshot(model)

    eager, a = run(False)
    model, b = run(True)
    st = model.graph_status()
    print("GRAPH", tf, period, faithful, unroll, {k: st[k] for k in ("graphs", "replays", "eager_iterations", "abi_launches_per_iteration")})
    assert st["active"] and st["error"] is None and st["replays"] > 0 and eager.graph_status()["replays"] == 0
    assert a["logged"][4] == iters * tf and a["logged"][2] > 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert {"rollout/exploration_rate", "train/loss"} <= set(model.logger.name_to_value)


def test_path_selection_logger_keys_and_callbacks(monkeypatch):
    from core.common.callbacks import BaseCallback

    n = 4
    kw = dict(n_envs=n, seed=1, batch_size=8, buffer_size=64 * n, learning_starts=n, train_freq=2, policy_kwargs=dict(net_arch=[16, 16]))
    model = make_model(3, **kw)
    assert model.fused_learner and model.replay_buffer.action_dim == 2 and model.action_space.n == 9
    model.learn(n * 8)
    keys = set(model.logger.name_to_value)
    assert {"train/loss", "train/n_updates", "train/learning_rate", "rollout/exploration_rate"} <= keys
    assert model._n_updates == 4 and model._n_calls == 8 and np.isfinite(float(model.logger.name_to_value["train/loss"]))
    sample = model.replay_buffer.sample(16)
    assert sample.actions.shape == (16, 2)  # the ring holds valve pairs ...
    levels = np.unique(np.round((sample.actions.cpu().numpy() + 1) * (3 - 1) / 2, 6))
    assert set(levels) <= {0.0, 1.0, 2.0}   # ... of the face's levels
    kw2 = dict(kw, policy_kwargs=dict(net_arch=[16, 16], optimizer_class=th.optim.SGD))
    sgd = make_model(3, **kw2)
    assert not sgd.fused_learner and isinstance(sgd.policy.optimizer, th.optim.SGD)
    before = sgd.policy.arena.flat.clone()
    sgd.learn(n * 8)
    assert sgd._n_updates == 4 and not th.equal(before, sgd.policy.arena.flat) and bool(th.isfinite(sgd.policy.arena.flat).all())

    class Stop(BaseCallback):
        def _on_step(self) -> bool:
            return self.n_calls < 3

    stopped = make_model(3, **kw)
    stopped.learn(n * 8, callback=Stop())
    assert stopped.num_timesteps == 3 * n
    # the rollout forward of many envs over a small face may take the whole-network launch: same Q values as the torch modules
    wide = make_model(2, n_envs=1100, seed=4)
    obs = th.rand(1100, 4, device=DEV) * 2 - 1
    with th.no_grad():
        want = wide.q_net(obs)
    got = wide._q_values(obs)
    assert got.shape == (1100, 4) and float((got - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1.0)
    wide.learn(1100 * 4 * 2)
    assert wide._n_updates == 2 and bool(th.isfinite(wide.policy.arena.flat).all())
    with pytest.raises(AssertionError, match="only supports"):
        from core.common.vec_env import CSTRVecEnv
        from core.dqn import DQN

        DQN("MlpPolicy", CSTRVecEnv(2, device=DEV), device=DEV)
    with pytest.warns(UserWarning, match="target network"):
        make_model(3, n_envs=4, target_update_interval=2)


def test_save_load_round_trip_continues_identically(golden, tmp_path):
    from core.common.vec_env import CSTRVecEnv
    from core.dqn import DQN

    g = golden("dqn_train_kat_small.npz")
    n = 4
    model = make_model(3, n_envs=n, seed=2, batch_size=32, buffer_size=64 * n, learning_starts=n, train_freq=2, exploration_fraction=0.9,
                       target_update_interval=5 * n, faithful_quirks=False, max_grad_norm=0.5, policy_kwargs=dict(net_arch=[64, 64]))
    model.learn(n * 10)
    path = os.path.join(tmp_path, "dqn.zip")
    model.save(path)
    with pytest.raises(ValueError, match="discrete_actions"):
        DQN.load(path, env=CSTRVecEnv(n, discrete_actions=4, device=DEV), device=DEV)
    loaded = quiet(DQN.load(path, env=CSTRVecEnv(n, discrete_actions=3, device=DEV), device=DEV))
    for k in ("exploration_rate", "_n_calls", "_n_updates", "num_timesteps", "target_update_interval", "exploration_fraction", "max_grad_norm",
              "faithful_quirks", "batch_size", "gamma", "tau"):
        assert getattr(loaded, k) == getattr(model, k), k
    assert loaded.exploration_rate > 0 and loaded._n_calls == 10
    for a, b in ((model.policy.arena.flat, loaded.policy.arena.flat), (model.policy.target_arena.flat, loaded.policy.target_arena.flat),
                 (model.policy.optimizer.exp_avg, loaded.policy.optimizer.exp_avg), (model.policy.optimizer.exp_avg_sq, loaded.policy.optimizer.exp_avg_sq)):
        assert th.equal(a, b)
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count == model._n_updates
    for m in (model, loaded):  # the next gradient step on the same batch
        m.batch_queue.append(fixture_batch(g, 0))
        m.train(gradient_steps=1, batch_size=32)
    assert th.equal(model.policy.arena.flat, loaded.policy.arena.flat) and th.equal(model.policy.optimizer.exp_avg_sq, loaded.policy.optimizer.exp_avg_sq)
    obs = g["step0/batch_observations"]
    assert np.array_equal(model.predict(obs, deterministic=True)[0], loaded.predict(obs, deterministic=True)[0])


def test_saved_replay_buffer_is_a_bcq_dataset(tmp_path):
    """the ring holds valve pairs: a buffer saved by a DQN run loads through BCQ's dataset reader and trains"""
    from core.bcq import BCQ
    from core.common.vec_env import CSTRVecEnv

    n = 4
    dqn = make_model(3, n_envs=n, seed=6, batch_size=8, buffer_size=64 * n, learning_starts=n, train_freq=2, policy_kwargs=dict(net_arch=[16, 16]))
    dqn.learn(n * 40)
    path = os.path.join(tmp_path, "dqn_buffer.pkl")
    dqn.save_replay_buffer(path)
    bcq = quiet(BCQ("MlpPolicy", CSTRVecEnv(1, device=DEV), dataset=path, seed=0, batch_size=32, device=DEV,
                    policy_kwargs=dict(critic_net_arch=[32, 32])))
    rb = bcq.replay_buffer
    assert rb.action_dim == 2 and rb.size() > 0 and float(rb.actions.abs().sum()) == float(dqn.replay_buffer.actions.abs().sum())
    levels = np.unique(rb.actions.cpu().numpy())
    assert set(np.round(levels, 6)) <= {-1.0, 0.0, 1.0}
    bcq.learn(4)
    act, _ = bcq.predict(np.zeros((1, 4), np.float32))
    assert bcq._n_updates == 4 and act.shape == (1, 2) and all(bool(th.isfinite(p).all()) for p in bcq.policy.parameters())


def test_dqn_learns_the_rewarded_index(golden):
    """A wiring check that needs no claim about CSTR rewards: the ring is filled with a one-step problem (done = 1, reward 1 iff the
    stored index equals a fixed function of the observation's sign pattern, 9 indices), train() runs 600 gradient steps of batch 64
    at learning rate 1e-3, and the greedy action is compared with the rewarded index on 512 held-out observations.
    The unmodified reference on the same data (CPU, tools/refharness/gen_golden.py --only dqn): 0.746 / 0.789 / 0.781 for seeds 0 / 1 /
    2, untrained 0.133 / 0.109 / 0.127. The bar is the midpoint between the reference's worst seed and the highest untrained value:
    (0.746 + 0.133) / 2 = 0.4395."""
    from core.common.vec_env.cstr_vec_env import decode_valve_index

    g = golden("dqn_wiring_kat.npz")
    K, B, steps = int(g["levels"]), int(g["batch_size"]), int(g["gradient_steps"])
    rows, n = g["index"].shape
    bar = (float(g["reference_accuracy"].min()) + float(g["untrained_accuracy"].max())) / 2
    assert abs(bar - 0.4395) < 1e-3
    model = make_model(K, n_envs=n, seed=0, batch_size=B, buffer_size=rows * n, learning_rate=float(g["learning_rate"]))
    rb = model.replay_buffer
    rb.observations.copy_(dev(g["obs"])), rb.next_observations.copy_(dev(g["obs"])), rb.actions.copy_(dev(decode_valve_index(g["index"], K)))
    rb.rewards.copy_(dev(g["reward"])), rb.dones.fill_(1.0), rb.timeouts.zero_()
    rb._adds = rows
    rb.ring.ctl.copy_(th.tensor([0, 1, 0, rows], dtype=th.int64))
    untrained = float((model.predict(g["held_obs"], deterministic=True)[0] == g["held_best"]).mean())
    model.train(gradient_steps=steps, batch_size=B)
    acc = float((model.predict(g["held_obs"], deterministic=True)[0] == g["held_best"]).mean())
    print(f"WIRING accuracy {acc:.3f} (untrained {untrained:.3f}, bar {bar:.4f}, reference {g['reference_accuracy'].tolist()})")
    assert acc > bar and untrained < 0.3
