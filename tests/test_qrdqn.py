"""GPU checks of QR-DQN on the HIP path (core/qrdqn, csrc/cstr_qrdqn.hip); the two entry points alone: tests/test_qrdqn_abi.py.

The folded head: the [n, M] values the rollout and `predict` select on against the fp64 mean of the atoms, with a bar measured in the
test on the CPU (4 x the error of torch's own float32 `quantile_net(obs).mean(1)`, the factor for the different summation order), and
the greedy indices on every row whose fp64 top-two gap exceeds 100 x that error (at most 2 % of the rows may fall below it).
Teacher-forced training against RefQRDQN (tests/_qrdqn_reference.py, float64): three gradient steps that straddle a target update, on
the kernel path, on it with CSTR_FUSED_LINEAR=0 (rocBLAS GEMMs) and on the torch statements; atoms and targets within 1e-5 of their
scale, weights at tests/test_tqc.py's weight bar (2e-5 of the tensor's scale + 1e-4 relative). Each run prints its worst error-to-bar
ratios before it asserts. Then hipGraph replay against eager launches bit for bit, the optional gradient clip, path selection and
logger keys, save / load, predict, and DQN's wiring check on a synthetic one-step problem.

A recorded run of this file and of tests/test_qrdqn_abi.py on the MI355X (`-s`: every printed figure): profiles/qrdqn_gpu_tests.txt."""
import os

import numpy as np
import pytest
import torch as th

import _qrdqn_reference as ref
from _parity_helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def quiet(model):
    from core.common.logger import Logger

    model.set_logger(Logger(folder=None, output_formats=[]))
    return model


def make_model(K, n_envs=4, **kw):
    from core.common.vec_env import CSTRVecEnv
    from core.qrdqn import QRDQN

    return quiet(QRDQN("MlpPolicy", CSTRVecEnv(n_envs, discrete_actions=K, device=DEV), device=DEV, **kw))


def cpu_policy(model, K):
    """the model's policy rebuilt on the CPU with the model's weights"""
    p = ref.make_policy(K, arch=model.policy.net_arch, n_quantiles=model.n_quantiles)
    p.load_state_dict({k: v.detach().cpu() for k, v in model.policy.state_dict().items()})
    return p


# ---- the folded head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Nq", [(3, 8), (5, 200), (16, 25), (16, 200)])
def test_folded_greedy_selection_against_the_fp64_mean_of_the_atoms(K, Nq):
    M, n = K * K, 1030
    model = make_model(K, seed=0, policy_kwargs=dict(n_quantiles=Nq))
    assert model.policy.net_arch == [64, 64]
    net32 = cpu_policy(model, K).quantile_net.quantile_net
    obs = np.random.default_rng(0).uniform(-1, 1, (n, 4)).astype(np.float32)
    with th.no_grad():
        q32 = net32(th.as_tensor(obs)).view(n, Nq, M).mean(dim=1).numpy().astype(np.float64)
        q64 = net32.double()(th.as_tensor(obs, dtype=th.float64)).view(n, Nq, M).mean(dim=1).numpy()
    err32 = float(np.abs(q32 - q64).max())  # what torch's own float32 statement shows on these inputs
    got = model._q_values(dev(obs))
    assert tuple(got.shape) == (n, M) and got.dtype == th.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - q64).max())
    top2 = np.sort(q64, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 100 * err32
    index = model.policy.predict(obs, deterministic=True)[0]
    wrong = int((index[decided] != q64.argmax(axis=1)[decided]).sum())
    print(f"FOLD K{K} Nq{Nq}: |folded - fp64| {err:.3e}, torch float32 on the CPU {err32:.3e} (bar {4 * err32:.3e}); rows below the gap "
          f"{int((~decided).sum())} of {n}; wrong indices among the others {wrong}")
    assert err <= 4 * err32
    assert (~decided).mean() <= 0.02
    assert wrong == 0 and index.dtype == np.int64 and index.shape == (n,)
    # the same selection through the atoms themselves
    assert np.array_equal(index[decided], model.quantile_net._predict(dev(obs)).cpu().numpy()[decided])


# ---- teacher-forced training -----------------------------------------------------------------------------------------------------------
def batches(K, B, n_steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_steps):
        obs = rng.uniform(-1, 1, (B, 4)).astype(np.float32)
        nobs = np.clip(obs + rng.normal(0, 0.05, obs.shape), -1, 1).astype(np.float32)
        out.append((obs, rng.integers(0, K * K, B), nobs, rng.uniform(-8, 0, B).astype(np.float32), (rng.uniform(size=B) < 0.2).astype(np.float32)))
    return out


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("tag", ["small", "default"])
def test_teacher_forced_train_matches_the_fp64_statement(tag, path, monkeypatch):
    """three steps on a seeded model, the target network updated after the second"""
    from core.common import fused

    K, Nq, arch, B = (3, 8, [32, 32], 16) if tag == "small" else (5, 200, [64, 64], 32)
    kw = dict(policy_kwargs=dict(n_quantiles=Nq, net_arch=arch), batch_size=B) if tag == "small" else {}
    model = make_model(K, seed=0, buffer_size=256, **kw)
    assert (model.n_quantiles, model.batch_size, model.gamma, model.tau, model.lr_schedule(1), model.max_grad_norm) == (Nq, B, 0.99, 1.0, 5e-5, None)
    assert model.policy.net_arch == arch and model.fused_learner and model.policy.optimizer.defaults["eps"] == 0.01 / B
    if path == "rocblas":  # the kernel path with every GEMM left to PyTorch-ROCm / rocBLAS (CSTR_FUSED_LINEAR=0)
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    if path == "torch":
        model.fused_learner = False
    refm = ref.RefQRDQN(cpu_policy(model, K), 5e-5, model.gamma, 0.01 / B)
    model.debug_capture = True
    lab = f"qrdqn_{tag}_{path}"
    for k, batch in enumerate(batches(K, B, 3, seed=17)):
        model.batch_queue.append(batch)
        model.train(gradient_steps=1, batch_size=B)
        want = refm.step(*batch)
        cap = model.train_capture[-1]
        cur, y = cap["current_q"].cpu().numpy().reshape(B, Nq), cap["target_q"].cpu().numpy().reshape(B, Nq)
        e_c = rel_err(cur, want["cur"], float(np.abs(want["cur"]).mean()))
        e_y = rel_err(y, want["y"], float(np.abs(want["y"]).mean()))
        e_l = rel_err(float(cap["loss"]), want["loss"], 1e-3)
        line = f"{lab} step {k}: error / 1e-5 of scale: atoms {e_c / 1e-5:.3f} targets {e_y / 1e-5:.3f} loss {e_l / 1e-5:.3f}"
        print(line)
        assert e_c < 1e-5 and e_y < 1e-5 and e_l < 1e-5, line
        np.testing.assert_array_equal(cap["next_index"].cpu().numpy(), want["next_index"], err_msg=lab)
        assert float(cap["grad_norm"]) == 0.0  # max_grad_norm is None: nothing computes the norm
        lv = model.logger.name_to_value
        assert abs(float(lv["train/loss"]) - float(cap["loss"])) <= 2 * np.spacing(np.float32(abs(float(cap["loss"]))))
        assert lv["train/n_updates"] == k + 1 == model._n_updates == model.policy.optimizer.step_count
        before = model.policy.target_arena.flat.clone()
        if k == 1:  # the class's own _on_step at the vec-step where _n_calls hits the period
            model._n_calls = model._target_period() - 1
            model._on_step()
            refm.update_target()
            assert th.equal(model.policy.target_arena.flat, model.policy.arena.flat)
        assert th.equal(before, model.policy.target_arena.flat) == (k != 1)
    worst = 0.0
    for nm, net in (("quantile_net", refm.net), ("quantile_net_target", refm.target)):
        wsd = net.state_dict()
        for key, v in getattr(model.policy, nm).state_dict().items():
            got, w = v.detach().cpu().numpy().astype(np.float64), wsd[key].numpy()
            scale = max(float(np.abs(w).max()), 1e-3)
            worst = max(worst, float((np.abs(got - w) / (2e-5 * scale + 1e-4 * np.abs(w))).max()))
    print(f"{lab}: weights of the two networks after 3 steps, worst err / (2e-5 scale + 1e-4 |w|) = {worst:.3f}")
    assert worst < 1.0 and not model.batch_queue


# ---- graph replay ------------------------------------------------------------------------------------------------------------------------
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
                           policy_kwargs=dict(net_arch=[32, 32], n_quantiles=8))
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


# ---- the optional clip, path selection, logger keys --------------------------------------------------------------------------------------
def counted(monkeypatch, name):
    from core.common import hip_ops

    calls, real = [0], getattr(hip_ops, name)

    def wrapped(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(hip_ops, name, wrapped)
    return calls


def test_max_grad_norm_none_runs_no_clip_launch(monkeypatch):
    K, Nq, B = 3, 8, 16
    clips, losses = counted(monkeypatch, "grad_clip"), counted(monkeypatch, "qrdqn_loss")
    kw = dict(seed=0, batch_size=B, buffer_size=256, policy_kwargs=dict(n_quantiles=Nq, net_arch=[32, 32]))
    batch = batches(K, B, 1, seed=3)[0]
    plain, clipped = make_model(K, **kw), make_model(K, max_grad_norm=0.05, **kw)
    want = ref.RefQRDQN(cpu_policy(plain, K), 5e-5, 0.99, 0.01 / B, max_grad_norm=0.05).step(*batch)
    assert want["grad_norm"] > 0.05  # the clip engages
    for model in (plain, clipped):
        model.debug_capture = True
        model.batch_queue.append(batch)
        model.train(gradient_steps=1, batch_size=B)
    assert clips[0] == 1 and losses[0] == 2
    assert float(plain.train_capture[-1]["grad_norm"]) == 0.0
    assert rel_err(float(clipped.train_capture[-1]["grad_norm"]), want["grad_norm"]) < 5e-5
    assert not th.equal(plain.policy.arena.flat, clipped.policy.arena.flat)
    for fused_learner in (True, False):  # the clipped step on both paths against the fp64 statement
        model = make_model(K, max_grad_norm=0.05, **kw)
        model.fused_learner = fused_learner
        refm = ref.RefQRDQN(cpu_policy(model, K), 5e-5, 0.99, 0.01 / B, max_grad_norm=0.05)
        model.batch_queue.append(batch)
        model.train(gradient_steps=1, batch_size=B)
        refm.step(*batch)
        for key, v in model.policy.quantile_net.state_dict().items():
            w = refm.net.state_dict()[key].numpy()
            got = v.detach().cpu().numpy().astype(np.float64)
            assert float((np.abs(got - w) / (2e-5 * max(float(np.abs(w).max()), 1e-3) + 1e-4 * np.abs(w))).max()) < 1.0, (fused_learner, key)


def test_path_selection_and_logger_keys(monkeypatch):
    n = 4
    folds, losses = counted(monkeypatch, "qrdqn_fold_head"), counted(monkeypatch, "qrdqn_loss")
    kw = dict(n_envs=n, seed=1, batch_size=8, buffer_size=64 * n, learning_starts=n, train_freq=2)
    model = make_model(3, policy_kwargs=dict(net_arch=[16, 16], n_quantiles=8), **kw)
    assert model.fused_learner and model.replay_buffer.action_dim == 2 and model.action_space.n == 9
    model.learn(n * 8)
    keys = set(model.logger.name_to_value)
    assert {"train/loss", "train/n_updates", "train/learning_rate", "rollout/exploration_rate"} <= keys
    assert model._n_updates == 4 and model._n_calls == 8 and np.isfinite(float(model.logger.name_to_value["train/loss"]))
    assert losses[0] == 4 and folds[0] == 7  # every vec-step behind the warm-up one folds the head first
    for pk in (dict(net_arch=[16, 16], n_quantiles=8, optimizer_class=th.optim.SGD), dict(net_arch=[16, 16], n_quantiles=300)):
        folds[0] = losses[0] = 0
        other = make_model(3, policy_kwargs=pk, **kw)
        assert not other.fused_learner and isinstance(other.policy.optimizer, th.optim.SGD) == ("optimizer_class" in pk)
        before = other.policy.arena.flat.clone()
        other.learn(n * 8)
        assert other._n_updates == 4 and not th.equal(before, other.policy.arena.flat) and bool(th.isfinite(other.policy.arena.flat).all())
        assert losses[0] == 0 and folds[0] == 7  # the torch statements train, the rollout keeps the folded head
        assert np.isfinite(float(other.logger.name_to_value["train/loss"]))
    with pytest.raises(AssertionError, match="only supports"):
        from core.common.vec_env import CSTRVecEnv
        from core.qrdqn import QRDQN

        QRDQN("MlpPolicy", CSTRVecEnv(2, device=DEV), device=DEV)
    with pytest.raises(ValueError, match="n_quantiles"):
        make_model(3, policy_kwargs=dict(n_quantiles=0))


# ---- save / load, predict ------------------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_continues_identically(tmp_path):
    from core.common.vec_env import CSTRVecEnv
    from core.qrdqn import QRDQN

    n, K = 4, 3
    model = make_model(K, n_envs=n, seed=2, batch_size=32, buffer_size=64 * n, learning_starts=n, train_freq=2, exploration_fraction=0.9,
                       target_update_interval=5 * n, faithful_quirks=False, max_grad_norm=0.5, policy_kwargs=dict(net_arch=[32, 32], n_quantiles=8))
    model.learn(n * 10)
    path = os.path.join(tmp_path, "qrdqn.zip")
    model.save(path)
    env = lambda k=K: CSTRVecEnv(n, discrete_actions=k, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="discrete_actions"):
        QRDQN.load(path, env=env(4), device=DEV)
    with pytest.raises(ValueError, match="n_quantiles"):
        QRDQN.load(path, env=env(), device=DEV, policy_kwargs=dict(net_arch=[32, 32], n_quantiles=16))
    loaded = quiet(QRDQN.load(path, env=env(), device=DEV))
    for k in ("n_quantiles", "exploration_rate", "_n_calls", "_n_updates", "num_timesteps", "target_update_interval", "exploration_fraction",
              "max_grad_norm", "faithful_quirks", "batch_size", "gamma", "tau"):
        assert getattr(loaded, k) == getattr(model, k), k
    assert loaded.exploration_rate > 0 and loaded._n_calls == 10 and loaded.policy.optimizer.defaults["eps"] == 0.01 / 32
    for a, b in ((model.policy.arena.flat, loaded.policy.arena.flat), (model.policy.target_arena.flat, loaded.policy.target_arena.flat),
                 (model.policy.optimizer.exp_avg, loaded.policy.optimizer.exp_avg), (model.policy.optimizer.exp_avg_sq, loaded.policy.optimizer.exp_avg_sq)):
        assert th.equal(a, b)
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count == model._n_updates
    batch = batches(K, 32, 1, seed=9)[0]
    for m in (model, loaded):  # the next gradient step on the same batch
        m.batch_queue.append(batch)
        m.train(gradient_steps=1, batch_size=32)
    assert th.equal(model.policy.arena.flat, loaded.policy.arena.flat) and th.equal(model.policy.optimizer.exp_avg_sq, loaded.policy.optimizer.exp_avg_sq)
    assert np.array_equal(model.predict(batch[0], deterministic=True)[0], loaded.predict(batch[0], deterministic=True)[0])
    # set_parameters changes the last layer under the folded head: the next selection folds the new one
    loaded.set_parameters({"policy": {k: th.zeros_like(v) if k.endswith("4.bias") else v for k, v in loaded.policy.state_dict().items()}}, exact_match=False)
    with th.no_grad():
        want = loaded.quantile_net(dev(batch[0])).mean(dim=1)
    assert float((loaded._q_values(dev(batch[0])) - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1.0)


def test_predict_shapes_and_dtype():
    K = 3
    model = make_model(K, n_envs=1, seed=3, policy_kwargs=dict(net_arch=[32, 32], n_quantiles=8))
    obs = np.random.default_rng(1).uniform(-1, 1, (33, 4)).astype(np.float32)
    with th.no_grad():
        want = model.quantile_net(dev(obs)).mean(dim=1).argmax(dim=1).cpu().numpy()
    act, state = model.predict(obs, deterministic=True)
    assert state is None and act.dtype == np.int64 and act.shape == (33,) and np.array_equal(act, want)
    for m in (1, 5):
        a, _ = model.predict(obs[:m], deterministic=True)
        assert a.shape == (m,) and np.array_equal(a, want[:m])
    one, _ = model.predict(obs[0], deterministic=True)
    assert isinstance(one, np.ndarray) and one.shape == () and one.dtype == np.int64 and int(one) == int(want[0])
    # rand() < exploration_rate: rate 0 never explores (and consumes one draw), rate 1 always does
    stream = model.replay_buffer.sampler_stream
    pos = int(stream[624])
    a, _ = model.predict(obs, deterministic=False)
    assert np.array_equal(a, want) and (int(stream[624]) - pos) % 624 == 2
    model.exploration_rate = 1.0
    a, _ = model.predict(obs, deterministic=False)
    assert a.shape == want.shape and a.dtype == np.int64 and not np.array_equal(a, want) and a.min() >= 0 and a.max() < K * K
    one, _ = model.predict(obs[0], deterministic=False)
    assert one.shape == () and 0 <= int(one) < K * K


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_qrdqn_learns_the_rewarded_index(golden):
    """tests/test_dqn.py's wiring check, which needs no claim about CSTR rewards: the ring is filled with a one-step problem (done = 1,
    reward 1 iff the stored index equals a fixed function of the observation's sign pattern, 9 indices), train() runs 600 gradient
    steps of batch 64 at learning rate 1e-3 with 8 atoms, and the greedy action is compared with the rewarded index on 512 held-out
    observations. tests/golden/qrdqn_wiring_kat.npz (written by tools/qrdqn_wiring_reference.py) holds what the float32 torch statement
    of tests/_qrdqn_reference.py reaches on the same data on the CPU: 0.760 / 0.736 / 0.773 for seeds 0 / 1 / 2, untrained 0.102 / 0.135 /
    0.086. The bar is DQN's construction: the midpoint between that statement's worst seed and the highest untrained value,
    (0.736 + 0.135) / 2 = 0.4355."""
    from core.common.vec_env.cstr_vec_env import decode_valve_index

    g, w = golden("dqn_wiring_kat.npz"), golden("qrdqn_wiring_kat.npz")
    K, B, steps, Nq = int(g["levels"]), int(g["batch_size"]), int(g["gradient_steps"]), int(w["n_quantiles"])
    rows, n = g["index"].shape
    bar = (float(w["reference_accuracy"].min()) + float(w["untrained_accuracy"].max())) / 2
    assert abs(bar - 0.4355) < 1e-3 and (K, B, steps, Nq) == (3, 64, 600, 8)
    assert (int(w["levels"]), int(w["batch_size"]), int(w["gradient_steps"]), float(w["learning_rate"])) == (K, B, steps, float(g["learning_rate"]))
    model = make_model(K, n_envs=n, seed=0, batch_size=B, buffer_size=rows * n, learning_rate=float(g["learning_rate"]), policy_kwargs=dict(n_quantiles=Nq))
    rb = model.replay_buffer
    rb.observations.copy_(dev(g["obs"])), rb.next_observations.copy_(dev(g["obs"])), rb.actions.copy_(dev(decode_valve_index(g["index"], K)))
    rb.rewards.copy_(dev(g["reward"])), rb.dones.fill_(1.0), rb.timeouts.zero_()
    rb._adds = rows
    rb.ring.ctl.copy_(th.tensor([0, 1, 0, rows], dtype=th.int64))
    untrained = float((model.predict(g["held_obs"], deterministic=True)[0] == g["held_best"]).mean())
    model.train(gradient_steps=steps, batch_size=B)
    acc = float((model.predict(g["held_obs"], deterministic=True)[0] == g["held_best"]).mean())
    print(f"WIRING accuracy {acc:.3f} (untrained {untrained:.3f}, bar {bar:.4f}, float32 torch statement {w['reference_accuracy'].tolist()})")
    assert acc > bar and untrained < 0.3
