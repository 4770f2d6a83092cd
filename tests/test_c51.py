"""C51 on the MI355X (csrc/cstr_c51.hip, core/c51): the fused atom head and the loss entry point against the NumPy float64 statements of
tests/_c51_reference.py on the same float32 inputs, then the class.

The bar, per output tensor, is tests/test_layernorm.py's: max |kernel - fp64| <= 4 x max |float32 ATen on the CPU - fp64| for the same
statement (core/c51/c51.py's c51_loss_torch for the loss). Each check prints both figures before it asserts; a recorded run (`-s`):
profiles/c51_gpu_tests.txt. Measured worst ratios there: head 2.07 (shape (16, 3, 64, 256)), loss launch 1.00 (B1 N2: both round the
same float64 value), class q_values 0.89, class torch-path logp 1.37."""
import os

import numpy as np
import pytest
import torch as th

import _c51_reference as ref
from _sentinel_bufs import DEV, SENT, Bufs, GuardedBufs

pytestmark = pytest.mark.gpu
V_MIN, V_MAX = -10.0, 10.0


def within(name, kernel, ref64, aten32):
    """the 4 x rule, measured against the reference"""
    got = kernel.detach().cpu().double().numpy() if isinstance(kernel, th.Tensor) else np.asarray(kernel, np.float64)
    ek = float(np.abs(got.reshape(np.shape(ref64)) - ref64).max())
    ea = float(np.abs(aten32.detach().double().numpy().reshape(np.shape(ref64)) - ref64).max())
    print(f"{name}: kernel {ek:.3e} aten {ea:.3e}")
    assert ek <= 4.0 * ea, f"{name}: kernel error {ek:.3e} above 4 x ATen's {ea:.3e}"


# (n, levels, N, H): one row, one MFMA step | a ragged row tile, N one past a column tile | the class shape, M no multiple of the wave
# count | N a whole number of tiles | N one past a four-tile pass, H at the cap | M and N at their caps, H no multiple of 16
HEAD_CASES = [((1, 2, 2, 4), ""), ((17, 2, 17, 64), "nan"), ((33, 5, 51, 64), "big"), ((16, 3, 64, 256), ""), ((40, 2, 65, 512), ""),
              ((19, 16, 256, 68), "")]


@pytest.mark.parametrize("shape,variant", HEAD_CASES)
def test_head_against_fp64(shape, variant):
    """`big`: logits of about +-80, where a softmax without the running maximum overflows; `nan`: one NaN bias, exactly that action's q"""
    from core.common import hip_ops

    n, K, N, H = shape
    M = K * K
    gen = th.Generator().manual_seed(n + 7 * N + H)
    h = th.randn(n, H + 3, generator=gen)[:, :H]
    w = th.randn(M * N, H, generator=gen) * ((80.0 if variant == "big" else 2.0) / np.sqrt(H))
    b = th.randn(M * N, generator=gen) * 0.1
    want = ref.head_q(h.numpy(), w.numpy(), b.numpy(), M, V_MIN, V_MAX)
    aten = (th.softmax((h @ w.T + b).view(n, M, N), dim=2) * th.linspace(V_MIN, V_MAX, N)).sum(dim=2)
    if variant == "nan":
        b[1 * N + 3] = float("nan")
    bufs = GuardedBufs()
    q = bufs.new_cols("q", n, M + 3, 1, M)
    hd, wd, bd = h._base.to(DEV)[:, :H], w.to(DEV), b.to(DEV)  # h keeps its row stride H + 3
    hip_ops.c51_head_q(hd, wd, bd, K, V_MIN, V_MAX, q)
    bufs.check(written=("q",))
    snap = bufs.snapshot()
    hip_ops.c51_head_q(hd, wd, bd, K, V_MIN, V_MAX, q)
    bufs.check(written=("q",))
    assert th.equal(bufs.bufs["q"][0].view(th.int32), snap["q"].view(th.int32))  # the same bits (a NaN never equals itself by value)
    got = q.cpu()
    if variant == "nan":
        assert bool(th.isnan(got[:, 1]).all()) and int(th.isnan(got).sum()) == n
        keep = [a for a in range(M) if a != 1]
        got, want, aten = got[:, keep], want[:, keep], aten[:, keep]
    within(f"head {shape} {variant}", got, want, aten)


def loss_inputs(B, K, N, pad=5):
    """rows 0 .. 4 where they exist: done = 1 | a reward that pushes Tz past v_max | one below v_min | gamma = 1, done = 0, reward = dz:
    integer positions | a fractional done, as an n-step fold gives it. One action per row is lifted so that the greedy one is decided."""
    M = K * K
    rng = np.random.default_rng(1000 * B + 10 * K + N)
    z, z_next = (np.ascontiguousarray(rng.normal(0, 2, (B, M * N + pad)), np.float32) for _ in range(2))
    for r in range(B):
        a = (7 * r + 1) % M
        z_next[r, a * N + N // 2:(a + 1) * N] += 8.0
    index = rng.integers(0, M, B)
    rew = rng.uniform(-3, 3, B).astype(np.float32)
    done = rng.uniform(0, 0.1, B).astype(np.float32)
    for r, (rw, dn) in enumerate(((1.0, 1.0), (50.0, 0.0), (-50.0, 0.0), ((V_MAX - V_MIN) / (N - 1), 0.0), (0.5, 0.2701))):
        if r < B:
            rew[r], done[r] = rw, dn
    return z, z_next, index, rew, done


@pytest.mark.parametrize("B,K,N", [(1, 2, 2), (5, 2, 51), (32, 5, 51), (33, 3, 64), (7, 2, 256)])
def test_loss_against_fp64(B, K, N):
    from core.c51.c51 import c51_loss_torch
    from core.common import hip_ops
    from core.common.vec_env.cstr_vec_env import decode_valve_index

    M, MN, gamma = K * K, K * K * N, 1.0
    z, z_next, index, rew, done = loss_inputs(B, K, N)
    want = ref.loss_step(z[:, :MN], z_next[:, :MN], index, rew, done, gamma, M, V_MIN, V_MAX)
    top2 = np.sort(want["q_next"], axis=1)[:, -2:]
    assert float((top2[:, 1] - top2[:, 0]).min()) >= 1e-3 * (V_MAX - V_MIN)  # a condition on the inputs: a* is decided on every row
    zt = th.tensor(z[:, :MN]).view(B, M, N).requires_grad_(True)
    aten = c51_loss_torch(zt, th.tensor(z_next[:, :MN]).view(B, M, N), th.as_tensor(index), th.tensor(rew).view(B, 1),
                          (1 - th.tensor(done).view(B, 1)) * gamma, V_MIN, V_MAX)
    aten["loss"].backward()
    bufs = Bufs()
    out = dict(loss_out=bufs.new("loss_out", 1), m_out=bufs.new("m_out", B, N), logp_out=bufs.new("logp_out", B, N),
               row_loss_out=bufs.new("row_loss_out", B), next_index_out=th.full((B,), -7, dtype=th.int64, device=DEV))
    gz_wide = bufs.new("gz", B, z.shape[1])
    d = lambda a: th.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)  # noqa: E731
    args = (d(z)[:, :MN], d(z_next)[:, :MN], d(decode_valve_index(index, K)), d(rew), d(done), gamma, K, N, V_MIN, V_MAX)
    ws = th.zeros(B, dtype=th.float64, device=DEV)
    hip_ops.c51_loss(*args, gz_wide[:, :MN], ws, **out)
    bufs.check(written=[n for n in bufs.flat if n != "gz"])
    snap = bufs.snapshot()
    hip_ops.c51_loss(*args, gz_wide[:, :MN], ws, **out)
    bufs.same_as(snap)  # two launches: the same bits
    gz = gz_wide[:, :MN].cpu()
    assert bool((gz_wide[:, MN:] == SENT).all())  # the gap behind every row still holds the sentinel
    lab = f"loss B{B} K{K} N{N}"
    within(f"{lab} m", out["m_out"], want["m"], aten["m"])
    within(f"{lab} logp", out["logp_out"], want["logp"], aten["logp"])
    within(f"{lab} row_loss", out["row_loss_out"], want["row_loss"], aten["row_loss"])
    within(f"{lab} loss", out["loss_out"], np.array([want["loss"]]), aten["loss"].reshape(1))
    within(f"{lab} gz", gz, want["gz"], zt.grad.reshape(B, MN))
    np.testing.assert_array_equal(out["next_index_out"].cpu().numpy(), want["next_index"])
    assert float((out["m_out"].double().sum(dim=1) - 1).abs().max()) <= 1e-6
    off = np.ones((B, M, N), bool)
    off[np.arange(B), index] = False
    assert (gz.numpy().reshape(B, M, N)[off] == 0).all()


# ---- the class ------------------------------------------------------------------------------------------------------------------------
def make_model(n_envs=64, **kw):
    from core.c51 import C51
    from core.common.logger import Logger
    from core.common.vec_env import CSTRVecEnv

    kw = dict(dict(batch_size=32, learning_starts=64, seed=0, policy_kwargs=dict(n_atoms=17), v_min=-40.0, v_max=5.0, device=DEV), **kw)
    model = C51("MlpPolicy", CSTRVecEnv(n_envs, discrete_actions=3, device=DEV), **kw)
    model.set_logger(Logger(folder=None, output_formats=[]))
    return model


def logits_of(sd, net, x):
    """the [64, 64] ReLU network of a policy state dict in x's dtype, on the CPU -> [B, M, N]"""
    for i in (0, 2, 4):
        x = x @ sd[f"{net}.categorical_net.{i}.weight"].cpu().to(x.dtype).T + sd[f"{net}.categorical_net.{i}.bias"].cpu().to(x.dtype)
        x = th.relu(x) if i < 4 else x
    return x.view(len(x), 9, -1)


def test_first_gradient_step_and_q_values():
    from core.c51.c51 import c51_loss_torch

    B, M = 32, 9
    rng = np.random.default_rng(3)
    obs = rng.uniform(-1, 1, (B, 4)).astype(np.float32)
    batch = (obs, rng.integers(0, M, B), np.clip(obs + rng.normal(0, 0.05, obs.shape), -1, 1).astype(np.float32),
             rng.uniform(-8, 0, B).astype(np.float32), (rng.uniform(size=B) < 0.2).astype(np.float32))
    for fused_learner in (True, False):
        model = make_model()
        assert model.fused_learner and model._head_kernel and (model.n_atoms, model.v_min, model.v_max) == (17, -40.0, 5.0)
        model.fused_learner, model.debug_capture = fused_learner, True
        sd = {k: v.detach().cpu().clone() for k, v in model.policy.state_dict().items()}  # the weights before the step
        x, nx = th.tensor(batch[0]), th.tensor(batch[2])
        z64, zn64 = logits_of(sd, "categorical_net", x.double()), logits_of(sd, "categorical_net_target", nx.double())
        want = ref.loss_step(z64.reshape(B, -1).numpy(), zn64.reshape(B, -1).numpy(), batch[1], batch[3], batch[4], model.gamma, M, -40.0, 5.0)
        aten = c51_loss_torch(logits_of(sd, "categorical_net", x), logits_of(sd, "categorical_net_target", nx), th.as_tensor(batch[1]),
                              th.tensor(batch[3]).view(B, 1), (1 - th.tensor(batch[4]).view(B, 1)) * model.gamma, -40.0, 5.0)
        if fused_learner:  # the rollout's values on the same weights
            q32 = (th.softmax(logits_of(sd, "categorical_net", x), dim=2) * th.linspace(-40.0, 5.0, 17)).sum(dim=2)
            within("class q_values", model._q_values(x.to(DEV)), ref.expected_q(z64.numpy(), -40.0, 5.0), q32)
        model.batch_queue.append(batch)
        model.train(gradient_steps=1, batch_size=B)
        cap = model.train_capture[-1]
        lab = "class fused" if fused_learner else "class torch"
        within(f"{lab} loss", cap["loss"], np.array([want["loss"]]), aten["loss"].reshape(1))
        within(f"{lab} m", cap["m"], want["m"], aten["m"])
        within(f"{lab} logp", cap["logp"], want["logp"], aten["logp"])
        np.testing.assert_array_equal(cap["next_index"].cpu().numpy(), want["next_index"])
        assert "train/loss" in model.logger.name_to_value and model.policy.optimizer.defaults["eps"] == 0.01 / B


def test_graph_replay_is_eager_bit_for_bit():
    n, tf, iters = 8, 4, 20

    def run(graph):
        model = make_model(n_envs=n, seed=5, batch_size=16, buffer_size=64 * n, learning_starts=2 * n, train_freq=tf,
                           target_update_interval=2 * tf * n, exploration_fraction=0.5, policy_kwargs=dict(net_arch=[32, 32], n_atoms=17))
        if graph:
            model.enable_graph_capture(True)
        model.learn(n * tf * iters)
        th.cuda.synchronize()
        return model

    eager, model = run(False), run(True)
    st = model.graph_status()
    assert st["active"] and st["error"] is None and st["replays"] > 0 and eager.graph_status()["replays"] == 0
    for a, b in ((eager.policy.arena.flat, model.policy.arena.flat), (eager.policy.target_arena.flat, model.policy.target_arena.flat),
                 (eager.policy.optimizer.exp_avg_sq, model.policy.optimizer.exp_avg_sq), (eager._denv.obs, model._denv.obs)):
        assert th.equal(a.view(th.int32), b.view(th.int32))
    assert eager._n_updates == model._n_updates > 0


def test_n_steps_and_save_load(tmp_path):
    from core.c51 import C51
    from core.common.vec_env import CSTRVecEnv

    model = make_model(n_envs=8, n_steps=3, buffer_size=64 * 8, learning_starts=16, train_freq=1)
    model.learn(8 * 8)
    assert model._n_updates > 0 and np.isfinite(float(model.logger.name_to_value["train/loss"]))
    path = os.path.join(tmp_path, "c51.zip")
    model.save(path)
    env = lambda: CSTRVecEnv(8, discrete_actions=3, device=DEV)  # noqa: E731
    loaded = C51.load(path, env=env(), device=DEV)
    assert (loaded.n_atoms, loaded.v_min, loaded.v_max, loaded.n_steps) == (17, -40.0, 5.0, 3)
    assert th.equal(loaded.policy.arena.flat, model.policy.arena.flat)
    with pytest.raises(ValueError, match="n_atoms"):
        C51.load(path, env=env(), device=DEV, policy_kwargs=dict(n_atoms=21))
