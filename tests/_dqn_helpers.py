"""NumPy restatements the DQN tests share (tests/test_dqn_abi.py checks them on the CPU against the reference-written fixtures before
tests/test_dqn.py uses them as the yardstick on the GPU): the discrete valve face, the fp64 statement of core/dqn/dqn.py:195-212, the
fp64 forward of the Q network, the action selection of cstr_dqn_act_f32 and its Philox4x32-10 uniforms."""
import numpy as np

DQN_STREAM_TAG = 0xD09A11C7


def valve_np(q, K):
    """v(q) = f32(-1) + f32(2 q) / f32(K - 1), every operation in float32"""
    q = np.asarray(q, np.int64)
    return np.float32(-1) + (2 * q).astype(np.float32) / np.float32(K - 1)


def level_np(v, K):
    """q = rint((v + 1) * (K - 1) / 2) in float32"""
    v = np.asarray(v, np.float32)
    return np.rint(((v + np.float32(1)) * np.float32(K - 1)) / np.float32(2)).astype(np.int64)


def pair_np(index, K):
    index = np.asarray(index, np.int64)
    return np.stack([valve_np(index // K, K), valve_np(index % K, K)], axis=-1)


def loss_f64(q, next_q, index, reward, done, gamma):
    """dqn.py:195-212 in float64 on float32 inputs (gamma rounded to float32 first, as the f32 arithmetic of the reference sees it):
    (current_q [B], target_q [B], loss, d loss / d q [B, M])"""
    q, next_q = np.asarray(q, np.float64), np.asarray(next_q, np.float64)
    reward, done = np.asarray(reward, np.float64).reshape(-1), np.asarray(done, np.float64).reshape(-1)
    index = np.asarray(index, np.int64).reshape(-1)
    B = q.shape[0]
    nq = np.where(np.isnan(next_q).any(axis=1), np.nan, next_q.max(axis=1))
    target = reward + ((1.0 - done) * np.float64(np.float32(gamma))) * nq
    cur = q[np.arange(B), index]
    d = cur - target
    z = np.abs(d)
    with np.errstate(invalid="ignore"):
        per = np.where(z < 1.0, 0.5 * z * z, z - 0.5)
    g = np.zeros_like(q)
    g[np.arange(B), index] = np.where(np.isnan(d), np.nan, np.clip(d, -1.0, 1.0)) / B
    return cur, target, per.mean(), g


def loss_f32(q, next_q, index, reward, done, gamma):
    """dqn.py:195-212 in float32 NumPy in the operation order include/cstr_rl_hip.h fixes (IEEE, no contraction: what the kernel must
    give bit for bit): target = reward + ((1 - done) * f32(gamma)) * max, d = cur - target, g = clamp(d, -1, 1) / f32(B)"""
    q, next_q = np.asarray(q, np.float32), np.asarray(next_q, np.float32)
    reward, done = np.asarray(reward, np.float32).reshape(-1), np.asarray(done, np.float32).reshape(-1)
    index = np.asarray(index, np.int64).reshape(-1)
    B = q.shape[0]
    target = reward + ((np.float32(1) - done) * np.float32(gamma)) * next_q.max(axis=1)
    cur = q[np.arange(B), index]
    d = cur - target
    g = np.zeros_like(q)
    g[np.arange(B), index] = np.clip(d, np.float32(-1), np.float32(1)) / np.float32(B)
    assert target.dtype == cur.dtype == g.dtype == np.float32
    return cur, target, g


def mlp_f64(sd, prefix, obs):
    """create_mlp(4, M, [H1, H2], ReLU) forward in float64 from a fixture's weights (keys prefix/q_net.{0,2,4}.{weight,bias})"""
    x = np.asarray(obs, np.float64)
    for i in (0, 2, 4):
        x = x @ np.asarray(sd[f"{prefix}/q_net.{i}.weight"], np.float64).T + np.asarray(sd[f"{prefix}/q_net.{i}.bias"], np.float64)
        if i != 4:
            x = np.maximum(x, 0.0)
    return x


def ulps(got, want64):
    """|got - f32(want)| in units of the spacing of float32 at f32(want); NaN matches NaN"""
    got = np.asarray(got, np.float32).reshape(-1)
    want = np.asarray(want64, np.float64).astype(np.float32).reshape(-1)
    both_nan = np.isnan(got) & np.isnan(want)
    sp = np.spacing(np.maximum(np.abs(want), np.float32(1e-30))).astype(np.float64)
    with np.errstate(invalid="ignore"):
        u = np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp
    u[both_nan] = 0.0
    u[np.isnan(u)] = np.inf
    return u


def philox4x32_10(c, k):
    """c uint32 [n, 4], k uint32 [2] -> uint32 [n, 4]"""
    c = [c[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k[0]), np.uint64(k[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        n0 = ((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32
        n2 = ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32
        c = [n0, p1 & m32, n2, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


def dqn_uniforms(seed, base, n):
    """u [n, 2] float32 of rows 0 .. n - 1 as cstr_dqn_act_f32 draws them: counter (base + row, 0, tag), key = seed; word >> 8 times 2^-24"""
    ctr = np.uint64(base) + np.arange(n, dtype=np.uint64)
    c = np.zeros((n, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 3] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32), DQN_STREAM_TAG
    x = philox4x32_10(c, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    return ((x[:, :2] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def act_np(q, K, mode, eps=None, flag=None, u=None):
    """index [n] of cstr_dqn_act_f32: greedy = first maximum; mode 1: every row random iff flag; mode 2: row r random iff u[r, 0] < eps;
    random index = min(floor(f32(u[r, 1] * M)), M - 1)"""
    q = np.asarray(q, np.float32)
    n, M = q.shape
    greedy = q.argmax(axis=1)
    if mode == 0:
        return greedy
    u = np.asarray(u, np.float32)
    rnd = np.minimum(np.floor(u[:, 1] * np.float32(M)), M - 1).astype(np.int64)
    explore = np.full(n, bool(flag)) if mode == 1 else (u[:, 0].astype(np.float64) < float(eps))
    return np.where(explore, rnd, greedy)
