"""NumPy / Python-int restatement of cstr_collect_episodes_f32's exploration draw (include/cstr_rl_hip.h, step b. of its contract): the
Philox4x32-10 block of (env, step), the explore flag and the two forms of the uniform action. Written on Python integers, independently of
the array restatement in tests/_dqn_helpers.py (which tests/_rowkernel_reference.py uses): tests/test_collect_episodes_abi.py checks one
against the other on shared counters."""
import numpy as np

COLLECT_TAG = 0xC011EC7D  # csrc/cstr_eval.hip
M32 = 0xFFFFFFFF
F = np.float32


def philox_block(c, key):
    """One Philox4x32-10 block: c = four 32-bit counter words, key = two 32-bit key words -> four 32-bit words (Python ints)."""
    c0, c1, c2, c3 = (int(x) & M32 for x in c)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(word) -> np.float32:
    """a Philox word as a float32 in [0, 1): (word >> 8) * 2^-24 (exact)"""
    return F(int(word) >> 8) * F(1.0 / 16777216.0)


def collect_block(seed: int, idx: int, step: int):
    """The block of env index `idx` (= index_offset + env, taken modulo 2^64) at stream step `step` (= step_offset + t < 2^32)."""
    idx, seed = int(idx) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    assert 0 <= step <= M32
    return philox_block((idx & M32, idx >> 32, step, COLLECT_TAG), (seed & M32, seed >> 32))


def explore_draw(seed: int, index_offset: int, step_offset: int, n_steps: int, n_envs: int, explore_prob: float, squashed: bool, low, high):
    """(flags bool [T, N], v float32 [T, N, A]): whether (step t, env i) explores and the head value an exploring row gets -- squashed:
    2 u - 1; otherwise low + u * (high - low), product and sum rounded to float32 separately. explore_prob == 0: no flag is set (the kernel
    evaluates no block)."""
    low, high = np.asarray(low, F), np.asarray(high, F)
    a = low.shape[0]
    flags, v = np.zeros((n_steps, n_envs), bool), np.zeros((n_steps, n_envs, a), F)
    p = F(explore_prob)
    if not p > 0:
        return flags, v
    for t in range(n_steps):
        for i in range(n_envs):
            w = collect_block(seed, index_offset + i, step_offset + t)
            flags[t, i] = uniform(w[0]) < p
            for j in range(a):
                u = uniform(w[1 + j])
                v[t, i, j] = (F(2.0) * u - F(1.0)) if squashed else F(low[j] + F(u * F(high[j] - low[j])))
    return flags, v
