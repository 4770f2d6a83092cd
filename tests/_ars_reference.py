"""Restatement of the ARS launches (csrc/cstr_ars.hip, include/cstr_rl_hip.h "Augmented Random Search") that uses none of the
package's kernels: the Philox / Box-Muller delta definition, candidate formation, the policy, predict()'s unscale / clip, the job model
on the oracle env (oracle/cstr_oracle.py: its f32 step and its PCG64 reset draws) and the update statement with its ordering rules.

Two precisions of the same statement: `dtype=np.float64` (the reference the kernel is judged against) and `dtype=np.float32` (the
kernel's own arithmetic order: acc = 0, acc += w[i] x[i] ascending, + bias, activation). They differ in candidate formation, the policy
and the action post-processing; the delta values (float32 by definition), the env step (the oracle's f32 step on the float32 action)
and the f64 return sums are shared. The distance between the two is what the GPU tests take as the unit of their tolerance.

The delta values are computed in float64 from the float32 uniforms and rounded once; the device evaluates logf / sqrtf / sincospif in
float32, so a device delta may differ from these by a few units in the last place."""
import numpy as np

from oracle import cstr_oracle as orc

ARS_TAG = 0xA4500D17
M32 = np.uint64(0xFFFFFFFF)
F = np.float32


def philox4x32_10(counters: np.ndarray, seed: int) -> np.ndarray:
    """counters uint32 [n, 4], 64-bit key -> uint32 [n, 4] (vectorised; checked against tests/_collect_reference.philox_block)"""
    c = [counters[:, i].astype(np.uint64) for i in range(4)]
    seed = int(seed) & (2**64 - 1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=1).astype(np.uint32)


def deltas(seed: int, update: int, n_delta: int, n_params: int) -> np.ndarray:
    """delta [n_delta, n_params] float32: block q = p >> 2 of direction k has counter (q, k, update, ARS_TAG); words (0, 1) and (2, 3)
    give two Box-Muller pairs (radius from the first word, angle from the second, cos then sin)."""
    nq = (n_params + 3) // 4
    k, q = np.meshgrid(np.arange(n_delta, dtype=np.uint32), np.arange(nq, dtype=np.uint32), indexing="ij")
    c = np.stack([q.reshape(-1), k.reshape(-1), np.full(k.size, update, np.uint32), np.full(k.size, ARS_TAG, np.uint32)], axis=1)
    w = philox4x32_10(c, seed)
    u = (((w >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)).astype(np.float64)  # the f32 uniform, exactly
    z = np.empty(w.shape, np.float64)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        ang = np.pi * (2.0 * u[:, b])
        z[:, a], z[:, b] = r * np.cos(ang), r * np.sin(ang)
    return z.astype(F).reshape(n_delta, 4 * nq)[:, :n_params].copy()


def n_params(spec) -> int:
    dims, b = [spec["obs_dim"], *spec["hidden"], spec["act_dim"]], 1 if spec["with_bias"] else 0
    return sum(o * (i + b) for i, o in zip(dims[:-1], dims[1:]))


def candidates(theta, delta, delta_std, dtype):
    """[2 n_delta, P]: theta + s delta_k, then theta - s delta_k; in float32 the product is rounded before the sum"""
    th_, d, s = np.asarray(theta, F).astype(dtype), delta.astype(dtype), dtype(F(delta_std))
    sd = (s * d).astype(dtype)
    return np.concatenate([(th_ + sd).astype(dtype), (th_ - sd).astype(dtype)], axis=0)


def _layers(vec, spec):
    dims, off, out = [spec["obs_dim"], *spec["hidden"], spec["act_dim"]], 0, []
    for i, o in zip(dims[:-1], dims[1:]):
        w = vec[off:off + o * i].reshape(o, i)
        off += o * i
        b = None
        if spec["with_bias"]:
            b = vec[off:off + o]
            off += o
        out.append((w, b))
    assert off == vec.size
    return out


def policy(vec, spec, x, dtype):
    """the deterministic output of create_mlp(...) on one observation, every operation in `dtype`, dot products ascending from 0"""
    h = np.asarray(x, F).astype(dtype)
    layers = _layers(vec.astype(dtype), spec)
    with np.errstate(invalid="ignore", over="ignore"):
        for li, (w, b) in enumerate(layers):
            acc = np.zeros(w.shape[0], dtype)
            for i in range(w.shape[1]):
                acc = (acc + (w[:, i] * h[i]).astype(dtype)).astype(dtype)
            if b is not None:
                acc = (acc + b).astype(dtype)
            if li < len(layers) - 1:
                acc = np.tanh(acc).astype(dtype) if spec["act"] == "tanh" else np.where(acc < 0, dtype(0), acc).astype(dtype)
            h = acc
        return np.tanh(h).astype(dtype) if spec["squash"] else h


def post(y, spec, low, high, dtype):
    """predict(): unscale low + 0.5 (y + 1) (high - low) when squashed, else clip (NaN passes); the env gets float32"""
    lo, hi = np.asarray(low, F).astype(dtype), np.asarray(high, F).astype(dtype)
    with np.errstate(invalid="ignore"):
        if spec["squash"]:
            a = lo + (dtype(0.5) * (y + dtype(1.0))).astype(dtype) * (hi - lo)
        else:
            a = np.where(np.isnan(y), y, np.minimum(np.maximum(y, lo), hi))
    return np.asarray(a, dtype).astype(F)


class SlotEnv:
    """one env slot on the oracle: layouts (4, 2) and (8, 4) (two trains side by side, reward rA + rB, one counter, one stream)"""

    def __init__(self, spec, coef, integrator, obs, step, pcg, static_init):
        self.twin = (spec["obs_dim"], spec["act_dim"]) == (8, 4)
        if not self.twin and (spec["obs_dim"], spec["act_dim"]) != (4, 2):
            raise NotImplementedError("the restatement covers the (4, 2) and (8, 4) layouts")
        self.coef, self.integ = coef, integrator
        self.obs, self.step = np.array(obs, F), int(step)
        self.pcg = np.array(pcg, dtype=np.uint64).reshape(1, 4).view(orc.PCG_DTYPE).reshape(1).copy()
        self.static = None if static_init is None else np.array(static_init, np.float64)

    def reset(self):
        parts = []
        for tr in range(2 if self.twin else 1):
            st = None if self.static is None else np.ascontiguousarray(self.static[4 * tr:4 * tr + 4].reshape(1, 4))
            parts.append(orc.reset_draw(self.pcg, None, st)[0])
            if st is not None:
                self.static[4 * tr:4 * tr + 4] = st[0]
        self.obs, self.step = np.concatenate(parts).astype(F), 0

    def step_env(self, act):
        rew, done, nxt = F(0), False, []
        for tr in range(2 if self.twin else 1):
            o, a = self.obs[4 * tr:4 * tr + 4].reshape(1, 4), np.asarray(act[2 * tr:2 * tr + 2], F).reshape(1, 2)
            n, _, r, d, _, st = orc.vec_step(o, a, np.array([self.step], np.int32), o, integrator=self.integ, coef=self.coef)
            nxt.append(n[0])
            rew = F(r[0]) if tr == 0 else F(rew + F(r[0]))
            done = done or bool(d[0] > 0)
        self.obs, self.step = np.concatenate(nxt).astype(F), self.step + 1
        return rew, done

    def pcg_words(self):
        return self.pcg.view(np.uint64).reshape(4).copy()


def run_population(theta, spec, delta_std, seed, update, n_delta, n_eval_episodes, alive_bonus_offset, coef, integrator, obs, step_count, pcg,
                   static_init, low, high, dtype):
    """The job model: job c on slot c % N, a slot's jobs in increasing c; a job = reset draw, n_eval_episodes episodes each followed by
    the auto-reset draw. Returns dict(returns f64 [2 n_delta], lengths [2 n_delta], obs, step_count, pcg uint64 [N, 4], static_init)."""
    n = obs.shape[0]
    cand = candidates(theta, deltas(seed, update, n_delta, n_params(spec)), delta_std, dtype)
    slots = [SlotEnv(spec, coef, integrator, obs[i], step_count[i], pcg[i], None if static_init is None else static_init[i]) for i in range(n)]
    returns, lengths = np.zeros(2 * n_delta, np.float64), np.zeros(2 * n_delta, np.int64)
    for c in range(2 * n_delta):
        env = slots[c % n]
        env.reset()
        total, length = 0.0, 0
        for _ in range(n_eval_episodes):
            cur = 0.0
            for _t in range(max(int(coef.max_steps), 1)):
                act = post(policy(cand[c], spec, env.obs, dtype), spec, low, high, dtype)
                rew, done = env.step_env(act)
                cur += float(rew)
                length += 1
                if done:
                    break
            total += cur
            env.reset()
        returns[c], lengths[c] = total + float(alive_bonus_offset) * float(length), length
    return dict(returns=returns, lengths=lengths, obs=np.stack([s.obs for s in slots]), step_count=np.array([s.step for s in slots], np.int32),
                pcg=np.stack([s.pcg_words() for s in slots]), static_init=None if static_init is None else np.stack([s.static for s in slots]))


def _beats(a, ia, b, ib) -> bool:
    an, bn = np.isnan(a), np.isnan(b)
    if an or bn:
        return bool(an and (not bn or ia < ib))
    return bool(a > b or (a == b and ia < ib))


def ranking(returns, n_delta, n_top):
    """kept directions in rank order: descending top_k = max(R+, R-) (NaN if either is), NaN the greatest, ties to the lower k"""
    r = np.asarray(returns, np.float64)
    plus, minus = r[:n_delta], r[n_delta:]
    with np.errstate(invalid="ignore"):
        top = np.where(np.isnan(plus) | np.isnan(minus), np.nan, np.maximum(plus, minus))
    rank = [sum(_beats(top[j], j, top[k], k) for j in range(n_delta)) for k in range(n_delta)]
    order = np.argsort(rank)
    return order[:n_top].astype(np.int64)


def update(theta, returns, n_delta, n_top, lr, delta):
    """the published update in float64 -> (theta_new float64 [P], step_size, return_std, kept)"""
    r = np.asarray(returns, np.float64)
    kept = ranking(r, n_delta, n_top)
    plus, minus = r[:n_delta][kept], r[n_delta:][kept]
    with np.errstate(invalid="ignore", divide="ignore"):
        both = np.concatenate([plus, minus])
        return_std = np.sqrt(((both - both.mean()) ** 2).sum() / (both.size - 1))
        step_size = lr / (n_top * return_std + 1e-6)
        new = np.asarray(theta, F).astype(np.float64) + step_size * ((plus - minus) @ delta[kept].astype(np.float64))
    return new, step_size, return_std, kept
