"""Reference statements of CQL (Kumar et al. 2020; the importance-sampled CQL(H) term on SAC, core/cql/cql.py) for
tests/test_cql_abi.py and tests/test_cql.py:

  * `candidates`: the 3N candidate rows per state and their corrections from given (u, eps), NumPy (float64 by default);
  * `q_loss_f64`: the TD target, the critic loss, its four logged scalars and the EXPLICIT gradient d loss / d q, NumPy float64;
  * `q_loss_torch`: the same as one torch statement in any dtype, gradient by autograd (float32: the "ATen distance" of the bars);
  * `cql_uniforms` / `cql_normals`: Python-integer Philox4x32-10 restatement of cstr_cql_candidates_f32's counter contract, on
    tests/_collect_reference.py's block function and uniform conversion and tests/_rowkernel_reference.py's Box-Muller statement;
  * `critic_step`: a small fp64 model (two frozen-architecture critics, a batch, noise) -- the loss, the parameter gradients -- with
    the mistakes a wrong implementation makes as `variant`s, and `same_step`, the comparator;
  * `RefCQL`: whole gradient steps in plain torch fp64; `dataset_gap`: the dataset mean of lse - Q(s, a) over both critics;
  * `synthetic_dataset`: BCQ's synthetic dataset (tests/test_bcq.py, tests/test_td3bc.py)."""
import math

import numpy as np
import torch as th
from torch.nn import functional as F

from _collect_reference import philox_block, uniform

CQL_TAG = 0xC0175E4A  # csrc/cstr_cql.hip
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = math.log(math.sqrt(2 * math.pi))
VARIANTS = ("corr_added", "unif_sign", "softmax_no_temp", "lse_no_T", "no_q_data_term", "sample_major", "next_at_next_state",
            "no_1_over_B_cand", "half_on_one_term", "entropy_in_target")


# ---- candidates ----------------------------------------------------------------------------------------------------------------------
def squashed_sample(mean, raw, eps, dtype=np.float64):
    """(action, log-prob) of SAC's squashed Gaussian for given eps; mean / raw [..., A] broadcast against eps [..., A]"""
    mean, raw, eps = (np.asarray(x, dtype) for x in (mean, raw, eps))
    sd = np.exp(np.clip(raw, dtype(LOG_STD_MIN), dtype(LOG_STD_MAX)))
    g = mean + sd * eps
    a = np.tanh(g)
    lp = (-((g - mean) ** 2) / (2 * sd * sd) - np.log(sd) - dtype(HALF_LOG_2PI)).sum(-1)
    return a, lp - np.log(1 - a * a + dtype(1e-6)).sum(-1)


def candidates(obs, params_cur, params_next, u, eps, dtype=np.float64, next_obs=None, unif_sign=1.0):
    """x [B * 3N, D + A] (row b * 3N + j = [obs_b | a_bj]: j < N uniform, < 2N ~ pi(.|s_b), < 3N ~ pi(.|s'_b), all at obs_b) and
    corr [B, 3N] = A log 0.5 | log pi(a | s) | log pi(a | s'). `next_obs` (a mistake): the pi(.|s') rows carry s' instead."""
    obs, pc, pn, u, eps = (np.asarray(x, dtype) for x in (obs, params_cur, params_next, u, eps))
    B, N, A = u.shape
    a_cur, lp_cur = squashed_sample(pc[:, None, :A], pc[:, None, A:], eps[:, :N], dtype)
    a_nxt, lp_nxt = squashed_sample(pn[:, None, :A], pn[:, None, A:], eps[:, N:], dtype)
    acts = np.concatenate([u, a_cur, a_nxt], axis=1)
    o = np.repeat(obs[:, None, :], 3 * N, axis=1)
    if next_obs is not None:
        o[:, 2 * N:] = np.asarray(next_obs, dtype)[:, None, :]
    corr = np.concatenate([np.full((B, N), unif_sign * A * math.log(0.5), dtype), lp_cur, lp_nxt], axis=1)
    return np.concatenate([o, acts], axis=2).reshape(B * 3 * N, -1), corr


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def td_target_f64(q1_t, q2_t, next_logp, rew, done, ent_coef, gamma):
    q1_t, q2_t, rew, done = (np.asarray(x, np.float64).reshape(-1) for x in (q1_t, q2_t, rew, done))
    qn = np.minimum(q1_t, q2_t)
    if next_logp is not None:
        qn = qn - float(ent_coef) * np.asarray(next_logp, np.float64).reshape(-1)
    return rew + (1 - done) * gamma * qn


def q_loss_f64(q, corr, with_data, q1_t, q2_t, next_logp, rew, done, ent_coef, gamma, w, T) -> dict:
    """q [2, (1 + 3N) B]: both critics on [data rows | candidate rows]. Returns target [B], loss, aux [4] = {bellman, conservative
    (x w), mean lse, mean Q(s, a)}, lse [2, B] and gq [2, (1 + 3N) B] = d loss / d q, written out term by term."""
    q = np.asarray(q, np.float64).reshape(2, -1)
    t = td_target_f64(q1_t, q2_t, next_logp, rew, done, ent_coef, gamma)
    B = t.shape[0]
    n3 = q.shape[1] // B - 1
    gq, lse = np.zeros_like(q), np.zeros((2, B))
    bell = cons = 0.0
    for i in range(2):
        qd, c = q[i, :B], q[i, B:].reshape(B, n3)
        c = c - np.asarray(corr, np.float64) if corr is not None else c
        if with_data:
            c = np.concatenate([c, qd[:, None]], axis=1)
        z = c / T
        m = z.max(axis=1, keepdims=True)
        m = np.where(np.isinf(m), 0.0, m)
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.exp(z - m)
            s = e.sum(axis=1, keepdims=True)
            lse[i] = T * (np.log(s) + m)[:, 0]
            p = e / s
        bell += 0.5 * ((qd - t) ** 2).mean()
        cons += 0.5 * w * (lse[i].mean() - qd.mean())
        gq[i, :B] = 0.5 * (2 * (qd - t) / B - w / B)
        gq[i, B:] = (0.5 * w / B * p[:, :n3]).reshape(-1)
        if with_data:
            gq[i, :B] += 0.5 * w / B * p[:, n3]
    return dict(target=t, loss=bell + cons, aux=np.array([bell, cons, lse.mean(), q[:, :B].mean()]), lse=lse, gq=gq)


def q_loss_torch(q, corr, with_data, q1_t, q2_t, next_logp, rew, done, ent_coef, gamma, w, T, dtype=th.float64, device="cpu") -> dict:
    """The statement as a user would write it in torch, evaluated in `dtype` on `device`; gq by autograd."""
    cv = lambda x: None if x is None else th.as_tensor(np.asarray(x)).to(device, dtype)  # noqa: E731
    q = cv(q).reshape(2, -1).clone().requires_grad_(True)
    q1_t, q2_t, rew, done = (cv(x).reshape(-1) for x in (q1_t, q2_t, rew, done))
    corr = cv(corr)
    with th.no_grad():
        qn = th.min(q1_t, q2_t)
        if next_logp is not None:
            qn = qn - cv(ent_coef).reshape(()) * cv(next_logp).reshape(-1)
        t = rew + (1 - done) * gamma * qn
    B = t.shape[0]
    n3 = q.shape[1] // B - 1
    bell, cons, lses = 0.0, 0.0, []
    for i in range(2):
        qd, c = q[i, :B], q[i, B:].reshape(B, n3)
        c = c - corr if corr is not None else c
        if with_data:
            c = th.cat([c, qd[:, None]], dim=1)
        lse = T * th.logsumexp(c / T, dim=1)
        lses.append(lse)
        bell = bell + 0.5 * F.mse_loss(qd, t)
        cons = cons + 0.5 * w * (lse.mean() - qd.mean())
    loss = bell + cons
    (gq,) = th.autograd.grad(loss, q)
    lse = th.stack(lses).detach()
    aux = th.stack([bell.detach(), cons.detach(), lse.mean(), q[:, :B].detach().mean()])
    return dict(target=t.cpu().numpy(), loss=loss.item(), aux=aux.cpu().numpy(), lse=lse.cpu().numpy(), gq=gq.cpu().numpy())


# ---- the counter contract of cstr_cql_candidates_f32 (include/cstr_rl_hip.h) -------------------------------------------------------------
def _block(seed: int, base: int, b: int, k: int, N: int, sub: int):
    seed, c = int(seed) & 0xFFFFFFFFFFFFFFFF, (int(base) + b * N + k) & 0xFFFFFFFFFFFFFFFF
    return philox_block((c & 0xFFFFFFFF, c >> 32, sub, CQL_TAG), (seed & 0xFFFFFFFF, seed >> 32))


def cql_uniforms(seed: int, base: int, B: int, N: int, A: int) -> np.ndarray:
    """u [B, N, A] float32, exact: counter (base + b N + k, sub 0), word j -> 2 * ((w >> 8) * 2^-24) - 1"""
    out = np.zeros((B, N, A), np.float32)
    for b in range(B):
        for k in range(N):
            w = _block(seed, base, b, k, N, 0)
            for j in range(A):
                out[b, k, j] = np.float32(2.0) * uniform(w[j]) - np.float32(1.0)
    return out


def _box_muller(a: int, b: int):
    """tests/_rowkernel_reference.py normal_stream's statement for one word pair, float64"""
    u1, u2 = ((a >> 8) + 0.5) * 2.0 ** -24, ((b >> 8) + 0.5) * 2.0 ** -24
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)


def cql_normals(seed: int, base: int, B: int, N: int, A: int) -> np.ndarray:
    """eps [B, 2N, A] float64: counter (base + b N + k, sub 1 + p): Box-Muller(words 0, 1) -> columns 2p, 2p + 1 of the pi(.|s) sample k
    (row k), Box-Muller(words 2, 3) -> those of the pi(.|s') sample k (row N + k)"""
    out = np.zeros((B, 2 * N, A))
    for b in range(B):
        for k in range(N):
            for p in range((A + 1) // 2):
                w = _block(seed, base, b, k, N, 1 + p)
                for row, z in ((k, _box_muller(w[0], w[1])), (N + k, _box_muller(w[2], w[3]))):
                    for cc in range(2):
                        if 2 * p + cc < A:
                            out[b, row, 2 * p + cc] = z[cc]
    return out


def cql_normal_slack(seed: int, base: int, B: int, N: int, A: int) -> np.ndarray:
    """[B, 2N, A]: what the float32 representation error of Box-Muller's u1 (up to 2^-25) moves the radius by, per element
    (tests/_rowkernel_reference.py normal_slack's statement on this stream's blocks)"""
    out = np.zeros((B, 2 * N, A))
    rad = lambda v: math.sqrt(-2.0 * math.log(min(v, 1.0)))  # noqa: E731
    for b in range(B):
        for k in range(N):
            for p in range((A + 1) // 2):
                w = _block(seed, base, b, k, N, 1 + p)
                for row, word in ((k, w[0]), (N + k, w[2])):
                    u1 = ((word >> 8) + 0.5) * 2.0 ** -24
                    s = max(abs(rad(u1 + 2.0 ** -25) - rad(u1)), abs(rad(u1 - 2.0 ** -25) - rad(u1)))
                    out[b, row, 2 * p:2 * p + 2] = s
    return out


def worst_ulps(x, want) -> float:
    """the worst |x - want| over the elements in float32 ulps of the reference value (NaN patterns and infinities must agree)"""
    x, want = (np.asarray(v, np.float64).reshape(-1) for v in (x, want))
    if not np.array_equal(np.isnan(x), np.isnan(want)):
        return float("inf")
    ok = np.isfinite(want)
    if not np.array_equal(x[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)]):
        return float("inf")
    if not ok.any():
        return 0.0
    return float((np.abs(x[ok] - want[ok]) / np.spacing(np.abs(want[ok]).astype(np.float32)).astype(np.float64)).max())


# ---- a small fp64 model of the critic step, with the mistakes --------------------------------------------------------------------------
def small_case(B=5, N=3, D=4, A=2, seed=0, w=5.0, T=0.7, importance=True) -> dict:
    rng = np.random.default_rng(seed)
    g = th.Generator().manual_seed(seed)
    critics = []
    for _ in range(2):
        critics.append([th.randn(D + A, 6, generator=g, dtype=th.float64) * 0.6, th.randn(6, generator=g, dtype=th.float64) * 0.3,
                        th.randn(6, 1, generator=g, dtype=th.float64), th.randn(1, generator=g, dtype=th.float64)])
    return dict(obs=rng.uniform(-1, 1, (B, D)), act=rng.uniform(-1, 1, (B, A)), next_obs=rng.uniform(-1, 1, (B, D)),
                rew=rng.uniform(-2, 0, B), done=(rng.uniform(size=B) < 0.3).astype(np.float64),
                params_cur=np.concatenate([rng.normal(0, 0.5, (B, A)), rng.normal(-1, 0.5, (B, A))], 1),
                params_next=np.concatenate([rng.normal(0, 0.5, (B, A)), rng.normal(-1, 0.5, (B, A))], 1),
                u=rng.uniform(-1, 1, (B, N, A)), eps=rng.normal(0, 1, (B, 2 * N, A)), q1_t=rng.normal(-3, 1, B), q2_t=rng.normal(-3, 1, B),
                next_logp=rng.normal(-1, 0.5, B), ent_coef=0.3, gamma=0.99, w=w, T=T, importance=importance, backup_entropy=False,
                critics=critics)


def critic_step(case: dict, variant=None, explicit: bool = False) -> dict:
    """loss, aux, target and the gradients of the critics' parameters for `case`. explicit: the gradient goes through q_loss_f64's
    term-by-term gq instead of autograd through the loss. `variant`: one of VARIANTS, a wrong implementation."""
    c = case
    B, N, A = c["u"].shape
    x_cand, corr = candidates(c["obs"], c["params_cur"], c["params_next"], c["u"], c["eps"],
                              next_obs=c["next_obs"] if variant == "next_at_next_state" else None,
                              unif_sign=-1.0 if variant == "unif_sign" else 1.0)
    x = th.as_tensor(np.concatenate([np.concatenate([c["obs"], c["act"]], 1), x_cand], 0))
    params = [[p.clone().requires_grad_(True) for p in net] for net in c["critics"]]
    q = th.stack([(th.tanh(x @ w1 + b1) @ w2 + b2)[:, 0] for w1, b1, w2, b2 in params])
    with_data = not c["importance"]
    corr_used = corr if c["importance"] else None
    next_logp = c["next_logp"] if (c["backup_entropy"] or variant == "entropy_in_target") else None
    w, T = c["w"], c["T"]
    flat = [p for net in params for p in net]
    if explicit and variant is None:
        r = q_loss_f64(q.detach().numpy(), corr_used, with_data, c["q1_t"], c["q2_t"], next_logp, c["rew"], c["done"], c["ent_coef"], c["gamma"], w, T)
        grads = th.autograd.grad(q, flat, grad_outputs=th.as_tensor(r["gq"]))
        return dict(loss=r["loss"], aux=r["aux"], target=r["target"], grads=np.concatenate([g.numpy().reshape(-1) for g in grads]))
    t = th.as_tensor(td_target_f64(c["q1_t"], c["q2_t"], next_logp, c["rew"], c["done"], c["ent_coef"], c["gamma"]))
    corr_t = None if corr_used is None else th.as_tensor(corr_used)
    bell, cons, lses, gq_fix = 0.0, 0.0, [], []
    for i in range(2):
        qd = q[i, :B]
        cm = q[i, B:].reshape(3 * N, B).t() if variant == "sample_major" else q[i, B:].reshape(B, 3 * N)
        if corr_t is not None:
            cm = cm + corr_t if variant == "corr_added" else cm - corr_t
        if with_data:
            cm = th.cat([cm, qd[:, None]], dim=1)
        lse = th.logsumexp(cm / T, dim=1) * (1.0 if variant == "lse_no_T" else T)
        lses.append(lse)
        bell = bell + 0.5 * F.mse_loss(qd, t)
        term = lse.mean() - (0.0 if variant == "no_q_data_term" else qd.mean())
        cons = cons + (1.0 if variant == "half_on_one_term" else 0.5) * w * term
        if variant in ("softmax_no_temp", "no_1_over_B_cand"):  # mistakes of the explicit gradient: the loss value stays right
            p = th.softmax(cm.detach() / (1.0 if variant == "softmax_no_temp" else T), dim=1)
            k = 0.5 * w * (1.0 if variant == "no_1_over_B_cand" else 1.0 / B)
            g = th.zeros_like(q[i])
            g[:B] = 0.5 * (2 * (qd.detach() - t) / B - w / B) + (0.5 * w / B * p[:, 3 * N] if with_data else 0.0)
            g[B:] = (k * p[:, :3 * N]).reshape(-1)
            gq_fix.append(g)
    loss = bell + cons
    if gq_fix:
        grads = th.autograd.grad(q, flat, grad_outputs=th.stack(gq_fix))
    else:
        grads = th.autograd.grad(loss, flat)
    lse = th.stack(lses).detach()
    aux = np.array([float(bell.detach()), float(cons.detach()), float(lse.mean()), float(q[:, :B].detach().mean())])
    return dict(loss=float(loss.detach()), aux=aux, target=t.numpy(), grads=np.concatenate([g.numpy().reshape(-1) for g in grads]))


def same_step(got: dict, want: dict, rtol: float = 1e-9) -> bool:
    """The comparator: loss, the four scalars, the TD target and the critics' parameter gradients agree to `rtol` of their scale."""
    if not abs(got["loss"] - want["loss"]) <= rtol * max(abs(want["loss"]), 1e-12):
        return False
    for k in ("aux", "target", "grads"):
        scale = float(np.abs(want[k]).max())
        if not np.abs(got[k] - want[k]).max() <= rtol * max(scale, 1e-300):
            return False
    return True


def gq_floor(q, corr, with_data, q1_t, q2_t, next_logp, rew, done, ent_coef, gamma, w, T) -> np.ndarray:
    """[2, (1 + 3N) B]: what the float32 arithmetic of the statement can move an element of gq by, whatever evaluates it: the part of the
    element-wise bar that does not depend on the luck of one float32 evaluation (torch's distance from fp64 can be zero for an element).
    One rounding moves a value x by at most u |x|, u = 2^-24.
      a candidate row, gq = ((0.5 w) / B) e_j / s with e_j = exp(z_j - m), z = (q - corr) / T: the subtraction and the division each move
        z_j by u |z_j| and z_j - m moves it by u |z_j - m|, all of which exp turns into relative error; expf itself 2 u. The sum s carries
        the same for its dominant entries (at most 2 u max_j |z_j| + 2 u) and six butterfly additions (6 u); then the division, (0.5 w) / B
        (two roundings) and the product (4 u). Together (2 |z_j| + |z_j - m| + 2 max_j |z_j| + 16) u <= (16 + 4 max_j |z_j| + |z_j - m|) u
        of the element.
      a data row, gq = (1 / B) (q - t) - (0.5 w) / B (+ ((0.5 w) / B) share of the appended entry): the float32 target's chain -- ent_coef *
        logp', the subtraction from min Qt, (1 - d) * gamma * (.) with gamma itself rounded to float32, the addition of r -- moves t by at
        most u (|r| + 5 (|min Qt| + |ent_coef logp'|)), and q - t is rounded once more; then three roundings of terms no larger than
        |q - t| / B + (0.5 w) / B, and the share's own relative error as above."""
    u = 2.0 ** -24
    q = np.asarray(q, np.float64).reshape(2, -1)
    t = td_target_f64(q1_t, q2_t, next_logp, rew, done, ent_coef, gamma)
    B = t.shape[0]
    n3 = q.shape[1] // B - 1
    qn = np.abs(np.minimum(np.asarray(q1_t, np.float64).reshape(-1), np.asarray(q2_t, np.float64).reshape(-1)))
    ent = np.abs(float(ent_coef) * np.asarray(next_logp, np.float64).reshape(-1)) if next_logp is not None else 0.0
    t_abs = np.abs(np.asarray(rew, np.float64).reshape(-1)) + 5 * (qn + ent)
    hw = 0.5 * w / B
    out = np.zeros_like(q)
    for i in range(2):
        qd, c = q[i, :B], q[i, B:].reshape(B, n3)
        c = c - np.asarray(corr, np.float64) if corr is not None else c
        if with_data:
            c = np.concatenate([c, qd[:, None]], axis=1)
        z = c / T
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.nanmax(z, axis=1, keepdims=True)
            p = np.exp(z - m)
            p = p / np.nansum(p, axis=1, keepdims=True)
            rel = (16 + 4 * np.nanmax(np.abs(z), axis=1, keepdims=True) + np.abs(z - m)) * u
        out[i, B:] = (hw * p[:, :n3] * rel[:, :n3]).reshape(-1)
        out[i, :B] = u / B * (np.abs(qd) + t_abs + np.abs(qd - t)) + 3 * 2 * u * (np.abs(qd - t) / B + hw)
        if with_data:
            out[i, :B] += hw * p[:, n3] * rel[:, n3]
    return np.nan_to_num(out, nan=0.0, posinf=0.0)


def close(got, want, aten, floor_ulp: float = 2.0, floor=None):
    """The element-wise bar of the loss launch: |got - want| <= max(4 |aten - want|, floor_ulp float32 ulps of want + floor), `floor` =
    `gq_floor`'s per-element conditioning (absolute), or nothing. Returns the worst ratio err / bar (NaN patterns must agree)."""
    got, want, aten = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, aten))
    floor = np.zeros_like(want) if floor is None else np.asarray(floor, np.float64).reshape(-1)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    if nan.all():
        return 0.0
    g, w_, a = got[~nan], want[~nan], aten[~nan]
    bar = np.maximum(4 * np.abs(a - w_), floor_ulp * np.spacing(np.abs(w_).astype(np.float32)).astype(np.float64) + floor[~nan])
    bar = np.where(np.isfinite(bar), bar, np.inf)
    err = np.abs(g - w_)
    err = np.where(np.isnan(err), 0.0, err)  # inf - inf of equal infinities
    same_inf = np.isinf(w_) & (g == w_)
    return float(np.where(same_inf, 0.0, err / np.maximum(bar, 1e-300)).max())


# ---- whole gradient steps ------------------------------------------------------------------------------------------------------------
def synthetic_dataset(rows=20_000, seed=0) -> dict:
    """BCQ's synthetic dataset: actions = clip(tanh(obs K) + N(0, 0.05)), default_rng(seed)"""
    rng = np.random.default_rng(seed)
    K = rng.normal(0, 0.8, (4, 2))
    obs = rng.uniform(-1, 1, (rows, 4))
    act = np.clip(np.tanh(obs @ K) + rng.normal(0, 0.05, (rows, 2)), -1, 1)
    nobs = np.clip(obs + rng.normal(0, 0.05, (rows, 4)), -1, 1)
    rew = rng.uniform(-8, 0, rows)
    done = (rng.uniform(size=rows) < 0.05).astype(np.float64)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(observations=f(obs), next_observations=f(nobs), actions=f(act), rewards=f(rew), dones=f(done), K=K)


def _dist_params(actor, obs):
    h = actor.latent_pi(obs)
    return actor.mu(h), actor.log_std(h)


def _sample(mean, raw, eps):
    sd = raw.clamp(LOG_STD_MIN, LOG_STD_MAX).exp()
    g = mean + sd * eps
    a = th.tanh(g)
    lp = (-((g - mean) ** 2) / (2 * sd ** 2) - sd.log() - HALF_LOG_2PI).sum(-1)
    return a, lp - th.log(1 - a ** 2 + 1e-6).sum(-1)


def _q(critic, x):
    return tuple(q(x) for q in critic.q_networks)


class RefCQL:
    """Whole CQL gradient steps in plain torch fp64 on the CPU, started from a model's weights. `policy` is a float64 copy of the
    model's SACPolicy modules (actor, critic, critic_target)."""

    def __init__(self, policy, lr, gamma, tau, w, N, T, importance=True, backup_entropy=False, log_ent_coef=0.0, target_entropy=-2.0,
                 learn_ent_coef=True, dtype=th.float64):
        """dtype: float64 is the reference; float32 (with a float32 `policy`) is the plain torch statement, whose distance from the
        reference says what a bar asks of float32 arithmetic"""
        self.dtype, self.np_dtype = dtype, (np.float64 if dtype == th.float64 else np.float32)
        self.p, self.gamma, self.tau, self.w, self.N, self.T = policy, gamma, tau, w, N, T
        self.importance, self.backup_entropy, self.target_entropy = importance, backup_entropy, target_entropy
        self.log_ent_coef = th.tensor([float(log_ent_coef)], dtype=dtype, requires_grad=learn_ent_coef)
        self.actor_opt = th.optim.Adam(policy.actor.parameters(), lr=lr)
        self.critic_opt = th.optim.Adam(policy.critic.parameters(), lr=lr)
        self.ent_opt = th.optim.Adam([self.log_ent_coef], lr=lr) if learn_ent_coef else None

    def critic_terms(self, obs, act, x_cand, corr, target):
        B, n3 = obs.shape[0], 3 * self.N
        q_all = _q(self.p.critic, th.cat([th.cat([obs, act], 1), x_cand], 0))
        bell = cons = 0.0
        lses = []
        for q in q_all:
            qd, c = q[:B], q[B:].reshape(B, n3)
            c = c - corr if self.importance else th.cat([c, qd], dim=1)
            lse = self.T * th.logsumexp(c / self.T, dim=1)
            lses.append(lse)
            bell = bell + 0.5 * F.mse_loss(qd, target)
            cons = cons + 0.5 * self.w * (lse.mean() - qd.mean())
        return q_all, bell, cons, th.stack(lses)

    def step(self, obs, act, next_obs, rew, done, eps_pi, eps_next, u, eps) -> dict:
        p, N = self.p, self.N
        obs, act, next_obs, rew, done, eps_pi, eps_next, u, eps = (th.as_tensor(np.asarray(x, self.np_dtype)) for x in
                                                                   (obs, act, next_obs, rew, done, eps_pi, eps_next, u, eps))
        rew, done = rew.reshape(-1, 1), done.reshape(-1, 1)
        B = obs.shape[0]
        mean, raw = _dist_params(p.actor, obs)
        a_pi, logp = _sample(mean, raw, eps_pi)
        logp = logp.reshape(-1, 1)
        ent_coef = th.exp(self.log_ent_coef.detach())
        out = {}
        if self.ent_opt is not None:
            ent_loss = -(self.log_ent_coef * (logp + self.target_entropy).detach()).mean()
            self.ent_opt.zero_grad()
            ent_loss.backward()
            self.ent_opt.step()
            out["ent_coef_loss"] = ent_loss.item()
        with th.no_grad():
            mean_n, raw_n = _dist_params(p.actor, next_obs)
            a_n, logp_n = _sample(mean_n, raw_n, eps_next)
            next_q, _ = th.min(th.cat(_q(p.critic_target, th.cat([next_obs, a_n], 1)), dim=1), dim=1, keepdim=True)
            if self.backup_entropy:
                next_q = next_q - ent_coef * logp_n.reshape(-1, 1)
            target = rew + (1 - done) * self.gamma * next_q
            a_cur, lp_cur = _sample(mean.detach()[:, None], raw.detach()[:, None], eps[:, :N])
            a_nxt, lp_nxt = _sample(mean_n[:, None], raw_n[:, None], eps[:, N:])
            cand = th.cat([u, a_cur, a_nxt], dim=1)
            corr = th.cat([th.full((B, N), u.shape[2] * math.log(0.5), dtype=self.dtype), lp_cur, lp_nxt], dim=1)
            x_cand = th.cat([obs[:, None, :].expand(B, 3 * N, -1), cand], dim=2).reshape(B * 3 * N, -1)
        q_all, bell, cons, lse = self.critic_terms(obs, act, x_cand, corr, target)
        critic_loss = bell + cons
        self.critic_opt.zero_grad()
        critic_loss.backward()
        self.critic_opt.step()
        q_pi = th.cat(_q(p.critic, th.cat([obs, a_pi], 1)), dim=1)
        actor_loss = (ent_coef * logp - th.min(q_pi, dim=1, keepdim=True)[0]).mean()
        self.actor_opt.zero_grad()
        actor_loss.backward()
        self.actor_opt.step()
        with th.no_grad():
            for s, d in zip(p.critic.parameters(), p.critic_target.parameters()):
                d.mul_(1.0 - self.tau).add_(s, alpha=self.tau)
        out.update(target_q=target.numpy().copy(), current_q=[q[:B].detach().numpy().copy() for q in q_all],
                   q_all=np.stack([q.detach().numpy()[:, 0] for q in q_all]), x_cand=x_cand.numpy().copy(), corr=corr.numpy().copy(),
                   critic_loss=critic_loss.item(), actor_loss=actor_loss.item(), ent_coef=ent_coef.item(), log_prob=logp.detach().numpy().copy(),
                   aux=np.array([bell.item(), cons.item(), lse.mean().item(), sum(q[:B].mean().item() for q in q_all) / len(q_all)]))
        return out


def dataset_gap(policy, data: dict, N: int, T: float, rows: int = 2048, seed: int = 123) -> float:
    """The mean over the first `rows` dataset rows and both critics of lse - Q(s, a) (importance-sampled form), with candidates from a
    fixed seeded draw: the quantity the conservative term pushes down."""
    g = th.Generator().manual_seed(seed)
    obs, act, nobs = (th.as_tensor(np.asarray(data[k][:rows], np.float64)) for k in ("observations", "actions", "next_observations"))
    B, A = act.shape
    u = th.rand(B, N, A, generator=g, dtype=th.float64) * 2 - 1
    eps = th.randn(B, 2 * N, A, generator=g, dtype=th.float64)
    with th.no_grad():
        mean, raw = _dist_params(policy.actor, obs)
        mean_n, raw_n = _dist_params(policy.actor, nobs)
        a_cur, lp_cur = _sample(mean[:, None], raw[:, None], eps[:, :N])
        a_nxt, lp_nxt = _sample(mean_n[:, None], raw_n[:, None], eps[:, N:])
        cand = th.cat([u, a_cur, a_nxt], dim=1)
        corr = th.cat([th.full((B, N), A * math.log(0.5), dtype=th.float64), lp_cur, lp_nxt], dim=1)
        x_cand = th.cat([obs[:, None, :].expand(B, 3 * N, -1), cand], dim=2).reshape(B * 3 * N, -1)
        gaps = []
        for q in _q(policy.critic, th.cat([th.cat([obs, act], 1), x_cand], 0)):
            lse = T * th.logsumexp((q[B:].reshape(B, 3 * N) - corr) / T, dim=1)
            gaps.append((lse - q[:B, 0]).mean().item())
    return float(np.mean(gaps))


# the conservative-effect case of tests/test_cql_abi.py (the reference alone) and tests/test_cql.py (the kernels)
GAP_ARGS = dict(steps=200, arch=(32, 32), B=64, N=4, T=1.0, seed=0, lr=3e-3)


def train_reference(data: dict, w: float, steps: int, arch=(32, 32), B: int = 64, N: int = 4, T: float = 1.0, seed: int = 0, lr: float = 3e-4):
    """A seeded SACPolicy in fp64 trained for `steps` reference steps on seeded batches of `data` -> the policy"""
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.sac.policies import SACPolicy

    set_random_seed(seed)
    pol = SACPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: lr, net_arch=list(arch)).double()
    refm = RefCQL(pol, lr, 0.99, 0.005, w, N, T)
    rng = np.random.default_rng(seed + 1)
    rows = data["rewards"].shape[0]
    for _ in range(steps):
        idx = rng.integers(0, rows, B)
        refm.step(data["observations"][idx], data["actions"][idx], data["next_observations"][idx], data["rewards"][idx], data["dones"][idx],
                  rng.normal(size=(B, 2)), rng.normal(size=(B, 2)), rng.uniform(-1, 1, (B, N, 2)), rng.normal(size=(B, 2 * N, 2)))
    return pol
