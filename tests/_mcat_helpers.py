"""What the MultiCategorical tests share (tests/test_multicategorical_abi.py checks the fp64 restatement on the CPU against the
reference-written fixtures before tests/test_multicategorical.py uses it as the yardstick on the GPU): the th.split layout, the fp64
log-softmax per valve, the valve values of a level pair, the Philox4x32-10 uniforms of cstr_multicategorical_act_f32 and the
reference's loss statements (core/ppo/ppo.py:213-264, core/a2c/a2c.py:150-171) on one torch Categorical per valve."""
import warnings

import numpy as np
import torch as th

from _dqn_helpers import philox4x32_10, valve_np

NVECS = ((2, 2), (3, 5), (16, 16), (31, 32), (32, 2))  # both bounds, an unequal pair either way, a prime, a half not filled
ROWS = (1, 3, 5, 1030)  # one wave, a partial workgroup, two workgroups, more than one pass of both launches' grids
MCAT_STREAM_TAG = 0x3CA7A11C  # csrc/cstr_multicategorical.hip
U24 = 2.0 ** -24


def split(z, nvec):
    """th.split order: valve 0's columns, then valve 1's"""
    return z[:, :nvec[0]], z[:, nvec[0]:nvec[0] + nvec[1]]


def logp64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    return z - lse, lse


def pair_logp64(z, nvec, pairs):
    """-> (fp64 log-prob of the pairs [n], the magnitude behind it [n] = sum over the valves of |z_a| + |logsumexp z|)"""
    r = np.arange(len(pairs))
    lp_sum, mag = np.zeros(len(pairs)), np.zeros(len(pairs))
    for g, zg in enumerate(split(z, nvec)):
        lp, lse = logp64(zg)
        lp_sum += lp[r, pairs[:, g]]
        mag += np.abs(np.asarray(zg, np.float64)[r, pairs[:, g]]) + np.abs(lse[:, 0])
    return lp_sum, mag


def logp_units(got, z, nvec, pairs):
    """test_categorical.logp_units on the pair: |got - want| / (2**-24 M), M the sum of the additive terms' magnitudes"""
    want, mag = pair_logp64(z, nvec, np.asarray(pairs))
    return np.abs(np.asarray(got, np.float64) - want) / (U24 * mag)


def head_case(n, nvec, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, nvec[0] + nvec[1])) * scale).astype(np.float32)


def valves_np(pairs, nvec):
    """(v_0(a_0), v_1(a_1)) in float32: the statement of CSTRVecEnv(multi_discrete_actions=...)"""
    pairs = np.asarray(pairs, np.int64)
    return np.stack([valve_np(pairs[:, 0], nvec[0]), valve_np(pairs[:, 1], nvec[1])], axis=-1).astype(np.float32)


def mcat_uniforms(seed, base, n):
    """u [n, 2] as cstr_multicategorical_act_f32 draws them: counter (base + row, 0, tag), key = seed; words 0 and 1 of the one
    block, each >> 8 times 2^-24"""
    ctr = np.uint64(base) + np.arange(n, dtype=np.uint64)
    c = np.zeros((n, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 3] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32), MCAT_STREAM_TAG
    x = philox4x32_10(c, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    return ((x[:, :2] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def loss_case(B, nvec, seed):
    rng = np.random.default_rng(seed)
    K0, K1 = nvec
    z = rng.normal(size=(B, K0 + K1)).astype(np.float32)
    a = np.stack([rng.integers(0, K0, B), rng.integers(0, K1, B)], axis=1)
    a[0] = (0, K1 - 1)
    a[-1] = (K0 - 1, 0)
    if B > 2:
        z[1, a[1, 0]] = 30.0                      # a saturated softmax on valve 0's taken level
        z[2, K0 + (a[2, 1] + 1) % K1] = 30.0      # ... and on a level of valve 1 that was not taken
    lp, _ = pair_logp64(z, nvec, a)
    old_lp = (lp + rng.normal(size=B) * 0.25).astype(np.float32)  # ratios on both sides of the clip range
    f = lambda: rng.normal(size=B).astype(np.float32)  # noqa: E731
    return dict(z=z, a=a, old_lp=old_lp, values=f(), old_values=f(), adv=f(), returns=f())


def loss_torch(c, nvec, objective, dtype, norm, ent_coef, vf_coef, clip_range=0.2, clip_range_vf=None):
    """test_categorical.loss_torch with the reference's MultiCategoricalDistribution (distributions.py:314-368: one Categorical per
    th.split, log-probs and entropies stacked and summed) -> (scalars, g_logits, g_value, log_prob, mags), the same tuple and the same
    magnitudes, the log-prob's being the sum over the valves of |z_a| + |logsumexp z|."""
    t = lambda x: th.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    z, values = t(c["z"]).requires_grad_(True), t(c["values"]).requires_grad_(True)
    actions = t(c["a"].astype(np.float32))
    dists = [th.distributions.Categorical(logits=s) for s in th.split(z, list(nvec), dim=1)]
    log_prob = th.stack([d.log_prob(a.long()) for d, a in zip(dists, th.unbind(actions, dim=1))], dim=1).sum(dim=1)
    entropy = th.stack([d.entropy() for d in dists], dim=1).sum(dim=1)
    adv, returns = t(c["adv"]), t(c["returns"])
    with th.no_grad():
        normed = norm and len(adv) > 1
        amag = (adv.abs() + adv.mean().abs()) / (adv.std() + 1e-8) if normed else adv.abs()
        lmag = sum(s.detach().gather(1, a.long().reshape(-1, 1)).reshape(-1).abs() + th.logsumexp(s.detach(), dim=1).abs()
                   for s, a in zip(th.split(z, list(nvec), dim=1), th.unbind(actions, dim=1)))
    if objective == 0:
        if norm and len(adv) > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = th.exp(log_prob - t(c["old_lp"]))
        pl1, pl2 = adv * ratio, adv * th.clamp(ratio, 1 - clip_range, 1 + clip_range)
        policy_loss = -th.min(pl1, pl2).mean()
        clip_fraction = th.mean((th.abs(ratio - 1) > clip_range).to(dtype))
        vp = values if clip_range_vf is None else t(c["old_values"]) + th.clamp(values - t(c["old_values"]), -clip_range_vf, clip_range_vf)
        value_loss = th.nn.functional.mse_loss(returns, vp)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
        lr = (log_prob - t(c["old_lp"])).detach()
        scalars = [policy_loss, value_loss, entropy_loss, loss, th.mean((th.exp(lr) - 1) - lr), clip_fraction]
        with th.no_grad():
            r = ratio.detach()
            cond = 1 + lmag + t(c["old_lp"]).abs()  # the exponent logp - old_logp carries 2**-24 of each operand into the ratio
            dr = (returns - vp).abs()
            m0 = (amag * th.maximum(r, th.clamp(r, 1 - clip_range, 1 + clip_range)) * cond).mean()
            m1 = value_loss + 2 * (dr * (returns.abs() + vp.abs())).mean()
            m4 = ((r - 1).abs() + lr.abs() + (r - 1).abs() * cond).mean()
            near = ((r - 1).abs() - clip_range).abs() < 1e-4  # a ratio on a clip bound may count either way
            mags = [m0, m1, entropy_loss.abs(), m0 + ent_coef * entropy_loss.abs() + vf_coef * m1, m4, near.to(dtype).mean()]
    else:
        if norm:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # torch.std of one element warns and gives NaN: the case under test
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        policy_loss = -(adv * log_prob).mean()
        value_loss = th.nn.functional.mse_loss(returns, values)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
        scalars = [policy_loss, value_loss, entropy_loss, loss]
        with th.no_grad():
            m0 = (amag * lmag).mean()
            m1 = value_loss + 2 * ((returns - values).abs() * (returns.abs() + values.abs())).mean()
            mags = [m0, m1, entropy_loss.abs(), m0 + ent_coef * entropy_loss.abs() + vf_coef * m1]
    loss.backward()
    return (np.array([float(s.detach()) for s in scalars]), z.grad.numpy().astype(np.float64), values.grad.numpy().astype(np.float64),
            log_prob.detach().numpy().astype(np.float64), np.array([float(m) for m in mags]))
