"""Reference statements of IQL (Kostrikov, Nair & Levine 2021) for tests/test_iql_abi.py and tests/test_iql.py:

  * `loss_f64`: everything cstr_iql_loss_f32 computes, in NumPy float64 with EXPLICIT gradients (no autograd);
  * `loss_torch`: the same as torch statements in any dtype, gradients by autograd (float64: the check of the explicit gradients;
    float32: the "ATen distance" of the element-wise bar);
  * `floors`: what float32 arithmetic can move each output by whatever evaluates it, rounding by rounding (the conditioning part of the
    element-wise bar); `close` is tests/_cql_reference.py's comparator: |got - want| <= max(4 |aten - want|, 2 ulp + floor);
  * `small_case`, `step_f64`, `same_step`: a small fp64 step with mixed-sign u, clipped and unclipped weights, an action at exactly
    +-1 and raw log-stds beyond both clamp bounds, the mistakes a wrong implementation makes as `variant`s, and the comparator that
    must reject each of them;
  * `RefIQL`: whole gradient steps in plain torch (fp64 the reference, fp32 the plain statement), `train_reference` / `dataset_value`
    the expectile-ordering experiment."""
import math

import numpy as np
import torch as th
from torch.nn import functional as F

from _cql_reference import close, synthetic_dataset  # noqa: F401  (re-exported: the comparator and BCQ's synthetic dataset)

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = math.log(math.sqrt(2 * math.pi))
EPS32 = float(np.finfo(np.float32).eps)

VARIANTS = ("expectile_swapped", "u_sign", "max_target", "v_in_target", "done_flipped", "w_unclipped", "w_not_detached", "beta_in_clip_only",
            "clamped_action_in_correction", "correction_added", "clamp_mask_open", "loss_mean_w_mean_logp")


def _f64(*xs):
    return tuple(np.asarray(x, np.float64) for x in xs)


def loss_f64(qt1, qt2, v, v_next, q1, q2, params, act, rew, done, gamma, expectile, beta, exp_adv_max) -> dict:
    """The statement of core/iql/iql.py with explicit gradients. Vectors [B], params [B, 2A] = [mean | raw log_std], act [B, A]."""
    qt1, qt2, v, v_next, q1, q2, params, act, rew, done = _f64(qt1, qt2, v, v_next, q1, q2, params, act, rew, done)
    qt1, qt2, v, v_next, q1, q2, rew, done = (x.reshape(-1) for x in (qt1, qt2, v, v_next, q1, q2, rew, done))
    B, A = act.shape
    mean, raw = params[:, :A], params[:, A:]
    with np.errstate(all="ignore"):
        u = np.minimum(qt1, qt2) - v  # np.minimum propagates NaN, as th.min
        we = np.where(u < 0, 1.0 - expectile, expectile)
        g_v = -2.0 * we * u / B
        y = rew + (1.0 - done) * gamma * v_next
        gq1, gq2 = (q1 - y) / B, (q2 - y) / B
        e = np.exp(beta * u)
        clipped = e > exp_adv_max
        w = np.where(clipped, exp_adv_max, e)
        x = np.where(np.isnan(act), act, np.clip(act, -1.0 + EPS32, 1.0 - EPS32))
        g = 0.5 * (np.log1p(x) - np.log1p(-x))
        ls = np.where(np.isnan(raw), raw, np.clip(raw, LOG_STD_MIN, LOG_STD_MAX))
        var = np.exp(2.0 * ls)
        d = g - mean
        logp = (-(d ** 2) / (2.0 * var) - ls - HALF_LOG_2PI).sum(axis=1) - np.log(1.0 - act ** 2 + 1e-6).sum(axis=1)
        c = (w / B)[:, None]
        g_mean = -c * d / var
        inside = (raw >= LOG_STD_MIN) & (raw <= LOG_STD_MAX)
        g_ls = np.where(inside, -c * (d ** 2 / var - 1.0), 0.0)
        losses = np.array([(we * u ** 2).mean(), 0.5 * (((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean()), (-w * logp).mean()])
        aux = np.array([u.mean(), w.mean(), clipped.mean(), logp.mean(), v.mean(), y.mean()])
    return dict(u=u, g_v=g_v, y=y, gq1=gq1, gq2=gq2, w=w, clipped=clipped, logp=logp, g_params=np.concatenate([g_mean, g_ls], axis=1),
                losses=losses, aux=aux)


def _logp_torch(mean, raw, act, variant=None):
    eps = EPS32
    a = act.clamp(-1.0 + eps, 1.0 - eps)
    g = 0.5 * (a.log1p() - (-a).log1p())
    ls = raw.clamp(LOG_STD_MIN, LOG_STD_MAX)
    if variant == "clamp_mask_open":  # the clamp's value, the identity's gradient
        ls = raw + (ls - raw).detach()
    std = ls.exp()
    lp = (-((g - mean) ** 2) / (2 * std ** 2) - std.log() - HALF_LOG_2PI).sum(dim=1)
    corr = th.log(1 - (a if variant == "clamped_action_in_correction" else act) ** 2 + 1e-6).sum(dim=1)
    return lp + corr if variant == "correction_added" else lp - corr


def loss_torch(qt1, qt2, v, v_next, q1, q2, params, act, rew, done, gamma, expectile, beta, exp_adv_max, dtype=th.float64, variant=None) -> dict:
    """The statement as a user would write it in torch, evaluated in `dtype`; the gradients are autograd's: g_v of the SUM of the three
    losses w.r.t. v (the actor term contributes nothing: w is a constant), gq of the critic loss, g_params of the actor loss.
    `variant`: one of VARIANTS, a wrong implementation."""
    t = lambda x: th.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    qt1, qt2, v, v_next, q1, q2, rew, done = (t(x).reshape(-1) for x in (qt1, qt2, v, v_next, q1, q2, rew, done))
    params, act = t(params), t(act)
    A = act.shape[1]
    v, q1, q2, params = (x.clone().requires_grad_(True) for x in (v, q1, q2, params))
    qt = th.max(qt1, qt2) if variant == "max_target" else th.min(qt1, qt2)
    u = v - qt if variant == "u_sign" else qt - v
    neg = (u < 0).to(dtype)
    we = th.abs(expectile - (1 - neg if variant == "expectile_swapped" else neg))
    value_loss = (we * u ** 2).mean()
    vt = v.detach() if variant == "v_in_target" else v_next
    y = rew + (done if variant == "done_flipped" else 1 - done) * gamma * vt
    critic_loss = 0.5 * (F.mse_loss(q1, y) + F.mse_loss(q2, y))
    ud = u if variant == "w_not_detached" else u.detach()
    e = th.exp(ud if variant == "beta_in_clip_only" else beta * ud)
    cap = beta * exp_adv_max if variant == "beta_in_clip_only" else exp_adv_max
    w = e if variant == "w_unclipped" else th.clamp(e, max=cap)
    logp = _logp_torch(params[:, :A], params[:, A:], act, variant)
    actor_loss = w.mean() * (-logp).mean() if variant == "loss_mean_w_mean_logp" else (-w * logp).mean()
    g_v, gq1, gq2, g_params = th.autograd.grad(value_loss + critic_loss + actor_loss, (v, q1, q2, params), allow_unused=True)
    n = lambda x: x.detach().to(th.float64).numpy().copy()  # noqa: E731
    return dict(u=n(u), g_v=n(g_v), y=n(y), gq1=n(gq1), gq2=n(gq2), w=n(w), clipped=(n(e) > cap), logp=n(logp), g_params=n(g_params),
                losses=np.array([value_loss.item(), critic_loss.item(), actor_loss.item()]),
                aux=np.array([u.mean().item(), w.mean().item(), (e > cap).to(dtype).mean().item(), logp.mean().item(), v.mean().item(), y.mean().item()]))


def floors(qt1, qt2, v, v_next, q1, q2, params, act, rew, done, gamma, expectile, beta, exp_adv_max) -> dict:
    """Per output, the absolute amount float32 arithmetic can move it by on these float32 inputs, whatever evaluates the statement (the
    part of the element-wise bar that does not depend on the luck of one float32 evaluation). One rounding moves x by at most e |x|,
    e = 2^-24; expf, logf, log1pf are taken as 2 e relative.
      u = qt - v: one rounding, inside the 2 ulp of the bar: no floor. g_v = -(2 we u) / B: we (the float32 expectile, or 1 - it), u, the
        product and the division: 4 e |g_v|.
      y = r + (1 - d) gamma v': gamma rounded to float32, two products, the sum: e (|r| + 5 |v'|) (tests/_cql_reference.py gq_floor).
      gq_i = (q_i - y) / B: y's error and the subtraction over B, then two roundings of the quotient and the scale.
      w = min(exp(beta u), M): beta u carries u's rounding, beta's and the product's, which exp turns into relative error 3 e |beta u|, and
        expf's own 2 e; a clipped w is M itself (e |M| for its float32 value).
      g_k = atanh(x) = 0.5 (log1p(x) - log1p(-x)): 2 e of each logarithm and the subtraction's e. d = g - mean: that and e |d|.
      the Gaussian term -d^2 / (2 sd^2) - log(sd) - c, sd = exp(ls): sd relative 2 e, sd^2 5 e, d^2 one more, the quotient one more, so
        (d^2 / (2 var)) (2 dd / |d| + 8 e); log(sd): 2 e from sd and 2 e |ls|; three additions of the term, e each of the partial sums.
      the correction log(s), s = 1 - a^2 + 1e-6: a^2 and 1 - a^2 are rounded to 2^-24 of 1 each (a^2 <= 1), the last sum once more and
        1e-6 itself is a float32 value: ds = e (2 + 2 s); log(s) moves by ds / s and logf's 2 e |log s|. Near |a| = 1 this is the large one:
        s ~ 1e-6 turns 2^-24 into 0.1 of the row's logp. (a^2 == 1 exactly at a = +-1, where the float32 s is the float32 1e-6.)
      logp: the sum of both, and e |partial sum| for each of the 2 A additions.
      g_mean = -(w / B) (d / var): w's relative error, w / B, d / var (var 5 e, the quotient), the product: |g_mean| (rel_w + 9 e) and
        (w / B) dd / var. g_ls = -(w / B) (d^2 / var - 1): (w / B) [(d^2 / var) (2 dd / |d| + 7 e) + e |d^2 / var - 1|] and |g_ls| (rel_w + 2 e).
      value loss: float64 sum of float32 factors: 3 e of each term; critic loss: float32 accumulation, B / 256 + 10 additions deep, of terms
        (q_i - y)^2 that carry 2 |q_i - y| times the difference's own error; actor loss and aux: the means of the element floors."""
    e = 2.0 ** -24
    ref = loss_f64(qt1, qt2, v, v_next, q1, q2, params, act, rew, done, gamma, expectile, beta, exp_adv_max)
    qt1, qt2, v, v_next, q1, q2, params, act, rew, done = _f64(qt1, qt2, v, v_next, q1, q2, params, act, rew, done)
    v_next, q1, q2, rew = (x.reshape(-1) for x in (v_next, q1, q2, rew))
    B, A = act.shape
    mean, raw = params[:, :A], params[:, A:]
    u, y, w = ref["u"], ref["y"], ref["w"]
    with np.errstate(all="ignore"):
        f_y = e * (np.abs(rew) + 5 * np.abs(v_next))
        f_gq = [(f_y + e * (np.abs(q) + np.abs(q - y))) / B + 6 * e * np.abs(q - y) / B for q in (q1, q2)]
        rel_w = np.where(ref["clipped"], e, (3 * np.abs(beta * u) + 2) * e)
        f_w = w * rel_w
        x = np.clip(act, -1.0 + EPS32, 1.0 - EPS32)
        g = 0.5 * (np.log1p(x) - np.log1p(-x))
        dg = e * (np.abs(np.log1p(x)) + np.abs(np.log1p(-x)) + np.abs(g))
        d = g - mean
        dd = dg + e * np.abs(d)
        ls = np.clip(raw, LOG_STD_MIN, LOG_STD_MAX)
        var = np.exp(2 * ls)
        quad = d ** 2 / (2 * var)
        f_gauss = quad * 8 * e + np.abs(d) * dd / var + 2 * e + 2 * e * np.abs(ls) + 3 * e * (quad + np.abs(ls) + HALF_LOG_2PI)
        s = 1.0 - act ** 2 + 1e-6
        f_corr = e * (2 + 2 * np.abs(s)) / np.abs(s) + 2 * e * np.abs(np.log(np.abs(s)))
        terms = np.abs(quad) + np.abs(ls) + HALF_LOG_2PI + np.abs(np.log(np.abs(s)))
        f_logp = (f_gauss + f_corr).sum(axis=1) + 2 * A * e * terms.sum(axis=1)
        c = (w / B)[:, None]
        g_mean, g_ls = ref["g_params"][:, :A], ref["g_params"][:, A:]
        f_gm = np.abs(g_mean) * (rel_w[:, None] + 9 * e) + c * dd / var
        f_gl = np.where(g_ls != 0, c * (2 * quad * (2 * dd / np.maximum(np.abs(d), 1e-300) + 7 * e) + e * np.abs(2 * quad - 1))
                        + np.abs(g_ls) * (rel_w[:, None] + 2 * e), 0.0)
        depth = B / 256 + 10
        f_critic = 0.5 * sum((2 * np.abs(q - y) * (f_y + e * (np.abs(q) + np.abs(q - y)))).mean() + depth * e * ((q - y) ** 2).mean()
                             for q in (q1, q2))
        f_actor = (np.abs(w) * f_logp + np.abs(ref["logp"]) * f_w).mean()
        f_losses = np.array([3 * e * abs(ref["losses"][0]), f_critic, f_actor])
        f_aux = np.array([e * np.abs(u).mean(), f_w.mean(), 0.0, f_logp.mean(), 0.0, f_y.mean()])
    z = lambda a: np.nan_to_num(a, nan=0.0, posinf=0.0)  # noqa: E731
    return dict(u=np.zeros(B), g_v=z(4 * e * np.abs(ref["g_v"])), y=z(f_y), gq1=z(f_gq[0]), gq2=z(f_gq[1]), w=z(f_w), logp=z(f_logp),
                g_params=z(np.concatenate([f_gm, f_gl], axis=1)), losses=z(f_losses), aux=z(f_aux))


# ---- the comparator and the mistakes ---------------------------------------------------------------------------------------------------
def small_case(B=12, A=2, seed=0) -> dict:
    """u of both signs, about half of the rows with exp(beta u) clipped, row 0 with an action at exactly +1 and -1, rows 1 and 2 with
    raw log-stds beyond the two clamp bounds, dones of both kinds, target critics that differ."""
    rng = np.random.default_rng(seed)
    qt1, qt2 = rng.normal(-3, 1.5, B), rng.normal(-3, 1.5, B)
    v = np.minimum(qt1, qt2) + rng.normal(0, 1.2, B)
    params = np.concatenate([rng.normal(0, 0.5, (B, A)), rng.normal(-1, 0.7, (B, A))], axis=1)
    act = np.tanh(rng.normal(0, 1, (B, A)))
    act[0] = [1.0 if k % 2 == 0 else -1.0 for k in range(A)]
    if B >= 3:
        # below the lower bound sd = exp(-20): the row's mean sits on atanh(a), or (g - mean)^2 / sd^2 ~ 1e17 would be the scale of everything
        x = np.clip(act[1], -1.0 + EPS32, 1.0 - EPS32)
        params[1, :A], params[1, A:] = 0.5 * (np.log1p(x) - np.log1p(-x)), -25.0
        params[2, A:] = 3.5
    done = (np.arange(B) % 3 == 0).astype(np.float64)
    return dict(qt1=qt1, qt2=qt2, v=v, v_next=rng.normal(-3, 1.5, B), q1=rng.normal(-3, 1.5, B), q2=rng.normal(-3, 1.5, B), params=params,
                act=act, rew=rng.uniform(-8, 0, B), done=done, gamma=0.99, expectile=0.7, beta=3.0, exp_adv_max=3.0)


def step_f64(case: dict, variant=None, explicit: bool = False) -> dict:
    return loss_f64(**case) if explicit else loss_torch(**case, variant=variant)


def same_step(got: dict, want: dict, rtol: float = 1e-9) -> bool:
    """The comparator: the three losses, u, w, y, logp and the four gradients agree to `rtol` of their scale."""
    for k in ("losses", "u", "w", "y", "logp", "g_v", "gq1", "gq2", "g_params"):
        scale = float(np.abs(want[k]).max())
        if not np.abs(got[k] - want[k]).max() <= rtol * max(scale, 1e-300):
            return False
    return True


# ---- whole gradient steps --------------------------------------------------------------------------------------------------------------
def _q(critic, x):
    return tuple(q(x) for q in critic.q_networks)


class RefIQL:
    """Whole IQL gradient steps in plain torch on the CPU, started from a model's weights. `policy` is a float64 (or float32) copy of
    the model's IQLPolicy modules (actor, critic, critic_target, value_net). Every loss is evaluated before any optimiser step."""

    def __init__(self, policy, lr, gamma, tau, expectile, beta, exp_adv_max, target_update_interval: int = 1, dtype=th.float64):
        self.dtype, self.np_dtype = dtype, (np.float64 if dtype == th.float64 else np.float32)
        self.p, self.gamma, self.tau, self.expectile, self.beta, self.M = policy, gamma, tau, expectile, beta, exp_adv_max
        self.interval, self.n = target_update_interval, 0
        self.opts = [th.optim.Adam(m.parameters(), lr=lr) for m in (policy.value_net, policy.critic, policy.actor)]

    def step(self, obs, act, next_obs, rew, done) -> dict:
        p = self.p
        obs, act, next_obs, rew, done = (th.as_tensor(np.asarray(x, self.np_dtype)) for x in (obs, act, next_obs, rew, done))
        rew, done = rew.reshape(-1, 1), done.reshape(-1, 1)
        x = th.cat([obs, act], dim=1)
        with th.no_grad():
            qt, _ = th.min(th.cat(_q(p.critic_target, x), dim=1), dim=1, keepdim=True)
            v_next = p.value_net.v_net(next_obs)
        v = p.value_net.v_net(obs)
        u = qt - v
        value_loss = (th.abs(self.expectile - (u < 0).to(self.dtype)) * u ** 2).mean()
        y = rew + (1 - done) * self.gamma * v_next
        qs = _q(p.critic, x)
        critic_loss = 0.5 * sum(F.mse_loss(q, y) for q in qs)
        w = th.clamp(th.exp(self.beta * u.detach()), max=self.M)
        h = p.actor.latent_pi(obs)
        logp = _logp_torch(p.actor.mu(h), p.actor.log_std(h), act).reshape(-1, 1)
        actor_loss = (-w * logp).mean()
        for opt, loss in zip(self.opts, (value_loss, critic_loss, actor_loss)):
            opt.zero_grad()
            loss.backward()
        for opt in self.opts:
            opt.step()
        if self.n % self.interval == 0:
            with th.no_grad():
                for s, d in zip(p.critic.parameters(), p.critic_target.parameters()):
                    d.mul_(1.0 - self.tau).add_(s, alpha=self.tau)
        self.n += 1
        n = lambda t: t.detach().to(th.float64).numpy().reshape(-1).copy()  # noqa: E731
        return dict(u=n(u), w=n(w), y=n(y), logp=n(logp), q=[n(q) for q in qs], v=n(v),
                    losses=np.array([value_loss.item(), critic_loss.item(), actor_loss.item()]))


def make_policy(seed: int = 0, arch=(256, 256), lr: float = 3e-4):
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.iql.policies import IQLPolicy

    set_random_seed(seed)
    return IQLPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: lr, net_arch=list(arch))


def dataset_value(policy, data: dict, rows: int = 2048) -> float:
    """the mean of V over the first `rows` dataset observations"""
    dt = next(policy.value_net.parameters()).dtype
    with th.no_grad():
        return float(policy.value_net.v_net(th.as_tensor(np.asarray(data["observations"][:rows])).to(dt)).mean())


def ordering_dataset(rows=4096, seed=0) -> dict:
    """The expectile-ordering dataset: actions uniform in (-1, 1)^2 whatever the state, reward -4 + 3 a_0, so that Q(s, .) spreads over the
    dataset actions of a state and an expectile of it is not its mean; default_rng(seed)"""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (rows, 4))
    act = rng.uniform(-1, 1, (rows, 2))
    nobs = np.clip(obs + rng.normal(0, 0.05, (rows, 4)), -1, 1)
    done = (rng.uniform(size=rows) < 0.05).astype(np.float64)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(observations=f(obs), next_observations=f(nobs), actions=f(act), rewards=f(-4.0 + 3.0 * act[:, 0]), dones=f(done))


# the expectile-ordering case of tests/test_iql_abi.py (the reference alone) and tests/test_iql.py (the device path)
ORDER_ARGS = dict(steps=300, arch=(32, 32), B=64, seed=0, lr=3e-3)


def train_reference(data: dict, expectile: float, steps: int, arch=(32, 32), B: int = 64, seed: int = 0, lr: float = 3e-4, beta: float = 3.0,
                    exp_adv_max: float = 100.0):
    """A seeded IQLPolicy in fp64 trained for `steps` reference steps on seeded batches of `data` -> the policy"""
    pol = make_policy(seed, arch, lr).double()
    refm = RefIQL(pol, lr, 0.99, 0.005, expectile, beta, exp_adv_max)
    rng = np.random.default_rng(seed + 1)
    rows = data["rewards"].shape[0]
    for _ in range(steps):
        idx = rng.integers(0, rows, B)
        refm.step(data["observations"][idx], data["actions"][idx], data["next_observations"][idx], data["rewards"][idx], data["dones"][idx])
    return pol
