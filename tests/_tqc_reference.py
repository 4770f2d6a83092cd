"""The fp64 restatement of TQC (Kuznetsov et al. 2020; core/tqc/tqc.py) the kernel and learner tests compare against. sb3_contrib is
not a dependency: this is the published statement, written out.

G critics of Nq atoms, k atoms dropped per critic, M = G * Nq, n_keep = M - k * G, tau_i = (i + 0.5) / Nq. The kernel-level functions
take the atoms as [G, B, Nq] (the layout of the stacked critic output, and of cstr_tqc_critic_loss_f32), NumPy in, float64 NumPy out:
  * `truncated_targets`: pool a row's M target atoms, torch.sort ascending, keep the first n_keep,
        y_j = r + (1 - d) * gamma * (z'_(j) - alpha * logp');
  * `quantile_huber`: mean over (b, g, i, j) of |tau_i - 1[delta < 0]| * Huber(delta), delta = y_j - z_{g,i};
  * `critic_loss`: both, with the gradient d loss / d z by autograd AND in closed form,
        -(1 / (B M n_keep)) * sum_j |tau_i - 1[delta < 0]| * clamp(delta, -1, 1), and the two logged means;
  * `actor_loss`: mean(alpha * logp - mean over (g, i) of z_pi), its two (constant) gradients and the row means;
  * `alpha_part`: SAC's entropy-coefficient loss -mean(log_alpha * (logp + H)), its gradient and alpha = exp(log_alpha);
  * `RefTQC`: whole gradient steps in SAC's order on a float64 (or float32) copy of a model's TQCPolicy modules, noise given."""
import math

import numpy as np
import torch as th

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def n_keep(G: int, Nq: int, k: int) -> int:
    return G * Nq - k * G


def _t(a, dtype=th.float64):
    return th.as_tensor(np.asarray(a), dtype=dtype)


def truncated_targets_t(z_next_bgn: th.Tensor, next_logp, rew, done, alpha, gamma: float, k: int) -> th.Tensor:
    """torch: z_next [B, G, Nq], next_logp / rew / done [B, 1] -> y [B, n_keep], ascending in each row"""
    B, G, Nq = z_next_bgn.shape
    z_sorted, _ = th.sort(z_next_bgn.reshape(B, -1), dim=1)
    kept = z_sorted[:, :n_keep(G, Nq, k)]
    return rew + (1 - done) * gamma * (kept - alpha * next_logp)


def quantile_huber_t(z_bgn: th.Tensor, y: th.Tensor) -> th.Tensor:
    """torch: z [B, G, Nq], y [B, n_keep] -> the scalar loss (quantile_huber_loss(..., sum_over_quantiles=False))"""
    Nq = z_bgn.shape[2]
    tau = (th.arange(Nq, dtype=z_bgn.dtype) + 0.5) / Nq
    delta = y[:, None, None, :] - z_bgn[:, :, :, None]
    ad = delta.abs()
    huber = th.where(ad > 1, ad - 0.5, delta ** 2 * 0.5)
    return (th.abs(tau[None, None, :, None] - (delta.detach() < 0).to(z_bgn.dtype)) * huber).mean()


def closed_form_grad_t(z_bgn: th.Tensor, y: th.Tensor) -> th.Tensor:
    B, G, Nq = z_bgn.shape
    tau = (th.arange(Nq, dtype=z_bgn.dtype) + 0.5) / Nq
    delta = y[:, None, None, :] - z_bgn[:, :, :, None]
    w = th.abs(tau[None, None, :, None] - (delta < 0).to(z_bgn.dtype))
    return -(w * delta.clamp(-1.0, 1.0)).sum(dim=3) / (B * G * Nq * y.shape[1])


def critic_loss(z, z_next, next_logp, rew, done, alpha: float, gamma: float, k: int, dtype=th.float64) -> dict:
    """z / z_next [G, B, Nq] -> dict(y [B, n_keep], loss, gz [G, B, Nq] by autograd, gz_closed, target_mean, atom_mean)"""
    zb = _t(z, dtype).permute(1, 0, 2).contiguous().requires_grad_(True)
    znb = _t(z_next, dtype).permute(1, 0, 2).contiguous()
    col = lambda a: _t(a, dtype).reshape(-1, 1)  # noqa: E731
    y = truncated_targets_t(znb, col(next_logp), col(rew), col(done), alpha, gamma, k)
    loss = quantile_huber_t(zb, y)
    loss.backward()
    n = lambda t: t.detach().to(th.float64).numpy().copy()  # noqa: E731
    return dict(y=n(y), loss=float(loss.detach()), gz=n(zb.grad.permute(1, 0, 2)), gz_closed=n(closed_form_grad_t(zb.detach(), y).permute(1, 0, 2)),
                target_mean=float(y.mean()), atom_mean=float(zb.detach().mean()))


def actor_loss(z_pi, logp, alpha: float, dtype=th.float64) -> dict:
    """z_pi [G, B, Nq], logp [B] -> dict(loss, gz_pi [G, B, Nq], g_logp [B], z_pi_mean [B])"""
    zb = _t(z_pi, dtype).permute(1, 0, 2).contiguous().requires_grad_(True)
    lp = _t(logp, dtype).reshape(-1, 1).requires_grad_(True)
    qf_pi = zb.mean(dim=2).mean(dim=1, keepdim=True)
    loss = (alpha * lp - qf_pi).mean()
    loss.backward()
    n = lambda t: t.detach().to(th.float64).numpy().copy()  # noqa: E731
    return dict(loss=float(loss.detach()), gz_pi=n(zb.grad.permute(1, 0, 2)), g_logp=n(lp.grad).reshape(-1), z_pi_mean=n(qf_pi).reshape(-1))


def alpha_part(log_alpha: float, logp_pi, target_entropy: float) -> dict:
    la = th.tensor([float(log_alpha)], dtype=th.float64, requires_grad=True)
    loss = -(la * (_t(logp_pi).reshape(-1, 1) + target_entropy)).mean()
    loss.backward()
    return dict(ent_coef=math.exp(float(log_alpha)), loss=float(loss.detach()), grad=float(la.grad))


# ---- whole gradient steps --------------------------------------------------------------------------------------------------------------
def _dist_params(actor, obs):
    h = actor.latent_pi(obs)
    return actor.mu(h), actor.log_std(h)


def _sample(mean, raw, eps):
    sd = raw.clamp(LOG_STD_MIN, LOG_STD_MAX).exp()
    g = mean + sd * eps
    a = th.tanh(g)
    lp = (-((g - mean) ** 2) / (2 * sd ** 2) - sd.log() - HALF_LOG_2PI).sum(-1)
    return a, lp - th.log(1 - a ** 2 + 1e-6).sum(-1)


def _z(critic, x):
    """[B, G, Nq]"""
    return th.stack(tuple(q(x) for q in critic.q_networks), dim=1)


class RefTQC:
    """Whole TQC gradient steps in plain torch on the CPU, started from a model's weights, in SAC's order (core/tqc/tqc.py). `policy`
    is a float64 copy of the model's TQCPolicy modules (actor, critic, critic_target); dtype float32 (with a float32 policy) is the
    plain torch statement, whose distance from the float64 one says what a bar asks of float32 arithmetic."""

    def __init__(self, policy, lr, gamma, tau, k, log_ent_coef=0.0, target_entropy=-2.0, target_update_interval: int = 1, dtype=th.float64):
        self.dtype, self.np_dtype = dtype, (np.float64 if dtype == th.float64 else np.float32)
        self.p, self.gamma, self.tau, self.k, self.target_entropy = policy, gamma, tau, k, target_entropy
        self.interval, self.n = target_update_interval, 0
        self.log_ent_coef = th.tensor([float(log_ent_coef)], dtype=dtype, requires_grad=True)
        self.actor_opt = th.optim.Adam(policy.actor.parameters(), lr=lr)
        self.critic_opt = th.optim.Adam(policy.critic.parameters(), lr=lr)
        self.ent_opt = th.optim.Adam([self.log_ent_coef], lr=lr)

    def step(self, obs, act, next_obs, rew, done, eps_pi, eps_next) -> dict:
        p = self.p
        obs, act, next_obs, rew, done, eps_pi, eps_next = (th.as_tensor(np.asarray(x, self.np_dtype)) for x in
                                                           (obs, act, next_obs, rew, done, eps_pi, eps_next))
        rew, done = rew.reshape(-1, 1), done.reshape(-1, 1)
        a_pi, logp = _sample(*_dist_params(p.actor, obs), eps_pi)
        logp = logp.reshape(-1, 1)
        ent_coef = th.exp(self.log_ent_coef.detach())
        ent_loss = -(self.log_ent_coef * (logp + self.target_entropy).detach()).mean()
        self.ent_opt.zero_grad()
        ent_loss.backward()
        self.ent_opt.step()
        with th.no_grad():
            a_n, logp_n = _sample(*_dist_params(p.actor, next_obs), eps_next)
            y = truncated_targets_t(_z(p.critic_target, th.cat([next_obs, a_n], 1)), logp_n.reshape(-1, 1), rew, done, ent_coef, self.gamma, self.k)
        z = _z(p.critic, th.cat([obs, act], 1))
        critic_loss_ = quantile_huber_t(z, y)
        self.critic_opt.zero_grad()
        critic_loss_.backward()
        self.critic_opt.step()
        qf_pi = _z(p.critic, th.cat([obs, a_pi], 1)).mean(dim=2).mean(dim=1, keepdim=True)
        actor_loss_ = (ent_coef * logp - qf_pi).mean()
        self.actor_opt.zero_grad()
        actor_loss_.backward()
        self.actor_opt.step()
        if self.n % self.interval == 0:
            with th.no_grad():
                for s, d in zip(p.critic.parameters(), p.critic_target.parameters()):
                    d.mul_(1.0 - self.tau).add_(s, alpha=self.tau)
        self.n += 1
        n = lambda t: t.detach().to(th.float64).numpy().copy()  # noqa: E731
        return dict(z=n(z), y=n(y), z_pi_mean=n(qf_pi).reshape(-1), log_prob=n(logp).reshape(-1), a_pi=n(a_pi), ent_coef=float(ent_coef),
                    ent_coef_loss=float(ent_loss.detach()), critic_loss=float(critic_loss_.detach()), actor_loss=float(actor_loss_.detach()),
                    target_mean=float(y.mean()), atom_mean=float(z.detach().mean()))


def make_policy(seed: int = 0, arch=(256, 256), lr: float = 3e-4, **kw):
    from core.common.spaces import Box
    from core.common.utils import set_random_seed
    from core.tqc.policies import TQCPolicy

    set_random_seed(seed)
    return TQCPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: lr, net_arch=list(arch), **kw)


def loss_inputs(B: int, G: int, Nq: int, seed: int, scale: float = 1.0, mode: str = "random") -> dict:
    """float32 inputs of the two loss launches. scale: the size of the atoms (about 1, about 300). mode: "random"; "done" (every done =
    1: y = r); "ties" (every critic holds the same atoms and each atom twice: all of them tied at least G-fold); "edges" (done = 1 and
    the atoms r, r + 1, r - 1 with dyadic r: delta exactly 0, -1, +1)."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    z = f(rng.normal(0.0, 1.0, (G, B, Nq)) * scale + (scale if scale > 1 else 0.0))
    z_next = f(rng.normal(0.0, 1.0, (G, B, Nq)) * scale + (scale if scale > 1 else 0.0))
    rew, done = f(rng.uniform(-8, 0, B)), f(rng.uniform(size=B) < 0.2)
    if mode == "done":
        done = f(np.ones(B))
    if mode == "ties":
        one = f(np.repeat(rng.normal(0.0, 1.0, (1, B, (Nq + 1) // 2)) * scale, 2, axis=2)[:, :, :Nq])
        z_next = np.tile(one, (G, 1, 1))
    if mode == "edges":
        done = f(np.ones(B))
        rew = f(np.round(rng.uniform(-8, 0, B) * 4) / 4)
        z = f(rew[None, :, None] + rng.integers(-1, 2, (G, B, Nq)))
    return dict(z=z, z_next=z_next, next_logp=f(rng.normal(-1.0, 1.0, B)), rew=rew, done=done, alpha=float(np.float32(0.37)), gamma=0.99,
                z_pi=f(rng.normal(0.0, 1.0, (G, B, Nq)) * scale), logp=f(rng.normal(-1.0, 1.0, B)), log_alpha=float(np.float32(-0.8)),
                target_entropy=-2.0)
