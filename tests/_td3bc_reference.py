"""Reference statements of TD3+BC (Fujimoto & Gu 2021) for tests/test_td3bc_abi.py and tests/test_td3bc.py:

  * `actor_loss_f64`: the actor loss -lam * mean(q) + mean((pi - a)^2), lam = alpha / mean|q| (a constant), in NumPy float64 with its
    explicit gradients gq = -lam / B and g_pi = 2 (pi - a) / (B A);
  * `actor_loss_torch`: the same as one torch statement in any dtype (the float32 form is the "ATen distance" of the 4 x ATen bar);
  * `act_bwd_rows_f32`: gz = (gy + coef * (y - act)) * act'(y) in NumPy float32, one rounding per operation, in the kernel's order;
  * `last_layer_step`: a small fp64 model of the actor's last layer in front of a frozen linear critic -- the loss, its autograd
    gradient w.r.t. the pre-activation, the explicit gradient -- with the mistakes a wrong implementation makes as `variant`s;
  * `same_step`: the comparator;
  * `RefTD3BC`: whole gradient steps (critic step, delayed actor step, soft updates) in plain torch fp64, `normalize_f64` /
    `statistics_f64` the state normalisation."""
import numpy as np
import torch as th
from torch.nn import functional as F

VARIANTS = ("lam_not_detached", "mean_in_lam", "q_sign", "bc_mean_over_B", "coef_after_act", "bc_on_preactivation")


def actor_loss_f64(q, pi, a, alpha: float) -> dict:
    q, pi, a = (np.asarray(x, np.float64) for x in (q, pi, a))
    q = q.reshape(-1)
    B, A = pi.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.float64(alpha) / np.abs(q).mean()
        q_term = -lam * q.mean()
    bc = ((pi - a) ** 2).mean()
    return dict(lam=lam, q_term=q_term, bc=bc, loss=q_term + bc, gq=np.full(B, -lam / B), g_pi=2.0 * (pi - a) / (B * A))


def actor_loss_torch(q, pi, a, alpha: float, dtype, device="cpu") -> dict:
    """The statement as a user would write it in torch, evaluated in `dtype` on `device`."""
    q, pi, a = (th.as_tensor(np.asarray(x)).to(device, dtype) for x in (q, pi, a))
    lam = alpha / q.abs().mean().detach()
    q_term, bc = -lam * q.mean(), F.mse_loss(pi, a)
    return dict(lam=lam.item(), q_term=q_term.item(), bc=bc.item(), loss=(q_term + bc).item())


def act_bwd_rows_f32(gy, y, act, coef, kind: int) -> np.ndarray:
    """kind 0: no activation, 1: ReLU, 2: Tanh (y is the activation's OUTPUT). coef == 0 adds nothing."""
    gy, y, act = (np.asarray(x, np.float32) for x in (gy, y, act))
    c = np.float32(coef)
    g = gy if c == 0 else gy + c * (y - act)
    if kind == 1:
        g = np.where(y > 0, g, np.float32(0))
    if kind == 2:
        g = g * (np.float32(1) - y * y)
    return g.astype(np.float32)


def last_layer_step(z, a, c, e, alpha: float, variant=None) -> dict:
    """pi = tanh(z) [B, A]; q_b = pi_b . c + e_b (a frozen linear critic: dq/dpi = c). Returns the loss, lam, bc, the autograd
    gradient w.r.t. z of the statement (`gz_autograd`) and the explicit one the kernels compute (`gz`):
    gz = (gq_b c + coef (pi - a)) * (1 - pi^2), coef = 2 / (B A). `variant`: one of VARIANTS, a wrong implementation."""
    z = th.as_tensor(np.asarray(z, np.float64)).clone().requires_grad_(True)
    a, c, e = (th.as_tensor(np.asarray(x, np.float64)) for x in (a, c, e))
    B, A = z.shape
    pi = th.tanh(z)
    q = pi @ c + e
    norm = q.mean() if variant == "mean_in_lam" else q.abs().mean()
    lam = alpha / (norm if variant == "lam_not_detached" else norm.detach())
    q_term = lam * q.mean() if variant == "q_sign" else -lam * q.mean()
    x = z if variant == "bc_on_preactivation" else pi
    bc = ((x - a) ** 2).sum(dim=1).mean() if variant == "bc_mean_over_B" else ((x - a) ** 2).mean()
    loss = q_term + bc
    (gz_auto,) = th.autograd.grad(loss, z)
    with th.no_grad():
        lam_c = lam.detach()
        gy = (-lam_c / B) * c.expand(B, A)
        coef = 2.0 / (B * A)
        dact = 1.0 - pi * pi
        gz = gy * dact + coef * (pi - a) if variant == "coef_after_act" else (gy + coef * (pi - a)) * dact
    explicit = gz if variant in (None, "coef_after_act") else gz_auto  # the other variants are wrong statements: their own gradient
    return dict(loss=loss.item(), lam=float(lam.detach()), bc=bc.item(), gz=explicit.numpy().copy(), gz_autograd=gz_auto.numpy().copy())


def same_step(got: dict, want: dict, rtol: float = 1e-9) -> bool:
    """The comparator: loss, lam, bc and the gradient w.r.t. the pre-activation agree to `rtol` of their scale."""
    for k in ("loss", "lam", "bc"):
        if not abs(got[k] - want[k]) <= rtol * max(abs(want[k]), 1e-12):
            return False
    scale = float(np.abs(want["gz"]).max())
    return bool(np.abs(got["gz"] - want["gz"]).max() <= rtol * max(scale, 1e-300))


def statistics_f64(observations):
    """per-column (mean, std(ddof=0) + 1e-3) of [R, D] rows, NumPy float64"""
    o = np.asarray(observations, np.float64)
    return o.mean(axis=0), o.std(axis=0, ddof=0) + 1e-3


def normalize_f64(x, mean, std):
    return (np.asarray(x, np.float64) - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)


def fold_first_layer_f64(w1, b1, mean, std):
    """W1' = W1 / std per input column, b1' = b1 - W1' @ mean"""
    w = np.asarray(w1, np.float64) / np.asarray(std, np.float64)[None, :]
    return w, np.asarray(b1, np.float64) - w @ np.asarray(mean, np.float64)


class RefTD3BC:
    """Whole TD3+BC gradient steps in plain torch fp64 on the CPU, started from a model's weights. `policy` is a float64 copy of the
    model's TD3Policy modules (actor, actor_target, critic, critic_target)."""

    def __init__(self, policy, lr: float, gamma: float, tau: float, policy_delay: int, noise_clip: float, alpha: float):
        self.p, self.gamma, self.tau, self.delay, self.clip, self.alpha = policy, gamma, tau, policy_delay, noise_clip, alpha
        self.actor_opt = th.optim.Adam(policy.actor.parameters(), lr=lr)
        self.critic_opt = th.optim.Adam(policy.critic.parameters(), lr=lr)
        self.n_updates = 0

    @staticmethod
    def _polyak(src, dst, tau: float) -> None:
        with th.no_grad():
            for s, d in zip(src.parameters(), dst.parameters()):
                d.mul_(1.0 - tau).add_(s, alpha=tau)

    @staticmethod
    def _q(critic, obs, act) -> tuple:
        """the Q networks themselves (the modules' feature extraction casts to float32)"""
        x = th.cat([obs, act], dim=1)
        return tuple(q(x) for q in critic.q_networks)

    def step(self, obs, act, next_obs, rew, done, noise) -> dict:
        """One gradient step on an already normalised fp64 batch; `noise` is the raw smoothing draw [B, A]."""
        p = self.p
        obs, act, next_obs, rew, done, noise = (th.as_tensor(np.asarray(x, np.float64)) for x in (obs, act, next_obs, rew, done, noise))
        self.n_updates += 1
        with th.no_grad():
            n = noise.clamp(-self.clip, self.clip)
            next_a = (p.actor_target.mu(next_obs) + n).clamp(-1, 1)
            next_q, _ = th.min(th.cat(self._q(p.critic_target, next_obs, next_a), dim=1), dim=1, keepdim=True)
            target = rew + (1 - done) * self.gamma * next_q
        current = self._q(p.critic, obs, act)
        critic_loss = sum(F.mse_loss(q, target) for q in current)
        self.critic_opt.zero_grad()
        critic_loss.backward()
        self.critic_opt.step()
        out = dict(target_q=target.numpy().copy(), current_q=[q.detach().numpy().copy() for q in current], critic_loss=critic_loss.item(),
                   actor_loss=None)
        if self.n_updates % self.delay == 0:
            pi = p.actor.mu(obs)
            q = self._q(p.critic, obs, pi)[0]
            lam = self.alpha / q.abs().mean().detach()
            q_term, bc = -lam * q.mean(), F.mse_loss(pi, act)
            actor_loss = q_term + bc
            self.actor_opt.zero_grad()
            actor_loss.backward()
            self.actor_opt.step()
            self._polyak(p.critic, p.critic_target, self.tau)
            self._polyak(p.actor, p.actor_target, self.tau)
            out.update(actor_loss=actor_loss.item(), lam=lam.item(), q_term=q_term.item(), bc=bc.item(), q_pi=q.detach().numpy().copy(),
                       pi=pi.detach().numpy().copy())
        return out
