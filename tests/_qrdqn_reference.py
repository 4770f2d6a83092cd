"""The fp64 restatement of QR-DQN (Dabney et al. 2018; sb3_contrib.QRDQN; core/qrdqn/qrdqn.py) the kernel and learner tests compare
against. sb3_contrib is not a dependency: this is the published statement, written out.

K valve levels, M = K * K actions, Nq atoms per action, tau_i = (i + 0.5) / Nq. A row of atoms is [Nq, M] flattened, atom i of action
a at i * M + a (`quantiles.view(-1, Nq, M)`, the layout of cstr_qrdqn_loss_f32). NumPy in, float64 NumPy out:
  * `quantile_huber`: current [B, Nq], target [B, Nq'] -> sum over the current quantile, mean over batch and target quantile of
        |tau_i - 1[delta < 0]| * Huber(delta), delta = target_j - current_i   (quantile_huber_loss(..., sum_over_quantiles=True));
  * `closed_form_grad`: -(1 / (B Nq')) * sum_j |tau_i - 1[delta < 0]| * clamp(delta, -1, 1);
  * `greedy_index`: first maximum over a of sum_i z[b, i, a] (i ascending in float64; a NaN is the greatest value, torch.argmax);
  * `loss_step`: greedy index, targets, gathered current atoms, loss, dense d loss / d z by autograd and in closed form;
  * `folded_head`: the mean over the atoms of the last layer's weight rows and biases;
  * `RefQRDQN`: whole gradient steps (Adam with the given eps, hard target update on request) on a float64 copy of a policy's networks;
  * `loss_inputs`: float32 inputs of the loss launch in four patterns."""
import copy

import numpy as np
import torch as th

from _dqn_helpers import level_np, pair_np


def _t(a, dtype=th.float64):
    return th.as_tensor(np.asarray(a), dtype=dtype)


def quantile_huber_t(cur: th.Tensor, tgt: th.Tensor) -> th.Tensor:
    """torch: cur [B, Nq], tgt [B, Nq'] -> the scalar loss"""
    nq = cur.shape[1]
    tau = ((th.arange(nq, dtype=cur.dtype) + 0.5) / nq).view(1, -1, 1)
    delta = tgt.unsqueeze(-2) - cur.unsqueeze(-1)  # [B, Nq (current), Nq' (target)]
    ad = delta.abs()
    huber = th.where(ad > 1, ad - 0.5, delta ** 2 * 0.5)
    return (th.abs(tau - (delta.detach() < 0).to(cur.dtype)) * huber).sum(dim=-2).mean()


def closed_form_grad_t(cur: th.Tensor, tgt: th.Tensor) -> th.Tensor:
    B, nq = cur.shape
    tau = ((th.arange(nq, dtype=cur.dtype) + 0.5) / nq).view(1, -1, 1)
    delta = tgt.unsqueeze(-2) - cur.unsqueeze(-1)
    w = th.abs(tau - (delta < 0).to(cur.dtype))
    return -(w * delta.clamp(-1.0, 1.0)).sum(dim=2) / (B * tgt.shape[1])


def quantile_huber(cur, tgt) -> float:
    return float(quantile_huber_t(_t(cur), _t(tgt)))


def closed_form_grad(cur, tgt) -> np.ndarray:
    return closed_form_grad_t(_t(cur), _t(tgt)).numpy()


def greedy_index(z_next_bnm) -> np.ndarray:
    """z_next [B, Nq, M] -> int64 [B]"""
    z = np.asarray(z_next_bnm, np.float64)
    s = np.zeros((z.shape[0], z.shape[2]))
    for i in range(z.shape[1]):
        s = s + z[:, i, :]
    return np.argmax(s, axis=1).astype(np.int64)  # the first maximum; a NaN counts as the greatest value


def loss_step(z, z_next, valve, rew, done, gamma: float, K: int) -> dict:
    """z / z_next [B, Nq * M] float32, valve [B, 2] -> dict(next_index [B], y [B, Nq], cur [B, Nq], loss, gz [B, Nq * M] by autograd,
    gz_closed)"""
    M = K * K
    B, NM = np.asarray(z).shape
    Nq = NM // M
    index = level_np(np.asarray(valve)[:, 0], K) * K + level_np(np.asarray(valve)[:, 1], K)
    zt = _t(z).reshape(B, Nq, M).clone().requires_grad_(True)
    zn = _t(z_next).reshape(B, Nq, M)
    nxt = greedy_index(zn.numpy())
    col = lambda a: _t(a).reshape(-1, 1)  # noqa: E731
    y = col(rew) + (1 - col(done)) * gamma * zn[th.arange(B), :, th.as_tensor(nxt)]
    cur = zt[th.arange(B), :, th.as_tensor(index)]
    loss = quantile_huber_t(cur, y)
    loss.backward()
    closed = np.zeros((B, Nq, M))
    closed[np.arange(B), :, index] = closed_form_grad_t(cur.detach(), y).numpy()
    n = lambda t: t.detach().numpy().copy()  # noqa: E731
    return dict(next_index=nxt, y=n(y), cur=n(cur), loss=float(loss.detach()), gz=n(zt.grad).reshape(B, NM), gz_closed=closed.reshape(B, NM))


def folded_head(w, b, Nq: int, M: int):
    """w [Nq * M, H], b [Nq * M] -> (w_mean [M, H], b_mean [M]) in float64"""
    w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
    return w.reshape(Nq, M, w.shape[1]).mean(axis=0), b.reshape(Nq, M).mean(axis=0)


class RefQRDQN:
    """Whole QR-DQN gradient steps in plain torch on the CPU, started from a policy's weights. `policy`: a QRDQNPolicy (modules on the
    CPU); its two networks are copied and cast to `dtype`."""

    def __init__(self, policy, lr: float, gamma: float, adam_eps: float, max_grad_norm=None, dtype=th.float64):
        self.dtype, self.np_dtype = dtype, (np.float64 if dtype == th.float64 else np.float32)
        self.net, self.target = copy.deepcopy(policy.quantile_net).to(dtype), copy.deepcopy(policy.quantile_net_target).to(dtype)
        self.gamma, self.max_grad_norm = gamma, max_grad_norm
        self.opt = th.optim.Adam(self.net.parameters(), lr=lr, eps=adam_eps)

    @staticmethod
    def _atoms(net, obs):
        """[B, Nq, M]; the Sequential itself (QuantileNetwork.forward casts its input to float32 first)"""
        return net.quantile_net(obs).view(-1, net.n_quantiles, net.n_actions)

    def update_target(self) -> None:
        self.target.load_state_dict(self.net.state_dict())  # polyak_update with tau = 1

    def step(self, obs, index, next_obs, rew, done) -> dict:
        obs, next_obs, rew, done = (th.as_tensor(np.asarray(x, self.np_dtype)) for x in (obs, next_obs, rew, done))
        rew, done = rew.reshape(-1, 1), done.reshape(-1, 1)
        B = obs.shape[0]
        index = th.as_tensor(np.asarray(index, np.int64).reshape(-1))
        with th.no_grad():
            zn = self._atoms(self.target, next_obs)
            nxt = zn.mean(dim=1).argmax(dim=1)
            y = rew + (1 - done) * self.gamma * zn[th.arange(B), :, nxt]
        cur = self._atoms(self.net, obs)[th.arange(B), :, index]
        loss = quantile_huber_t(cur, y)
        self.opt.zero_grad()
        loss.backward()
        norm = float(th.sqrt(sum((p.grad.double() ** 2).sum() for p in self.net.parameters())))
        if self.max_grad_norm is not None:
            th.nn.utils.clip_grad_norm_(self.net.parameters(), self.max_grad_norm)
        self.opt.step()
        n = lambda t: t.detach().to(th.float64).numpy().copy()  # noqa: E731
        return dict(cur=n(cur), y=n(y), next_index=nxt.numpy().copy(), loss=float(loss.detach()), grad_norm=norm)


def make_policy(K: int, seed: int = 0, arch=(64, 64), lr: float = 5e-5, **kw):
    from core.common.spaces import Box, Discrete
    from core.common.utils import set_random_seed
    from core.qrdqn.policies import QRDQNPolicy

    set_random_seed(seed)
    return QRDQNPolicy(Box(-1, 1, (4,)), Discrete(K * K), lambda _: lr, net_arch=list(arch), **kw)


def loss_inputs(B: int, K: int, Nq: int, seed: int, scale: float = 1.0, mode: str = "random") -> dict:
    """float32 inputs of the loss launch: z / z_next [B, Nq * M], valve [B, 2], index [B], rew, done [B]. scale: the size of the atoms
    (about 1, about 300). mode: "random"; "done" (every done = 1: y = r); "edges" (done = 1 and the atoms r, r + 1, r - 1 with dyadic r:
    delta exactly 0, -1, +1); "ties" (actions 1 and M - 1 hold the same next atoms, above every other action's: the first must win)."""
    rng = np.random.default_rng(seed)
    M = K * K
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    off = scale if scale > 1 else 0.0
    z = f(rng.normal(0.0, 1.0, (B, Nq, M)) * scale + off)
    z_next = f(rng.normal(0.0, 1.0, (B, Nq, M)) * scale + off)
    rew, done = f(rng.uniform(-8, 0, B)), f(rng.uniform(size=B) < 0.2)
    index = rng.integers(0, M, B)
    if mode == "done":
        done = f(np.ones(B))
    if mode == "edges":
        done = f(np.ones(B))
        rew = f(np.round(rng.uniform(-8, 0, B) * 4) / 4)
        z = f(rew[:, None, None] + rng.integers(-1, 2, (B, Nq, M)))
    if mode == "ties":
        z_next[:, :, 1] += f(8.0 * scale)
        z_next[:, :, M - 1] = z_next[:, :, 1]
    return dict(z=z.reshape(B, Nq * M), z_next=z_next.reshape(B, Nq * M), valve=f(pair_np(index, K)), index=index, rew=rew, done=done, gamma=0.99)
