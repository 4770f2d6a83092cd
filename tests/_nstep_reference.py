"""NumPy float64 statement of NStepReplayBuffer._get_samples for explicit (row, env) pairs; shares no code with the kernels."""
import numpy as np


def valid_pairs(rows: int, n_envs: int, pos: int, full: bool, pending: bool):
    """every (row, env) a sampler may draw: all rows of a full ring, else the written ones (the pending row is written)"""
    upper = rows if full else pos + int(pending)
    r, e = np.meshgrid(np.arange(upper), np.arange(n_envs), indexing="ij")
    return r.reshape(-1), e.reshape(-1)


def nstep_reference(f: dict, row, env, n_steps: int, gamma: float, pos: int, full: bool, pending: bool) -> dict:
    """f: observations / next_observations [R, N, D], actions [R, N, A], rewards / dones / timeouts [R, N]"""
    R = f["rewards"].shape[0]
    newest = pos if pending else (pos - 1) % R
    k = np.arange(n_steps)
    rk, ek = (row[:, None] + k) % R, env[:, None]
    r, d, t = (f[n][rk, ek].astype(np.float64) for n in ("rewards", "dones", "timeouts"))
    stop = (d != 0) | (t != 0) | (rk == newest)
    stop[:, -1] = True
    j = stop.argmax(axis=1)
    b = np.arange(len(row))
    inside = k <= j[:, None]
    terms = float(gamma) ** k * np.where(inside, r, 0.0)  # steps behind the window (unwritten rows among them) never enter
    dones = d[b, j] * (1.0 - t[b, j])
    return dict(observations=f["observations"][row, env], actions=f["actions"][row, env],
                next_observations=f["next_observations"][rk[b, j], env], dones=dones, rewards=terms.sum(axis=1),
                reward_scale=np.abs(terms).sum(axis=1), m=j + 1, discounts=float(gamma) ** (j + 1),
                fold=1.0 - (1.0 - dones) * float(gamma) ** j)
