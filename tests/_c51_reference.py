"""C51 in NumPy float64 on the float32 inputs (include/cstr_rl_hip.h, the C51 block): the head's expected values and the loss launch's
outputs. A row of logits is [M][N], atom i of action a at a * N + i; the support is z_i = v_min + i * dz, dz = (v_max - v_min) / (N - 1)."""
import numpy as np


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def support(n_atoms, v_min, v_max):
    return v_min + np.arange(n_atoms) * ((v_max - v_min) / (n_atoms - 1))


def expected_q(logits, v_min, v_max):
    """logits [.., M, N] -> sum_i z_i softmax_i [.., M]"""
    logits = np.asarray(logits, np.float64)
    return (softmax(logits) * support(logits.shape[-1], v_min, v_max)).sum(axis=-1)


def head_q(h, w, bias, n_actions, v_min, v_max):
    logits = np.asarray(h, np.float64) @ np.asarray(w, np.float64).T + np.asarray(bias, np.float64)
    return expected_q(logits.reshape(len(logits), n_actions, -1), v_min, v_max)


def loss_step(z, z_next, index, reward, done, gamma, n_actions, v_min, v_max):
    """z / z_next [B, M * N], index [B] the taken action -> m, logp [B, N], row_loss [B], loss, gz [B, M * N], next_index [B] (a*), q_next"""
    z, z_next = (np.asarray(t, np.float64).reshape(len(t), n_actions, -1) for t in (z, z_next))
    B, M, N = z.shape
    rows, dz = np.arange(B), (v_max - v_min) / (N - 1)
    q_next = expected_q(z_next, v_min, v_max)
    a_star = q_next.argmax(axis=1)
    p = softmax(z_next[rows, a_star])
    coef = (1.0 - np.asarray(done, np.float64).reshape(B, 1)) * gamma
    tz = np.clip(np.asarray(reward, np.float64).reshape(B, 1) + coef * support(N, v_min, v_max), v_min, v_max)
    b = np.clip((tz - v_min) / dz, 0, N - 1)
    hat = np.maximum(0.0, 1.0 - np.abs(b[:, None, :] - np.arange(N)[None, :, None]))  # [B, i, j]
    m = (hat * p[:, None, :]).sum(axis=2)
    x = z[rows, index]
    x = x - x.max(axis=1, keepdims=True)
    e = np.exp(x)
    logp = x - np.log(e.sum(axis=1, keepdims=True))
    row_loss = -(m * logp).sum(axis=1)
    gz = np.zeros((B, M, N))
    gz[rows, index] = ((e / e.sum(axis=1, keepdims=True)) * m.sum(axis=1, keepdims=True) - m) / B
    return dict(m=m, logp=logp, row_loss=row_loss, loss=row_loss.sum() / B, gz=gz.reshape(B, M * N), next_index=a_star, q_next=q_next)
