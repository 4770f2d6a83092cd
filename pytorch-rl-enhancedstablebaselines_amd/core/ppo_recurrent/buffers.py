"""`RecurrentRolloutBuffer`: the device RolloutBuffer plus the LSTM states the rollout saw, and the segment tables of RecurrentPPO's
minibatches.

States: `hidden[name]` [T + 1, N, H] for name in pi_h, pi_c, vf_h, vf_c. Slot t holds the state BEFORE step t (what sb3_contrib stores),
slot T the state behind the last step, which the next rollout copies to slot 0. Memory: 4 tensors x (T + 1) x N x H x 4 bytes.

Minibatches: rows are flattened env-major (row = env * T + step). One `split` per epoch (np.random.randint(T * N), from the buffer's
`permutation_rng` where set), the order is rows split .. T * N - 1 then 0 .. split - 1, cut into consecutive chunks of batch_size. Within a
chunk a segment starts at the chunk's first row and wherever the env changes (step 0 of any env counts); its initial state is the stored
state of its first row, and episode starts inside it are the kernel's mask. The table needs `split` alone: nothing is read from the device."""
from typing import Generator, Optional

import numpy as np
import torch as th

from core.common import hip_ops
from core.common.buffers import RolloutBuffer

STATE_NAMES = ("pi_h", "pi_c", "vf_h", "vf_c")


def segment_tables(split: int, n_steps: int, n_envs: int, batch_size: int):
    """-> (row order [T * N], table int32 [n_seg, 3] = (first row WITHIN its chunk, length, state row = step * N + env), bounds [n_chunks + 1]:
    chunk i owns the segments bounds[i] .. bounds[i + 1] - 1)"""
    total = n_steps * n_envs
    idx = np.concatenate([np.arange(split, total), np.arange(0, split)]).astype(np.int64)
    env, step = idx // n_steps, idx % n_steps
    new = np.ones(total, dtype=bool)
    new[1:] = (env[1:] != env[:-1]) | (step[1:] == 0)
    new[::batch_size] = True
    starts = np.flatnonzero(new)
    lengths = np.diff(np.append(starts, total))
    table = np.stack([starts % batch_size, lengths, step[starts] * n_envs + env[starts]], axis=1).astype(np.int32)
    n_chunks = (total + batch_size - 1) // batch_size
    return idx, table, np.searchsorted(starts // batch_size, np.arange(n_chunks + 1))


class RecurrentRolloutBuffer(RolloutBuffer):
    def __init__(self, buffer_size: int, observation_space, action_space, hidden_size: int, device="auto", gae_lambda: float = 1,
                 gamma: float = 0.99, n_envs: int = 1, permutation_rng=None):
        super().__init__(buffer_size, observation_space, action_space, device, gae_lambda=gae_lambda, gamma=gamma, n_envs=n_envs,
                         permutation_rng=permutation_rng)
        self.hidden_size = hidden_size
        self.hidden = {k: th.zeros(buffer_size + 1, n_envs, hidden_size, dtype=th.float32, device=self.device) for k in STATE_NAMES}
        self.forced_splits: list = []  # teacher-forcing hook: each get() pops its split from here first (tests)
        self.last_split: Optional[int] = None
        self._es_flat = th.zeros(buffer_size * n_envs, dtype=th.float32, device=self.device)

    def state_rows(self, name: str) -> th.Tensor:
        """the stored pre-step states as [T * N, H] rows (row = step * N + env: the table's third column)"""
        return self.hidden[name][:self.buffer_size].reshape(-1, self.hidden_size)

    def carry_over(self) -> None:
        """a new rollout starts from the state behind the last one's final step"""
        for v in self.hidden.values():
            v[0].copy_(v[self.buffer_size])

    def get(self, batch_size: Optional[int] = None) -> Generator[tuple, None, None]:
        """yields (RolloutBufferSamples of the chunk, its episode starts [rows], its LstmSegments in the chunk's own row numbers)"""
        assert self.full, ""
        total = self.buffer_size * self.n_envs
        batch_size = total if batch_size is None else batch_size
        if self.forced_splits:
            split = int(self.forced_splits.pop(0))
        else:
            split = int((np.random if self.permutation_rng is None else self.permutation_rng).randint(total))
        self.last_split = split
        indices, table, bounds = segment_tables(split, self.buffer_size, self.n_envs, batch_size)
        self.last_indices = indices
        with th.cuda.device(self.device):
            idx = th.from_numpy(indices).to(self.device)
            segs = hip_ops.LstmSegments(table, self.device)
            self._es_flat.copy_(self.episode_starts.t().reshape(-1))
            es = self._es_flat[idx]
            for i, start in enumerate(range(0, total, batch_size)):
                part = idx[start:start + batch_size]
                mb = self._minibatch(part.shape[0])
                self._gather(part, mb)
                yield mb, es[start:start + batch_size], segs.part(int(bounds[i]), int(bounds[i + 1]))
