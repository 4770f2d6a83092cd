"""Minimal `Box` space (the space of the CSTR path), `Discrete` (DQN's discretised valve face) and `MultiDiscrete` (the factored valve
face of PPO / A2C). gymnasium is not a dependency of this stack:
any object with `low`, `high`, `shape`, `dtype` (e.g. a real gymnasium.spaces.Box) is accepted wherever a
Box is expected; `as_box` normalises it. Mirrors the attributes the reference reads
(core/common/preprocessing.py:152-197, core/common/base_class.py:215-218)."""
from typing import Optional, Sequence

import numpy as np


class Space:
    def __init__(self, shape, dtype):
        self._shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self._np_random: Optional[np.random.Generator] = None

    @property
    def shape(self):
        return self._shape

    def seed(self, seed: Optional[int] = None):
        ss = np.random.SeedSequence(seed)
        self._np_random = np.random.Generator(np.random.PCG64(ss))
        return [ss.entropy]

    @property
    def np_random(self) -> np.random.Generator:
        if self._np_random is None:
            self.seed()
        return self._np_random


class Box(Space):
    def __init__(self, low, high, shape: Optional[Sequence[int]] = None, dtype=np.float32, seed=None):
        dtype = np.dtype(dtype)
        if shape is None:
            shape = np.shape(low) if not np.isscalar(low) else np.shape(high)
        shape = tuple(int(s) for s in shape)
        self.low = np.full(shape, low, dtype=dtype) if np.isscalar(low) else np.array(low, dtype=dtype)
        self.high = np.full(shape, high, dtype=dtype) if np.isscalar(high) else np.array(high, dtype=dtype)
        if self.low.shape != shape or self.high.shape != shape:
            raise ValueError(f"low/high shape mismatch: {self.low.shape} {self.high.shape} vs {shape}")
        super().__init__(shape, dtype)
        if seed is not None:
            self.seed(seed)

    def sample_batch(self, n: int) -> np.ndarray:
        """`np.array([space.sample() for _ in range(n)])` (off_policy_algorithm.py:388) in one call: n sequential
        bounded-Box draws from one Generator fill row-major, i.e. one uniform(size=(n, *shape)) draw.
        (gymnasium's own Box.sample is not available here: UNPINNED, see DESIGN.md.)"""
        u = self.np_random.uniform(low=self.low, high=self.high, size=(n, *self.shape))
        return u.astype(self.dtype)

    def sample(self) -> np.ndarray:
        return self.sample_batch(1)[0]

    def contains(self, x) -> bool:
        x = np.asarray(x)
        return bool(x.shape == self.shape and np.all(x >= self.low) and np.all(x <= self.high))

    def is_bounded(self) -> bool:
        return bool(np.all(np.isfinite(self.low)) and np.all(np.isfinite(self.high)))

    def __eq__(self, other):
        return (hasattr(other, "low") and hasattr(other, "high") and tuple(other.shape) == self.shape
                and np.array_equal(np.asarray(other.low), self.low) and np.array_equal(np.asarray(other.high), self.high))

    def __repr__(self):
        return f"Box({self.low.min()}, {self.high.max()}, {self.shape}, {self.dtype})"


class Discrete(Space):
    """`n` indices start, ..., start + n - 1 (gymnasium.spaces.Discrete: dtype int64, shape ()). `sample()` draws from the space's own
    Generator; gymnasium's own draw order is not available here (UNPINNED, as for Box.sample)."""

    def __init__(self, n: int, seed=None, start: int = 0):
        if not (isinstance(n, (int, np.integer)) and n > 0):
            raise ValueError(f"n (counts) have to be positive, got {n!r}")
        self.n, self.start = int(n), int(start)
        super().__init__((), np.int64)
        if seed is not None:
            self.seed(seed)

    def sample_batch(self, count: int) -> np.ndarray:
        """`np.array([space.sample() for _ in range(count)])` (dqn.py:251) in one call"""
        return self.start + self.np_random.integers(0, self.n, size=count, dtype=np.int64)

    def sample(self) -> np.int64:
        return np.int64(self.sample_batch(1)[0])

    def contains(self, x) -> bool:
        if isinstance(x, (np.generic, np.ndarray)):
            if not (np.issubdtype(np.asarray(x).dtype, np.integer) and np.asarray(x).shape == ()):
                return False
            x = int(x)
        elif not isinstance(x, int) or isinstance(x, bool):
            return False
        return self.start <= x < self.start + self.n

    def __eq__(self, other):
        return hasattr(other, "n") and not hasattr(other, "low") and int(other.n) == self.n and int(getattr(other, "start", 0)) == self.start

    def __repr__(self):
        return f"Discrete({self.n})" if self.start == 0 else f"Discrete({self.n}, start={self.start})"


class MultiDiscrete(Space):
    """One Discrete per component: component g takes 0 .. nvec[g] - 1 (gymnasium.spaces.MultiDiscrete with a 1-D `nvec`: dtype int64,
    shape (len(nvec),)). `sample()` draws from the space's own Generator (UNPINNED, as for Discrete.sample)."""

    def __init__(self, nvec, seed=None):
        nvec = np.array(nvec, dtype=np.int64, copy=True)
        if nvec.ndim != 1 or nvec.size == 0 or not (nvec > 0).all():
            raise ValueError(f"nvec (counts) have to be a non-empty 1-D array of positive counts, got {nvec!r}")
        self.nvec = nvec
        super().__init__(nvec.shape, np.int64)
        if seed is not None:
            self.seed(seed)

    def sample_batch(self, count: int) -> np.ndarray:
        return self.np_random.integers(0, self.nvec, size=(count, len(self.nvec)), dtype=np.int64)

    def sample(self) -> np.ndarray:
        return self.sample_batch(1)[0]

    def contains(self, x) -> bool:
        if isinstance(x, (list, tuple)):
            x = np.array(x)
        return bool(isinstance(x, np.ndarray) and x.shape == self.shape and x.dtype != bool and np.issubdtype(x.dtype, np.integer)
                    and (x >= 0).all() and (x < self.nvec).all())

    def __eq__(self, other):
        nvec = getattr(other, "nvec", None)
        return nvec is not None and not hasattr(other, "low") and np.ndim(nvec) == 1 and np.array_equal(np.asarray(nvec), self.nvec)

    def __repr__(self):
        return f"MultiDiscrete({self.nvec})"


class Dict(Space):
    """A dictionary of spaces with SORTED keys, as gymnasium.spaces.Dict orders a plain dict (the goal face of the env: achieved_goal,
    desired_goal, observation). The device-side observation is the flat row of the sub-spaces in key order."""

    def __init__(self, spaces=None, seed=None, **kwargs):
        given = dict(spaces or {}, **kwargs)
        self.spaces = {k: given[k] for k in sorted(given)}
        for k, s in self.spaces.items():
            if not isinstance(s, Space):
                raise ValueError(f"Dict space element is not an instance of Space: key={k!r}, space={s!r}")
        self._shape, self.dtype, self._np_random = None, None, None
        if seed is not None:
            self.seed(seed)

    @property
    def shape(self):
        return None

    def seed(self, seed: Optional[int] = None):
        ss = np.random.SeedSequence(seed)
        for sub, child in zip(self.spaces.values(), ss.spawn(len(self.spaces))):
            sub._np_random = np.random.Generator(np.random.PCG64(child))
        return [ss.entropy]

    def keys(self):
        return self.spaces.keys()

    def items(self):
        return self.spaces.items()

    def values(self):
        return self.spaces.values()

    def __getitem__(self, key):
        return self.spaces[key]

    def sample(self) -> dict:
        return {k: s.sample() for k, s in self.spaces.items()}

    def contains(self, x) -> bool:
        return isinstance(x, dict) and x.keys() == self.spaces.keys() and all(s.contains(x[k]) for k, s in self.spaces.items())

    def flat_dim(self) -> int:
        return int(sum(np.prod(s.shape) for s in self.spaces.values()))

    def __eq__(self, other):
        return isinstance(getattr(other, "spaces", None), dict) and list(other.spaces.keys()) == list(self.spaces.keys()) and all(
            self.spaces[k] == other.spaces[k] for k in self.spaces)

    def __repr__(self):
        return "Dict(" + ", ".join(f"{k!r}: {s}" for k, s in self.spaces.items()) + ")"


def as_discrete(space) -> Optional[Discrete]:
    """`space` as a Discrete (itself, or a scalar-shaped object with a count `n` and no bounds, e.g. a gymnasium.spaces.Discrete; a
    MultiBinary(n) has shape (n,) and is none), else None."""
    if isinstance(space, Discrete):
        return space
    if hasattr(space, "n") and not hasattr(space, "low") and np.isscalar(space.n) and tuple(getattr(space, "shape", None) or ()) == ():
        return Discrete(int(space.n), start=int(getattr(space, "start", 0)))
    return None


def as_multi_discrete(space) -> Optional[MultiDiscrete]:
    """`space` as a MultiDiscrete (itself, or any object with a 1-D `nvec`, e.g. a gymnasium.spaces.MultiDiscrete), else None."""
    if isinstance(space, MultiDiscrete):
        return space
    nvec = getattr(space, "nvec", None)
    if nvec is not None and np.ndim(nvec) == 1 and np.size(nvec) > 0:
        return MultiDiscrete(np.asarray(nvec))
    return None


class IndexedBox(Box):
    """Box that remembers which indices of the global vector it covers
    (reference: core/common/envs/multi_agent_envs.py:7-29)."""

    def __init__(self, low, high, indices, dtype=np.float32):
        super().__init__(low=low, high=high, dtype=dtype)
        self.indices = np.array(indices)

    def map_to_original(self, values):
        values = np.array(values) if isinstance(values, list) else values
        assert values.shape == self.shape, f"value shape {values.shape} does not match space shape {self.shape}"
        return self.indices, values


def split_spaces(observation_space: Box, action_space: Box, observation_splits, action_splits) -> tuple:
    """reference: core/common/envs/multi_agent_envs.py:32-61 -> (obs_subspaces, action_subspaces)"""
    def cut(space, splits):
        out = []
        for idx in splits:
            idx = np.array(idx)
            out.append(IndexedBox(np.asarray(space.low)[idx], np.asarray(space.high)[idx], idx, dtype=space.dtype))
        return out

    return cut(observation_space, observation_splits), cut(action_space, action_splits)


def as_box(space) -> Box:
    if isinstance(space, Box):
        return space
    if all(hasattr(space, a) for a in ("low", "high", "shape", "dtype")):
        return Box(np.asarray(space.low), np.asarray(space.high), tuple(space.shape), space.dtype)
    raise ValueError(f"Unsupported space {space!r}: this stack supports Box observation/action spaces only")


def get_obs_shape(space) -> tuple:
    return tuple(as_box(space).shape)


def get_action_dim(space) -> int:
    """reference: core/common/preprocessing.py:184-210 -- a Discrete action is a single int, a MultiDiscrete one an int per component"""
    if as_discrete(space) is not None:
        return 1
    multi = as_multi_discrete(space)
    if multi is not None:
        return int(len(multi.nvec))
    return int(np.prod(as_box(space).shape))
