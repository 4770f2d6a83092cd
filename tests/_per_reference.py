"""float64 NumPy statements of the prioritized-replay launches (csrc/cstr_per.hip), for tests/test_per.py."""
import numpy as np


def children_sums(level):
    """the parents of a level: sums over consecutive groups of 64 nodes, the last group padded with zeros"""
    level = np.asarray(level, np.float64)
    return np.pad(level, (0, (-len(level)) % 64)).reshape(-1, 64).sum(axis=1)


def update_f64(leaves, max_priority, idx, td_abs, alpha, min_priority):
    """the sequential loop of the published implementations: (new leaves, new max_priority); a non-finite error stores the
    max_priority the call found and does not raise it"""
    leaves, found = np.array(leaves, np.float64), max_priority
    for i, t in zip(idx, np.abs(np.asarray(td_abs, np.float64))):
        if np.isfinite(t):
            leaves[i] = (t + min_priority) ** alpha
            max_priority = max(max_priority, t + min_priority)
        else:
            leaves[i] = found ** alpha
    return leaves, max_priority


def weights_f64(p_leaf, total, n_filled, beta):
    w = (n_filled * np.asarray(p_leaf, np.float64) / total) ** -beta
    return w / w.max()
