"""Self-checks of the ARS restatement (tests/_ars_reference.py), CPU only; they pass with or without the feature: the update against a
direct torch transcription of the published lines, the delta stream's moments and reproducibility, its Philox against the Python-int
restatement of tests/_collect_reference.py, and the tie / NaN orderings against torch.argsort(descending=True) where torch's order is
defined."""
import numpy as np
import torch as th

import _ars_reference as ref
import _collect_reference as cref


def _published_update(theta, returns, n_delta, n_top, lr, delta):
    """sb3_contrib/ars/ars.py, _do_one_update, on float64 tensors"""
    candidate_returns = th.as_tensor(returns, dtype=th.float64)
    deltas, weights = th.as_tensor(delta, dtype=th.float64), th.as_tensor(theta, dtype=th.float64)
    plus_returns, minus_returns = candidate_returns[:n_delta], candidate_returns[n_delta:]
    top_returns, _ = th.max(th.vstack((plus_returns, minus_returns)), dim=0)
    top_idx = th.argsort(top_returns, descending=True)[:n_top]
    plus_returns, minus_returns, deltas = plus_returns[top_idx], minus_returns[top_idx], deltas[top_idx]
    return_std = th.cat([plus_returns, minus_returns]).std()
    step_size = lr / (n_top * return_std + 1e-6)
    return weights + step_size * ((plus_returns - minus_returns) @ deltas), float(step_size), float(return_std), top_idx.numpy()


def test_update_equals_the_published_lines():
    rng = np.random.default_rng(0)
    for n_delta, n_top, p in ((1, 1, 3), (5, 2, 36), (8, 8, 77), (33, 7, 130)):
        theta = rng.normal(size=p).astype(np.float32)
        returns = rng.normal(size=2 * n_delta) * 10 - 50  # distinct with probability 1: torch's order is defined
        delta = ref.deltas(11, 3, n_delta, p)
        new, step, std, kept = ref.update(theta, returns, n_delta, n_top, 0.02, delta)
        want, w_step, w_std, w_idx = _published_update(theta, returns, n_delta, n_top, 0.02, delta)
        assert np.array_equal(kept, w_idx)
        assert abs(step - w_step) <= 1e-12 * abs(w_step) and abs(std - w_std) <= 1e-12 * abs(w_std)
        np.testing.assert_allclose(new, want.numpy(), rtol=1e-12, atol=1e-14)


def test_delta_stream_moments_and_reproducibility():
    d = ref.deltas(5, 2, 50, 2000)  # 1e5 draws
    assert d.dtype == np.float32 and d.shape == (50, 2000) and np.isfinite(d).all()
    assert abs(float(d.mean())) < 4 / np.sqrt(d.size)                     # 4 sigma of the mean of 1e5 N(0, 1) draws
    assert abs(float(d.var()) - 1.0) < 4 * np.sqrt(2.0 / d.size)           # 4 sigma of their variance
    assert np.array_equal(d, ref.deltas(5, 2, 50, 2000))
    assert np.array_equal(d[7:9, :37], ref.deltas(5, 2, 9, 37)[7:9])       # (seed, update, k, p) alone decide a value
    assert not np.array_equal(d[:, :8], ref.deltas(5, 3, 50, 8)) and not np.array_equal(d[:, :8], ref.deltas(6, 2, 50, 8))


def test_philox_equals_the_python_int_restatement():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2**32, (16, 4), dtype=np.uint64).astype(np.uint32)
    seed = 0x0123456789ABCDEF
    got = ref.philox4x32_10(c, seed)
    for i in range(16):
        assert tuple(int(x) for x in got[i]) == cref.philox_block(c[i], (seed & 0xFFFFFFFF, seed >> 32))


def test_tie_and_nan_orderings():
    nan = float("nan")
    # distinct values, a NaN among them: torch puts the NaN first in a descending sort
    plus, minus = np.array([1.0, 5.0, nan, 2.0, 0.0]), np.array([0.5, 1.0, 3.0, 4.0, -1.0])
    top = th.maximum(th.as_tensor(plus), th.as_tensor(minus))
    for n_top in (1, 2, 5):
        assert np.array_equal(ref.ranking(np.concatenate([plus, minus]), 5, n_top), th.argsort(top, descending=True)[:n_top].numpy())
    # a NaN in R- alone still makes the direction the greatest
    assert ref.ranking(np.array([1.0, 2.0, 3.0, 0.0, nan, 0.0]), 3, 1).tolist() == [1]
    # ties go to the lower k: what a stable descending sort gives
    plus, minus = np.array([3.0, 7.0, 7.0, 1.0, 7.0]), np.array([7.0, 0.0, 2.0, 1.0, 6.0])
    top = th.maximum(th.as_tensor(plus), th.as_tensor(minus))
    want = th.sort(top, descending=True, stable=True).indices.numpy()
    assert np.array_equal(ref.ranking(np.concatenate([plus, minus]), 5, 5), want) and want.tolist() == [0, 1, 2, 4, 3]
    # equal returns: std 0, the step size is lr / 1e-6 and theta does not move
    new, step, std, kept = ref.update(np.ones(4, np.float32), np.full(10, -3.0), 5, 5, 0.02, ref.deltas(1, 0, 5, 4))
    assert std == 0.0 and step == 0.02 / 1e-6 and kept.tolist() == [0, 1, 2, 3, 4] and np.array_equal(new, np.ones(4))
    # a kept NaN: every parameter becomes NaN
    new, step, std, kept = ref.update(np.ones(4, np.float32), np.array([1.0, nan, 2.0, 0.0, 0.0, 0.0]), 3, 1, 0.02, ref.deltas(1, 0, 3, 4))
    assert kept.tolist() == [1] and np.isnan(step) and np.isnan(new).all()
