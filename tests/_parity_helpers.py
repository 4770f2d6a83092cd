"""Helpers of the teacher-forced parity checks (the bars of tests/test_learner_parity.py), shared by the critic-ensemble tests.

Q values / TD targets: |dq_i| <= 1e-5 * max(|q_i|, mean|q|), and per element |dq_i| / |q_i| below the bound of the code path; weights
after the steps within 2e-5 of the tensor's scale + 1e-4 relative."""
import numpy as np
import torch as th


def rel_err(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))) if a.size else 0.0


def strict_bound(label) -> float:
    """Per-element |dq_i| / |q_i| of each code path: hand-written kernels 5e-5, rocBLAS GEMMs 6e-5, stock ATen on the GPU 1e-4."""
    lab = str(label)
    return 1e-4 if lab.endswith("_aten") else 6e-5 if lab.endswith("_rocblas") else 5e-5


def q_err(got, want, label):
    """Asserts the per-element bound of `label`'s path and returns the error relative to the batch's Q scale."""
    want = np.asarray(want, np.float64)
    per = np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1e-3)
    strict = float(per.max()) if per.size else 0.0
    assert strict < strict_bound(label), (label, strict)
    return rel_err(got, want, float(np.abs(want).mean()))


def check_init(model, g, mods):
    """Seeded initial weights == the reference's: bit-exact, or via the digests of a class-default fixture."""
    for nm in mods:
        for k, v in getattr(model, nm).state_dict().items():
            a, key = v.cpu().numpy(), f"before/{nm}/{k}"
            if key in g:
                np.testing.assert_array_equal(a, g[key], err_msg=f"init {nm}/{k}")
            else:
                np.testing.assert_array_equal(a.reshape(-1)[:64], g[key + "#head"], err_msg=key)
                assert a.astype(np.float64).sum() == float(g[key + "#sum"]), key


def load_ring(model, g):
    rb = model.replay_buffer
    for name, key in (("observations", "ring_obs"), ("next_observations", "ring_next_obs"), ("actions", "ring_act"),
                      ("rewards", "ring_rew"), ("dones", "ring_done"), ("timeouts", "ring_timeout")):
        getattr(rb, name).copy_(th.as_tensor(g[key]))
    pos, full = int(g["ring_pos"]), bool(g["ring_full"])
    rb._adds = pos + (rb.buffer_size if full else 0)
    rb.ring.ctl[0], rb.ring.ctl[1] = pos, int(full)


def check_weights(model, g, prefix, modules):
    worst = 0.0
    for nm in modules:
        for k, v in getattr(model, nm).state_dict().items():
            got = v.detach().cpu().numpy()
            key = f"{prefix}/{nm}/{k}"
            if key in g:
                want = g[key]
                scale = max(float(np.abs(want).max()), 1e-3)
                err = np.abs(got - want) / (2e-5 * scale + 1e-4 * np.abs(want))
                worst = max(worst, float(err.max()))
            else:  # big tensors of a class-default fixture are stored as digests
                np.testing.assert_allclose(got.reshape(-1)[:64], g[key + "#head"], rtol=1e-4, atol=2e-5 * float(np.abs(got).max()))
                assert abs(got.astype(np.float64).sum() - float(g[key + "#sum"])) < 1e-4 * float(g[key + "#abs"]) + 1e-4
    assert worst < 1.0, worst
