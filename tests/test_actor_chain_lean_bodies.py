"""The lean actor forward chain kernel against the generic one (cstr_sac_actor_chain_fwd_f32, csrc/cstr_chain.hip).

Both write the same bits: the lean kernel changes where a workgroup's arguments come from, the order of its requests and which rows
mode, head width and input source are compiled in, never an expression, an MFMA operand or the order of a sum. Every case runs the
launch twice from identical seeded inputs, once per setting of cstr_chain_lean, and compares every buffer the launch may write byte
for byte -- head_part, a_h1, a_h2, eps_all, x_data, x_pi, x_next, out_done, out_rew and the four ring control words -- each float
buffer with 64 sentinel floats behind it that must survive. tests/test_chain_kernels.py is the fp64 statement of the launch; this
module only ties the two kernels together, at the smallest shapes at which the hand-over can go wrong: one obs and one next_obs row
group (batch 16) and two of each (32), both layouts with 256 x 256 instantiations, one, two and four tiles per workgroup, a gather
from a 3-row x 32-env ring whose indices repeat and touch ring row 0, the last row, the row at the ring position, env 0 and the last
env, the ring position advanced across the wrap and not advanced, the packed form, noise drawn and not drawn. Shapes nobody
instantiated lean (64 x 64, the (8, 4) layout, obs-only rows) run the generic kernel under both settings: the switch must not touch
them. The actor backward launch has no lean kernel (profiles/actor_chain_lean_ab.txt, section 6), hence no cases here."""
import numpy as np
import pytest
import torch as th

from _sentinel_bufs import DEV, SENT, Bufs

pytestmark = pytest.mark.gpu
H = 256
RING_ROWS, RING_ENVS = 3, 32


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


@pytest.fixture(scope="module")
def nv():
    from core import _native

    return _native


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def actor_weights(rng, D, H1, H2, hn):
    w = (rng.standard_normal((H1, D)) * 0.4, rng.standard_normal(H1) * 0.1, rng.standard_normal((H2, H1)) * 0.08, rng.standard_normal(H2) * 0.1,
         rng.standard_normal((hn, H2)) * 0.1, rng.standard_normal(hn) * 0.1)
    return [dev(v) for v in w]


def both(ops, launch):
    """launch(lean) -> {name: bytes-comparable numpy array}; the switch is restored whatever happens"""
    out = []
    for lean in (0, 1):
        was = ops.chain_lean(lean)
        try:
            out.append(launch(lean))
            th.cuda.synchronize()
        finally:
            ops.chain_lean(was)
    assert out[0].keys() == out[1].keys()
    for name in out[0]:
        a, b = out[0][name], out[1][name]
        assert a.tobytes() == b.tobytes(), f"{name}: {int((a.view(np.int32) != b.view(np.int32)).sum())} of {a.size} words differ between the two kernels"


def collect(b, written, extra):
    b.check(written=written)
    out = {name: f.cpu().numpy().copy() for name, (f, _) in b.flat.items()}
    out.update({name: t.cpu().numpy().copy().view(np.int32) for name, t in extra.items()})
    return out


# ---- forward ------------------------------------------------------------------------------------------------------------------------
# (D, A, H1, H2, B, tiles, source, advance_ring, eps_all drawn, rows)
FWD_CASES = [
    (4, 2, H, H, 16, 2, "ring", True, True, "pair"),     # SAC's launch in the replayed graph
    (4, 2, H, H, 32, 1, "ring", False, True, "pair"),
    (8, 2, H, H, 32, 4, "ring", True, False, "pair"),
    (8, 2, H, H, 16, 2, "ring", False, False, "pair"),
    (4, 2, H, H, 32, 4, "packed", False, True, "pair"),  # SAC's launch of the eager step
    (8, 2, H, H, 16, 1, "packed", False, True, "pair"),
    (4, 2, H, H, 16, 2, "packed", False, False, "pair"),
    (8, 2, H, H, 32, 2, "packed", False, False, "pair"),
    (4, 2, 64, 64, 32, 1, "ring", True, True, "pair"),   # run-time widths: the generic kernel under both settings
    (8, 4, H, H, 16, 2, "ring", True, True, "pair"),     # a layout without a lean instantiation: the same
    (4, 2, H, H, 16, 2, "ring", True, True, "obs"),      # obs-only rows: the same
]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward(ops, nv, case):
    D, A, H1, H2, B, tiles, source, advance, draw, rows = case
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H1, tiles, forward=True)
    rng = np.random.default_rng(sum(case[:6]) + 3 * advance + 5 * draw + len(source))
    W, G = D + A, ops.chain_colgroups(H2, tiles)
    pair = rows == "pair"
    mode, M = (nv.CHAIN_ROWS_PAIR, 2 * B) if pair else (nv.CHAIN_ROWS_OBS, B)
    weights = actor_weights(rng, D, H1, H2, 2 * A)
    actor = ops.sac_actor_desc(D, A, *weights)
    pos = RING_ROWS - 1 if advance else 1  # with advance_ring the position stands on the last row: the wrap sets the full flag
    ring = idx = None
    if source == "ring":
        ring = ops.DeviceRing(RING_ROWS, RING_ENVS, D, A, DEV)
        for k in ("observations", "next_observations", "actions", "rewards"):
            getattr(ring, k).copy_(dev(rng.standard_normal(tuple(getattr(ring, k).shape))))
        ring.dones.copy_(dev(rng.uniform(0, 1, (RING_ROWS, RING_ENVS)) < 0.5))
        ring.timeouts.copy_(dev(rng.uniform(0, 1, (RING_ROWS, RING_ENVS)) < 0.5))
        ri, ei = rng.integers(0, RING_ROWS, B), rng.integers(0, RING_ENVS, B)
        # ring row 0 / the last row, env 0 / the last env in every combination, the row at the ring position, a repeated pair
        ri[:8], ei[:8] = [0, 0, RING_ROWS - 1, RING_ROWS - 1, pos, pos, 1, 1], [0, RING_ENVS - 1, 0, RING_ENVS - 1, 5, 0, 7, 7]
        ri[B - 1], ei[B - 1] = ri[0], ei[0]  # ... and one across the row group (batch 32: across the two row groups)
        idx = dev(np.stack((ri, ei)), th.int32)
    x_obs, x_nxt = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
    rng_ctl = ops.new_rng_ctl(77, DEV) if draw else None
    ctl_before = None if rng_ctl is None else rng_ctl.clone()

    def launch(lean):
        b = Bufs()
        x_pi, x_next, x_data = b.new("x_pi", B, W), b.new("x_next", B, W), b.new("x_data", B, W)
        out_done, out_rew = b.new("out_done", B, 1), b.new("out_rew", B, 1)
        a_h1, a_h2, head_part = b.new("a_h1", B, H1), b.new("a_h2", B, H2), b.new("head_part", G, M, 2 * A)
        kw = dict(rows_mode=mode, head_n=2 * A)
        written, extra = ["head_part", "a_h1", "a_h2"], {}
        if draw:
            kw.update(head_rng_ctl=rng_ctl, head_rng_offset=5, eps_all=b.new("eps_all", M, A))
            written.append("eps_all")
        if source == "ring":
            ring.ctl.copy_(th.tensor([pos, 0, 0, 4]))
            ops.sac_actor_chain_fwd(actor, B, x_data, x_pi, x_next if pair else None, out_done, out_rew, a_h1, a_h2, head_part, tiles, ring=ring,
                                    sample_idx=idx, advance_ring=advance, **kw)
            written += ["x_data", "out_done", "out_rew"]
            extra["ring_ctl"] = ring.ctl
        else:
            x_pi[:, :D], x_next[:, :D] = dev(x_obs), dev(x_nxt)
            ops.sac_actor_chain_fwd(actor, B, None, x_pi, x_next, None, None, a_h1, a_h2, head_part, tiles, **kw)
        out = collect(b, written, extra)
        xp, xn = out["x_pi"][:B * W].reshape(B, W), out["x_next"][:B * W].reshape(B, W)
        assert (xp[:, D:] == np.float32(SENT)).all() and (xn[:, D:] == np.float32(SENT)).all(), lean  # the action columns belong to the next launch
        if source == "ring":
            assert ring.ctl.tolist() == ([0, 1, 0, 5] if advance else [pos, 0, 0, 4]), lean
            o = (ri, ei)
            assert np.array_equal(xp[:, :D], ring.observations.cpu().numpy()[o]), lean
            if pair:
                assert np.array_equal(xn[:, :D], ring.next_observations.cpu().numpy()[o]), lean
            xd = out["x_data"][:B * W].reshape(B, W)
            assert np.array_equal(xd[:, :D], xp[:, :D]) and np.array_equal(xd[:, D:], ring.actions.cpu().numpy()[o]), lean
            assert np.array_equal(out["out_rew"][:B], ring.rewards.cpu().numpy()[o]), lean
            assert np.array_equal(out["out_done"][:B], (ring.dones.cpu().numpy()[o] * (np.float32(1) - ring.timeouts.cpu().numpy()[o])).astype(np.float32)), lean
        else:
            assert all(bool((out[k] == np.float32(SENT)).all()) for k in ("x_data", "out_done", "out_rew")), lean
        if draw:
            assert th.equal(rng_ctl, ctl_before), lean  # the launch only reads the stream position
        return out

    both(ops, launch)
    del weights
