"""CPU checks of tests/_chain_reference.py: the comparator of tests/test_chain_kernels.py accepts the float32 ATen evaluation of every
launch's statement and rejects the mistakes such kernels make. No GPU.

The bars: for every output kind the float32 ATen evaluation is re-measured over the GPU tests' own cases, in units of 2**-24 * M; it
must pass its bar, the bar must be four times that figure (ATen builds differ a little: within a factor of two either way) and no
bar may exceed 64 units.

The teeth: on widths with a ragged reduction (K = 20 and K = 300) the fp64 statement is compared with a deliberately wrong fp64
statement, per output kind the mistake reaches, and the comparator must reject it: the last 4 columns of K left out, one column group's
partial dropped or counted twice, b3 of twin 0 used for twin 1, the next rows read from the pi rows, `done` without (1 - done), relu'(h1)
of the other twin, a tile's 16 columns shifted by one tile, `scale` applied twice, dW accumulated over B - 16 rows. (The alpha part's
outputs depend on none of these; every other kind is reached by at least one.)

The Adam parameter statement that the GPU test feeds the launch's own moments (adam_param_f32) is tied to oracle/cstr_oracle.c's
adam_f32_cpu bit for bit."""
import numpy as np
import pytest

import _chain_reference as R

TEETH_SHAPES = [(20, 20, 48), (300, 300, 16)]  # (H1, H2, B): K = 20 and K = 300 in every hidden reduction, two and 19 column groups
D, A = 4, 2


@pytest.fixture(scope="module")
def aten():
    return R.measure_aten()


def test_float32_aten_passes_every_bar_and_no_bar_exceeds_the_cap(aten):
    assert set(aten) == set(R.BARS)
    for kind, fig in sorted(aten.items()):
        print(f"ATEN {kind}: {fig:.3f} units, bar {R.BARS[kind]:.2f}")
        assert fig <= R.BARS[kind], (kind, fig)
        assert R.BARS[kind] <= R.CAP, kind
        assert 2.0 * fig <= R.BARS[kind] <= 8.0 * fig, (kind, fig, R.BARS[kind])  # 4 x ATen, whatever BLAS build measures it
    assert max(R.BARS["h1"], R.BARS["h2"]) <= R.MARGIN_BAR


def _launch(name, shape, mut=None, mag=False):
    H1, H2, B = shape
    if name == "actor_fwd":
        return R.actor_fwd_stmt(R.actor_fwd_inputs(11, D, A, H1, H2, 2 * B, 2 * A), 1, mag=mag, mut=mut)
    if name == "q_fwd":
        inp = R.q_fwd_inputs(12, D, A, H1, H2, B, 1)
        return R.q_fwd_stmt(inp["xs"][0], inp["nets"][0], 1, mag=mag, mut=mut)
    if name.startswith("q_bwd"):
        mode = name[6:]
        return R.q_bwd_stmt(R.q_bwd_inputs(13, D, A, H1, H2, B, mode, 1, with_alpha=mode == "td"), 1, mag=mag, mut=mut, with_gact=mode != "td")
    if name.startswith("actor_bwd"):
        return R.actor_bwd_stmt(R.actor_bwd_inputs(14, D, A, H1, H2, B, name[10:], 2, 3), mag=mag, mut=mut)
    assert name == "wgrad"
    return R.wgrad_stmt(R.wgrad_inputs(15, 3 * B, H1, H2), mag=mag, mut=mut)


TEETH = [
    ("k_tail", "actor_fwd", ("h2", "head_part")), ("k_tail", "q_fwd", ("h2", "q_part")), ("k_tail", "q_bwd_sac_actor", ("dz1", "gact_part")),
    ("k_tail", "q_bwd_td", ("dz1",)), ("k_tail", "actor_bwd_gauss", ("dz1",)), ("k_tail", "actor_bwd_det", ("dz1",)),
    ("drop_group", "q_bwd_td", ("q_out", "target_out", "gq_out", "loss", "dz2", "dz1")), ("drop_group", "q_bwd_neg_mean", ("q_out", "loss")),
    ("drop_group", "actor_bwd_gauss", ("dz2", "dz1")), ("drop_group", "actor_bwd_det", ("dz2", "dz1")),
    ("dup_group", "q_bwd_td", ("q_out", "target_out", "gq_out", "loss", "dz2", "dz1")), ("dup_group", "q_bwd_sac_actor", ("q_out", "loss")),
    ("dup_group", "actor_bwd_gauss", ("dz2", "dz1")), ("dup_group", "actor_bwd_det", ("dz2", "dz1")),
    ("b3_twin", "q_bwd_td", ("q_out", "gq_out", "loss", "dz2", "dz1")), ("b3_twin", "q_bwd_sac_actor", ("q_out", "loss")),
    ("done_raw", "q_bwd_td", ("target_out", "gq_out", "loss", "dz2", "dz1")),
    ("relu_twin", "q_bwd_td", ("dz1",)), ("relu_twin", "q_bwd_sac_actor", ("dz1", "gact_part")),
    ("tile_shift", "actor_fwd", ("h1", "h2", "head_part")), ("tile_shift", "q_fwd", ("h1", "h2", "q_part")), ("tile_shift", "q_bwd_td", ("dz1",)),
    ("tile_shift", "q_bwd_neg_mean", ("dz1", "gact_part")), ("tile_shift", "actor_bwd_gauss", ("dz1",)),
    ("scale_twice", "q_bwd_td", ("gq_out", "loss", "dz2", "dz1")),
    ("rows_short", "wgrad", ("dw", "db")),
]


@pytest.mark.parametrize("shape", TEETH_SHAPES, ids=lambda s: "K%d" % s[0])
@pytest.mark.parametrize("mut,launch,kinds", TEETH, ids=lambda v: v if isinstance(v, str) else None)
def test_comparator_rejects_the_mistake(mut, launch, kinds, shape):
    ref, wrong, mag = R.np64(_launch(launch, shape)), R.np64(_launch(launch, shape, mut=mut)), R.np64(_launch(launch, shape, mag=True))
    for k in kinds:
        assert R.accepts(k, ref[k], ref[k], mag[k])
        fig = R.worst(wrong[k], ref[k], mag[k])[0]
        print(f"TEETH {mut} {launch} {k}: {fig:.3g} units against a bar of {R.bar_of(k):.2f}")
        assert not R.accepts(k, wrong[k], ref[k], mag[k]), (mut, launch, k, fig)


@pytest.mark.parametrize("shape", TEETH_SHAPES, ids=lambda s: "K%d" % s[0])
def test_comparator_rejects_next_rows_read_from_the_pi_rows(shape):
    """next_offset = 0: the target critics' action columns come from the pi(obs) rows of the actor pass. The finalised actions miss
    the head's tolerance, and every matrix stage of the Q forward launch behind them misses its bar."""
    H1, H2, B = shape
    act_in = R.actor_fwd_inputs(21, D, A, H1, H2, 2 * B, 2 * A)
    part = R.actor_fwd_stmt(act_in, 1)["head_part"].numpy().astype(np.float32)
    eps = np.random.default_rng(22).standard_normal((2 * B, A)).astype(np.float32)
    a_next, lp_next = R.fin_gaussian(R.params_f32(part, act_in["b3"], B, B), eps[B:])
    a_wrong, lp_wrong = R.fin_gaussian(R.params_f32(part, act_in["b3"], 0, B), eps[:B])
    assert np.abs(a_wrong - a_next).max() > 5e-6 and (np.abs(lp_wrong - lp_next) / np.maximum(np.abs(lp_next), 1.0)).max() > 1e-4
    q_in = R.q_fwd_inputs(23, D, A, H1, H2, B, 1)
    x = q_in["xs"][0].copy()
    x_wrong = x.copy()
    x[:, D:], x_wrong[:, D:] = a_next, a_wrong
    ref, wrong, mag = (R.np64(R.q_fwd_stmt(v, q_in["nets"][0], 1, mag=m)) for v, m in ((x, False), (x_wrong, False), (x, True)))
    for k in ("h1", "h2", "q_part"):
        assert not R.accepts(k, wrong[k], ref[k], mag[k]), k


def test_every_output_kind_is_reached_by_a_mistake():
    reached = {R.KIND_OF.get(k, k) for _, _, kinds in TEETH for k in kinds}
    assert reached == set(R.BARS) - {"alpha"}


def test_a_dropped_term_of_the_widest_reduction_is_far_above_the_cap():
    """one term of a K = 512 reduction is about M / 512 = 3e4 units: the cap of 64 leaves no room for it"""
    inp = R.q_fwd_inputs(31, D, A, 512, 16, 16, 1)
    ref, mag = (R.np64(R.q_fwd_stmt(inp["xs"][0], inp["nets"][0], 1, mag=m)) for m in (False, True))
    w2 = inp["nets"][0]["w2"].astype(np.float64)
    j = int(np.argmax(ref["h1"][0]))  # an active unit of row 0
    z2_wrong = ref["z2"].copy()
    z2_wrong[0] -= ref["h1"][0, j] * w2[:, j]
    fig = np.median(R.units(z2_wrong[0], ref["z2"][0], mag["z2"][0]))
    assert fig > 100 * R.CAP, fig


def test_seed_search_leaves_a_mask_margin_and_fixes_the_seed():
    for i in (2, 3, 15):
        a, b = R.actor_fwd_case(i), R.actor_fwd_case(i)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        tiles = R.ACTOR_FWD_CASES[i][5]
        ref, mag = R.actor_fwd_stmt(a, tiles), R.actor_fwd_stmt(a, tiles, mag=True)
        assert min(R.mask_margin(p, m, R.MARGIN_BAR) for p, m in R._pre(ref, mag)) >= 1.0


def test_every_mutation_name_is_used_by_a_teeth_case():
    assert {m for m, _, _ in TEETH} == set(R.MUTATIONS)


@pytest.mark.parametrize("hyper", [dict(step=4, lr=3e-4, betas=(0.9, 0.999), eps=1e-8), dict(step=8, lr=7e-3, betas=(0.8, 0.99), eps=1e-6),
                                   dict(step=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)], ids=lambda h: "step%d" % h["step"])
def test_adam_parameter_statement_is_the_oracles_bit_for_bit(hyper):
    """adam_param_f32 on the oracle's own new moments gives the oracle's own new parameter: the two cannot drift apart"""
    from oracle import cstr_oracle as orc

    rng = np.random.default_rng(hyper["step"])
    n = 20000
    p, g = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    m, v = (1e-3 * rng.standard_normal(n)).astype(np.float32), (1e-5 * rng.uniform(0, 1, n)).astype(np.float32)
    v[:100], m[:100], g[:50] = 0.0, 0.0, 0.0  # fresh state, and elements the step leaves where they are
    b1, b2 = hyper["betas"]
    op, om, ov = orc.adam_step(p, g, m, v, hyper["step"], hyper["lr"], b1, b2, hyper["eps"])
    assert not np.array_equal(op, p)
    assert np.array_equal(R.adam_param_f32(p, om, ov, hyper["step"], hyper["lr"], hyper["betas"], hyper["eps"]), op)


def test_helpers_state_what_they_document():
    w = np.arange(20 * 36, dtype=np.float32).reshape(20, 36)
    s = R.swizzle(w)
    assert s.size == 2 * 3 * 256
    assert s[((1 * 3 + 0) * 64 + 35) * 4 + 1] == w[16 + 3, 4 * 2 + 1]  # tile 1, chunk 0, lane 35 = (r 3, h 2), e 1
    assert s[((1 * 3 + 2) * 64 + 19) * 4 + 3] == 0.0  # column 32 + 4 + 3 = 39 lies outside the matrix
    assert R.groups(40, 2) == [(0, 32), (32, 40)] and R.groups(16, 4) == [(0, 16)]
    p, t = np.float32(0.3), np.float32(-1.7)
    assert R.polyak_f32(p, t, 0.005) == np.float32(np.float64(np.float32(0.005)) * np.float64(p) + np.float64(t * np.float32(0.995)))
    parts = np.random.default_rng(0).standard_normal((3, 5, 4)).astype(np.float32)
    want = ((parts[0] + parts[1]).astype(np.float32) + parts[2]).astype(np.float32) + np.float32(0.25)
    assert np.array_equal(R.params_f32(parts, np.full(4, 0.25, np.float32), 0, 5), want.astype(np.float32))
