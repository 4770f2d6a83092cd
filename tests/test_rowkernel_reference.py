"""CPU checks of tests/_rowkernel_reference.py: the comparator of tests/test_rowkernels.py accepts the float32 evaluation of every
statement and rejects the mistakes such kernels make. No GPU.

The bars: per output kind the float32 ATen evaluation of the statement is re-measured over the GPU module's own cases in units of
2**-24 * M; it must pass its bar, the bar must be four times that figure (ATen builds differ a little: within a factor of two either
way; a kind that float32 evaluates exactly keeps a bar of 2 units, one rounding of the result and one of the comparison) and no bar may
exceed 64 units. The drawn normals: the float32 NumPy Box-Muller against the fp64 one over the drawn launches of the GPU module, four times its worst error is
the bar, not above 1e-5.

The ties: every explicit backward statement equals fp64 autograd through the forward statement (1e-9 of the tensor's scale), and
normal_stream equals the counter contract worked by hand on _dqn_helpers.philox4x32_10 (element order, odd tail, 64-bit carry).

The teeth: each listed mutation of the fp64 statement is rejected by the comparator at the bars, on the GPU module's cases.

The input conditions (a) and (b) of the sweep cases are asserted here and again in the GPU module before each launch."""
import numpy as np
import pytest
import torch as th

import _rowkernel_reference as R


@pytest.fixture(scope="module")
def aten():
    return R.measure_aten()


EXACT_FLOOR = 2.0  # the bar of a kind whose float32 evaluation is exact or nearly so


def test_float32_aten_passes_every_bar_and_no_bar_exceeds_the_cap(aten):
    assert set(aten) == set(R.BARS)
    for kind, fig in sorted(aten.items()):
        print(f"ATEN {kind}: {fig:.3f} units, bar {R.BARS[kind]:.2f}")
        assert fig <= R.BARS[kind] <= R.CAP, (kind, fig)
        assert R.BARS[kind] <= max(8.0 * fig, EXACT_FLOOR) and R.BARS[kind] >= min(2.0 * fig, EXACT_FLOOR), (kind, fig, R.BARS[kind])


def test_float32_box_muller_sets_the_bar_of_the_drawn_normals():
    w, ws = R.measure_normals()
    print(f"NORMALS float32 NumPy Box-Muller vs fp64: worst {w:.3g}, inside the slack elements {ws:.3g} beyond the slack; bar {R.NORMAL_BAR:.3g}")
    assert w <= R.NORMAL_BAR <= R.NORMAL_CAP and ws <= R.NORMAL_BAR
    assert 2.0 * w <= R.NORMAL_BAR <= 8.0 * w
    for n, seed, base, tag in R.draw_cases():
        share = float((R.normal_slack(seed, base, n, tag) > 0).mean())
        assert share <= 1e-3 and (n > 1000 or share == 0), (n, share)
        assert R.normal_accepts(R.normal_stream(seed, base, n, tag, np.float32), seed, base, n, tag)
    assert sum(n > 2 * R.GRID_PAIRS for n, _, _, _ in R.draw_cases()) >= 6  # the three drawing kernels, first and second launch


def test_normal_stream_statement():
    """the stream by hand for one pair, element order, the odd tail, the 64-bit counter carry"""
    from _dqn_helpers import philox4x32_10

    seed, base = (5 << 32) | 9, 2 ** 32 - 1
    z = R.normal_stream(seed, base, 5, R.SDE_TAG)
    for p in range(3):
        ctr = base + p
        r = philox4x32_10(np.array([[ctr & 0xFFFFFFFF, ctr >> 32, 0, R.SDE_TAG]], np.uint32), np.array([9, 5], np.uint64))[0]
        u1, u2 = ((int(r[0]) >> 8) + 0.5) / 2 ** 24, ((int(r[1]) >> 8) + 0.5) / 2 ** 24
        rad = np.sqrt(-2 * np.log(u1))
        assert z[2 * p] == rad * np.cos(2 * np.pi * u2)
        if 2 * p + 1 < 5:
            assert z[2 * p + 1] == rad * np.sin(2 * np.pi * u2)
    assert np.array_equal(R.normal_stream(seed, base + 1, 3, R.SDE_TAG), z[2:5])
    big = R.normal_stream(3, 0, 200001, R.BCQ_TAG)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01


def test_sweep_cases_meet_the_input_conditions():
    seen, engaged = set(), []
    for si, (B, L, A) in enumerate(R.SDE_SHAPES):
        for vi, (full, expln, noise, below, clip) in enumerate(R.sde_variants(si)):
            seen |= {("below", noise, below), ("clip", noise, clip)}
            inp = R.sde_case(si, vi)
            f, m = R.sde_fwd_stmt(inp), R.sde_fwd_stmt(inp, mag=True)
            sat = R.sat_rows(f["x"].numpy())
            assert R.hardtanh_margin(f["pre"].numpy(), m["pre"].numpy(), clip, R.BARS["pre"]) >= 1.0
            assert sat.sum() <= (B // 16 if B >= 16 else 0)
            if L >= 63:
                assert (inp["log_std"] > 0).any() and (inp["log_std"] < 0).any()
            if clip > 0:
                engaged.append(np.abs(f["pre"].numpy()).reshape(-1) >= clip)
    assert 0.1 <= float(np.concatenate(engaged).mean()) <= 0.3  # the Hardtanh is engaged on part of the sweep
    for noise in R.SDE_NOISE:  # every value of below_act and clip_mean meets every noise form
        assert all(("below", noise, b) in seen for b in (0, 1, 2)) and all(("clip", noise, c) in seen for c in (1.0, 0.0))


def _scale_close(a, b, what):
    a, b = a.detach().numpy(), b.detach().numpy()
    assert np.abs(a - b).max() <= 1e-9 * max(np.abs(b).max(), 1e-30), what


@pytest.mark.parametrize("si", range(len(R.SDE_SHAPES)))
def test_explicit_sde_backward_equals_autograd(si):
    """fp64 autograd through get_std, the matrices and the head forward, against sde_bwd_stmt / sde_param_stmt on the fp64 forward"""
    for vi in range(12):
        inp = R.sde_case(si, vi)
        A, noise = inp["w"].shape[0], inp["noise"]
        h, w, b, ls = (th.as_tensor(inp[k], dtype=th.float64).requires_grad_(True) for k in ("h", "w", "b", "log_std"))
        std = R.sde_std_stmt(ls, inp["expln"], A)
        z = th.as_tensor(inp["z"], dtype=th.float64)
        mats = None if noise == "mode" else (z * std if noise == "per_row" else z[0] * std)
        f = R.sde_fwd_stmt(dict(inp, h=h, w=w, b=b, std=std, mats=mats))
        loss = (f["action"] * th.as_tensor(inp["g_action"], dtype=th.float64)).sum() + (f["logp"] * th.as_tensor(inp["g_logp"], dtype=th.float64)).sum()
        loss.backward()
        aux = th.cat((f["pre"], f["var"]), 1).detach().numpy()
        binp = dict(inp, std=std.detach().numpy(), mats=None if mats is None else mats.detach().numpy(), action=f["action"].detach().numpy(), aux=aux)
        bw = R.sde_bwd_stmt(binp)
        hv = th.as_tensor(inp["h"], dtype=th.float64)
        below = {0: th.ones_like(hv), 1: (hv > 0).double(), 2: 1.0 - hv * hv}[inp["below"]]
        _scale_close(bw["dh"], h.grad * below, "dh")  # h.grad is d / d(latent); the statement carries the activation gradient below it
        pinp = dict(binp, z=inp["z"][0] if noise == "shared" else None, **{k: bw[k].numpy() for k in ("g_pre", "g_x", "g_var")})
        pg = R.sde_param_stmt(pinp)
        _scale_close(pg["dw"], w.grad, "dw"), _scale_close(pg["db"], b.grad, "db")
        if noise != "per_row":  # one shared z: the launch's d log_std is the whole gradient
            _scale_close(pg["dlog_std"], ls.grad, "dlog_std")


def test_explicit_bcq_backward_equals_autograd():
    for i, (B, D, L) in enumerate(R.BCQ_LATENT_SHAPES):
        inp = R.bcq_latent_inputs(R.BCQ_SEED_BASE + i, B, D, L)
        p = th.as_tensor(inp["params"], dtype=th.float64).requires_grad_(True)
        s = th.exp(th.clamp(p[:, L:], R.BCQ_LS_MIN, R.BCQ_LS_MAX))
        z = p[:, :L] + s * th.as_tensor(inp["eps"], dtype=th.float64)
        gm, gs = th.as_tensor(inp["g_mean_kl"], dtype=th.float64), th.as_tensor(inp["g_std_kl"], dtype=th.float64)
        ((z * th.as_tensor(inp["g_z"], dtype=th.float64)).sum() + (p[:, :L] * gm).sum() + (s * gs).sum()).backward()
        bw = R.bcq_latent_bwd_stmt(dict(inp, std=s.detach().numpy()))
        _scale_close(bw["bcq_g_mean"], p.grad[:, :L], "g_mean")
        assert np.abs(bw["bcq_g_ls"].numpy() - p.grad[:, L:].numpy()).max() <= 1e-9 * np.abs(p.grad[:, L:].numpy()).max()
    for i, (B, A, L) in enumerate(R.BCQ_VAE_SHAPES):
        inp = R.bcq_vae_inputs(R.BCQ_SEED_BASE + 100 + i, B, A, L)
        r, m, s = (th.as_tensor(v, dtype=th.float64).requires_grad_(True) for v in (inp["recon"], inp["params"][:, :L], inp["std"]))
        a = th.as_tensor(inp["act"], dtype=th.float64)
        loss = th.nn.functional.mse_loss(r, a) + 0.5 * (-0.5 * (1 + th.log(s.pow(2)) - m.pow(2) - s.pow(2)).mean())  # bcq.py:145-149
        loss.backward()
        st = R.bcq_vae_stmt(inp)
        _scale_close(st["vae_loss"], loss.reshape(1), "loss"), _scale_close(st["vae_g_recon"], r.grad, "g_recon")
        _scale_close(st["vae_g_mean"], m.grad, "g_mean"), _scale_close(st["vae_g_std"], s.grad, "g_std")
    inp = R.bcq_perturb_inputs(R.BCQ_SEED_BASE + 3002, 257, 3)
    p = th.as_tensor(inp["p"], dtype=th.float64).requires_grad_(True)
    out = th.clamp(th.as_tensor(inp["a_vae"], dtype=th.float64) + float(np.float32(inp["mp"])) * p, -1.0, 1.0)
    (out * th.as_tensor(inp["g"], dtype=th.float64)).sum().backward()
    st = R.bcq_perturb_stmt(inp)
    _scale_close(st["perturb"], out, "perturb"), _scale_close(st["perturb_g"], p.grad, "perturb_g")


# ---- teeth --------------------------------------------------------------------------------------------------------------------------------
def _sde_bwd_case(si, vi):
    inp = R.sde_case(si, vi)
    f = R.sde_fwd_stmt(inp)
    return inp, R.sde_bwd_inputs(inp, f["action"].numpy(), th.cat((f["pre"], f["var"]), 1).numpy()), ~R.sat_rows(f["x"].numpy())


def _variants(si, **want):
    names = ("full", "expln", "noise", "below", "clip")
    return [vi for vi, v in enumerate(R.sde_variants(si)) if all(dict(zip(names, v))[k] == x for k, x in want.items())]


def _rejects(kind, wrong, ref, mag, what):
    """1 when the comparator rejects the wrong statement; 0 when the case cannot see the mistake (the two statements coincide on it)"""
    assert R.accepts(kind, ref, ref, mag)
    if np.array_equal(wrong, ref):
        return 0
    fig = R.worst(wrong, ref, mag)[0]
    print(f"TEETH {what} {kind}: {fig:.3g} units against a bar of {R.BARS[kind]:.2f}")
    assert not R.accepts(kind, wrong, ref, mag), (what, kind, fig)
    return 1


@pytest.mark.parametrize("mut,kind", [("no_var", "dh"), ("no_below", "dh"), ("hardtanh_open", "g_pre")])
def test_comparator_rejects_the_head_backward_mistake(mut, kind):
    hit = 0
    for si in range(1, len(R.SDE_SHAPES)):
        want = dict(clip=1.0) if mut == "hardtanh_open" else {}
        for vi in _variants(si, **want):
            inp, binp, keep = _sde_bwd_case(si, vi)
            if (mut == "no_below" and inp["below"] == 0) or (mut == "hardtanh_open" and inp["h"].shape[0] < 3):
                continue
            ref, wrong, mag = (R.np64(R.sde_bwd_stmt(binp, mag=m, mut=u)) for m, u in ((False, None), (False, mut), (True, None)))
            hit += _rejects(kind, wrong[kind][keep], ref[kind][keep], mag[kind][keep], f"{mut} {R.SDE_SHAPES[si]} variant {vi}")
    assert hit >= 7


@pytest.mark.parametrize("mut,kind", [("ls_nosum", "dlog_std"), ("expln_exp", "dlog_std"), ("db_256", "db"), ("dw_tail", "dw")])
def test_comparator_rejects_the_parameter_gradient_mistake(mut, kind):
    hit = 0
    for si, (B, L, A) in enumerate(R.SDE_SHAPES):
        if (mut == "db_256" and B <= 256) or (mut == "dw_tail" and L % 64 == 0) or (mut == "ls_nosum" and A == 1) or (mut == "expln_exp" and L < 63):
            continue
        want = dict(full=False) if mut == "ls_nosum" else (dict(expln=True) if mut == "expln_exp" else {})
        for vi in _variants(si, **want):
            inp, binp, _ = _sde_bwd_case(si, vi)
            if inp["noise"] == "per_row":
                continue
            bw = R.sde_bwd_stmt(binp)
            pinp = dict(inp, z=inp["z"][0] if inp["noise"] == "shared" else None, **{k: bw[k].numpy().astype(np.float32) for k in ("g_pre", "g_x", "g_var")})
            ref, wrong, mag = (R.np64(R.sde_param_stmt(pinp, mag=m, mut=u)) for m, u in ((False, None), (False, mut), (True, None)))
            hit += _rejects(kind, wrong[kind], ref[kind], mag[kind], f"{mut} {R.SDE_SHAPES[si]} variant {vi}")
    assert hit >= 2


def test_comparator_rejects_open_bcq_clamp_masks():
    for i, (B, D, L) in enumerate(R.BCQ_LATENT_SHAPES):
        inp = R.bcq_latent_inputs(R.BCQ_SEED_BASE + i, B, D, L)
        inp["std"] = R.bcq_latent_fwd_stmt(inp)["std"].numpy().astype(np.float32)
        ref, wrong, mag = (R.np64(R.bcq_latent_bwd_stmt(inp, mag=m, mut=u)) for m, u in ((False, None), (False, "clamp_open"), (True, None)))
        assert _rejects("bcq_g_ls", wrong["bcq_g_ls"], ref["bcq_g_ls"], mag["bcq_g_ls"], f"clamp_open latent {(B, D, L)}")
    for rows in R.BCQ_PERTURB_ROWS:
        for A in R.BCQ_PERTURB_ACT:
            inp = R.bcq_perturb_inputs(R.BCQ_SEED_BASE + 1000 * rows + A, rows, A)
            ref, wrong, mag = (R.np64(R.bcq_perturb_stmt(inp, mag=m, mut=u)) for m, u in ((False, None), (False, "clamp_open"), (True, None)))
            assert _rejects("perturb_g", wrong["perturb_g"], ref["perturb_g"], mag["perturb_g"], f"clamp_open perturb {(rows, A)}")


def test_comparator_rejects_a_swapped_grouping_and_the_last_maximum():
    for i, (n, S, N) in enumerate(R.BCQ_TARGET_CASES):
        inp = R.bcq_target_inputs(R.BCQ_SEED_BASE + 300 + i, n, S, N)
        sel, cand = inp["q"][0], np.random.default_rng(i).uniform(-1, 1, (n * S, 2)).astype(np.float32)
        idx, act = R.bcq_select_stmt(sel, cand, n, S)
        idx_l, act_l = R.bcq_select_stmt(sel, cand, n, S, mut="last_max")
        if S >= 10 and n >= 64:  # one-decimal Q values over >= 10 candidates of >= 64 states: some state has its maximum twice
            assert not np.array_equal(idx, idx_l) and not np.array_equal(act, act_l), (n, S)
        if n == 1 or S == 1:
            continue  # one group either way
        for grouping in (0, 1):
            ref, wrong, mag = (R.np64(R.bcq_target_stmt(inp, grouping, mag=m, mut=u)) for m, u in ((False, None), (False, "group_swap"), (True, None)))
            assert _rejects("target", wrong["target"], ref["target"], mag["target"], f"group_swap {(n, S, N)} grouping {grouping}")
            assert not np.array_equal(ref["max_q"], wrong["max_q"])


@pytest.mark.parametrize("mut", ["half_advance", "no_hi", "other_tag"])
def test_comparator_rejects_the_stream_mistake(mut):
    hit = 0
    first = R.draw_cases()[:len(R.draw_cases()) // 2]
    for n, seed, base, tag in first:  # judged on the second launch of each control block: its offset is base + pairs
        pairs = (n + 1) // 2
        if mut == "half_advance" and pairs < 2:
            continue
        if mut == "no_hi" and base + 2 * pairs < 2 ** 32:
            continue  # the high word is zero throughout: the case cannot see it
        wrong = R.mutated_stream(seed, base + pairs, n, tag, mut, launch_pairs=pairs)
        err = np.abs(wrong - R.normal_stream(seed, base + pairs, n, tag))
        print(f"TEETH {mut} n {n} base {base}: worst {err.max():.3g}, median {np.median(err):.3g} against a bar of {R.NORMAL_BAR:.3g}")
        assert not R.normal_accepts(wrong, seed, base + pairs, n, tag)
        hit += 1
    assert hit >= 4
