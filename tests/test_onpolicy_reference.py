"""CPU checks of tests/_onpolicy_reference.py: the bars that tests/test_onpolicy_guards.py holds the PPO / A2C loss launches to past
their grid cap are loose enough for a correct float32 kernel and tight enough for a wrong one.

The float32 NumPy model of the launch (the kernel's operation order, its grid, stride loop, f64 per-thread sums, tree and partials)
stays below 0.75 of every bar at every size of CAP_SIZES, with exp(log_std) moved by -1 / 0 / +1 ulp; with each of five mistakes
injected it exceeds a bar. The chunked norm model changes with its second chunk dropped; the DQN loss model stays under its bar."""
import numpy as np
import pytest

import _onpolicy_reference as R

MARGIN = 0.75


@pytest.fixture(scope="module")
def refs():
    """every (B, A, algorithm variant) of the cap cases once: (case, fp64 reference)"""
    out = {}
    for B, A in R.CAP_SIZES:
        case = R.loss_inputs(True, B, A)
        for vf, norm in R.PPO_VARIANTS:
            out[(True, B, A, vf, norm)] = (case, R.loss_reference(case, True, vf, norm))
        case = R.loss_inputs(False, B, A)
        for norm in (True, False):
            out[(False, B, A, None, norm)] = (case, R.loss_reference(case, False, None, norm))
    return out


@pytest.mark.parametrize("B,A", R.CAP_SIZES)
def test_float32_model_stays_below_the_bars(refs, B, A):
    worst = {}
    for (ppo, b, a, vf, norm), (case, ref) in refs.items():
        if (b, a) != (B, A):
            continue
        if ppo:
            assert np.min(np.abs(np.abs(ref["ratio"] - 1) - R.CLIP_RANGE)) > 1e-3  # clip_fraction compares exactly
        for ulp in (-1, 0, 1):
            fig = R.loss_figures(R.loss_model_f32(case, ppo, vf, norm, sig_ulp=ulp), ref)
            for k, v in fig.items():
                key = ("ppo " if ppo else "a2c ") + k
                worst[key] = max(worst.get(key, 0.0), v)
    print(f"MODEL B={B} A={A}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= MARGIN, worst


# which sizes a mistake can show at: the stride loop's second pass exists above 16384 rows, the 64th partial from 16129 rows on
MISTAKE_SIZES = {"skip_second_pass": [s for s in R.CAP_SIZES if s[0] > 16384], "63_partials": [s for s in R.CAP_SIZES if s[0] > 63 * 256],
                 "row_twice": list(R.CAP_SIZES), "inv_b_grid": [s for s in R.CAP_SIZES if s[0] != 64 * 256], "vclip_open": list(R.CAP_SIZES)}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_comparator_rejects_the_mistakes(refs, mistake):
    assert MISTAKE_SIZES[mistake]
    for B, A in MISTAKE_SIZES[mistake]:
        for ppo in (True, False):
            if mistake == "vclip_open":  # needs value steps ON the bound: 0.25 is exact in float32, the generators' 0.2 is not
                if not ppo:
                    continue
                case = R.on_the_value_clip_bound(R.loss_inputs(True, B, A))
                vf, norm = 0.25, True
                ref = R.loss_reference(case, True, vf, norm)
                assert (ref["g_value"][:8] != 0).all()  # the statement passes the gradient at both ends
                assert max(R.loss_figures(R.loss_model_f32(case, True, vf, norm), ref).values()) <= MARGIN
            else:
                vf, norm = (0.2, True) if ppo else (None, True)
                case, ref = refs[(ppo, B, A, vf, norm)]
            fig = R.loss_figures(R.loss_model_f32(case, ppo, vf, norm, mistake=mistake), ref)
            over = {k: round(v, 2) for k, v in fig.items() if v > 1.0}
            print(f"TEETH {mistake} B={B} A={A} {'ppo' if ppo else 'a2c'}: over the bar {over}")
            assert over, (mistake, B, A, ppo, fig)


def test_the_terms_behind_the_sums_are_the_statement_s():
    """loss_reference asserts the tie itself (signed sums of its terms = the autograd results); here: it did so on a case with clipped
    rows on both sides, and the bars it builds are wider than the plain bar only by the sums' condition"""
    case = R.loss_inputs(True, 1030, 2)
    ref = R.loss_reference(case, True, 0.2, True)
    assert (ref["ratio"] < 0.8).any() and (ref["ratio"] > 1.2).any()
    assert ref["policy_abs"] >= abs(ref["scalars"][0]) and ref["loss_abs"] >= abs(ref["scalars"][3])
    assert (ref["log_std_abs"] >= np.abs(ref["g_log_std"])).all()
    assert 1.0 < ref["policy_abs"] / abs(ref["scalars"][0]) < 1e3


@pytest.mark.parametrize("A,seed,drawn", [(2, R.LANE_CAP + 3, False), (4, R.LANE_CAP + 5, False), (2, 3, True)])
def test_head_bars_hold_a_float32_evaluation_and_reject_a_wrong_row(A, seed, drawn):
    """the three launches of tests/test_onpolicy_guards.py past the lane cap; `drawn`: the noise is the Philox stream of seed 1234"""
    n = R.LANE_CAP + 1
    mean, log_std, eps, low, high = R.head_inputs(n, A, seed)
    if drawn:
        eps = R.normal_stream(1234, 0, n * A, R.PPO_STREAM_TAG, np.float32).reshape(n, A)
    a64, _, lp64 = R.head_f64(mean, log_std, eps, low, high)
    worst = [0.0, 0.0, 0.0, 0.0]
    for ulp in (-1, 0, 1):
        act, lp = R.head_model_f32(mean, log_std, eps, ulp)
        fa, fl = R.head_figures(act, lp, mean, log_std, eps, low, high)
        plain_a = float((np.abs(act - a64) / R.bar(a64)).max())
        plain_l = float((np.abs(lp - lp64) / R.bar(lp64)).max())
        worst = [max(w, v) for w, v in zip(worst, (fa, fl, plain_a, plain_l))]
    print(f"MODEL head n={n} A={A} drawn={drawn}: action {worst[0]:.3f}, log_prob {worst[1]:.3f} of head_bars; {worst[2]:.3f}, {worst[3]:.3f} of bar(want)")
    assert worst[0] <= MARGIN and worst[1] <= MARGIN
    act, lp = R.head_model_f32(mean, log_std, eps)
    for wrong in (dict(sig=np.float32(1 + 1e-5)), dict(shift=True)):  # sigma off by 1e-5; the last row computed from its neighbour's noise
        e = eps.copy()
        if "shift" in wrong:
            e[-1] = eps[-2]
        a2, l2 = R.head_model_f32(mean, (log_std.astype(np.float64) + np.log(float(wrong.get("sig", 1.0)))).astype(np.float32), e)
        fa, fl = R.head_figures(a2, l2, mean, log_std, eps, low, high)
        print(f"TEETH head {sorted(wrong)}: action {fa:.2f}, log_prob {fl:.2f}")
        assert max(fa, fl) > 1.0


def test_chunked_norm_model_notices_a_dropped_second_chunk():
    rng = np.random.default_rng(16385)
    g = rng.normal(size=16385).astype(np.float32)
    g[-1] = 3.0
    full, cut = R.device_norm(g), R.device_norm_first_chunk(g)
    assert full.dtype == np.float32 and full != cut
    assert abs(float(full) - np.sqrt((g.astype(np.float64) ** 2).sum())) <= 2e-6 * float(full)
    assert R.device_norm_first_chunk(g[:16384]) == R.device_norm(g[:16384])  # exactly one chunk: nothing to drop


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("B", [16384, 16385, 32769])
def test_dqn_loss_model_stays_below_its_bar(B, K):
    q, nq, index, rew, done = R.dqn_cap_case(B, K)
    want = R.dqn_loss_f64(q, nq, index, rew, done, 0.99)[2]
    got = R.dqn_loss_model_f32(q, nq, index, rew, done, 0.99)
    fig = abs(float(got) - want) / float(R.bar(want))
    print(f"MODEL dqn loss B={B} K={K}: {fig:.3f}")
    assert fig <= MARGIN
    drop = R.dqn_loss_model_f32(q[:-1], nq[:-1], index[:-1], rew[:-1], done[:-1], 0.99) * np.float32((B - 1) / B)  # the last row dropped, / B kept
    assert abs(float(drop) - want) / float(R.bar(want)) > 1.0
