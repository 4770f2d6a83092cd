"""GPU checks of the row-chain kernels (csrc/cstr_chain.hip) and of cstr_linear_bwd_weight_adam_sets_f32, launch by launch.

Every launch is compared with the fp64 statement of its own contract (tests/_chain_reference.py) on the float32 inputs it reads.
Matrix-stage outputs are measured per element in units of 2**-24 * M, M from the statement's magnitude pass; the bar of an output kind
is four times the worst figure of the float32 ATen evaluation of the same statement over the cases of this module (measured on the
CPU, re-checked by tests/test_chain_reference.py; no bar above 64 units). A `BAR ...` line is printed before every assertion.

    kind        ATen     bar    kernel worst
    h1          3.320  13.29    2.440
    h2          1.156   4.63    0.945
    partials    0.346   1.39    0.352
    q_out       2.532  10.13    2.532
    target_out  1.724   6.90    1.724
    gq_out      1.787   7.15    1.787
    loss        0.409   1.64    0.586
    alpha       1.100   4.40    1.813
    dz2         2.696  10.79    2.696
    dz1         1.885   7.54    1.375
    gact_part   0.565   2.26    0.265
    dw          4.547  18.19    1.740
    db          0.959   3.84    1.189

Transcendental stages (head finalisation, head backward) are compared with the fp64 formula applied to the launch's own upstream
output at the tolerances tests/test_hip_mlp_glue.py applies to the unfused Gaussian head: actions 5e-6, log-probs 1e-4, the head's
gradient 2e-6; per element |got - want| / max(|want|, floor), the floor 1 for actions and log-probs and max(1, max |reference|) for the
head's gradient, as that module sets them. Kernel worst: actions 8.3e-8, log-probs 2.0e-5, head gradient 4.6e-8. Gathers, partial-sum finalisations, shadow copies, soft target
updates and control words are compared bit for bit. Every output buffer is filled with a sentinel and followed by 64 sentinel floats;
every launch runs twice and must repeat itself bit for bit. The 256 x 256 and 400 x 300 cases run the exact-width instantiations
(tests/test_exact_shapes.py ties the run-time-width kernels at those widths to them)."""
import numpy as np
import pytest
import torch as th

import _chain_reference as R
from _parity_helpers import rel_err
from _sentinel_bufs import DEV, PAD, SENT, Bufs  # noqa: F401

pytestmark = pytest.mark.gpu
FIGS, TOLS = {}, {}


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


def host(t):
    return t.detach().cpu().numpy()


def bar(kind, got, want, mag, what, bad):
    """the kernel's worst element of one output in units of 2**-24 * M: printed, recorded, judged against the kind's bar"""
    got = host(got) if isinstance(got, th.Tensor) else got
    want, mag = (host(v) if isinstance(v, th.Tensor) else v for v in (want, mag))
    fig, at = R.worst(got, want, mag)
    key = R.KIND_OF.get(kind, kind)
    FIGS[key] = max(FIGS.get(key, 0.0), fig)
    g, w = np.asarray(got, np.float64).reshape(-1)[at], np.asarray(want, np.float64).reshape(-1)[at]
    print(f"BAR {what} {kind}: {fig:.3f} of {R.bar_of(kind):.2f} units (got {g:.9g}, want {w:.9g}, element {at})")
    if not fig <= R.bar_of(kind):
        bad.append((what, kind, round(fig, 3)))


def tol(kind, got, want, limit, what, bad, floor=1.0):
    """transcendental stages: the worst element of |got - want| / max(|want|, floor) against the unfused head's tolerance. Actions and
    log-probs: floor 1 (test_gaussian_head_with_its_linear_inside); the head's gradient: floor max(1, max |reference|)
    (test_gaussian_head_backward_carried_through_its_linear)"""
    got, want = host(got) if isinstance(got, th.Tensor) else got, np.asarray(want, np.float64)
    err = rel_err(got, want, floor)
    TOLS[kind] = max(TOLS.get(kind, 0.0), err)
    print(f"BAR {what}: {err / limit:.3f} (error {err:.3g}, tolerance {limit:g}, floor {floor:g})")
    if not err < limit:
        bad.append((what, err))


def margin(pairs, what):
    """asserted on the reference before its launch: no fp64 pre-activation within the bar of zero"""
    m = min(R.mask_margin(p, g, R.MARGIN_BAR) for p, g in pairs)
    print(f"BAR {what} ReLU-mask margin: {m:.3f} (>= 1)")
    assert m >= 1.0, (what, m)


def ident(case):
    return "-".join(str(v) for v in case)


# ---- sac_actor_chain_fwd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.ACTOR_FWD_CASES)), ids=lambda i: ident(R.ACTOR_FWD_CASES[i]))
def test_sac_actor_chain_fwd(ops, nv, i):
    D, A, H1, H2, B, tiles, mode, head, source = R.ACTOR_FWD_CASES[i]
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H1, tiles, forward=True)
    what = f"actor fwd {ident(R.ACTOR_FWD_CASES[i])}"
    inp = R.actor_fwd_case(i)
    ref, mag = R.actor_fwd_stmt(inp, tiles), R.actor_fwd_stmt(inp, tiles, mag=True)
    margin(R._pre(ref, mag), what)
    W, M, hn = D + A, R.rows_of(B, mode), inp["w3"].shape[0]
    G = ops.chain_colgroups(H2, tiles)
    weights = [dev(inp[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    actor = ops.sac_actor_desc(D, A, *weights)
    x = inp["x"]
    obs_rows, next_rows = (x[:B], x[B:]) if mode == R.PAIR else ((None, x) if mode == R.NEXT else (x, None))
    rng = np.random.default_rng(i)
    ring = idx = None
    if source == "ring":  # every sampled (row, env) pair is distinct: the ring holds the case's rows at those positions
        rows_r, n_envs = 3, B
        ring = ops.DeviceRing(rows_r, n_envs, D, A, DEV)
        fields = {k: rng.standard_normal(tuple(getattr(ring, k).shape)).astype(np.float32) for k in ("observations", "next_observations", "actions", "rewards")}
        fields["dones"] = (rng.uniform(0, 1, (rows_r, n_envs)) < 0.5).astype(np.float32)
        fields["timeouts"] = (rng.uniform(0, 1, (rows_r, n_envs)) < 0.5).astype(np.float32)
        ri, ei = (np.arange(B) % rows_r).astype(np.int32), rng.permutation(B).astype(np.int32)
        if obs_rows is not None:
            fields["observations"][ri, ei] = obs_rows
        if next_rows is not None:
            fields["next_observations"][ri, ei] = next_rows
        for k, v in fields.items():
            getattr(ring, k).copy_(dev(v))
        idx = dev(np.stack((ri, ei)), th.int32)

    def launch(advance):
        b = Bufs()
        x_pi, x_next, x_data = b.new("x_pi", B, W), b.new("x_next", B, W), b.new("x_data", B, W)
        out_done, out_rew = b.new("out_done", B, 1), b.new("out_rew", B, 1)
        keep = mode != R.NEXT
        a_h1, a_h2 = (b.new("a_h1", B, H1), b.new("a_h2", B, H2)) if keep else (None, None)
        head_part = b.new("head_part", G, M, hn)
        kw = dict(rows_mode=mode, head_n=hn)
        if source == "draw":
            kw.update(head_rng_ctl=rng_ctl, head_rng_offset=5, eps_all=b.new("eps_all", M, A))
        if source == "ring":
            ops.sac_actor_chain_fwd(actor, B, x_data, x_pi, x_next, out_done, out_rew, a_h1, a_h2, head_part, tiles, ring=ring, sample_idx=idx,
                                    advance_ring=advance, **kw)
        else:  # packed observation columns
            if obs_rows is not None:
                x_pi[:, :D] = dev(obs_rows)
            if next_rows is not None:
                x_next[:, :D] = dev(next_rows)
            ops.sac_actor_chain_fwd(actor, B, None, x_pi if obs_rows is not None else None, x_next if next_rows is not None else None, None, None,
                                    a_h1, a_h2, head_part, tiles, **kw)
        b.check(written=["head_part"] + (["a_h1", "a_h2"] if keep else []) + (["eps_all"] if source == "draw" else []))
        return b

    rng_ctl = ops.new_rng_ctl(77, DEV) if source == "draw" else None
    if ring is not None:
        ring.ctl.copy_(th.tensor([1, 0, 0, 4]))
    b = launch(False)
    if ring is not None:
        assert ring.ctl.tolist() == [1, 0, 0, 4]  # the ring position moves only with advance_ring
        ring.ctl.copy_(th.tensor([rows_r - 1, 0, 0, 4]))
    b2 = launch(True)
    b2.same_as(b.snapshot())
    if ring is not None:
        assert ring.ctl.tolist() == [0, 1, 0, 5]  # ReplayBuffer.add's epilogue: the position wraps and the ring is full
    bad = []
    get = lambda name: b.flat[name][0][:b.flat[name][1]]  # noqa: E731
    if mode != R.NEXT:
        bar("h1", get("a_h1").view(B, H1), ref["h1"][:B], mag["h1"][:B], what, bad)
        bar("h2", get("a_h2").view(B, H2), ref["h2"][:B], mag["h2"][:B], what, bad)
    hp = host(get("head_part").view(G, M, hn))
    for g in range(G):
        bar("head_part", hp[g], ref["head_part"][g], mag["head_part"][g], f"{what} group {g}", bad)
    x_pi, x_next = host(get("x_pi").view(B, W)), host(get("x_next").view(B, W))
    assert (x_pi[:, D:] == np.float32(SENT)).all() and (x_next[:, D:] == np.float32(SENT)).all()  # the action columns belong to the next launch
    if source == "ring":
        o = (ri, ei)
        x_data = host(get("x_data").view(B, W))
        assert np.array_equal(x_data[:, :D], fields["observations"][o]) and np.array_equal(x_data[:, D:], fields["actions"][o])
        assert np.array_equal(x_next[:, :D], fields["next_observations"][o]) and np.array_equal(x_pi[:, :D], fields["observations"][o])
        assert np.array_equal(host(get("out_rew")), fields["rewards"][o])
        assert np.array_equal(host(get("out_done")), (fields["dones"][o] * (np.float32(1) - fields["timeouts"][o])).astype(np.float32))
    else:
        for name in ("x_data", "out_done", "out_rew"):
            assert bool((get(name) == SENT).all()), name
    if source == "draw":  # the stream positions of cstr_gaussian_head_fwd_f32 on an M-row pass that starts 5 draws further on
        ctl2 = ops.new_rng_ctl(77, DEV)
        ctl2[1] = 5
        eps2 = th.empty(M, A, device=DEV)
        ops.gaussian_head_fwd_(th.zeros(M, 2 * A, device=DEV), None, eps2, ctl2, th.empty(M, A, device=DEV), None)
        assert th.equal(get("eps_all").view(M, A), eps2) and rng_ctl.tolist() == ops.new_rng_ctl(77, DEV).tolist()
    assert not bad, bad
    del weights


# ---- q_chain_fwd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.Q_FWD_CASES)), ids=lambda i: ident(R.Q_FWD_CASES[i]))
def test_q_chain_fwd(ops, nv, i):
    """every network's h1, h2 and q_part per column group against fp64, and the pending actor head's finalisation. One network is not
    compared in value: in `nostore` (roles PLAIN, NEXT) nothing stores the actions that the NEXT network finalises for itself, so its
    h1, h2 and q_part are checked for being written, for their padding and for repeating themselves only; the NEXT role is compared in
    value in `sac4` and `td4`, beside a NEXT_STORE network whose stored actions it shares"""
    D, A, H1, H2, B, tiles, cfg, n_parts = R.Q_FWD_CASES[i]
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H1, tiles, forward=True)
    what = f"q fwd {ident(R.Q_FWD_CASES[i])}"
    inp = R.q_fwd_case(i)
    W, n, G = D + A, len(inp["nets"]), ops.chain_colgroups(H2, tiles)
    P, S, NX, NS, PI = nv.CHAIN_ROLE_PLAIN, nv.CHAIN_ROLE_STORE_PI, nv.CHAIN_ROLE_NEXT, nv.CHAIN_ROLE_NEXT_STORE, nv.CHAIN_ROLE_PI
    roles = {"sac4": [S, P, NS, NX], "td4": [P, P, NS, NX], "pi1": [PI], "nostore": [P, NX]}.get(cfg, [P] * n)
    own = [r in (NX, NS, PI) for r in roles]
    pre = []
    for x, net in zip(inp["xs"], inp["nets"]):
        pre += R._pre(R.q_fwd_stmt(x, net, tiles), R.q_fwd_stmt(x, net, tiles, mag=True))
    margin(pre, what)
    gauss = cfg in ("sac4", "nostore")
    wts = [[dev(net[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")] for net in inp["nets"]]
    fin_in = [dev(inp[k]) for k in ("head_part", "hb", "eps")] if n_parts else None

    def launch():
        b = Bufs()
        xs = []
        for g in range(n):
            if own[g]:  # the action columns are written by the launch: x_next / x_pi of the head finalisation
                nm = "x_pi" if roles[g] == PI else "x_next"
                if nm not in b.flat:
                    b.new(nm, B, W)[:, :D] = dev(inp["xs"][g][:, :D])
                xs.append(b.flat[nm][0][:B * W].view(B, W))
            else:
                xs.append(dev(inp["xs"][g]))
        fin = None
        if n_parts:
            x_pi = b.flat["x_pi"][0][:B * W].view(B, W) if "x_pi" in b.flat else b.new("x_pi", B, W)
            x_next = b.flat["x_next"][0][:B * W].view(B, W) if "x_next" in b.flat else b.new("x_next", B, W)
            params, logp_pi, logp_next = b.new("params", B, 2 * A), b.new("logp_pi", B), b.new("logp_next", B)
            rows = 2 * B if gauss else B
            fin = nv.SacHeadFin(fin_in[0].data_ptr(), fin_in[1].data_ptr(), fin_in[2].data_ptr(), n_parts, A, D,
                                nv.CHAIN_HEAD_GAUSSIAN if gauss else nv.CHAIN_HEAD_DETERMINISTIC, rows, inp["next_offset"], R.SIGMA, R.CLIP,
                                x_pi.data_ptr(), x_next.data_ptr(), *((params.data_ptr(), logp_pi.data_ptr(), logp_next.data_ptr()) if gauss else (None, None, None)))
        nets = []
        for g in range(n):
            layers = ((wts[g][0], wts[g][1]), (wts[g][2], wts[g][3]), (wts[g][4].view(-1), wts[g][5]))
            nets.append(ops.chain_net(layers, xs[g], b.new(f"h1_{g}", B, H1), b.new(f"h2_{g}", B, H2), b.new(f"q_part_{g}", G, B), roles[g]))
        ops.q_chain_fwd(nets, W, D, H1, H2, B, tiles, fin)
        b.check(written=[f"{k}_{g}" for g in range(n) for k in ("h1", "h2", "q_part")])
        return b, xs

    b, xs = launch()
    b2, _ = launch()
    b2.same_as(b.snapshot())
    bad = []
    view = lambda name, *shape: host(b.flat[name][0][:b.flat[name][1]].view(*shape))  # noqa: E731
    # ---- the pending actor head: finalised from the launch's own inputs, stored by the STORE roles only
    if n_parts:
        x_pi, x_next = view("x_pi", B, W), view("x_next", B, W)
        stored_pi, stored_next = S in roles or PI in roles, NS in roles
        sent = np.float32(SENT)
        if gauss and S in roles:
            params = view("params", B, 2 * A)
            assert np.array_equal(params, R.params_f32(inp["head_part"], inp["hb"], 0, B))  # partials in ascending order, then the bias
            a, lp = R.fin_gaussian(params, inp["eps"][:B])
            tol("actions", x_pi[:, D:], a, 5e-6, f"{what} pi actions", bad), tol("log-probs", view("logp_pi", B), lp, 1e-4, f"{what} logp_pi", bad)
        if gauss and NS in roles:
            a, lp = R.fin_gaussian(R.params_f32(inp["head_part"], inp["hb"], B, B), inp["eps"][B:])
            tol("actions", x_next[:, D:], a, 5e-6, f"{what} next actions", bad), tol("log-probs", view("logp_next", B), lp, 1e-4, f"{what} logp_next", bad)
        if not gauss and NS in roles:
            mu = R.params_f32(inp["head_part"], inp["hb"], 0, B)
            a = R.fin_deterministic(mu, inp["eps"], R.SIGMA, R.CLIP, smooth=True)
            raw = np.asarray(inp["eps"], np.float64) * R.SIGMA
            assert (np.abs(raw) > R.CLIP).any() and (np.abs(np.tanh(mu.astype(np.float64)) + np.clip(raw, -R.CLIP, R.CLIP)) > 1).any()  # both clamps bind
            tol("actions", x_next[:, D:], a, 5e-6, f"{what} smoothed target actions", bad)
        if PI in roles:
            tol("actions", x_pi[:, D:], R.fin_deterministic(R.params_f32(inp["head_part"], inp["hb"], 0, B)), 5e-6, f"{what} pi actions", bad)
        # what no role of this launch stores keeps the sentinel
        if not stored_pi:
            assert (x_pi == sent).all()
        elif PI not in roles:
            assert (x_pi[:, :D] == sent).all()  # STORE_PI writes the action columns only
        if not stored_next:
            assert (x_next[:, D:] == sent).all()
        if not (gauss and S in roles):
            assert (view("params", B, 2 * A) == sent).all() and (view("logp_pi", B) == sent).all()
        if not (gauss and NS in roles):
            assert (view("logp_next", B) == sent).all()
    # ---- the matrix stages, per network and column group; networks that read finalised actions are stated on the stored ones
    for g in range(n):
        if roles[g] == NX and NS not in roles:
            continue  # nothing stored the actions this network finalised for itself: written, padded and repeatable, not compared (docstring)
        x = host(xs[g]) if own[g] else inp["xs"][g]
        ref, mag = R.q_fwd_stmt(x, inp["nets"][g], tiles), R.q_fwd_stmt(x, inp["nets"][g], tiles, mag=True)
        if own[g]:  # the reference on the stored actions keeps the margin the case was searched for
            margin(R._pre(ref, mag), f"{what} net {g} on the stored actions")
        tag = f"{what} net {g}"
        bar("h1", view(f"h1_{g}", B, H1), ref["h1"], mag["h1"], tag, bad), bar("h2", view(f"h2_{g}", B, H2), ref["h2"], mag["h2"], tag, bad)
        qp = view(f"q_part_{g}", G, B)
        for cg in range(G):
            bar("q_part", qp[cg], ref["q_part"][cg], mag["q_part"][cg], f"{tag} group {cg}", bad)
    assert not bad, bad
    del wts, fin_in


# ---- q_chain_bwd ------------------------------------------------------------------------------------------------------------------
class _Opt:
    """what chain_root reads of an optimiser: its control words and betas"""

    def __init__(self, ops, step, betas):
        self.ctl, self.param_groups = ops.new_adam_ctl(DEV, step, *betas), [dict(betas=betas)]


def adam_ctl_after(step, betas, launches):
    """state["step"] += 1 and the running beta powers, as f64 multiplications"""
    p1, p2 = float(betas[0]) ** step, float(betas[1]) ** step
    for _ in range(launches):
        step, p1, p2 = step + 1, p1 * betas[0], p2 * betas[1]
    return [step, 0] + np.array([p1, p2], np.float64).view(np.int64).tolist()


@pytest.mark.parametrize("i", range(len(R.Q_BWD_CASES)), ids=lambda i: ident(R.Q_BWD_CASES[i]))
def test_q_chain_bwd(ops, nv, i):
    D, A, H1, H2, B, tiles, mode, alpha, ft = R.Q_BWD_CASES[i]
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H2, tiles)
    what = f"q bwd {ident(R.Q_BWD_CASES[i])}"
    inp = R.q_bwd_case(i)
    W, nd, G1 = D + A, inp["n_diff"], ops.chain_colgroups(H1, tiles)
    P = inp["q_part"][0].shape[0]
    gact = mode != "td"
    ref, mag = R.q_bwd_stmt(inp, tiles, with_gact=gact), R.q_bwd_stmt(inp, tiles, mag=True, with_gact=gact)
    if mode == "sac_actor":  # the first minimum must not hang on the last bits of q
        gap = (ref["q_out"][0] - ref["q_out"][1]).abs() / (R.U * (mag["q_out"][0] + mag["q_out"][1]))
        print(f"BAR {what} min(q1, q2) margin: {float(gap.min()) / (2 * R.bar_of('q_out')):.3f} (>= 1)")
        assert float(gap.min()) >= 2 * R.bar_of("q_out")
    wts = [[dev(net[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")] for net in inp["nets"]]
    h1, h2, q_parts = [dev(v) for v in inp["h1"]], [dev(v) for v in inp["h2"]], [dev(v) for v in inp["q_part"]]
    rew, done, next_logp, logp = (dev(inp[k]) for k in ("rew", "done", "next_logp", "logp"))
    ent_coef, log_alpha = dev(np.array([inp["ent_coef"]])), (dev(np.array([inp["log_alpha"]])) if alpha else None)
    betas = [(0.9, 0.999), (0.8, 0.99)]
    opts = [_Opt(ops, 3, betas[0]), _Opt(ops, 7, betas[1])][:2 if mode == "td" else 1]
    rng_ctl, adv = ops.new_rng_ctl(5, DEV), 2 * B + 3
    rng_ctl[1] = 1000
    b = Bufs()
    out = {k: b.new(k, *s) for k, s in (("q_out", (nd, B)), ("gq_out", (nd, B)), ("loss_out", (1,)), ("dz2", (nd, B, H2)), ("dz1", (nd, B, H1)))}
    written = ["q_out", "gq_out", "loss_out", "dz2", "dz1"]
    if mode == "td":
        out["target_out"] = b.new("target_out", B)
        written.append("target_out")
    if gact:
        out["gact_part"] = b.new("gact_part", nd, G1, B, A)
        written.append("gact_part")
    loss_sum = th.tensor([2.5], device=DEV)
    adict = None
    if alpha:
        a_out = {k: b.new("alpha_" + k, 1) for k in ("grad_out", "ent_coef_out", "loss_out")}
        written += ["alpha_" + k for k in a_out]
        a_sum = dict(loss_sum=th.tensor([1.5], device=DEV), ent_coef_sum=th.tensor([0.75], device=DEV))
        adict = dict(log_alpha=log_alpha, logp_pi=logp, target_entropy=inp["target_entropy"], **a_out, **a_sum)
    root = ops.chain_root(mode, B, q_parts, [w[5] for w in wts], P, gamma=inp["gamma"], scale=inp["scale"], next_logp=next_logp if inp["sac"] else None,
                          rew=rew, done=done, ent_coef=ent_coef, logp=logp, target_out=out.get("target_out"), q_out=out["q_out"], gq_out=out["gq_out"],
                          loss_out=out["loss_out"], loss_sum=loss_sum, alpha=adict, rng_advance=(rng_ctl, adv), adam_advance=opts)
    nets = [ops.chain_net(((wts[g][0], wts[g][1]), (wts[g][2], wts[g][3]), (wts[g][4].view(-1), wts[g][5])), None, h1[g], h2[g]) for g in range(nd)]
    run = lambda: ops.q_chain_bwd(nets, root, W, D, H1, H2, tiles, dz2=out["dz2"], dz1=out["dz1"], gact_part=out.get("gact_part"))  # noqa: E731
    run()
    b.check(written=written)
    snap = b.snapshot()
    run()
    b.check(written=written)
    b.same_as(snap)
    bad = []
    for kind in ("q_out", "target_out", "gq_out", "dz2", "dz1"):
        if kind in out:
            bar(kind, out[kind], ref[kind], mag[kind], what, bad)
    bar("loss", out["loss_out"], ref["loss"], mag["loss"], what, bad)
    if gact:
        gp = host(out["gact_part"])
        for g in range(nd):
            for cg in range(G1):
                bar("gact_part", gp[g, cg], ref["gact_part"][g, cg], mag["gact_part"][g, cg], f"{what} net {g} group {cg}", bad)
    f32 = np.float32
    loss = host(out["loss_out"])[0]
    assert host(loss_sum)[0] == f32(f32(f32(2.5) + loss) + loss)  # accumulates, launch by launch
    if alpha:
        got = np.array([host(a_out[k])[0] for k in ("grad_out", "ent_coef_out", "loss_out")])
        bar("alpha", got, ref["alpha"], mag["alpha"], what, bad)
        assert host(a_sum["loss_sum"])[0] == f32(f32(f32(1.5) + got[2]) + got[2]) and host(a_sum["ent_coef_sum"])[0] == f32(f32(f32(0.75) + got[1]) + got[1])
    assert rng_ctl.tolist() == [5, 1000 + 2 * adv] + [0] * (nv.RNG_CTL_WORDS - 2)  # rng_ctl[1] advances by exactly rng_advance per launch
    for k, o in enumerate(opts):  # the host's step + 1 and running beta products, bit for bit
        assert o.ctl.tolist() == adam_ctl_after((3, 7)[k], betas[k], 2), k
    assert not bad, bad
    del wts


# ---- sac_actor_chain_bwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.ACTOR_BWD_CASES)), ids=lambda i: ident(R.ACTOR_BWD_CASES[i]))
def test_sac_actor_chain_bwd(ops, nv, i):
    D, A, H1, H2, B, tiles, head, n_nets, n_parts = R.ACTOR_BWD_CASES[i]
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H2, tiles)
    what = f"actor bwd {ident(R.ACTOR_BWD_CASES[i])}"
    inp = R.actor_bwd_case(i)
    ref, mag = R.actor_bwd_stmt(inp), R.actor_bwd_stmt(inp, mag=True)
    net, det = inp["net"], head == "det"
    hn = A if det else 2 * A
    weights = [dev(net[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    actor = ops.sac_actor_desc(D, A, *weights)
    gact, x_pi, a_h1, a_h2 = (dev(inp[k]) for k in ("gact_part", "x_pi", "a_h1", "a_h2"))
    ent_coef, params, eps = (None, None, None) if det else (dev(np.array([inp["ent_coef"]])), dev(inp["params"]), dev(inp["eps"]))
    b = Bufs()
    g_params, dz2, dz1 = b.new("g_params", B, hn), b.new("dz2", B, H2), b.new("dz1", B, H1)
    run = lambda: ops.sac_actor_chain_bwd(actor, gact, n_nets, n_parts, ent_coef, x_pi, params, eps, a_h1, a_h2, g_params, dz2, dz1, B, tiles,  # noqa: E731
                                          kind=nv.CHAIN_HEAD_DETERMINISTIC if det else nv.CHAIN_HEAD_GAUSSIAN)
    run()
    b.check(written=["g_params", "dz2", "dz1"])
    snap = b.snapshot()
    run()
    b.check()
    b.same_as(snap)
    bad = []
    tol("g_params", g_params, ref["g_params"].numpy(), 2e-6, f"{what} g_params", bad, floor=max(1.0, float(ref["g_params"].abs().max())))
    if not det:
        assert float(g_params[0, A]) == 0.0 and float(ref["g_params"][0, A]) == 0.0  # log_std outside the clamp: its gradient is cut
    bar("dz2", dz2, ref["dz2"], mag["dz2"], what, bad), bar("dz1", dz1, ref["dz1"], mag["dz1"], what, bad)
    assert not bad, bad
    del weights


# ---- chain_sum_parts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("cols", [2, 4])
@pytest.mark.parametrize("rows", [16, 33])
@pytest.mark.parametrize("n_parts", [1, 7])
def test_chain_sum_parts(ops, n_parts, rows, cols, strided):
    part = np.random.default_rng(100 * n_parts + rows + cols).standard_normal((n_parts, rows, cols)).astype(np.float32)
    want = part[0].copy()
    for p in range(1, n_parts):
        want = (want + part[p]).astype(np.float32)  # ascending p
    b = Bufs()
    wide = b.new("out", rows, 8 + cols if strided else cols)
    out = wide[:, 8:] if strided else wide
    ops.chain_sum_parts(dev(part), out)
    b.check()
    snap = b.snapshot()
    ops.chain_sum_parts(dev(part), out)
    b.same_as(snap)
    assert np.array_equal(host(out), want)
    if strided:  # the action columns of a wider matrix: the other columns keep the sentinel
        assert bool((wide[:, :8] == SENT).all())


# ---- linear_bwd_weight_adam_sets --------------------------------------------------------------------------------------------------
def ulps(got, want):
    return np.abs(np.asarray(got, np.float32).reshape(-1).view(np.int32).astype(np.int64) - np.asarray(want, np.float32).reshape(-1).view(np.int32).astype(np.int64))


@pytest.mark.parametrize("M", R.WGRAD_ROWS)
def test_linear_bwd_weight_adam_sets(ops, nv, M):
    """four Linears of different shapes in one launch: a row-strided x, the explicit quadruple form, a shadow copy, an own-target soft
    update, two optimisers (pre-advanced through a chain root) and two flat segments (an Adam range, a polyak run). Every tensor the
    launch writes has 64 sentinel floats behind it: the plain ones come from Bufs, and in the arenas a 64-float parameter that belongs to
    no set follows every parameter, so values, gradients and both moments are each followed by sentinels (the alignment gaps hold them too)"""
    from torch import nn

    from core.common.arena import FlatAdam, ParamArena
    from oracle import cstr_oracle as orc

    what = f"dW + Adam M={M}"
    cases = [R.wgrad_case(M, j) for j in range(len(R.WGRAD_SHAPES))]
    hyper = [dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, step=3), dict(lr=7e-3, betas=(0.8, 0.99), eps=1e-6, grad_scale=0.125, step=7)]
    opt_of, tau = [0, 1, 0, 1], 0.005
    # sets 0, 1, 3: parameters of two arenas; set 2 (1 x 40): explicit (values, gradient, exp_avg, exp_avg_sq) views, the merged heads' form
    lin = {j: (nn.Parameter(th.tensor(cases[j]["w"])), nn.Parameter(th.tensor(cases[j]["b"]))) for j in (0, 1, 3)}
    guard = lambda: nn.Parameter(th.zeros(PAD))  # noqa: E731
    arenas = [ParamArena([q for p in ps for q in (p, guard())], DEV) for ps in (list(lin[0]), list(lin[1]) + list(lin[3]))]
    opts = []
    for k, h in enumerate(hyper):
        o = FlatAdam(arenas[k], lr=h["lr"], betas=h["betas"], eps=h["eps"])
        o.grad_scale = h["grad_scale"]
        ops.set_adam_step(o.ctl, h["step"], *h["betas"])
        opts.append(o)
    for j in (0, 1, 3):
        for p, (mk, vk) in zip(lin[j], (("w_m", "w_v"), ("b_m", "b_v"))):
            m, v = opts[opt_of[j]].moments_of(p)
            m.copy_(dev(cases[j][mk]).view(-1)), v.copy_(dev(cases[j][vk]).view(-1))
    # what lies between and behind the sets' parameters in the arenas' four buffers, and every gradient element, starts at the sentinel
    own, outside = [], []
    for k, ar in enumerate(arenas):
        inside = th.zeros(ar.numel, dtype=th.bool, device=DEV)
        for j in (0, 1, 3):
            if opt_of[j] == k:
                for p in lin[j]:
                    inside[ar.offset_of[id(p)]:ar.offset_of[id(p)] + p.numel()] = True
        assert int(inside.sum()) + len(ar.params) // 2 * PAD <= ar.numel
        own.append((ar.flat, ar.grad, opts[k].exp_avg, opts[k].exp_avg_sq))
        outside.append(~inside)
        for t in own[k]:
            t[outside[k]] = SENT
        ar.grad.fill_(SENT)

    def arenas_check(written):
        for k, ar in enumerate(arenas):
            for name, t in zip(("values", "gradient", "exp_avg", "exp_avg_sq"), own[k]):
                assert bool((t[outside[k]] == SENT).all()), f"arena {k} {name}: written outside the sets' parameters"
            if written:
                assert not bool((ar.grad[~outside[k]] == SENT).any()), f"arena {k}: gradient elements left unwritten"

    b = Bufs()
    quad = {k: b.put(k + "2", cases[2][k]) for k in ("w", "b", "w_m", "w_v", "b_m", "b_v")}
    quad["dw"], quad["db"] = b.new("dw2", 1, 40), b.new("db2", 1)
    shadow = b.new("shadow", ops.swizzled_numel(20, 36))
    ops.policy_swizzle(lin[1][0].detach(), shadow)  # as FlatAdam.add_weight_shadow leaves it: the launch keeps it current
    t_w, t_b = b.put("t_w", cases[0]["w"] * 0.5 + 0.1), b.put("t_b", cases[0]["b"] * 0.5 - 0.1)
    t_w0, t_b0 = host(t_w).copy(), host(t_b).copy()
    xs = [dev(c["x"])[:, :c["k"]] for c in cases]  # set 0: rows K + 2 floats apart
    assert xs[0].stride(0) == 8 and not xs[0].is_contiguous()
    dzs = [dev(c["dz"]) for c in cases]
    sets = [(dzs[0], xs[0], lin[0][0], lin[0][1], 0, None, (t_w, t_b, tau)), (dzs[1], xs[1], lin[1][0], lin[1][1], 1, shadow),
            (dzs[2], xs[2], (quad["w"], quad["dw"], quad["w_m"], quad["w_v"]), (quad["b"], quad["db"], quad["b_m"], quad["b_v"]), 0, None),
            (dzs[3], xs[3], lin[3][0], lin[3][1], 1, None)]
    # flat segments: an Adam range on optimiser 0's control words (SAC's entropy coefficient rides like this) and a soft target update
    rng = np.random.default_rng(M)
    fl = {k: rng.standard_normal(37).astype(np.float32) * s for k, s in (("p", 1.0), ("g", 0.01), ("m", 1e-3))}
    fl["v"] = (rng.uniform(0, 1, 37) * 1e-5).astype(np.float32)
    fd = {k: (b.put("flat_" + k, v) if k != "g" else dev(v)) for k, v in fl.items()}
    src, tgt = rng.standard_normal(1030).astype(np.float32), rng.standard_normal(1030).astype(np.float32)
    src_d, tgt_d = dev(src), b.put("tgt", tgt)
    h0 = hyper[0]
    flat = [(fd["p"], fd["g"], fd["m"], fd["v"], opts[0].ctl, opts[0].lr_dev, *h0["betas"], h0["eps"], h0["grad_scale"]), ("polyak", src_d, tgt_d, tau)]
    # state["step"] += 1 of both optimisers by the loss workgroup of a chain root, as on the training path
    binp = R.q_bwd_case(0)
    bw = [[dev(net[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")] for net in binp["nets"]]
    bh1, bh2, bq = [dev(v) for v in binp["h1"]], [dev(v) for v in binp["h2"]], [dev(v) for v in binp["q_part"]]
    brew, bdone = dev(binp["rew"]), dev(binp["done"])
    broot = ops.chain_root("td", 16, bq, [w[5] for w in bw], bq[0].shape[0], gamma=0.97, scale=1.0, rew=brew, done=bdone, adam_advance=opts)
    bnets = [ops.chain_net(((bw[g][0], bw[g][1]), (bw[g][2], bw[g][3]), (bw[g][4].view(-1), bw[g][5])), None, bh1[g], bh2[g]) for g in range(2)]
    bdz2, bdz1 = th.empty(2, 16, 16, device=DEV), th.empty(2, 16, 16, device=DEV)
    ops.q_chain_bwd(bnets, broot, 6, 4, 16, 16, 1, dz2=bdz2, dz1=bdz1)
    ctl_before = [o.ctl.tolist() for o in opts]
    assert ctl_before == [adam_ctl_after(h["step"], h["betas"], 1) for h in hyper]
    old = {j: {k: host(t).copy() for k, t in (("w", lin[j][0].detach()), ("b", lin[j][1].detach()))} for j in (0, 1, 3)}
    ops.linear_bwd_weight_adam_sets(sets, opts, flat)
    b.check(written=["dw2", "db2"])
    arenas_check(written=True)
    assert [o.ctl.tolist() for o in opts] == ctl_before  # control words are read, never written
    bad, first = [], {}
    for j, c in enumerate(cases):
        h = hyper[opt_of[j]]
        step = h["step"] + 1
        ref, mag = R.wgrad_stmt(c), R.wgrad_stmt(c, mag=True)
        if j == 2:
            got = {k: host(quad[k]) for k in ("dw", "db", "w", "b", "w_m", "w_v", "b_m", "b_v")}
            before = {k: cases[2][k] for k in ("w", "b")}
        else:
            w, bb = lin[j]
            (wm, wv), (bm, bv) = opts[opt_of[j]].moments_of(w), opts[opt_of[j]].moments_of(bb)
            got = dict(dw=host(w.grad), db=host(bb.grad), w=host(w.detach()), b=host(bb.detach()), w_m=host(wm), w_v=host(wv), b_m=host(bm), b_v=host(bv))
            before = old[j]
        tag = f"{what} set {j} {R.WGRAD_SHAPES[j]}"
        first[j] = (got["dw"].copy(), got["db"].copy())
        bar("dw", got["dw"].reshape(ref["dw"].shape), ref["dw"], mag["dw"], tag, bad), bar("db", got["db"].reshape(-1), ref["db"], mag["db"], tag, bad)
        for p, g, mk, vk in (("w", "dw", "w_m", "w_v"), ("b", "db", "b_m", "b_v")):
            # the moments against the oracle's float32 Adam fed the launch's own gradient; the parameter against the float32 statement fed
            # the launch's own moments; tests/test_hip_kernels.py test_adam_vs_torch_and_oracle's ulp limits
            gs = (got[g].reshape(-1) * np.float32(h["grad_scale"])).astype(np.float32)
            _, om, ov = orc.adam_step(before[p], gs, c[mk], c[vk], step, h["lr"], h["betas"][0], h["betas"][1], h["eps"])
            op = R.adam_param_f32(np.asarray(before[p]).reshape(-1), got[mk].reshape(-1), got[vk].reshape(-1), step, h["lr"], h["betas"], h["eps"])
            for name, a, w_ in ((mk, got[mk], om), (vk, got[vk], ov), (p, got[p], op)):
                u = ulps(a, w_)
                print(f"BAR {tag} {name}: {u.max()} ulp of 4, {(u > 1).mean():.2g} above one ulp of 1e-3")
                if not (u.max() <= 4 and (u > 1).mean() < 1e-3):
                    bad.append((tag, name, int(u.max())))
    # bit for bit: the shadow copy of the new weight, the own target, the flat polyak run
    assert np.array_equal(host(shadow), R.swizzle(host(lin[1][0].detach())))
    om_tile = np.float32(1) - np.float32(tau)
    for t, t0, p in ((t_w, t_w0, lin[0][0]), (t_b, t_b0, lin[0][1])):
        want = (host(p.detach()).astype(np.float64) * np.float64(np.float32(tau)) + (t0 * om_tile).astype(np.float64)).astype(np.float32)
        assert np.array_equal(host(t), want)
    assert np.array_equal(host(tgt_d), R.polyak_f32(src, tgt, tau)) and np.array_equal(host(src_d), src)
    _, fm, fv = orc.adam_step(fl["p"], (fl["g"] * np.float32(h0["grad_scale"])).astype(np.float32), fl["m"], fl["v"], h0["step"] + 1, h0["lr"], *h0["betas"], h0["eps"])
    fp = R.adam_param_f32(fl["p"], host(fd["m"]), host(fd["v"]), h0["step"] + 1, h0["lr"], h0["betas"], h0["eps"])
    for name, a, w_ in (("flat exp_avg", fd["m"], fm), ("flat exp_avg_sq", fd["v"], fv), ("flat parameter", fd["p"], fp)):
        u = ulps(host(a), w_)
        print(f"BAR {what} {name}: {u.max()} ulp of 4")
        assert u.max() <= 4 and (u > 1).mean() < 1e-3, name
    # the gradients of a second launch on the same dz and x repeat the first bit for bit (the parameters move on)
    ops.linear_bwd_weight_adam_sets(sets, opts, flat)
    b.check()
    arenas_check(written=False)
    for j in range(len(cases)):
        dw, db = (quad["dw"], quad["db"]) if j == 2 else (lin[j][0].grad, lin[j][1].grad)
        assert np.array_equal(host(dw), first[j][0]) and np.array_equal(host(db), first[j][1]), j
    assert not bad, bad
    del bw


def test_zz_kernel_worst_figures():
    """a record, not a check: prints the worst figure per output kind that the tests of this run measured (it runs last; under -k or
    another order it prints what ran before it, possibly nothing). Every figure is asserted where it is measured"""
    for kind in sorted(FIGS):
        print(f"KERNEL {kind}: {FIGS[kind]:.3f} units, bar {R.BARS[kind]:.2f}")
    for kind in sorted(TOLS):
        print(f"KERNEL {kind}: {TOLS[kind]:.3g}")
    assert all(FIGS[k] <= R.BARS[k] for k in FIGS)
