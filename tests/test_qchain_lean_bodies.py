"""The lean Q chain kernels against the generic ones (cstr_q_chain_fwd_f32 / cstr_q_chain_bwd_f32, csrc/cstr_chain.hip).

Both write the same bits: the lean kernels change where a workgroup's arguments come from and which loss mode, head kind, store set and
partial-sum bucket are compiled in, never an expression, an MFMA operand or the order of a sum. Every case runs the launch twice from
identical seeded inputs, once per setting of cstr_chain_lean, and compares every buffer the launch may write byte for byte -- backward:
dz1, dz2, gact_part, q_out, gq_out, target_out, the loss slots, the alpha part's outputs, the Adam control words and the Philox
control words; forward: q_part, h1, h2, x_next / x_pi, logp_next / logp_pi, params -- each float buffer with 64 sentinel floats behind
it that must survive. tests/test_chain_kernels.py is the fp64 statement of both launches; this module only ties the two kernels
together, at the smallest shapes at which the argument hand-over, the variant dispatch and each partial-sum bucket can go wrong:
one and two row groups beside the loss workgroup (batch 16, 32), both layouts with 256 x 256 instantiations, 4 / 8 / 16 partial sums
(and 7: lanes beyond n must read zeros), every loss root the learners dispatch plus one nobody dispatches (alpha part without
next_logp: generic kernel under both settings), rows where Q1 == Q2, a partial sum of -0.0 only, and run-time widths (64 x 64),
which the switch must not touch. Lean instantiations exist for 256 x 256 only, so 400 x 300 is not a case here."""
import numpy as np
import pytest
import torch as th

from _sentinel_bufs import DEV, SENT, Bufs

pytestmark = pytest.mark.gpu
H = 256


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


def net_weights(rng, W, H1, H2, b3=None):
    w = dict(w1=rng.standard_normal((H1, W)) * 0.4, b1=rng.standard_normal(H1) * 0.1, w2=rng.standard_normal((H2, H1)) * 0.08,
             b2=rng.standard_normal(H2) * 0.1, w3=rng.standard_normal(H2) * 0.1, b3=np.array([rng.standard_normal() if b3 is None else b3]))
    return {k: dev(v) for k, v in w.items()}


def layers(w):
    return ((w["w1"], w["b1"]), (w["w2"], w["b2"]), (w["w3"], w["b3"]))


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


def test_switch(ops):
    assert ops.chain_lean(-1) == 1  # the lean kernels are the default
    assert ops.chain_lean(0) == 1 and ops.chain_lean(-1) == 0 and ops.chain_lean(5) == 0 and ops.chain_lean(-1) == 1


# ---- forward ------------------------------------------------------------------------------------------------------------------------
# (D, A, H1, H2, B, tiles, configuration, partial sums of the pending head)
FWD_CASES = [
    (4, 2, H, H, 32, 2, "sac4", 8),
    (8, 2, H, H, 16, 4, "sac4", 4),
    (4, 2, H, H, 16, 1, "sac4", 16),
    (4, 2, H, H, 32, 2, "sac4", 7),
    (8, 2, H, H, 32, 2, "td4", 8),
    (4, 2, H, H, 16, 2, "pi2", 8),
    (4, 2, H, H, 16, 4, "pi2", 16),
    (8, 2, H, H, 32, 2, "plain", 0),
    (4, 2, H, H, 16, 1, "plain", 0),
    (4, 2, 64, 64, 32, 1, "sac4", 4),  # run-time widths: the generic kernel under both settings
]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward(ops, nv, case):
    D, A, H1, H2, B, tiles, cfg, n_parts = case
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H1, tiles, forward=True)
    rng = np.random.default_rng(sum(case[:6]) + n_parts)
    W, G = D + A, ops.chain_colgroups(H2, tiles)
    P, S, NX, NS, PI = nv.CHAIN_ROLE_PLAIN, nv.CHAIN_ROLE_STORE_PI, nv.CHAIN_ROLE_NEXT, nv.CHAIN_ROLE_NEXT_STORE, nv.CHAIN_ROLE_PI
    roles = {"sac4": [S, P, NS, NX], "td4": [P, P, NS, NX], "pi2": [PI, PI], "plain": [P, P]}[cfg]
    gauss = cfg == "sac4"
    n = len(roles)
    wts = [net_weights(rng, W, H1, H2) for _ in range(n)]
    x_obs = [rng.standard_normal((B, W)).astype(np.float32) for _ in range(n)]
    fin_in = None
    if n_parts:
        rows, hn = (2 * B, 2 * A) if gauss else (B, A)
        head_part = (rng.standard_normal((n_parts, rows, hn)) * 0.3).astype(np.float32)
        head_part[:, 1, 0] = -0.0  # a sum of -0.0 only (the zero padding of the bucket turns it into +0.0 in both kernels)
        head_part[:, rows - 2, hn - 1] = -0.0
        fin_in = [dev(head_part), dev(rng.standard_normal(hn) * 0.1), dev(rng.standard_normal((rows, A)))]

    def launch(lean):
        b = Bufs()
        xs = []
        for g in range(n):
            if roles[g] in (NX, NS, PI):  # the action columns are the launch's to write
                nm = "x_pi" if roles[g] == PI else "x_next"
                if nm not in b.flat:
                    b.new(nm, B, W)[:, :D] = dev(x_obs[0][:, :D])
                xs.append(b.flat[nm][0][:B * W].view(B, W))
            else:
                xs.append(dev(x_obs[g]))
        fin = None
        if n_parts:
            x_pi = b.flat["x_pi"][0][:B * W].view(B, W) if "x_pi" in b.flat else b.new("x_pi", B, W)
            x_next = b.flat["x_next"][0][:B * W].view(B, W) if "x_next" in b.flat else b.new("x_next", B, W)
            params, logp_pi, logp_next = b.new("params", B, 2 * A), b.new("logp_pi", B), b.new("logp_next", B)
            fin = nv.SacHeadFin(fin_in[0].data_ptr(), fin_in[1].data_ptr(), fin_in[2].data_ptr(), n_parts, A, D,
                                nv.CHAIN_HEAD_GAUSSIAN if gauss else nv.CHAIN_HEAD_DETERMINISTIC, 2 * B if gauss else B, B if gauss else 0, 0.2, 0.5,
                                x_pi.data_ptr(), x_next.data_ptr(), *((params.data_ptr(), logp_pi.data_ptr(), logp_next.data_ptr()) if gauss else (None, None, None)))
        nets = [ops.chain_net(layers(wts[g]), xs[g], b.new(f"h1_{g}", B, H1), b.new(f"h2_{g}", B, H2), b.new(f"q_part_{g}", G, B), roles[g]) for g in range(n)]
        ops.q_chain_fwd(nets, W, D, H1, H2, B, tiles, fin)
        written = [f"{k}_{g}" for g in range(n) for k in ("h1", "h2", "q_part")]
        if gauss:
            written += ["params", "logp_pi", "logp_next"]
        out = collect(b, written, {})
        if n_parts:  # the stored action columns: STORE_PI / PI write x_pi's, NEXT_STORE x_next's
            for nm, stored in (("x_pi", S in roles or PI in roles), ("x_next", NS in roles)):
                cols = out[nm][:B * W].reshape(B, W)[:, D:]
                assert bool((cols != np.float32(SENT)).all()) == stored and bool((cols == np.float32(SENT)).all()) != stored, (nm, lean)
        return out

    both(ops, launch)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
class _Opt:
    """what chain_root reads of an optimiser: its control words and betas"""

    def __init__(self, ops, step, betas):
        self.ctl, self.param_groups = ops.new_adam_ctl(DEV, step, *betas), [dict(betas=betas)]


# (D, A, H1, H2, B, tiles, partial sums, root, alpha part, next_logp)
BWD_CASES = [
    (4, 2, H, H, 32, 2, 8, "td", True, True),      # SAC, ent_coef "auto"
    (8, 2, H, H, 16, 2, 8, "td", False, True),     # SAC, fixed coefficient
    (4, 2, H, H, 16, 2, 8, "td", False, False),    # TD3 / MADDPG / BCQ
    (4, 2, H, H, 16, 2, 8, "td", True, False),     # nobody's: the generic kernel under both settings
    (4, 2, H, H, 32, 4, 4, "td", True, True),
    (8, 2, H, H, 16, 1, 16, "td", True, True),
    (4, 2, H, H, 16, 2, 7, "td", False, True),
    (4, 2, H, H, 32, 2, 8, "sac_actor", False, False),
    (8, 2, H, H, 16, 4, 4, "sac_actor", False, False),
    (4, 2, H, H, 16, 1, 16, "sac_actor", False, False),
    (4, 2, H, H, 32, 2, 8, "neg_mean", False, False),
    (8, 2, H, H, 16, 4, 3, "neg_mean", False, False),
    (4, 2, 64, 64, 32, 1, 4, "td", True, True),    # run-time widths
    (4, 2, 64, 64, 16, 1, 4, "sac_actor", False, False),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_backward(ops, nv, case):
    D, A, H1, H2, B, tiles, P, mode, alpha, with_logp = case
    assert ops.chain_supported(H1, H2, B) and ops.chain_tiles_ok(H2, tiles)
    rng = np.random.default_rng(sum(case[:7]) + 7 * len(mode) + 2 * alpha + with_logp)
    W, G1 = D + A, ops.chain_colgroups(H1, tiles)
    nd, need = (1, 1) if mode == "neg_mean" else (2, 4 if mode == "td" else 2)
    td = mode == "td"
    b3 = 0.125  # one bias for every head, so that equal partial sums are equal Q values
    wts = [net_weights(rng, W, H1, H2, b3) for _ in range(need)]
    h1 = [dev(np.maximum(rng.standard_normal((B, H1)), 0.0)) for _ in range(nd)]
    h2 = [dev(np.maximum(rng.standard_normal((B, H2)), 0.0)) for _ in range(nd)]
    qp = [(rng.standard_normal((P, B)) * 0.5).astype(np.float32) for _ in range(need)]
    if need > 1:
        qp[1][:, [0, B - 3]] = qp[0][:, [0, B - 3]]  # Q1 == Q2: the first minimum takes the gradient
    if need == 4:
        qp[3][:, 5] = qp[2][:, 5]
    qp[0][:, 2] = -0.0  # a partial sum of -0.0 only
    qp[need - 1][:, B - 1] = -0.0
    q_parts = [dev(q) for q in qp]
    rew, done = dev(rng.standard_normal(B)), dev((rng.uniform(0, 1, B) < 0.3).astype(np.float32))
    next_logp, logp = dev(rng.standard_normal(B) - 1.0), dev(rng.standard_normal(B) - 1.0)
    ent_coef, log_alpha = dev(np.array([0.37])), dev(np.array([-0.6]))

    def launch(lean):
        b = Bufs()
        outs = {k: b.new(k, *s) for k, s in (("q_out", (nd, B)), ("gq_out", (nd, B)), ("loss_out", (1,)))}
        written = ["q_out", "gq_out", "loss_out"]
        loss_sum = b.put("loss_sum", np.array([2.5], np.float32))
        kw = {}
        if td:
            outs["target_out"] = b.new("target_out", B)
            kw = dict(dz2=b.new("dz2", nd, B, H2), dz1=b.new("dz1", nd, B, H1))
            written += ["target_out", "dz2", "dz1"]
        else:
            kw = dict(gact_part=b.new("gact_part", nd, G1, B, A))
            written.append("gact_part")
        adict = None
        if alpha:
            a_out = {k: b.new("alpha_" + k, 1) for k in ("grad_out", "ent_coef_out", "loss_out")}
            written += ["alpha_" + k for k in a_out]
            a_sum = dict(loss_sum=b.put("alpha_loss_sum", np.array([1.5], np.float32)), ent_coef_sum=b.put("alpha_ent_coef_sum", np.array([0.75], np.float32)))
            adict = dict(log_alpha=log_alpha, logp_pi=logp, target_entropy=-float(A), **a_out, **a_sum)
        opts = [_Opt(ops, 3, (0.9, 0.999)), _Opt(ops, 7, (0.8, 0.99))][:2 if td else 1]
        rng_ctl = ops.new_rng_ctl(5, DEV)
        rng_ctl[1] = 1000
        root = ops.chain_root(mode, B, q_parts, [w["b3"] for w in wts], P, gamma=0.97, scale=0.5, next_logp=next_logp if with_logp else None,
                              rew=rew, done=done, ent_coef=ent_coef, logp=logp, target_out=outs.get("target_out"), q_out=outs["q_out"],
                              gq_out=outs["gq_out"], loss_out=outs["loss_out"], loss_sum=loss_sum, alpha=adict, rng_advance=(rng_ctl, 2 * B + 3),
                              adam_advance=opts)
        nets = [ops.chain_net(layers(wts[g]), None, h1[g], h2[g]) for g in range(nd)]
        ops.q_chain_bwd(nets, root, W, D, H1, H2, tiles, **kw)
        out = collect(b, written, dict(rng_ctl=rng_ctl, **{f"adam_ctl_{i}": o.ctl for i, o in enumerate(opts)}))
        assert int(rng_ctl[1]) == 1000 + 2 * B + 3 and [int(o.ctl[0]) for o in opts] == [4, 8][:len(opts)], lean  # the loss workgroup ran
        assert out["loss_sum"][0] == np.float32(np.float32(2.5) + out["loss_out"][0])
        if mode == "sac_actor":  # the tie rows: the first network takes the gradient, the second none
            gq = out["gq_out"][:nd * B].reshape(nd, B)
            assert gq[0, 0] == np.float32(-1.0 / B) and gq[1, 0] == 0.0 and gq[0, B - 3] == np.float32(-1.0 / B) and gq[1, B - 3] == 0.0
        return out

    both(ops, launch)
