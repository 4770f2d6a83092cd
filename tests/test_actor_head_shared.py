"""The squashed-Gaussian head's element arithmetic is ONE set of device functions (csrc/cstr_gaussian_device.h) that every head
launch calls, so launches fed the same (mean, raw log_std, eps) give the same bits: squashed_gaussian_fwd, gaussian_head_fwd_
(no bias, given eps) and gaussian_head_gemm_fwd (K = 8, one-hot weight rows and a zero bias: products with zero and sums of
zeros are exact, so the reduced values ARE the inputs); squashed_gaussian_bwd and gaussian_head_bwd likewise. The inputs cover
both sides of the log-std clamp, both bounds exactly, and |u| where tanhf saturates. (The evaluation kernel against the policy
launch, and the two policy kernels against each other, are pinned bit for bit by test_eval_episodes.py / test_hip_mlp_glue.py.)"""
import pytest
import torch as th

pytestmark = pytest.mark.gpu

B, K = 65, 8


def bits(t):
    return t.contiguous().view(th.int32)


@pytest.fixture(scope="module", params=[1, 3, 4])
def head_io(request):
    """(A, mu, raw, eps) plus every launch's outputs, computed once per action width."""
    assert th.cuda.is_available()
    from core.common import hip_ops

    A = request.param
    g = th.Generator().manual_seed(100 + A)
    mu, raw, eps = th.randn(B, A, generator=g), th.randn(B, A, generator=g) * 3 - 1, th.randn(B, A, generator=g)
    raw[0, 0], raw[1, -1], raw[2, 0], raw[3, -1] = -25.0, 3.5, -20.0, 2.0  # below / above the clamp, exactly on both bounds
    raw[4, 0], raw[5, 0] = -20.000002, 2.0000002                             # the neighbours just outside
    mu[6, 0], mu[7, -1], eps[8, 0], raw[8, 0] = 12.0, -15.0, 6.0, 2.0        # |u| where tanhf has saturated to +-1
    eps[9, 0] = 0.0                                                          # the mode
    mu, raw, eps = mu.cuda(), raw.cuda(), eps.cuda()
    params = th.cat((mu, raw), dim=1).contiguous()
    out = dict(A=A, mu=mu, raw=raw, eps=eps)
    u = mu + th.clamp(raw, -20, 2).exp() * eps
    assert float(u.abs().max()) > 10 and bool((raw < -20).any()) and bool((raw > 2).any())

    a, lp = th.empty(B, A, device="cuda"), th.empty(B, device="cuda")
    hip_ops.squashed_gaussian_fwd(params[:, :A], params[:, A:], eps, a, lp)
    out["sg"] = (a, lp)

    p, a, lp = params.clone(), th.empty(B, A, device="cuda"), th.empty(B, device="cuda")
    hip_ops.gaussian_head_fwd_(p, None, eps, None, a, lp)
    out["head"] = (a, lp, p)

    hidden, w = th.zeros(B, K, device="cuda"), th.zeros(2 * A, K, device="cuda")
    hidden[:, :2 * A] = params
    w[th.arange(2 * A), th.arange(2 * A)] = 1.0
    p, a, lp = th.empty(B, 2 * A, device="cuda"), th.empty(B, A, device="cuda"), th.empty(B, device="cuda")
    hip_ops.gaussian_head_gemm_fwd(hidden, w, th.zeros(2 * A, device="cuda"), p, eps, None, a, lp)
    out["gemm"] = (a, lp, p)

    gg = th.Generator().manual_seed(200 + A)
    ga, gl = th.randn(B, A, generator=gg).cuda(), th.randn(B, generator=gg).cuda()
    action = out["sg"][0]
    gp_sg, gp_head = th.empty(B, 2 * A, device="cuda"), th.empty(B, 2 * A, device="cuda")
    hip_ops.squashed_gaussian_bwd(ga, gl, action, params[:, A:], eps, gp_sg[:, :A], gp_sg[:, A:])
    hip_ops.gaussian_head_bwd(ga, gl, action, params, eps, gp_head, None)
    out["bwd"] = (gp_sg, gp_head)
    th.cuda.synchronize()
    return out


def test_forward_bits_agree(head_io):
    A, (a0, lp0) = head_io["A"], head_io["sg"]
    assert bool(th.isfinite(a0).all()) and bool(th.isfinite(lp0).all())
    assert float(a0.abs().max()) == 1.0  # the saturated rows are in the batch
    for name in ("head", "gemm"):
        a, lp, p = head_io[name]
        assert th.equal(bits(p[:, :A]), bits(head_io["mu"])) and th.equal(bits(p[:, A:]), bits(head_io["raw"])), name
        assert th.equal(bits(a), bits(a0)), name
        assert th.equal(bits(lp), bits(lp0)), name


def test_backward_bits_agree(head_io):
    A, raw = head_io["A"], head_io["raw"]
    gp_sg, gp_head = head_io["bwd"]
    assert bool(th.isfinite(gp_sg).all())
    assert th.equal(bits(gp_head), bits(gp_sg))
    # outside the clamp the log-std gradient is cut, on the bounds it is not
    outside = (raw < -20) | (raw > 2)
    assert bool((gp_sg[:, A:][outside] == 0).all()) and bool(outside.any())
    assert float(gp_sg[2, A].abs()) > 0 and float(gp_sg[3, 2 * A - 1].abs()) > 0
