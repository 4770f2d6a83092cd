"""fp64 statements of the gSDE launches (csrc/cstr_sde.hip) and of the BCQ launches (csrc/cstr_bcq.hip), their magnitude passes, the
NumPy statement of the in-kernel normal streams, the comparator, the case lists and the seeded input generators. CPU only.

Every statement is written from the reference's expressions (core/common/distributions.py:421-617: get_std, sample_weights,
proba_distribution, get_noise, log_prob through the atanh round trip; core/bcq/bcq.py:137-213, core/bcq/policies.py:67-166, :244-253,
:426-435). A statement takes the float32 arrays its launch reads and

    dtype  torch.float64 = the reference; torch.float32 = the same statement on stock ATen, which sets the bars
    mag    the magnitude pass: every additive term replaced by its absolute value, every subtraction by an addition, the masks
           dropped (divisors keep their true value). Its result M bounds the sum of absolute terms behind each output element
    mut    one of MUTATIONS: a deliberately wrong statement (tests/test_rowkernel_reference.py shows the comparator rejects each)

The backward statements are explicit expressions so that they have a magnitude pass; tests/test_rowkernel_reference.py ties each of
them to fp64 autograd through the forward statement. Errors are per element in units of 2**-24 * M (_chain_reference.units). BARS
holds, per output kind, four times the worst figure of the float32 ATen evaluation over the cases below; the CPU module re-measures
the figures and asserts 4 * ATen <= bar <= 64.

Drawn normals. normal_stream is the documented counter contract in fp64. A float32 kernel cannot hold u1 = (x + 0.5) / 2**24 for x >=
2**23 (25 significant bits: x + 0.5 rounds to x or x + 1), and the radius sqrt(-2 ln u1) has the derivative -1 / (u1 r), unbounded as
u1 -> 1. normal_slack is that representation error carried through the radius exactly: max |r(u1 +- 2**-25) - r(u1)| per pair. It
is below NORMAL_SLACK_FLOOR (a tenth of the cap of the bar) for all but ~5e-4 of the pairs (asserted: at most 1e-3 of a case); those
elements alone get bar + slack, every other element the bar. Without it no launch beyond one pass of the grid (> 2**19 pairs) could
meet a bar under 1e-5: some 2 to 3 of its pairs have 1 - u1 < 4.5e-6, where the representation error alone moves the radius by more
than 1e-5. A counter mistake gives errors of order 1 on every element."""
import functools

import numpy as np
import torch as th

from _chain_reference import CAP, F32, F64, U, np64, units  # noqa: F401  (the per-element figure is shared, not forked)
from _dqn_helpers import philox4x32_10

SDE_TAG, BCQ_TAG = 0x5DE5DE5D, 0xBC0BC0B1  # csrc/cstr_sde.hip SDE_STREAM_TAG, csrc/cstr_bcq.hip BCQ_STREAM_TAG
SDE_EPS = 1e-6
TANH_CLAMP = 1.0 - float(np.finfo(np.float32).eps)
HALF_LOG_2PI = 0.91893853320467274178
BCQ_LS_MIN, BCQ_LS_MAX = -4.0, 15.0
BELOW_NONE, BELOW_RELU, BELOW_TANH = 0, 1, 2
X_SAT = 4.0  # |x| beyond which atanh(tanh(x)) of a float32 tanh is ill-conditioned: rows left out of the logp / gradient comparison
GRID_PAIRS = 2048 * 256  # pairs one pass of a drawing kernel's grid covers: beyond it the grid-stride loop iterates

# 4 x the worst float32 ATen figure over the cases of this module (measured figures: the docstring of tests/test_rowkernels.py)
BARS = {
    "pre": 20.81, "var": 49.35, "g_pre": 8.80, "g_x": 13.62, "g_var": 18.34, "dh": 12.78, "dw": 15.24, "db": 6.52, "dlog_std": 17.78,
    "bcq_z": 7.40, "bcq_g_mean": 4.00, "bcq_g_ls": 10.72, "vae_loss": 7.16, "vae_g_recon": 6.87, "vae_g_mean": 3.97, "vae_g_std": 8.94,
    "perturb": 5.42, "perturb_g": 3.80, "target": 6.81,
}
NORMAL_CAP = 1e-5
NORMAL_BAR = 9.78e-06  # 4 x the worst |float32 NumPy Box-Muller - fp64| over draw_cases() outside the slack elements
NORMAL_SLACK_FLOOR = 1e-6
MUTATIONS = ("no_var", "no_below", "ls_nosum", "expln_exp", "db_256", "dw_tail", "hardtanh_open", "clamp_open", "group_swap", "last_max",
             "half_advance", "no_hi", "other_tag")


def _t(a, dtype, mag=False):
    t = a.to(dtype) if isinstance(a, th.Tensor) else th.as_tensor(np.asarray(a)).to(dtype)  # a tensor passes through (autograd ties)
    return t.abs() if mag else t


def worst(got, want, mag):
    """_chain_reference.units over the elements that have operands; an element without any (M = 0: a latent column that is zero in
    every row) must equal the reference exactly, or the figure is infinite. Returns (figure, flat index among the elements with M > 0)"""
    got, want, mag = (np.asarray(v, np.float64).reshape(-1) for v in (got, want, mag))
    has = mag > 0
    if not np.array_equal(got[~has], want[~has]):
        return float("inf"), -1
    if not has.any():
        return 0.0, -1
    u = units(got[has], want[has], mag[has])
    i = int(np.argmax(u))
    return float(u[i]), i


def accepts(kind, got, want, mag):
    return worst(got, want, mag)[0] <= BARS[kind]


# ---- the normal streams --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _uniform_pairs(seed, base, pairs, tag, mut=None):
    """r0 >> 8, r1 >> 8 of pairs 0 .. pairs - 1: counter (lo32(base + p), hi32(base + p), 0, tag), key (lo32(seed), hi32(seed)). Cached: the
    stream and its slack share one Philox pass; callers do not write into the result"""
    m32 = np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        ctr = np.uint64(base & 0xFFFFFFFFFFFFFFFF) + np.arange(pairs, dtype=np.uint64)  # wraps at 2**64 like the kernel's uint64_t
    c = np.zeros((pairs, 4), np.uint32)
    c[:, 0] = (ctr & m32).astype(np.uint32)
    c[:, 1] = 0 if mut == "no_hi" else (ctr >> np.uint64(32)).astype(np.uint32)
    c[:, 3] = np.uint32(tag)
    r = philox4x32_10(c, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    return r[:, 0] >> np.uint32(8), r[:, 1] >> np.uint32(8)


def normal_stream(seed, base, n_elems, tag, dtype=np.float64, mut=None):
    """elements 0 .. n - 1 of the stream at offset `base`: pair p = i // 2, u = ((r >> 8) + 0.5) / 2**24, z0 = sqrt(-2 ln u1) cos(2 pi
    u2), z1 = ... sin(...); element 2 p + k = z_k. dtype float32: every operation rounded to float32 (what sets the bar)."""
    pairs = (n_elems + 1) // 2
    a, b = _uniform_pairs(seed, base, pairs, tag, mut)
    f = np.dtype(dtype).type
    u1 = (a.astype(dtype) + f(0.5)) * f(2.0 ** -24)
    u2 = (b.astype(dtype) + f(0.5)) * f(2.0 ** -24)
    r = np.sqrt(f(-2.0) * np.log(u1))
    ang = f(2.0 * np.pi) * u2
    z = np.stack((r * np.cos(ang), r * np.sin(ang)), 1).astype(dtype)
    return z.reshape(-1)[:n_elems]


def normal_slack(seed, base, n_elems, tag):
    """per element: what the float32 representation error of u1 (up to 2**-25, see the module docstring) moves the radius by, 0 where
    that is below NORMAL_SLACK_FLOOR"""
    pairs = (n_elems + 1) // 2
    a, _ = _uniform_pairs(seed, base, pairs, tag)
    u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -24
    rad = lambda u: np.sqrt(-2.0 * np.log(np.minimum(u, 1.0)))  # noqa: E731
    s = np.maximum(np.abs(rad(u1 + 2.0 ** -25) - rad(u1)), np.abs(rad(u1 - 2.0 ** -25) - rad(u1)))
    s = np.where((a >= 2 ** 23) & (s >= NORMAL_SLACK_FLOOR), s, 0.0)
    return np.repeat(s, 2)[:n_elems]


def normal_worst(got, seed, base, n_elems, tag):
    """(worst |got - stream| over the elements without slack, worst of (|got - stream| - slack) over those with, share of slack elements)"""
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - normal_stream(seed, base, n_elems, tag))
    slack = normal_slack(seed, base, n_elems, tag)
    plain = slack == 0
    return float(err[plain].max()), float((err - slack)[~plain].max()) if (~plain).any() else 0.0, float((~plain).mean())


def normal_accepts(got, seed, base, n_elems, tag, bar=None):
    w, ws, share = normal_worst(got, seed, base, n_elems, tag)
    bar = NORMAL_BAR if bar is None else bar
    return w <= bar and ws <= bar and share <= 1e-3


def mutated_stream(seed, base, n_elems, tag, mut, launch_pairs=0):
    """what a kernel with the mistake would draw for a launch that FOLLOWS one of launch_pairs pairs on the same control block"""
    if mut == "half_advance":
        return normal_stream(seed, base - launch_pairs + launch_pairs // 2, n_elems, tag)
    if mut == "other_tag":
        return normal_stream(seed, base, n_elems, BCQ_TAG if tag == SDE_TAG else SDE_TAG)
    return normal_stream(seed, base, n_elems, tag, mut=mut)


# the drawn launches of tests/test_rowkernels.py: an odd element count, z_keep in {0, 1, all}, a counter that carries into the high word
# inside the launch, a seed with bits above 32, one launch per kernel beyond one pass of the grid
HI_SEED = (0xABCDE << 32) | 17
SDE_DRAWS = [(1, 5, 3, 1, 11, 0), (2, 5, 3, 1, 12, 7), (258, 5, 3, 0, 16, 2 ** 32 - 3), (258, 7, 1, 258, HI_SEED, 0),
             (4100, 256, 1, 1, 21, 2 ** 32 - 3)]  # (n_mats, L, A, z_keep, seed, base)
BCQ_LATENT_DRAWS = [(1, 3, 1, 31, 0), (3, 5, 7, HI_SEED, 2 ** 32 - 3), (257, 8, 33, 33, 5), (4100, 4, 256, 34, 0)]  # (B, D, L, seed, base)
BCQ_EXPAND_DRAWS = [(5, 1, 3, 7, 41, 0, 0.5), (5, 3, 4, 32, HI_SEED, 2 ** 32 - 3, 0.5), (4100, 1, 4, 256, 43, 1, 100.0)]  # (n, S, D, L, seed, base, clip)


def draw_cases():
    """(n_elems, seed, base, tag) of every drawn launch above and of the second launch on its control block"""
    out = []
    for n, L, A, _, seed, base in SDE_DRAWS:
        out.append((n * L * A, seed, base, SDE_TAG))
    for B, _, L, seed, base in BCQ_LATENT_DRAWS:
        out.append((B * L, seed, base, BCQ_TAG))
    for n, S, _, L, seed, base, _ in BCQ_EXPAND_DRAWS:
        out.append((n * S * L, seed, base, BCQ_TAG))
    return out + [(n, seed, base + (n + 1) // 2, tag) for n, seed, base, tag in out]


# ---- gSDE ----------------------------------------------------------------------------------------------------------------------------
def sde_std_stmt(log_std, expln, A, dtype=F64, mut=None):
    """get_std: exp, or expln = exp(x) for x <= 0 and log1p(x + eps) + 1 above; a [L, 1] log_std is spread over the A columns"""
    ls = _t(log_std, dtype)
    if expln and mut != "expln_exp":
        std = th.exp(ls) * (ls <= 0) + (th.log1p(ls * (ls > 0) + SDE_EPS) + 1.0) * (ls > 0)
    else:
        std = th.exp(ls)
    return std if std.shape[1] == A else std * th.ones(ls.shape[0], A, dtype=dtype)


def sde_dstd(log_std, expln, dtype=F64, mut=None):
    """d std / d log_std of get_std (the masks are constants)"""
    ls = _t(log_std, dtype)
    if expln and mut != "expln_exp":
        return th.where(ls <= 0, th.exp(ls), 1.0 / (1.0 + (ls + SDE_EPS)))
    return th.exp(ls)


def sde_fwd_stmt(inp, dtype=F64, mag=False):
    """pre = h W^T + b, mean = Hardtanh(pre), var = h^2 (std^2), x = mean (+ h M, one matrix or one per row), action = tanh(x), logp =
    Normal(mean, sqrt(var + eps)).log_prob(atanh(clamp(action))).sum - log(1 - tanh(.)^2 + eps).sum. std [L, A] and mats are given."""
    h, w, b, std = _t(inp["h"], dtype, mag), _t(inp["w"], dtype, mag), _t(inp["b"], dtype, mag), _t(inp["std"], dtype, mag)
    clip = inp["clip"]
    pre = h @ w.T + b
    var = (h * h) @ (std * std)
    out = dict(pre=pre, var=var)
    if mag:
        return out
    mean = th.clamp(pre, -clip, clip) if clip > 0 else pre
    if inp["noise"] == "mode":
        x = mean
    elif inp["noise"] == "per_row":
        x = mean + th.bmm(h.unsqueeze(1), _t(inp["mats"], dtype)).squeeze(1)
    else:
        x = mean + h @ _t(inp["mats"], dtype)
    act = th.tanh(x)
    scale = th.sqrt(var + SDE_EPS)
    c = act.clamp(-TANH_CLAMP, TANH_CLAMP)
    ga = 0.5 * (c.log1p() - (-c).log1p())
    lp = (-((ga - mean) ** 2) / (2 * scale ** 2) - scale.log() - HALF_LOG_2PI).sum(1) - th.log(1.0 - th.tanh(ga) ** 2 + SDE_EPS).sum(1)
    out.update(mean=mean, x=x, action=act, logp=lp)
    return out


def sde_bwd_stmt(inp, dtype=F64, mag=False, mut=None):
    """Gradients of sum_rows(g_action . action + g_logp * logp) on GIVEN action [B, A] and aux = (pre | var) [B, 2A] (the forward
    launch's stored outputs): g_pre (through the Hardtanh: zero at and beyond the bounds), g_x (through x = mean + noise; zero for the
    mode), g_var, and dh = (g_pre W + g_x M^T + 2 h (g_var (std^2)^T)) * below'(h)."""
    A = inp["w"].shape[0]
    sub = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    clip = inp["clip"]
    act = _t(inp["action"], dtype, mag)
    pre, var = _t(inp["aux"][:, :A], dtype), _t(inp["aux"][:, A:], dtype)
    B = act.shape[0]
    gl = _t(inp["g_logp"], dtype, mag).reshape(B, 1) if inp.get("g_logp") is not None else th.zeros(B, 1, dtype=dtype)
    gact = _t(inp["g_action"], dtype, mag) if inp.get("g_action") is not None else th.zeros(B, A, dtype=dtype)
    mean = th.clamp(pre, -clip, clip) if clip > 0 else pre
    if mag:
        mean = mean.abs()
    v2 = var + SDE_EPS
    scale = th.sqrt(v2)
    c = act.clamp(-TANH_CLAMP, TANH_CLAMP)
    ga = 0.5 * sub(c.log1p(), (-c).log1p()) if not mag else 0.5 * (c.log1p() + (-c).log1p().abs())
    d = sub(ga, mean)
    t = th.tanh(ga)
    omt_true = 1.0 - t * t
    omt = sub(1.0, t * t)
    g_ga = gl * ((d / v2 if mag else -d / v2) + 2.0 * t * omt / (omt_true + SDE_EPS))
    g_c = g_ga * 0.5 * (1.0 / (1.0 + c) + 1.0 / (1.0 - c))
    inside = th.ones_like(act) if mag else ((act >= -TANH_CLAMP) & (act <= TANH_CLAMP)).to(dtype)
    g_x = (gact + inside * g_c) * sub(1.0, act * act)
    g_mean = g_x + gl * (d / v2)
    g_scale = gl * sub((d * d) / (scale * v2), 1.0 / scale)
    g_var = g_scale * 0.5 / scale
    if clip > 0 and not mag:
        passes = ((pre >= -clip) & (pre <= clip)) if mut == "hardtanh_open" else ((pre > -clip) & (pre < clip))
        g_pre = g_mean * passes.to(dtype)
    else:
        g_pre = g_mean
    noise = inp["noise"]
    gx_out = g_x if noise != "mode" else th.zeros_like(g_x)
    out = dict(g_pre=g_pre, g_x=gx_out, g_var=g_var)
    h, w, std = _t(inp["h"], dtype, mag), _t(inp["w"], dtype, mag), _t(inp["std"], dtype, mag)
    dh = g_pre @ w
    if noise == "per_row":
        dh = dh + th.bmm(_t(inp["mats"], dtype, mag), g_x.unsqueeze(2)).squeeze(2)
    elif noise == "shared":
        dh = dh + g_x @ _t(inp["mats"], dtype, mag).T
    if mut != "no_var":
        dh = dh + 2.0 * h * (g_var @ (std * std).T)
    below = inp["below"]
    if mut != "no_below":
        if below == BELOW_RELU and not mag:
            dh = dh * (_t(inp["h"], dtype) > 0).to(dtype)
        elif below == BELOW_TANH:
            dh = dh * sub(1.0, h * h)
    out["dh"] = dh
    return out


def sde_param_stmt(inp, dtype=F64, mag=False, mut=None):
    """On GIVEN g_pre, g_x, g_var [B, A]: dw [A, L] = g_pre^T h, db [A] = column sums of g_pre, d std = z * (h^T g_x) + 2 std * ((h^2)^T
    g_var), d log_std = d std * std'(log_std), summed over A for a [L, 1] log_std; z None (the mode): no noise term"""
    h = _t(inp["h"], dtype, mag)
    gp, gx, gv = (_t(inp[k], dtype, mag) for k in ("g_pre", "g_x", "g_var"))
    std = _t(inp["std"], dtype, mag)
    L = h.shape[1]
    dw = gp.T @ h
    if mut == "dw_tail" and L % 64:
        dw = dw.clone()
        dw[:, L - L % 64:] = 0.0
    db = (gp[:256] if mut == "db_256" else gp).sum(0)
    dstd = 2.0 * std * ((h * h).T @ gv)
    if inp.get("z") is not None:
        dstd = dstd + _t(inp["z"], dtype, mag) * (h.T @ gx)
    dls = dstd * sde_dstd(inp["log_std"], inp["expln"], dtype, mut)
    if inp["log_std"].shape[1] == 1:
        dls = dls[:, :1] if mut == "ls_nosum" else dls.sum(1, keepdim=True)
    return dict(dw=dw, db=db, dlog_std=dls)


# (B, L, A): smallest; below one 64-lane stride; exact stride; one lane in the second stride and column block; several strides and
# blocks; ragged L twice; the learner's width with B > 256 (the db block's strided loop) and B % 4 == 1
SDE_SHAPES = [(1, 3, 1), (3, 63, 1), (5, 64, 3), (7, 65, 4), (66, 129, 4), (130, 100, 2), (33, 300, 3), (257, 256, 2)]
SDE_NOISE = ("shared", "per_row", "mode")
SDE_STRIDED = (3, 5)  # the shapes whose launches also run with strided h / action / g_action and with each optional operand left out
SDE_SEED_BASE = 20261019


def sde_variants(si):
    """the 12 (full, expln, noise, below, clip) of shape si: below_act and clip_mean spread so that every value meets every noise form"""
    out = []
    for j, (full, expln, noise) in enumerate((f, e, n) for f in (True, False) for e in (False, True) for n in SDE_NOISE):
        k = SDE_NOISE.index(noise)
        out.append((full, expln, noise, (si + k + j // 3) % 3, 1.0 if (si + j // 3 + k) % 2 == 0 else 0.0))
    return out


def sde_inputs(seed, B, L, A, full, expln, noise, below, clip):
    """the sweep generator: h = relu(N(0, 1)) sqrt(2 / L), w ~ N(0, 0.7), b ~ N(0, 0.3), log_std ~ N(-1, 0.8), z ~ N(0, 1); std and
    mats are the fp64 statements rounded to float32 (the GPU test replaces them by the draw launch's own output)"""
    g = np.random.default_rng(seed)
    h = (np.maximum(g.normal(0, 1, (B, L)), 0) * np.sqrt(2.0 / L)).astype(np.float32)
    w, b = g.normal(0, 0.7, (A, L)).astype(np.float32), g.normal(0, 0.3, A).astype(np.float32)
    ls = g.normal(-1.0, 0.8, (L, A if full else 1)).astype(np.float32)
    n = B if noise == "per_row" else 1
    z = g.normal(0, 1, (n, L, A)).astype(np.float32)
    std = sde_std_stmt(ls, expln, A).numpy().astype(np.float32)
    mats = (z.astype(np.float64) * std.astype(np.float64)).astype(np.float32)
    return dict(h=h, w=w, b=b, log_std=ls, expln=expln, z=z, std=std, mats=None if noise == "mode" else (mats if noise == "per_row" else mats[0]),
                noise=noise, below=below, clip=clip, g_action=g.normal(0, 1, (B, A)).astype(np.float32), g_logp=g.normal(0, 1, B).astype(np.float32))


def hardtanh_margin(pre, mag, clip, bar):
    """the smallest distance of an fp64 pre-activation from +-clip in units of bar * 2**-24 * M (>= 1: no float32 evaluation within the
    bar flips the mask); entries exactly on a bound are there on purpose and skipped"""
    if clip <= 0:
        return np.inf
    pre, mag = np.asarray(pre, np.float64), np.asarray(mag, np.float64)
    dist = np.minimum(np.abs(pre - clip), np.abs(pre + clip))
    dist = np.where(dist == 0, np.inf, dist)
    return float((dist / (bar * U * mag)).min())


def sat_rows(x):
    """rows with an |x| > X_SAT"""
    return (np.abs(np.asarray(x, np.float64)) > X_SAT).any(1)


def sde_case_ok(inp):
    f, m = sde_fwd_stmt(inp), sde_fwd_stmt(inp, mag=True)
    B = inp["h"].shape[0]
    sat = sat_rows(f["x"].numpy())
    return (hardtanh_margin(f["pre"].numpy(), m["pre"].numpy(), inp["clip"], BARS["pre"]) >= 1.0
            and sat.sum() <= (B // 16 if B >= 16 else 0))


def sde_case(si, vi):
    """the first seed at which conditions (a) and (b) hold: no pre-activation within the bar of the Hardtanh bounds, at most B / 16
    rows with |x| > 4 (none for B < 16)"""
    B, L, A = SDE_SHAPES[si]
    for seed in range(SDE_SEED_BASE + 10000 * si + 100 * vi, SDE_SEED_BASE + 10000 * si + 100 * vi + 100):
        inp = sde_inputs(seed, B, L, A, *sde_variants(si)[vi])
        if sde_case_ok(inp):
            return inp
    raise AssertionError("no seed meets the input conditions")


def sde_bwd_inputs(inp, action, aux, on_bound=True):
    """the backward launch's inputs: the forward's stored action / aux (float32); rows 1 and 2 get a pre-clip mean exactly on +-clip on
    purpose (the Hardtanh gradient is zero AT the bound)"""
    out = dict(inp, action=np.array(action, np.float32), aux=np.array(aux, np.float32))
    if on_bound and inp["clip"] > 0 and out["aux"].shape[0] >= 3:
        out["aux"][1, 0], out["aux"][2, 0] = inp["clip"], -inp["clip"]
    return out


# ---- BCQ -----------------------------------------------------------------------------------------------------------------------------
def bcq_latent_fwd_stmt(inp, dtype=F64, mag=False, std=None):
    """std = exp(clamp(raw, -4, 15)); z = mean + std * eps (on a GIVEN std when passed: the launch's own output)"""
    p, eps = _t(inp["params"], dtype), _t(inp["eps"], dtype, mag)
    L = eps.shape[1]
    s = th.exp(th.clamp(p[:, L:], BCQ_LS_MIN, BCQ_LS_MAX)) if std is None else _t(std, dtype)
    mean = p[:, :L].abs() if mag else p[:, :L]
    return dict(std=s, bcq_z=mean + s * eps)


def bcq_latent_bwd_stmt(inp, dtype=F64, mag=False, mut=None):
    """g_mean = g_z + g_mean_kl; g_raw = (g_z * eps + g_std_kl) * std where -4 <= raw <= 15 (clamp's closed interval), else 0"""
    p, eps, std = _t(inp["params"], dtype), _t(inp["eps"], dtype, mag), _t(inp["std"], dtype, mag)
    L = eps.shape[1]
    z0 = th.zeros_like(eps)
    gz, gm, gs = (_t(inp[k], dtype, mag) if inp.get(k) is not None else z0 for k in ("g_z", "g_mean_kl", "g_std_kl"))
    raw = p[:, L:]
    keep = ((raw > BCQ_LS_MIN) & (raw < BCQ_LS_MAX)) if mut == "clamp_open" else ((raw >= BCQ_LS_MIN) & (raw <= BCQ_LS_MAX))
    g_ls = (gz * eps + gs) * std
    return dict(bcq_g_mean=gz + gm, bcq_g_ls=g_ls if mag else g_ls * keep.to(dtype))


def bcq_vae_stmt(inp, dtype=F64, mag=False):
    """mse(recon, act) + 0.5 * (-0.5 * mean(1 + log(std^2) - mean^2 - std^2)) and its gradients w.r.t. recon, mean, std"""
    sub = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    r, a, s = _t(inp["recon"], dtype, mag), _t(inp["act"], dtype, mag), _t(inp["std"], dtype, mag)
    L = s.shape[1]
    m = _t(inp["params"][:, :L], dtype, mag)
    d = sub(r, a)
    logs = th.log(s * s).abs() if mag else th.log(s * s)
    kl_terms = sub(sub(1.0 + logs, m * m), s * s)
    rec, kl = (d * d).mean(), 0.5 * kl_terms.mean()
    loss = rec + 0.5 * kl if mag else rec - 0.5 * kl
    n_rec, n_lat = float(r.numel()), float(s.numel())
    return dict(vae_loss=loss.reshape(1), vae_g_recon=2.0 * d / n_rec, vae_g_mean=0.5 * m / n_lat,
                vae_g_std=0.25 * sub(2.0 * s, 2.0 / s) / n_lat)


def bcq_expand_stmt(state, noise, S, clip):
    """rows r = [state[r % n] | clamp(noise[r], -clip, clip)]: copies and clamps of given values, compared bit for bit"""
    return np.tile(np.asarray(state, np.float32), (S, 1)), np.clip(np.asarray(noise, np.float32), np.float32(-clip), np.float32(clip))


def bcq_perturb_stmt(inp, dtype=F64, mag=False, mut=None):
    """out = clamp(a + mp * p, -1, 1); g_p = g * mp where -1 <= a + mp * p <= 1 (closed), else 0. mp is the float32 the launch receives"""
    a, p = _t(inp["a_vae"], dtype, mag), _t(inp["p"], dtype, mag)
    mp = float(np.float32(inp["mp"]))
    x = a + p * mp
    out = dict(perturb_x=x, perturb=x if mag else th.clamp(x, -1.0, 1.0))
    if inp.get("g") is not None:
        g = _t(inp["g"], dtype, mag)
        keep = ((x > -1.0) & (x < 1.0)) if mut == "clamp_open" else ((x >= -1.0) & (x <= 1.0))
        out["perturb_g"] = g * mp if mag else g * mp * keep.to(dtype)
    return out


def bcq_target_stmt(inp, grouping, dtype=F64, mag=False, mut=None):
    """min over the N critics per row, max over groups of S rows: grouping 0 = S consecutive flat rows (the reference's reshape(n, S)),
    grouping 1 = a state's own candidates i, i + n, ...; target = rew + (1 - done) * gamma * max. max_q is a selection: bit for bit"""
    q = _t(inp["q"], dtype)
    n, S = inp["n"], inp["S"]
    qmin = q.min(0)[0]
    if mut == "group_swap":
        grouping = 1 - grouping
    best = qmin.reshape(n, S).max(1)[0] if grouping == 0 else qmin.reshape(S, n).max(0)[0]
    rew, done = _t(inp["rew"], dtype, mag), _t(inp["done"], dtype, mag)
    gamma = float(np.float32(inp["gamma"]))
    keep = (1.0 + done) if mag else (1.0 - done)
    return dict(max_q=best, target=rew + keep * gamma * (best.abs() if mag else best))


def bcq_select_stmt(q1, cand, n, S, mut=None):
    """per state the first maximum of q1 over its candidates i, i + n, ... (argmax) and that row of cand"""
    q = np.asarray(q1, np.float32).reshape(S, n)
    s = (S - 1 - q[::-1].argmax(0)) if mut == "last_max" else q.argmax(0)
    idx = s * n + np.arange(n)
    return idx.astype(np.int64), np.asarray(cand, np.float32)[idx]


def perturb_margin(x, mag, bar):
    """as hardtanh_margin, for the perturbation's clamp at +-1"""
    return hardtanh_margin(x, mag, 1.0, bar)


BCQ_LATENT_SHAPES = [(1, 3, 1), (3, 5, 7), (96, 4, 32), (257, 8, 33), (260, 4, 256)]  # (B, D, L): odd B L; the learner's; ragged; the widest latent
BCQ_VAE_SHAPES = [(64, 2, 32), (256, 2, 32), (37, 3, 5), (1, 1, 1), (300, 4, 33)]  # (B, A, L)
# (n, S, D, L, A, kind): the scalar path (D % 4 != 0), VEC with 6-float xa / xb rows (va = vb = false), VEC with 8-float rows (va = vb =
# true), va true and vb false (xb 4 bytes off a 16-byte boundary), a misaligned state view (VEC off)
BCQ_EXPAND_CASES = [(3, 100, 5, 6, 3, "scalar"), (5, 1, 3, 7, 2, "scalar"), (64, 10, 4, 32, 2, "vec"), (5, 3, 4, 32, 4, "vec_ab"), (3, 2, 8, 8, 4, "vec_ab"),
                    (7, 3, 4, 8, 4, "vec_a"), (5, 3, 4, 32, 4, "misaligned")]
BCQ_PERTURB_ROWS, BCQ_PERTURB_ACT = (1, 3, 257), (1, 2, 3, 64)
BCQ_TARGET_CASES = [(1, 1, 1), (1, 100, 2), (64, 2, 3), (64, 100, 16), (64, 10, 2), (257, 10, 2), (257, 1, 16), (257, 2, 1), (1000, 10, 3), (1000, 2, 16),
                    (1000, 1, 1)]  # (n, S, N)
BCQ_SEED_BASE = 20261119


def bcq_latent_inputs(seed, B, D, L):
    """both clamp bounds engaged and rows exactly on them (spread over whatever rows the case has)"""
    g = np.random.default_rng(seed)
    params = g.normal(0, 1.5, (B, 2 * L)).astype(np.float32)
    k = B * L
    params[0, L] = -4.0                             # exactly on a bound: the gradient passes
    if k > 1:
        params[B - 1, 2 * L - 1] = 15.0
    if k > 4:
        params[B - 1, L], params[0, 2 * L - 1] = -6.5, 17.25  # beyond: the gradient is cut
    if B >= 18:
        params[2:10, L:] = g.uniform(-9, -4.5, (8, L))
        params[10:16, L:] = g.uniform(15.5, 20, (6, L))
        params[16, L:], params[17, L:] = -4.0, 15.0
    f = lambda *s: g.normal(0, 1, s).astype(np.float32)  # noqa: E731
    return dict(params=params, obs=g.uniform(-1, 1, (B, D)).astype(np.float32), eps=f(B, L), g_z=f(B, L), g_mean_kl=(0.1 * f(B, L)).astype(np.float32),
                g_std_kl=(0.1 * f(B, L)).astype(np.float32))


def bcq_vae_inputs(seed, B, A, L):
    g = np.random.default_rng(seed)
    return dict(recon=np.tanh(g.normal(0, 1, (B, A))).astype(np.float32), act=g.uniform(-1, 1, (B, A)).astype(np.float32),
                params=g.normal(0, 1, (B, 2 * L)).astype(np.float32), std=np.exp(np.clip(g.normal(-1, 2, (B, L)), -4, 15)).astype(np.float32))


def bcq_perturb_inputs(seed, rows, A, mp=0.05):
    """rows exactly on +-1 (a = +-1, p = 0: the sum is exact in any precision) and beyond; every other entry clear of the bounds by the
    bar (condition (a)), searched over seeds"""
    for s in range(seed, seed + 200):
        g = np.random.default_rng(s)
        a, p = np.tanh(g.normal(0, 2, (rows, A))).astype(np.float32), np.tanh(g.normal(0, 2, (rows, A))).astype(np.float32)
        a[0, 0], p[0, 0] = 1.0, 0.0
        if A > 1:
            a[0, 1], p[0, 1] = -1.0, 0.0
        if rows > 2:
            a[1], p[1] = 1.0, 1.0
            a[2], p[2] = -1.0, -1.0
        inp = dict(a_vae=a, p=p, mp=mp, g=g.normal(0, 1, (rows, A)).astype(np.float32))
        if perturb_margin(bcq_perturb_stmt(inp)["perturb_x"].numpy(), bcq_perturb_stmt(inp, mag=True)["perturb_x"].numpy(), BARS["perturb"]) >= 1.0:
            return inp
    raise AssertionError("no seed with a clamp margin")


def bcq_target_inputs(seed, n, S, N):
    """Q values rounded to one decimal: plenty of ties, across critics and across candidates"""
    g = np.random.default_rng(seed)
    return dict(q=np.round(g.normal(-3, 2, (N, n * S)), 1).astype(np.float32), n=n, S=S, gamma=0.99, rew=g.uniform(-8, 0, n).astype(np.float32),
                done=(g.uniform(size=n) < 0.3).astype(np.float32))


# ---- the bars -------------------------------------------------------------------------------------------------------------------------
def measure_aten():
    """worst float32-ATen figure per output kind over the cases above, in units of 2**-24 * M (rows with |x| > 4 left out of the gSDE
    backward kinds, as in the GPU comparison)"""
    fig = {}

    def take(stmt, kinds, rows=None):
        ref, f32, mag = np64(stmt(F64, False)), np64(stmt(F32, False)), np64(stmt(F64, True))
        for k in kinds:
            r, f, m = ref[k], f32[k], mag[k]
            if rows is not None and r.ndim == 2 and r.shape[0] == rows.shape[0]:
                r, f, m = r[rows], f[rows], m[rows]
            if r.size:
                fig[k] = max(fig.get(k, 0.0), worst(f, r, m)[0])

    for si in range(len(SDE_SHAPES)):
        for vi in range(12):
            inp = sde_case(si, vi)
            fwd = sde_fwd_stmt(inp)
            take(lambda dt, mg: sde_fwd_stmt(inp, dt, mg), ("pre", "var"))
            keep = ~sat_rows(fwd["x"].numpy())
            aux = th.cat((fwd["pre"], fwd["var"]), 1).numpy()
            binp = sde_bwd_inputs(inp, fwd["action"].numpy(), aux)
            take(lambda dt, mg: sde_bwd_stmt(binp, dt, mg), ("g_pre", "g_x", "g_var", "dh"), keep)
            if inp["noise"] != "per_row":
                bw = sde_bwd_stmt(binp)
                pinp = dict(inp, z=inp["z"][0] if inp["noise"] == "shared" else None, **{k: bw[k].numpy().astype(np.float32) for k in ("g_pre", "g_x", "g_var")})
                take(lambda dt, mg: sde_param_stmt(pinp, dt, mg), ("dw", "db", "dlog_std"))
    for i, (B, D, L) in enumerate(BCQ_LATENT_SHAPES):
        inp = bcq_latent_inputs(BCQ_SEED_BASE + i, B, D, L)
        std32 = bcq_latent_fwd_stmt(inp)["std"].numpy().astype(np.float32)
        take(lambda dt, mg: bcq_latent_fwd_stmt(inp, dt, mg, std=std32), ("bcq_z",))
        binp = dict(inp, std=std32)
        take(lambda dt, mg: bcq_latent_bwd_stmt(binp, dt, mg), ("bcq_g_mean", "bcq_g_ls"))
    for i, (B, A, L) in enumerate(BCQ_VAE_SHAPES):
        inp = bcq_vae_inputs(BCQ_SEED_BASE + 100 + i, B, A, L)
        take(lambda dt, mg: bcq_vae_stmt(inp, dt, mg), ("vae_loss", "vae_g_recon", "vae_g_mean", "vae_g_std"))
    for rows in BCQ_PERTURB_ROWS:
        for A in BCQ_PERTURB_ACT:
            inp = bcq_perturb_inputs(BCQ_SEED_BASE + 1000 * rows + A, rows, A)
            take(lambda dt, mg: bcq_perturb_stmt(inp, dt, mg), ("perturb", "perturb_g"))
    for i, (n, S, N) in enumerate(BCQ_TARGET_CASES):
        inp = bcq_target_inputs(BCQ_SEED_BASE + 300 + i, n, S, N)
        for grouping in (0, 1):
            take(lambda dt, mg: bcq_target_stmt(inp, grouping, dt, mg), ("target",))
    return fig


def measure_normals():
    """worst |float32 NumPy Box-Muller - fp64| over draw_cases() outside the slack elements, and with the slack taken off inside them"""
    w = ws = 0.0
    for n, seed, base, tag in draw_cases():
        a, b, _ = normal_worst(normal_stream(seed, base, n, tag, np.float32), seed, base, n, tag)
        w, ws = max(w, a), max(ws, b)
    return w, ws
