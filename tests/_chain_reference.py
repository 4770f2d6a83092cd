"""fp64 statements of the row-chain launches and of the dW + Adam launch (include/cstr_rl_hip.h, "row-chain kernels" and the
cstr_linear_bwd_weight_adam_sets_f32 block), their magnitude passes, the comparator and the case generators. CPU only.

Every launch has an `*_inputs(...)` generator (float32 numpy arrays from a fixed seed: what the launch reads) and an `*_stmt(inputs,
dtype, mag, mut)` statement of its contract on those inputs:

    dtype  torch.float64 = the reference; torch.float32 = the same statement on stock ATen, which sets the bars
    mag    the magnitude pass: every operand replaced by its absolute value, every subtraction by an addition, the ReLU masks dropped.
           Its result M bounds the sum of absolute terms behind each output element
    mut    one of MUTATIONS: a deliberately wrong statement (tests/test_chain_reference.py shows the comparator rejects each)

Errors are expressed per element in units of 2**-24 * M, the forward-error scale of a float32 dot product: it does not loosen where
terms cancel and does not borrow scale from another element. BARS holds, per output kind, four times the worst figure of the float32
ATen evaluation over the GPU tests' own cases (a different summation order over the same number of operands errs on the same
scale); tests/test_chain_reference.py re-measures the ATen figures and asserts 4 * ATen <= bar <= 64."""
import numpy as np
import torch as th

U = 2.0 ** -24
F64, F32 = th.float64, th.float32
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = 0.91893853320467274178
CAP = 64.0
MARGIN_BAR = 16.0  # >= the bars of h1 and h2: the ReLU-mask margin of the forward cases is searched and asserted at this figure

# 4 x the worst float32 ATen figure over the cases of tests/test_chain_kernels.py (measured figures: that module's docstring)
BARS = {
    "h1": 13.29, "h2": 4.63, "partials": 1.39, "q_out": 10.13, "target_out": 6.90, "gq_out": 7.15, "loss": 1.64, "alpha": 4.40,
    "dz2": 10.79, "dz1": 7.54, "gact_part": 2.26, "dw": 18.19, "db": 3.84,
}
KIND_OF = {"head_part": "partials", "q_part": "partials"}

# the values of `mut`. The issue's tenth mistake, next rows read from the pi rows (next_offset = 0), is no statement's `mut`: it changes which
# rows the head finalisation reads, and tests/test_chain_reference.py builds it from params_f32 / fin_gaussian / q_fwd_stmt directly
MUTATIONS = ("k_tail", "drop_group", "dup_group", "b3_twin", "done_raw", "relu_twin", "tile_shift", "scale_twice", "rows_short")


def groups(width, tiles):
    """column ranges of the column groups: 16 * tiles columns each"""
    step = 16 * tiles
    return [(c, min(c + step, width)) for c in range(0, width, step)]


def _t(a, dtype, mag=False):
    t = th.as_tensor(np.asarray(a)).to(dtype)
    return t.abs() if mag else t


def _relu(z, mag):
    return z if mag else th.relu(z)


def _tail(k, mut):
    return k - 4 if mut == "k_tail" else k


def _shift(a, mut):
    """a tile's 16 columns shifted by one tile: columns 16 .. 31 hold what belongs to columns 0 .. 15"""
    if mut != "tile_shift" or a.shape[-1] <= 16:
        return a
    a = a.clone()
    hi = min(32, a.shape[-1])
    a[..., 16:hi] = a[..., 0:hi - 16].clone()
    return a


def units(got, want, mag):
    """per element |got - want| / (2**-24 * M)"""
    got, want, mag = (np.asarray(v, np.float64) for v in (got, want, mag))
    assert got.shape == want.shape == mag.shape, (got.shape, want.shape, mag.shape)
    assert (mag > 0).all(), "magnitude pass: an output without operands"
    return np.abs(got - want) / (U * mag)


def worst(got, want, mag):
    u = units(got, want, mag)
    i = int(np.argmax(u))
    return float(u.reshape(-1)[i]), i


def bar_of(kind):
    return BARS[KIND_OF.get(kind, kind)]


def accepts(kind, got, want, mag):
    return worst(got, want, mag)[0] <= bar_of(kind)


def np64(d):
    return {k: (v.numpy().astype(np.float64) if isinstance(v, th.Tensor) else v) for k, v in d.items()}


def mask_margin(pre, mag, bar):
    """the smallest |fp64 pre-activation| in units of bar * 2**-24 * M: >= 1 means no float32 evaluation within the bar can flip a mask"""
    pre, mag = np.asarray(pre, np.float64), np.asarray(mag, np.float64)
    return float((np.abs(pre) / (bar * U * mag)).min())


# ---- networks ---------------------------------------------------------------------------------------------------------------------
def _mlp_weights(rng, k, h1, h2, n_out):
    f = lambda *s: rng.standard_normal(s)  # noqa: E731
    return dict(w1=(f(h1, k) / np.sqrt(k)).astype(np.float32), b1=(0.1 * f(h1)).astype(np.float32),
                w2=(f(h2, h1) / np.sqrt(h1)).astype(np.float32), b2=(0.1 * f(h2)).astype(np.float32),
                w3=(f(n_out, h2) / np.sqrt(h2)).astype(np.float32), b3=(0.1 * f(n_out)).astype(np.float32))


def two_layers(x, net, dtype, mag=False, mut=None):
    """z1 = x W1^T + b1, h1 = relu(z1), z2 = h1 W2^T + b2, h2 = relu(z2)"""
    x, w1, b1, w2, b2 = (_t(net[k] if k != "x" else x, dtype, mag) for k in ("x", "w1", "b1", "w2", "b2"))
    z1 = x @ w1.T + b1
    h1 = _shift(_relu(z1, mag), mut)
    k = _tail(h1.shape[1], mut)
    z2 = h1[:, :k] @ w2[:, :k].T + b2
    h2 = _shift(_relu(z2, mag), mut)
    return z1, h1, z2, h2


def head_parts(h2, w3, tiles, dtype, mag=False):
    """[G][rows][n_out]: per column group of h2 the narrow layer's partial sums (no bias)"""
    w3 = _t(w3, dtype, mag)
    return th.stack([h2[:, a:b] @ w3[:, a:b].T for a, b in groups(h2.shape[1], tiles)])


def sum_parts(parts, dtype, mag=False, mut=None):
    """partials added in ascending group order"""
    parts = _t(parts, dtype, mag)
    s = parts[0].clone()
    for p in range(1, parts.shape[0]):
        if mut == "drop_group" and p == parts.shape[0] - 1:
            continue
        s = s + parts[p]
    if mut == "dup_group":
        s = s + parts[-1]
    if mut == "drop_group" and parts.shape[0] == 1:
        s = s * 0
    return s


# ---- actor forward ----------------------------------------------------------------------------------------------------------------
def actor_fwd_inputs(seed, D, A, H1, H2, rows, head_n):
    rng = np.random.default_rng(seed)
    net = _mlp_weights(rng, D, H1, H2, head_n)
    net["w3"] = (0.5 * net["w3"]).astype(np.float32)  # small heads: the sampled actions stay away from tanh's saturation
    return dict(x=rng.uniform(-1, 1, (rows, D)).astype(np.float32), **net)


def actor_fwd_stmt(inp, tiles, dtype=F64, mag=False, mut=None):
    z1, h1, z2, h2 = two_layers(inp["x"], inp, dtype, mag, mut)
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, head_part=head_parts(h2, inp["w3"], tiles, dtype, mag))


# ---- head finalisation (transcendental: compared against the launch's own upstream output) ------------------------------------------
def fin_gaussian(params, eps):
    """cstr_sac_head_fin_t, Gaussian head, fp64: params [B][2A] = (mean | raw log_std) -> action, logp"""
    p, e = np.asarray(params, np.float64), np.asarray(eps, np.float64)
    A = e.shape[1]
    mu, raw = p[:, :A], p[:, A:]
    sd = np.exp(np.clip(raw, LOG_STD_MIN, LOG_STD_MAX))
    u = mu + sd * e
    a = np.tanh(u)
    lp = (-((u - mu) ** 2) / (2 * sd * sd) - np.log(sd) - HALF_LOG_2PI) - np.log(1 - a * a + 1e-6)
    return a, lp.sum(1)


def fin_deterministic(mu, eps=None, sigma=0.0, clip=0.0, smooth=False):
    """deterministic head: tanh; next rows with target smoothing: clamp(tanh(.) + clamp(sigma * eps, -clip, clip), -1, 1)"""
    a = np.tanh(np.asarray(mu, np.float64))
    if smooth:
        a = np.clip(a + np.clip(np.asarray(eps, np.float64) * sigma, -clip, clip), -1.0, 1.0)
    return a


def params_f32(head_part, hb, row0, rows):
    """the documented float32 order: partials of rows [row0, row0 + rows) in ascending group order, then + hb"""
    hp = np.asarray(head_part, np.float32)
    s = hp[0, row0:row0 + rows].copy()
    for g in range(1, hp.shape[0]):
        s = (s + hp[g, row0:row0 + rows]).astype(np.float32)
    return (s + np.asarray(hb, np.float32)).astype(np.float32)


# ---- Q forward ------------------------------------------------------------------------------------------------------------------------
def q_fwd_inputs(seed, D, A, H1, H2, B, n_nets):
    rng = np.random.default_rng(seed)
    nets = [_mlp_weights(rng, D + A, H1, H2, 1) for _ in range(n_nets)]
    xs = [np.concatenate((rng.uniform(-1, 1, (B, D)), np.tanh(rng.standard_normal((B, A)))), 1).astype(np.float32) for _ in range(n_nets)]
    return dict(nets=nets, xs=xs)


def q_fwd_stmt(x, net, tiles, dtype=F64, mag=False, mut=None):
    z1, h1, z2, h2 = two_layers(x, net, dtype, mag, mut)
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, q_part=head_parts(h2, net["w3"], tiles, dtype, mag)[:, :, 0])


# ---- root + Q backward --------------------------------------------------------------------------------------------------------------
def q_bwd_inputs(seed, D, A, H1, H2, B, mode, fwd_tiles, with_alpha=False):
    """what cstr_q_chain_bwd_f32 reads: the forward launch's stored activations and partials (fp64 forward statement rounded to
    float32), the batch's rewards / dones / log-probs and the root's scalars"""
    rng = np.random.default_rng(seed)
    n_diff = 1 if mode == "neg_mean" else 2
    n_all = 4 if mode == "td" else n_diff
    nets = [_mlp_weights(rng, D + A, H1, H2, 1) for _ in range(n_all)]
    x = np.concatenate((rng.uniform(-1, 1, (B, D)), np.tanh(rng.standard_normal((B, A)))), 1).astype(np.float32)
    x_next = np.concatenate((rng.uniform(-1, 1, (B, D)), np.tanh(rng.standard_normal((B, A)))), 1).astype(np.float32)
    h1, h2, q_part = [], [], []
    for g, net in enumerate(nets):
        f = q_fwd_stmt(x if g < 2 else x_next, net, fwd_tiles)
        q_part.append(f["q_part"].numpy().astype(np.float32))
        if g < n_diff:
            h1.append(f["h1"].numpy().astype(np.float32)), h2.append(f["h2"].numpy().astype(np.float32))
    done = (rng.uniform(0, 1, B) < 0.25).astype(np.float32)
    return dict(nets=nets, x=x, act_dim=A, h1=h1, h2=h2, q_part=q_part, mode=mode, n_diff=n_diff, rew=rng.normal(-1.0, 1.0, B).astype(np.float32), done=done,
                next_logp=rng.normal(-1.0, 1.0, B).astype(np.float32), logp=rng.normal(-1.0, 1.0, B).astype(np.float32),
                ent_coef=np.float32(0.37), log_alpha=np.float32(-0.61) if with_alpha else None, target_entropy=-float(A), gamma=0.97,
                scale=0.5 if with_alpha or mode != "td" else 1.0, sac=bool(with_alpha or rng.integers(0, 2)))


def root_stmt(inp, dtype=F64, mag=False, mut=None):
    """cstr_chain_root_t: q = sum of partials + b3; mode td: t = rew + (1 - done) * gamma * (min(q1_t, q2_t) - ent_coef * next_logp),
    gq_k = scale * 2 / B * (q_k - t), loss = scale * (mean (q1 - t)^2 + mean (q2 - t)^2), the alpha part: mean = mean(logp_pi +
    target_entropy), grad = -mean, ent_coef = exp(log_alpha), loss = -(log_alpha * mean); sac_actor: loss = mean(ent_coef * logp -
    min(q1, q2)), gq = -1 / B on the first minimum; neg_mean: loss = -mean(q1), gq = -1 / B"""
    mode, B = inp["mode"], inp["rew"].shape[0]
    sgn = 1.0 if mag else -1.0
    q = []
    for g, parts in enumerate(inp["q_part"]):
        b3 = inp["nets"][0 if (mut == "b3_twin" and g == 1) else g]["b3"]
        q.append(sum_parts(parts, dtype, mag, mut) + _t(b3, dtype, mag))
    out = dict(q_out=th.stack(q[:inp["n_diff"]]))
    scale = inp["scale"] * (inp["scale"] if mut == "scale_twice" else 1.0)
    if mode == "td":
        alpha = inp["log_alpha"] is not None
        la = _t(inp["log_alpha"], dtype) if alpha else None
        ec = th.exp(la) if alpha else _t(inp["ent_coef"], dtype)
        qn = (q[2] + q[3]) if mag else th.minimum(q[2], q[3])
        if inp["sac"]:
            qn = qn + sgn * ec * _t(inp["next_logp"], dtype, mag)
        done = _t(inp["done"], dtype, mag)
        keep = done if mut == "done_raw" else (1.0 + sgn * done)
        t = _t(inp["rew"], dtype, mag) + keep * inp["gamma"] * qn
        d = [q[g] + sgn * t for g in range(2)]
        out["target_out"] = t
        out["gq_out"] = th.stack([scale * 2.0 / B * d[g] for g in range(2)])
        out["loss"] = (scale * ((d[0] * d[0]).sum() / B + (d[1] * d[1]).sum() / B)).reshape(1)
        if alpha:
            lp = _t(inp["logp"], dtype, mag)
            mean = (lp + abs(inp["target_entropy"]) if mag else lp + inp["target_entropy"]).sum() / B
            out["alpha"] = th.stack([mean if mag else -mean, ec, (la.abs() * mean) if mag else -(la * mean)])
    elif mode == "sac_actor":
        ec = _t(inp["ent_coef"], dtype)
        first = q[0] <= q[1]
        inv = th.full_like(q[0], 1.0 / B)
        out["gq_out"] = inv.repeat(2, 1) if mag else th.stack([th.where(first, -inv, 0 * inv), th.where(first, 0 * inv, -inv)])
        qm = (q[0] + q[1]) if mag else th.minimum(q[0], q[1])
        out["loss"] = ((ec * _t(inp["logp"], dtype, mag) + sgn * qm).sum() / B).reshape(1)
    else:
        out["gq_out"] = th.full_like(q[0], (1.0 if mag else -1.0) / B).reshape(1, B)
        out["loss"] = (sgn * q[0].sum() / B).reshape(1)
    return out


def q_bwd_stmt(inp, tiles, dtype=F64, mag=False, mut=None, with_gact=False):
    """root, then per differentiated network dz2 = gq * w3 * relu'(h2), dz1 = (dz2 W2) * relu'(h1) and, for the actor loss, the partial
    action gradients gact_part [net][G][B][A] = dz1[:, group] W1[group, D:]"""
    out = root_stmt(inp, dtype, mag, mut)
    W = inp["nets"][0]["w1"].shape[1]
    dz2s, dz1s, gparts = [], [], []
    for g in range(inp["n_diff"]):
        net = inp["nets"][g]
        w1, w2, w3 = (_t(net[k], dtype, mag) for k in ("w1", "w2", "w3"))
        h2 = th.as_tensor(inp["h2"][g])
        h1 = th.as_tensor(inp["h1"][1 - g if (mut == "relu_twin" and inp["n_diff"] == 2) else g])
        dz2 = out["gq_out"][g].reshape(-1, 1) * w3.reshape(1, -1)
        if not mag:
            dz2 = dz2 * (h2 > 0).to(dtype)
        k = _tail(dz2.shape[1], mut)
        dz1 = dz2[:, :k] @ w2[:k, :]
        if not mag:
            dz1 = dz1 * (h1 > 0).to(dtype)
        dz1 = _shift(dz1, mut)
        dz2s.append(dz2), dz1s.append(dz1)
        if with_gact:
            a0 = W - inp["act_dim"]
            gparts.append(th.stack([dz1[:, a:b] @ w1[a:b, a0:] for a, b in groups(dz1.shape[1], tiles)]))
    out["dz2"], out["dz1"] = th.stack(dz2s), th.stack(dz1s)
    if with_gact:
        out["gact_part"] = th.stack(gparts)
    return out


# ---- actor backward -----------------------------------------------------------------------------------------------------------------
def actor_bwd_inputs(seed, D, A, H1, H2, B, kind, n_nets, n_parts):
    """what cstr_sac_actor_chain_bwd_f32 reads: the critic's action-gradient partials, the head's stored params / eps / actions and
    the actor's stored activations (fp64 forward statement rounded to float32)"""
    rng = np.random.default_rng(seed)
    hn = A if kind == "det" else 2 * A
    fwd = actor_fwd_inputs(seed + 1, D, A, H1, H2, B, hn)
    f = actor_fwd_stmt(fwd, 1)
    params = (f["head_part"].sum(0) + th.as_tensor(fwd["b3"]).double()).numpy().astype(np.float32)
    eps = rng.standard_normal((B, A)).astype(np.float32)
    if kind == "det":
        act = fin_deterministic(params)
    else:
        params[:, A:] -= 1.0  # log_std around -1
        params[0, A] = 2.5    # outside the clamp: the log_std gradient is cut there
        act, _ = fin_gaussian(params, eps)
    x_pi = np.concatenate((fwd["x"], act), 1).astype(np.float32)
    gact = (rng.standard_normal((n_nets, n_parts, B, A)) / (B * np.sqrt(n_parts))).astype(np.float32)
    return dict(net=fwd, kind=kind, gact_part=gact, ent_coef=np.float32(0.37), x_pi=x_pi, params=params, eps=eps, act_dim=A,
                a_h1=f["h1"].numpy().astype(np.float32), a_h2=f["h2"].numpy().astype(np.float32))


def actor_bwd_stmt(inp, dtype=F64, mag=False, mut=None):
    """d(loss)/d(action) = sum of gact_part over (network, group); Gaussian: gl = ent_coef / B, s = exp(clamp(raw)), g_mean = ga * (1 -
    a^2) + gl * 2 a (1 - a^2) / (1 - a^2 + 1e-6), g_log_std = g_mean * eps * s - gl inside the clamp, else 0; deterministic: g = ga * (1 -
    a^2); dz2 = (g_params hw) * relu'(a_h2); dz1 = (dz2 W2) * relu'(a_h1)"""
    A, net = inp["act_dim"], inp["net"]
    B = inp["x_pi"].shape[0]
    sgn = 1.0 if mag else -1.0
    gp = inp["gact_part"]
    ga = sum_parts(gp.reshape(-1, B, A), dtype, mag, mut)
    a = _t(inp["x_pi"][:, -A:], dtype, mag)
    one_m = 1.0 + sgn * a * a
    if inp["kind"] == "det":
        g_params = ga * one_m
    else:
        raw, eps = _t(inp["params"][:, A:], dtype), _t(inp["eps"], dtype, mag)
        gl = float(inp["ent_coef"]) / B
        s = th.exp(th.clamp(raw, LOG_STD_MIN, LOG_STD_MAX))
        g_mu = ga * one_m + gl * (2.0 * a * one_m / (one_m + 1e-6))
        inside = ((raw >= LOG_STD_MIN) & (raw <= LOG_STD_MAX)).to(dtype)
        g_ls = (g_mu * eps * s + sgn * gl) * (1.0 if mag else inside)
        g_params = th.cat((g_mu, g_ls), 1)
    hw, w2 = _t(net["w3"], dtype, mag), _t(net["w2"], dtype, mag)
    dz2 = g_params @ hw
    if not mag:
        dz2 = dz2 * (th.as_tensor(inp["a_h2"]) > 0).to(dtype)
    k = _tail(dz2.shape[1], mut)
    dz1 = dz2[:, :k] @ w2[:k, :]
    if not mag:
        dz1 = dz1 * (th.as_tensor(inp["a_h1"]) > 0).to(dtype)
    return dict(g_params=g_params, dz2=dz2, dz1=_shift(dz1, mut))


# ---- dW, db and the Adam step -------------------------------------------------------------------------------------------------------
def wgrad_inputs(seed, M, N, K, ldx=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, ldx or K)).astype(np.float32)
    return dict(dz=(rng.standard_normal((M, N)) / M).astype(np.float32), x=x, k=K, w=(rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32),
                b=(0.1 * rng.standard_normal(N)).astype(np.float32), w_m=(1e-3 * rng.standard_normal((N, K))).astype(np.float32),
                w_v=(1e-5 * rng.uniform(0, 1, (N, K))).astype(np.float32), b_m=(1e-3 * rng.standard_normal(N)).astype(np.float32),
                b_v=(1e-5 * rng.uniform(0, 1, N)).astype(np.float32))


def wgrad_stmt(inp, dtype=F64, mag=False, mut=None):
    """dw[n][k] = sum_m dz[m][n] * x[m][k], db[n] = sum_m dz[m][n]"""
    dz, x = _t(inp["dz"], dtype, mag), _t(inp["x"][:, :inp["k"]], dtype, mag)
    m = dz.shape[0] - (16 if mut == "rows_short" else 0)
    return dict(dw=dz[:m].T @ x[:m], db=dz[:m].sum(0))


def adam_param_f32(p, m, v, step, lr, betas, eps):
    """the parameter update of torch.optim.Adam in float32 on GIVEN new moments: oracle/cstr_oracle.c adam_f32_cpu's last two lines with
    its rounding points (the oracle takes the old moments only; tests/test_chain_reference.py ties the two bit for bit)"""
    f32 = np.float32
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    step_size, bc2_sqrt = f32(lr / bc1), f32(bc2 ** 0.5)
    denom = (np.sqrt(np.asarray(v, f32)) / bc2_sqrt + f32(eps)).astype(f32)
    return (np.asarray(p, f32) + ((-step_size) * np.asarray(m, f32)).astype(f32) / denom).astype(f32)


def polyak_f32(p, t, tau):
    """target = fma(tau, p, target * (1 - tau)) in float32 (the product p * tau is exact in fp64; the fp64 sum is rounded once more, to
    float32: the two roundings differ from one only where the fp64 sum lands on a float32 tie, about 2**-29 per element)"""
    tf, om = np.float32(tau), np.float32(1.0 - tau)
    return (np.asarray(p, np.float64) * np.float64(tf) + (np.asarray(t, np.float32) * om).astype(np.float64)).astype(np.float32)


def swizzle(w):
    """cstr_policy_swizzle_f32's layout: out[((tile * ceil(k/16) + chunk) * 64 + lane) * 4 + e] = w[16 tile + (lane & 15)][16 chunk + 4 (lane >> 4) + e]"""
    n, k = w.shape
    nt, kc = -(-n // 16), -(-k // 16)
    pad = np.zeros((16 * nt, 16 * kc), np.float32)
    pad[:n, :k] = w
    return pad.reshape(nt, 16, kc, 4, 4).transpose(0, 2, 3, 1, 4).reshape(-1).copy()


def find_seed(base, build, pre_of, bar, tries=400):
    """the first seed >= base at which no fp64 pre-activation of the case lies within bar * 2**-24 * M of zero"""
    for seed in range(base, base + tries):
        inp = build(seed)
        if min(mask_margin(p, m, bar) for p, m in pre_of(inp)) >= 1.0:
            return seed, inp
    raise AssertionError("no seed with a mask margin")


# ---- the GPU tests' cases (tests/test_chain_kernels.py), shared with the CPU measurement of the bars ----------------------------------
# widths: (16,16) one chunk, waves with an empty split-K share; (20,36) not multiples of 16; (72,40); (256,256) and (400,300) the
# exact-width instantiations; (456,512) the widest the forward chains admit. Forward tiles = 4 at H1 = 400 / 456: the per-wave share of 32.
PAIR, NEXT, OBS = 0, 1, 2
# (D, A, H1, H2, B, tiles, rows_mode, head, source)
ACTOR_FWD_CASES = [
    (4, 2, 16, 16, 16, 1, PAIR, "gauss", "packed"), (4, 2, 16, 16, 16, 4, PAIR, "gauss", "packed"), (4, 2, 20, 36, 48, 2, PAIR, "gauss", "ring"),
    (8, 2, 20, 36, 1024, 1, NEXT, "det", "packed"), (8, 4, 72, 40, 48, 2, OBS, "det", "packed"), (8, 4, 72, 40, 16, 4, PAIR, "gauss", "draw"),
    (4, 2, 256, 256, 48, 1, PAIR, "gauss", "ring"), (4, 2, 256, 256, 16, 2, PAIR, "gauss", "packed"), (8, 2, 256, 256, 16, 4, PAIR, "gauss", "packed"),
    (8, 4, 256, 256, 16, 2, OBS, "det", "packed"), (4, 2, 400, 300, 48, 2, NEXT, "det", "ring"), (4, 2, 400, 300, 16, 1, OBS, "det", "packed"),
    (8, 4, 400, 300, 16, 4, NEXT, "det", "packed"), (8, 4, 400, 300, 16, 2, OBS, "det", "packed"), (4, 2, 456, 512, 16, 4, PAIR, "gauss", "packed"),
    (8, 2, 456, 512, 48, 2, PAIR, "gauss", "packed"), (8, 4, 456, 512, 16, 1, NEXT, "det", "ring"),
]
# (D, A, H1, H2, B, tiles, configuration, partials of the pending actor head)
Q_FWD_CASES = [
    (4, 2, 16, 16, 16, 1, "plain1", 0), (4, 2, 16, 16, 16, 4, "sac4", 1), (4, 2, 20, 36, 48, 2, "sac4", 3), (8, 2, 20, 36, 1024, 1, "plain2", 0),
    (8, 2, 20, 36, 16, 2, "td4", 2), (8, 4, 72, 40, 48, 4, "sac4", 9), (8, 4, 72, 40, 16, 1, "pi1", 3), (8, 4, 72, 40, 16, 2, "plain16", 0),
    (4, 2, 256, 256, 48, 2, "sac4", 8), (8, 2, 256, 256, 16, 4, "sac4", 4), (4, 2, 256, 256, 16, 1, "nostore", 2), (4, 2, 400, 300, 48, 2, "td4", 10),
    (4, 2, 400, 300, 16, 1, "pi1", 19), (8, 4, 400, 300, 16, 4, "td4", 5), (8, 4, 400, 300, 16, 2, "plain2", 0), (4, 2, 456, 512, 16, 4, "sac4", 17),
    (8, 4, 456, 512, 48, 2, "td4", 32), (8, 2, 456, 512, 16, 1, "plain1", 0),
]
# (D, A, H1, H2, B, tiles, mode, alpha part, tiles of the forward launch that wrote the partials)
Q_BWD_CASES = [
    (4, 2, 16, 16, 16, 1, "td", True, 1), (4, 2, 16, 16, 16, 4, "sac_actor", False, 1), (4, 2, 20, 36, 48, 2, "td", False, 1),
    (8, 2, 20, 36, 1024, 1, "td", True, 2), (8, 2, 20, 36, 16, 4, "neg_mean", False, 1), (8, 4, 72, 40, 48, 2, "sac_actor", False, 1),
    (8, 4, 72, 40, 16, 1, "neg_mean", False, 2), (8, 4, 72, 40, 16, 4, "td", True, 4), (4, 2, 256, 256, 48, 2, "td", True, 2),
    (4, 2, 256, 256, 16, 1, "sac_actor", False, 1), (8, 2, 256, 256, 16, 4, "td", False, 4), (8, 4, 256, 256, 16, 2, "neg_mean", False, 2),
    (4, 2, 400, 300, 48, 2, "td", False, 2), (4, 2, 400, 300, 16, 1, "neg_mean", False, 1), (8, 4, 400, 300, 16, 2, "sac_actor", False, 4),
    (4, 2, 456, 512, 16, 2, "td", True, 1), (8, 4, 456, 512, 48, 1, "sac_actor", False, 2), (8, 2, 456, 512, 16, 2, "neg_mean", False, 4),
]
# (D, A, H1, H2, B, tiles, head, networks, column groups of the critic's partial action gradients)
ACTOR_BWD_CASES = [
    (4, 2, 16, 16, 16, 1, "gauss", 2, 1), (4, 2, 16, 16, 16, 4, "det", 1, 1), (4, 2, 20, 36, 48, 2, "gauss", 2, 2), (8, 2, 20, 36, 1024, 1, "det", 1, 2),
    (8, 4, 72, 40, 48, 4, "gauss", 2, 5), (8, 4, 72, 40, 16, 1, "det", 1, 3), (4, 2, 256, 256, 48, 1, "gauss", 2, 8), (8, 2, 256, 256, 16, 2, "gauss", 2, 16),
    (8, 4, 256, 256, 16, 4, "det", 1, 4), (4, 2, 400, 300, 48, 2, "det", 1, 13), (8, 4, 400, 300, 16, 1, "det", 1, 25), (8, 4, 400, 300, 16, 2, "gauss", 2, 7),
    (4, 2, 456, 512, 16, 2, "gauss", 2, 29), (8, 4, 456, 512, 48, 1, "det", 1, 15),
]
WGRAD_SHAPES = [(256, 6), (20, 36), (1, 40), (300, 400)]
WGRAD_ROWS = [48, 256]
SEED_BASE = 20261018


def rows_of(B, rows_mode):
    return 2 * B if rows_mode == PAIR else B


def actor_fwd_case(i):
    D, A, H1, H2, B, tiles, rows_mode, head, _ = ACTOR_FWD_CASES[i]
    hn = A if head == "det" else 2 * A
    bar = MARGIN_BAR
    return find_seed(SEED_BASE + 1000 * i, lambda s: actor_fwd_inputs(s, D, A, H1, H2, rows_of(B, rows_mode), hn), lambda inp: _pre(actor_fwd_stmt(inp, tiles), actor_fwd_stmt(inp, tiles, mag=True)), bar)[1]


def _pre(ref, mag):
    return [(ref["z1"].numpy(), mag["z1"].numpy()), (ref["z2"].numpy(), mag["z2"].numpy())]


Q_FWD_NETS = {"plain1": 1, "plain2": 2, "sac4": 4, "td4": 4, "pi1": 1, "plain16": 16, "nostore": 2}
SIGMA, CLIP = 0.5, 0.3  # target smoothing of the deterministic head's next rows: both clamps bind on part of every batch


def q_fwd_case(i):
    """the networks and their input rows; with a pending actor head (n_parts > 0) also its partials, bias and noise, and the action
    columns of the networks that read finalised actions are set to the fp64 finalisation of those partials (the launch's own differ
    from it within the head's tolerance; the GPU test then states the matrix stages on the launch's own stored actions)"""
    D, A, H1, H2, B, tiles, cfg, n_parts = Q_FWD_CASES[i]
    n = Q_FWD_NETS[cfg]

    def build(seed):
        inp = q_fwd_inputs(seed, D, A, H1, H2, B, n)
        inp["cfg"] = cfg
        if n_parts:
            rng = np.random.default_rng(seed + 7)
            gauss = cfg in ("sac4", "nostore")
            rows, hn = (2 * B, 2 * A) if gauss else (B, A)
            scale = 0.6 if gauss else 1.2  # the deterministic head's tanh reaches its flanks: the outer clamp of the smoothing binds
            inp["head_part"] = (rng.standard_normal((n_parts, rows, hn)) * (scale / np.sqrt(n_parts))).astype(np.float32)
            inp["hb"] = (0.1 * rng.standard_normal(hn)).astype(np.float32)
            inp["eps"] = rng.standard_normal((rows, A)).astype(np.float32)
            inp["next_offset"] = B if gauss else 0
            if gauss:
                inp["hb"][A:] -= 1.0  # log_std around -1
                a_next, _ = fin_gaussian(params_f32(inp["head_part"], inp["hb"], B, B), inp["eps"][B:])
            elif cfg == "td4":
                a_next = fin_deterministic(params_f32(inp["head_part"], inp["hb"], 0, B), inp["eps"], SIGMA, CLIP, smooth=True)
            else:
                a_next = fin_deterministic(params_f32(inp["head_part"], inp["hb"], 0, B))
            xd, xn = inp["xs"][0], inp["xs"][-1].copy()
            xn[:, D:] = a_next
            inp["xs"] = {"sac4": [xd, xd, xn, xn], "td4": [xd, xd, xn, xn], "nostore": [xd, xn], "pi1": [xn]}[cfg]
        return inp

    def pre(inp):
        out = []
        for x, net in zip(inp["xs"], inp["nets"]):
            out += _pre(q_fwd_stmt(x, net, tiles), q_fwd_stmt(x, net, tiles, mag=True))
        return out
    return find_seed(SEED_BASE + 100000 + 1000 * i, build, pre, MARGIN_BAR)[1]


def q_bwd_case(i):
    D, A, H1, H2, B, tiles, mode, alpha, ft = Q_BWD_CASES[i]
    return q_bwd_inputs(SEED_BASE + 200000 + 1000 * i, D, A, H1, H2, B, mode, ft, alpha)


def actor_bwd_case(i):
    D, A, H1, H2, B, tiles, head, n_nets, n_parts = ACTOR_BWD_CASES[i]
    return actor_bwd_inputs(SEED_BASE + 300000 + 1000 * i, D, A, H1, H2, B, head, n_nets, n_parts)


def wgrad_case(M, j):
    N, K = WGRAD_SHAPES[j]
    return wgrad_inputs(SEED_BASE + 400000 + 1000 * j + M, M, N, K, ldx=K + 2 if j == 0 else None)


def measure_aten():
    """worst float32-ATen figure per output kind over the cases above, in units of 2**-24 * M"""
    fig = {}

    def take(stmt, kinds):
        ref, f32, mag = np64(stmt(F64, False)), np64(stmt(F32, False)), np64(stmt(F64, True))
        for k in kinds:
            if k in ref:
                kk = KIND_OF.get(k, k)
                fig[kk] = max(fig.get(kk, 0.0), worst(f32[k], ref[k], mag[k])[0])
    for i, c in enumerate(ACTOR_FWD_CASES):
        inp = actor_fwd_case(i)
        take(lambda dt, mg: actor_fwd_stmt(inp, c[5], dt, mg), ("h1", "h2", "head_part"))
    for i, c in enumerate(Q_FWD_CASES):
        inp = q_fwd_case(i)
        for x, net in zip(inp["xs"], inp["nets"]):
            take(lambda dt, mg: q_fwd_stmt(x, net, c[5], dt, mg), ("h1", "h2", "q_part"))
    for i, c in enumerate(Q_BWD_CASES):
        inp = q_bwd_case(i)
        take(lambda dt, mg: q_bwd_stmt(inp, c[5], dt, mg, with_gact=c[6] != "td"), ("q_out", "target_out", "gq_out", "loss", "alpha", "dz2", "dz1", "gact_part"))
    for i, c in enumerate(ACTOR_BWD_CASES):
        inp = actor_bwd_case(i)
        take(lambda dt, mg: actor_bwd_stmt(inp, dt, mg), ("dz2", "dz1"))
    for M in WGRAD_ROWS:
        for j in range(len(WGRAD_SHAPES)):
            inp = wgrad_case(M, j)
            take(lambda dt, mg: wgrad_stmt(inp, dt, mg), ("dw", "db"))
    return fig
