"""fp64 statements of TRPO's train() (core/trpo/trpo.py, csrc/cstr_trpo.hip), their magnitude passes, the comparators, the case lists
and the seeded input generators. CPU only.

A statement takes the float32 arrays its launch reads and

    dtype  torch.float64 = the reference; torch.float32 = the same statement on stock ATen, which sets the bars
    mag    the magnitude pass (_rowkernel_reference's convention): every additive term replaced by its absolute value, every
           subtraction by an addition, the masks dropped. Its result M bounds the sum of absolute terms behind each output element

An actor is dict(ws=[(W, b), ...], log_std or None, act, head); head = ("gauss", A) | ("cat", n) | ("mcat", (k0, k1)). Vectors over
its parameters are flat in `policy.named_parameters()` order: log_std first (where there is one), then W1, b1, W2, b2, W3, b3.

Two Fisher-vector products: `fvp_double_backward` is the published form (autograd through the gradient of the mean KL);
`fvp_fisher` is the explicit form the kernels take -- tangent layers, the head's metric, the per-layer backward -- written as
expressions so that it has a magnitude pass. tests/test_trpo_reference.py ties the two together at rtol 1e-10.

Errors of the float32 MFMA kinds (tangent layer, head metric, whole product) are per element in units of 2**-24 * M
(_chain_reference.units); BARS holds four times the worst float32 ATen figure over the cases below, re-measured and asserted in
tests/test_trpo_reference.py. The launches that compute in float64 and store float32 (objective, KL, CG step, apply step, value
loss) take the project's kernel-against-fp64 bar `close64`: |got - want| <= 2e-6 |want| + 1e-7 max |want|."""
import numpy as np
import torch as th

from _chain_reference import CAP, F32, F64, U, mask_margin, units  # noqa: F401  (shared, not forked)

# 4 x the worst float32 ATen figure over the cases of this module (measured figures: the docstring of tests/test_trpo_abi.py)
BARS = {"tangent": 16.62, "head": 38.51, "fvp": 4.88}
TANH_MAX = 1.0 - 2.0 ** -12  # tanh outputs stay below it: 1 - y^2 keeps at least half its bits
ACTS = ("none", "relu", "tanh")
ACT_ID = {"none": 0, "relu": 1, "tanh": 2}
TANGENT_ROWS = (1, 3, 16, 17, 65, 257)
TANGENT_KN = ((4, 64), (64, 64), (64, 2), (64, 9), (64, 8), (64, 25), (12, 20), (128, 64), (136, 20))
# (12, 20): net_arch [12, 20], no multiple of 16; K = 128 and 136: a second trip of the kernel's 64-wide K loop, whole and with a tail
HEADS = (("gauss", 2), ("cat", 9), ("mcat", (3, 5)))
FLAT_ROWS = (2, 3, 65, 255, 257, 1025, 16384 + 77)  # the last: beyond one pass of the objective launch's grid (64 x 256 lanes)
CG_LENGTHS = (1, 63, 65, 1023, 1025, 4612)


def _t(a, dtype, mag=False):
    t = a.to(dtype) if isinstance(a, th.Tensor) else th.as_tensor(np.asarray(a)).to(dtype)
    return t.abs() if mag else t


def close64(got, want):
    """the kernel-against-fp64 bar: (worst |got - want| / (2e-6 |want| + 1e-7 max |want|), holds)"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    bar = 2e-6 * np.abs(want) + 1e-7 * np.abs(want).max()
    if not np.isfinite(got).all():
        return float("inf"), False
    w = float((np.abs(got - want) / np.maximum(bar, 1e-300)).max()) if want.size else 0.0
    return w, bool((np.abs(got - want) <= bar).all())


def worst(got, want, mag):
    u = units(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(mag, np.float64))
    return float(u.max())


# ---- actors and batches ----------------------------------------------------------------------------------------------------------------
def head_width(head):
    kind, k = head
    return k if kind != "mcat" else sum(k)


def make_actor(seed, head, hidden=(64, 64), obs_dim=4, act="tanh", scale=1.0):
    rng = np.random.default_rng(seed)
    dims = (obs_dim, *hidden, head_width(head))
    ws = [((scale * rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32))
          for k, n in zip(dims[:-1], dims[1:])]
    log_std = (0.3 * rng.standard_normal(head[1])).astype(np.float32) if head[0] == "gauss" else None
    return dict(ws=ws, log_std=log_std, act=act, head=head)


def flat_of(actor):
    parts = [] if actor["log_std"] is None else [actor["log_std"].reshape(-1)]
    for w, b in actor["ws"]:
        parts += [w.reshape(-1), b.reshape(-1)]
    return np.concatenate(parts).astype(np.float32)


def split(actor, theta):
    """(log_std, [(W, b), ...]) views of a flat torch vector"""
    at, log_std = 0, None
    if actor["log_std"] is not None:
        a = actor["log_std"].size
        log_std, at = theta[:a], a
    ws = []
    for w, b in actor["ws"]:
        ws.append((theta[at:at + w.size].reshape(w.shape), theta[at + w.size:at + w.size + b.size]))
        at += w.size + b.size
    assert at == theta.numel()
    return log_std, ws


def _act(z, act):
    return th.tanh(z) if act == "tanh" else (th.relu(z) if act == "relu" else z)


def _dact(y, act, mag=False):
    if act == "tanh":
        return 1.0 + y * y if mag else 1.0 - y * y
    if act == "relu":
        return th.ones_like(y) if mag else (y > 0).to(y.dtype)
    return th.ones_like(y)


def forward(actor, theta, obs, with_pre=False):
    """[obs, y1, y2, dist] at theta (the last layer has no activation)"""
    _, ws = split(actor, theta)
    acts, pres = [_t(obs, theta.dtype)], []
    for i, (w, b) in enumerate(ws):
        pre = acts[-1] @ w.T + b
        pres.append(pre)
        acts.append(_act(pre, actor["act"]) if i < len(ws) - 1 else pre)
    return (acts, pres) if with_pre else acts


def _blocks(head):
    kind, k = head
    return [k] if kind == "cat" else list(k)


def logp_kl(head, dist, log_std, old_dist, old_log_std, actions):
    """(log_prob [R], KL(new || old) [R]) in the dtype of dist; actions float rows as the buffer stores them"""
    dt = dist.dtype
    actions = _t(actions, dt)
    if head[0] == "gauss":
        sig, sig0 = th.exp(log_std), th.exp(old_log_std)
        logp = (-((actions - dist) ** 2) / (2 * sig * sig) - th.log(sig) - 0.5 * np.log(2 * np.pi)).sum(1)
        vr = (sig / sig0) ** 2
        kl = (0.5 * (vr + ((dist - old_dist) / sig0) ** 2 - 1 - th.log(vr))).sum(1)
        return logp, kl
    actions = actions.reshape(dist.shape[0], -1).long()
    logp, kl, at = 0, 0, 0
    for j, k in enumerate(_blocks(head)):
        lp = th.log_softmax(dist[:, at:at + k], 1)
        lq = th.log_softmax(old_dist[:, at:at + k], 1)
        logp = logp + lp.gather(1, actions[:, j:j + 1]).squeeze(1)
        kl = kl + (lp.exp() * (lp - lq)).sum(1)
        at += k
    return logp, kl


def normalize(adv, dtype=F64):
    adv = _t(adv, dtype)
    return (adv - adv.mean()) / (adv.std() + 1e-8)


def objective_kl(actor, theta, batch, old_dist, old_log_std, normalize_advantage=True, dist=None):
    """(objective, kl) of step 3 at theta; old = the actor's output at theta0, held constant"""
    dt = theta.dtype
    log_std, _ = split(actor, theta)
    dist = forward(actor, theta, batch["obs"])[-1] if dist is None else dist
    logp, kl = logp_kl(actor["head"], dist, log_std, old_dist, old_log_std, batch["actions"])
    adv = normalize(batch["adv"], dt) if normalize_advantage else _t(batch["adv"], dt)
    ratio = th.exp(logp - _t(batch["old_log_prob"], dt))
    return (adv * ratio).mean(), kl.mean()


def make_batch(seed, actor, rows, obs_dim=4, drift=0.05):
    """a rollout-like batch: actions drawn near the policy, old_log_prob = the log-prob at theta0 plus a small drift (so the ratio is
    not 1 and the objective has a scale), advantages with a mean and a spread"""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (rows, obs_dim)).astype(np.float32)
    theta = th.as_tensor(flat_of(actor)).to(F64)
    dist = forward(actor, theta, obs)[-1]
    head = actor["head"]
    if head[0] == "gauss":
        sig = np.exp(actor["log_std"].astype(np.float64))
        actions = (dist.numpy() + sig * rng.standard_normal(dist.shape)).astype(np.float32)
    else:
        actions = np.stack([rng.integers(0, k, rows) for k in _blocks(head)], 1).astype(np.float32)
        if head[0] == "cat":
            actions = actions.reshape(rows)
    ls = None if actor["log_std"] is None else theta[:actor["log_std"].size]
    logp, _ = logp_kl(head, dist, ls, dist, ls, actions)
    old_log_prob = (logp.numpy() + drift * rng.standard_normal(rows)).astype(np.float32)
    adv = (0.7 + 1.3 * rng.standard_normal(rows)).astype(np.float32)
    returns = rng.standard_normal(rows).astype(np.float32)
    return dict(obs=obs, actions=actions, old_log_prob=old_log_prob, adv=adv, returns=returns)


def old_of(actor, theta0, obs):
    with th.no_grad():
        log_std, _ = split(actor, theta0)
        return forward(actor, theta0, obs)[-1].clone(), (None if log_std is None else log_std.clone())


def objective_grad(actor, theta0, batch, normalize_advantage=True):
    """(objective, kl, g = d objective / d theta) at theta0 by fp64 autograd"""
    th0 = theta0.detach().clone().requires_grad_(True)
    old_dist, old_ls = old_of(actor, th0.detach(), batch["obs"])
    obj, kl = objective_kl(actor, th0, batch, old_dist, old_ls, normalize_advantage)
    (g,) = th.autograd.grad(obj, th0)
    return obj.detach(), kl.detach(), g


# ---- Fisher-vector products ------------------------------------------------------------------------------------------------------------
def fvp_double_backward(actor, theta0, obs, v, damping):
    """the published form: d/d theta ((d kl / d theta) . v) + damping v, genuine double backward through autograd on the mean KL"""
    th0 = theta0.detach().clone().requires_grad_(True)
    old_dist, old_ls = old_of(actor, th0.detach(), obs)
    log_std, _ = split(actor, th0)
    dist = forward(actor, th0, obs)[-1]
    kind, k = actor["head"]
    batch_actions = np.zeros((obs.shape[0], k if kind == "gauss" else (1 if kind == "cat" else 2)), np.float32)  # the KL does not read them
    _, kl = logp_kl(actor["head"], dist, log_std, old_dist, old_ls, batch_actions)
    (gk,) = th.autograd.grad(kl.mean(), th0, create_graph=True)
    (hv,) = th.autograd.grad(gk @ v, th0)
    return hv + damping * v


def tangent_layer(x, x_dot, w, w_dot, b_dot, y, act, dtype=F64, mag=False):
    """z_dot = f'(y) * (x w_dot^T + x_dot w^T + b_dot); x_dot None: the first layer"""
    x, w_dot, b_dot = _t(x, dtype, mag), _t(w_dot, dtype, mag), _t(b_dot, dtype, mag)
    z = x @ w_dot.T + b_dot
    if x_dot is not None:
        z = z + _t(x_dot, dtype, mag) @ _t(w, dtype, mag).T
    return z if act == "none" else z * _dact(_t(y, dtype), act, mag)


def head_metric(head, dist_dot, dist, log_std, rows, dtype=F64, mag=False):
    """the Fisher metric of the head times the tangent, over R: what the backward takes as d / d (mean | logits)"""
    dd = _t(dist_dot, dtype, mag)
    if head[0] == "gauss":
        return dd * th.exp(-2.0 * _t(log_std, dtype)) / rows
    z = _t(dist, dtype)
    out, at = [], 0
    for k in _blocks(head):
        p = th.softmax(z[:, at:at + k], 1)
        pz = p * dd[:, at:at + k]
        dot = pz.sum(1, keepdim=True)
        out.append((pz + p * dot if mag else pz - p * dot) / rows)
        at += k
    return th.cat(out, 1)


def backward_layers(actor, ws, acts, up, dtype=F64, mag=False):
    """the per-layer backward from `up` = d / d (mean | logits): [(dW, db), ...] in layer order"""
    gz, out = _t(up, dtype, mag), []
    for i in range(len(ws) - 1, -1, -1):
        w, x = _t(ws[i][0], dtype, mag), _t(acts[i], dtype, mag)
        out.append((gz.T @ x, gz.sum(0)))
        if i > 0:
            gz = (gz @ w) * _dact(_t(acts[i], dtype), actor["act"], mag)
    return out[::-1]


def fvp_fisher(actor, theta0, acts, v, damping, dtype=F64, mag=False, parts=False):
    """Fvp(v) = (1/R) sum_r J_r^T M_r J_r v + damping v from the activations at theta0 (float32 arrays [obs, y1, y2, dist]): tangent
    pass, head metric, backward. Flat order of the result: as v."""
    log_std, ws = split(actor, _t(theta0, dtype))
    v_ls, vs = split(actor, _t(v, dtype))
    rows = acts[0].shape[0]
    x_dot, tans = None, []
    for i, ((w, _), (wd, bd)) in enumerate(zip(ws, vs)):
        act = actor["act"] if i < len(ws) - 1 else "none"
        x_dot = tangent_layer(acts[i], x_dot, w, wd, bd, acts[i + 1], act, dtype, mag)
        tans.append(x_dot)
    up = head_metric(actor["head"], x_dot, acts[-1], log_std, rows, dtype, mag)
    grads = backward_layers(actor, ws, acts, up, dtype, mag)
    flat = [] if log_std is None else [2.0 * (v_ls.abs() if mag else v_ls)]
    for dw, db in grads:
        flat += [dw.reshape(-1), db.reshape(-1)]
    vv = _t(v, dtype, mag)
    out = th.cat(flat) + damping * vv
    return (out, tans, up) if parts else out


# ---- conjugate gradient, line search, critic -------------------------------------------------------------------------------------------
def cg_solve(fvp, g, x0, max_iter, tol=1e-10):
    """conjugate_gradient_solver of step 6, literally -> (x, [rr after the init and after every completed iteration], iterations run)"""
    x = x0.clone()
    r = g - fvp(x)
    p = r.clone()
    rr = r @ r
    hist, iters = [float(rr)], 0
    if rr < tol:
        return x, hist, iters
    for i in range(max_iter):
        ap = fvp(p)
        alpha = rr / (p @ ap)
        x = x + alpha * p
        iters += 1
        if i == max_iter - 1:
            return x, hist, iters
        r = r - alpha * ap
        new_rr = r @ r
        if new_rr < tol:
            break
        beta = new_rr / rr
        rr = new_rr
        hist.append(float(rr))
        p = r + beta * p
    return x, hist, iters


def cg_step_stmt(x, r, p, ap, rr, damping, last, tol=1e-10):
    """one CG launch on float32 vectors in fp64: ap is F p WITHOUT damping -> dict(x, r, p, rr, alpha, beta, done)"""
    x, r, p, ap = (_t(a, F64) for a in (x, r, p, ap))
    apd = ap + damping * p
    alpha = rr / float(p @ apd)
    x = x + alpha * p
    if last:
        return dict(x=x, r=r, p=p, rr=rr, alpha=alpha, done=True)
    r = r - alpha * apd
    new_rr = float(r @ r)
    if new_rr < tol:
        return dict(x=x, r=r, p=p, rr=rr, alpha=alpha, done=True)
    beta = new_rr / rr
    return dict(x=x, r=r, p=r + beta * p, rr=new_rr, alpha=alpha, beta=beta, done=False)


def line_search(evaluate, theta0, s, step, objective0, target_kl, shrink, max_iter):
    """step 8 -> (theta, accepted coefficient or None, [(coeff, objective', kl', accepted)]); evaluate(theta) -> (objective', kl')"""
    coeff, recs = 1.0, []
    for _ in range(max_iter):
        theta = theta0 + coeff * step * s
        obj, kl = evaluate(theta)
        ok = bool(kl < target_kl and obj > objective0)
        recs.append((coeff, float(obj), float(kl), ok))
        if ok:
            return theta, coeff, recs
        coeff *= shrink
    return theta0.clone(), None, recs


def ls_margins(recs, objective0, target_kl):
    """per iteration the two conditions' margins (|kl' - target_kl|, |objective' - objective|) over the close64 bar of the quantity"""
    out = []
    for _, obj, kl, _ in recs:
        out.append(min(abs(kl - target_kl) / (2.1e-6 * max(abs(kl), abs(target_kl))), abs(obj - objective0) / (2.1e-6 * max(abs(obj), abs(objective0)))))
    return out


def mlp_value(vws, obs, act):
    x = obs
    for i, (w, b) in enumerate(vws):
        x = x @ w.T + b
        if i < len(vws) - 1:
            x = _act(x, act)
    return x.reshape(-1)


def critic_pass(vws, act, minibatches, lr, eps=1e-5, betas=(0.9, 0.999), dtype=F64):
    """step 9: per minibatch (obs, returns) mse(returns, V(obs)), backward, one Adam step (torch.optim.Adam's statement, moments from
    zero) -> (the new [(W, b)], [value_loss per minibatch])"""
    params = [_t(a, dtype).clone().requires_grad_(True) for wb in vws for a in wb]
    m, v = [th.zeros_like(p) for p in params], [th.zeros_like(p) for p in params]
    losses = []
    for t, (obs, ret) in enumerate(minibatches, 1):
        ws = [(params[2 * i], params[2 * i + 1]) for i in range(len(vws))]
        loss = ((_t(ret, dtype) - mlp_value(ws, _t(obs, dtype), act)) ** 2).mean()
        grads = th.autograd.grad(loss, params)
        losses.append(float(loss.detach()))
        with th.no_grad():
            for p, g, mi, vi in zip(params, grads, m, v):
                mi.mul_(betas[0]).add_(g, alpha=1 - betas[0])
                vi.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
                denom = (vi.sqrt() / np.sqrt(1 - betas[1] ** t)) + eps
                p.addcdiv_(mi, denom, value=-lr / (1 - betas[0] ** t))
    return [(params[2 * i].detach(), params[2 * i + 1].detach()) for i in range(len(vws))], losses


# ---- cases and the float32 ATen figures that set the bars -------------------------------------------------------------------------------
def tangent_case(rows, k, n, act, with_xdot, seed0=0):
    """one layer's operands; the seed is searched until the input conditions hold: no ReLU pre-activation within the bar of zero, tanh
    outputs below TANH_MAX"""
    for seed in range(seed0, seed0 + 200):
        rng = np.random.default_rng(1000003 * seed + 7919 * rows + 131 * k + n)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
        x, w, b = f(rows, k), (f(n, k) / np.sqrt(k)).astype(np.float32), (0.1 * f(n)).astype(np.float32)
        pre = _t(x, F64) @ _t(w, F64).T + _t(b, F64)
        pmag = _t(x, F64, True) @ _t(w, F64, True).T + _t(b, F64, True)
        y = _act(pre, act).numpy().astype(np.float32)
        if act == "relu" and mask_margin(pre.numpy(), pmag.numpy(), CAP) < 1.0:
            continue
        if act == "tanh" and np.abs(y).max() >= TANH_MAX:
            continue
        return dict(x=x, x_dot=f(rows, k) if with_xdot else None, w=w, w_dot=f(n, k), b_dot=f(n), y=y, act=act, pre=pre.numpy(), pmag=pmag.numpy())
    raise AssertionError("no seed meets the input conditions")


def tangent_cases():
    for rows in TANGENT_ROWS:
        for k, n in TANGENT_KN:
            for act in ACTS:
                for with_xdot in (False, True):
                    yield rows, k, n, act, with_xdot


def assert_conditions(c):
    if c["act"] == "relu":
        assert mask_margin(c["pre"], c["pmag"], CAP) >= 1.0
    if c["act"] == "tanh":
        assert np.abs(c["y"]).max() < TANH_MAX


def tangent_eval(c, dtype=F64, mag=False):
    return tangent_layer(c["x"], c["x_dot"], c["w"], c["w_dot"], c["b_dot"], c["y"], c["act"], dtype, mag).numpy()


def head_case(head, rows, seed=0):
    rng = np.random.default_rng(77 * seed + rows + 13 * head_width(head))
    n = head_width(head)
    return dict(head=head, rows=rows, dist_dot=rng.standard_normal((rows, n)).astype(np.float32),
                dist=(1.5 * rng.standard_normal((rows, n))).astype(np.float32),
                log_std=(0.3 * rng.standard_normal(n)).astype(np.float32) if head[0] == "gauss" else None,
                v_log_std=rng.standard_normal(n).astype(np.float32) if head[0] == "gauss" else None)


def head_eval(c, dtype=F64, mag=False):
    return head_metric(c["head"], c["dist_dot"], c["dist"], c["log_std"], c["rows"], dtype, mag).numpy()


FVP_CASES = [(head, rows, act) for head in HEADS for rows in (3, 65, 257) for act in ("tanh", "relu")]


def fvp_case(head, rows, act, seed0=0):
    """a whole actor at theta0, its float32 activations on a batch, a tangent v; seed searched for the input conditions"""
    for seed in range(seed0, seed0 + 200):
        actor = make_actor(31 * seed + rows, head, act=act)
        rng = np.random.default_rng(5 * seed + rows + 1)
        obs = rng.uniform(-1, 1, (rows, 4)).astype(np.float32)
        theta0 = flat_of(actor)
        acts64, pres = forward(actor, th.as_tensor(theta0).to(F64), obs, with_pre=True)
        acts32 = [a.numpy().astype(np.float32) for a in forward(actor, th.as_tensor(theta0), obs)]
        ok = True
        for i, pre in enumerate(pres[:-1]):
            _, ws = split(actor, th.as_tensor(theta0).to(F64))
            pmag = acts64[i].abs() @ ws[i][0].abs().T + ws[i][1].abs()
            if act == "relu" and (mask_margin(pre.numpy(), pmag.numpy(), CAP) < 1.0 or not np.array_equal(acts32[i + 1] > 0, pre.numpy() > 0)):
                ok = False
            if act == "tanh" and np.abs(acts32[i + 1]).max() >= TANH_MAX:
                ok = False
        if ok:
            v = rng.standard_normal(theta0.size).astype(np.float32)
            return dict(actor=actor, theta0=theta0, obs=obs, acts=acts32, v=v, damping=0.1)
    raise AssertionError("no seed meets the input conditions")


def fvp_eval(c, dtype=F64, mag=False):
    return fvp_fisher(c["actor"], c["theta0"], c["acts"], c["v"], c["damping"], dtype, mag).numpy()


def measure_aten():
    """the worst float32 ATen figure per kind over this module's cases, in units of 2**-24 * M"""
    fig = {"tangent": 0.0, "head": 0.0, "fvp": 0.0}
    for case in tangent_cases():
        c = tangent_case(*case)
        fig["tangent"] = max(fig["tangent"], worst(tangent_eval(c, F32), tangent_eval(c), tangent_eval(c, mag=True)))
    for head in HEADS + (("gauss", 4), ("cat", 64), ("mcat", (32, 32))):
        for rows in (1, 3, 65, 257):
            c = head_case(head, rows)
            fig["head"] = max(fig["head"], worst(head_eval(c, F32), head_eval(c), head_eval(c, mag=True)))
    for case in FVP_CASES:
        c = fvp_case(*case)
        fig["fvp"] = max(fig["fvp"], worst(fvp_eval(c, F32), fvp_eval(c), fvp_eval(c, mag=True)))
    return fig
