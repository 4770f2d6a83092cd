"""GPU checks of A2C on the HIP path.

Kernels (csrc/cstr_a2c.hip): the loss launch against an fp64 autograd statement of core/a2c/a2c.py:150-171 at rtol 2e-6 / atol 1e-7
(the bar of tests/test_ppo.py; every figure is printed in units of that bar before it is asserted); the flat RMSprop step bit for
bit against the NumPy float32 statement kept in tests/test_a2c_abi.py, the clip coefficient from a NumPy restatement of the kernel's
fixed summation order; the fused clip + step bit for bit against cstr_grad_clip_f32 followed by the unclipped step; FlatRMSprop's
state_dict against torch.optim.RMSprop. Then the classes: two consecutive teacher-forced train() steps against fixtures written by
the unmodified reference (tests/golden/a2c_*.npz, tools/refharness/gen_golden.py --only a2c) on the kernel path, with
CSTR_FUSED_LINEAR=0 and on the torch-statement path; the teacher-forced device rollout; in-place evaluation against get(None);
NumPy's global stream; logger keys, save / load, refusals, optimiser routing and a short learning run."""
import numpy as np
import pytest
import torch as th

from _parity_helpers import check_weights, q_err, rel_err
from test_a2c_abi import rmsprop_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-6, 1e-7
LOG_SQRT_2PI = float(np.log(np.sqrt(2 * np.pi)))
ROLLOUT_FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def bar(got, want, what):
    """max |got - want| / (2e-6 |want| + 1e-7), the project's bar = 1; printed, then asserted"""
    got = got.detach().cpu().numpy() if isinstance(got, th.Tensor) else got
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    units = np.abs(got - want) / (RTOL * np.abs(want) + ATOL)
    worst = int(np.argmax(units))
    print(f"BAR {what}: {units[worst]:.3f} (got {got[worst]:.9g}, want {want[worst]:.9g}, |d| {abs(got[worst] - want[worst]):.3g})")
    assert units[worst] <= 1.0, (what, units[worst], got[worst], want[worst])


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


# ---- loss --------------------------------------------------------------------------------------------------------------------
def a2c_loss_f64(mean, log_std, actions, values, adv, returns, normalize, ent_coef, vf_coef):
    """core/a2c/a2c.py:150-171 in fp64 autograd"""
    t = lambda a, g=False: th.tensor(np.asarray(a, np.float64), requires_grad=g)  # noqa: E731
    mean, log_std, values = t(mean, True), t(log_std, True), t(values, True)
    actions, adv, returns = t(actions), t(adv), t(returns)
    dist = th.distributions.Normal(mean, th.ones_like(mean) * log_std.exp())
    log_prob, entropy = dist.log_prob(actions).sum(1), dist.entropy().sum(1)
    if normalize:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # std of one element: the degrees-of-freedom warning
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    policy_loss = -(adv * log_prob).mean()
    value_loss = th.nn.functional.mse_loss(returns, values)
    entropy_loss = -th.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    scalars = [float(x) for x in (policy_loss, value_loss, entropy_loss, loss)]
    return scalars, mean.grad.numpy(), values.grad.numpy(), log_std.grad.numpy(), log_prob.detach().numpy()


def loss_case(B, A, seed, constant_adv=False):
    rng = np.random.default_rng(seed)
    log_std = rng.uniform(-0.7, 0.2, A).astype(np.float32)
    mean = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    actions = (mean + np.exp(log_std) * rng.normal(size=(B, A))).astype(np.float32)
    values = rng.normal(-20, 5, B).astype(np.float32)
    adv = np.full(B, 1.5, np.float32) if constant_adv else rng.normal(0, 3, B).astype(np.float32)
    returns = (values + rng.normal(0, 2, B)).astype(np.float32)
    return mean, log_std, actions, values, adv, returns


def run_loss(ops, case, normalize, ent_coef=0.01, vf_coef=0.5):
    mean, log_std, actions, values, adv, returns = case
    B, A = actions.shape
    g_mean, g_value, g_ls = th.empty(B, A, device=DEV), th.empty(B, device=DEV), th.empty(A, device=DEV)
    scal, logp, ws = th.zeros(4, device=DEV), th.empty(B, device=DEV), ops.new_ppo_workspace(DEV)
    ops.a2c_loss(dev(mean), dev(log_std), dev(actions), dev(values), dev(adv), dev(returns), normalize, ent_coef, vf_coef, g_mean, g_value,
                 g_ls, ws, scalars_out=scal, log_prob_out=logp)
    assert int(ws[0]) == 0  # the ticket reset itself
    return scal, g_mean, g_value, g_ls, logp


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,A", [(1, 2), (1, 4), (2, 2), (2, 4), (12, 2), (12, 4), (100, 2), (100, 4), (1030, 2), (1030, 4)])  # 1030 rows: five workgroups
def test_loss_against_fp64_autograd(ops, B, A, normalize):
    # The bar is relative, and policy_loss, loss and d/d log_std are sums of f32 terms of either sign: where they nearly cancel, one
    # ulp in exp(log_std) alone moves the result by more than the bar, whatever the kernel does. The seed offset is the one, of 60
    # tried, at which a NumPy float32 model of the arithmetic with exp(log_std) moved by -1, 0 and +1 ulp stays below 0.75 of the
    # bar in every case; it was fixed before the kernel ran.
    case = loss_case(B, A, seed=17 * B + A + 58000)
    want, gm, gv, gl, lp = a2c_loss_f64(*case, normalize, 0.01, 0.5)
    scal, g_mean, g_value, g_ls, logp = run_loss(ops, case, normalize)
    tag = f"a2c loss B={B} A={A} norm={normalize}"
    got = scal.cpu().numpy().astype(np.float64)
    bar(logp, lp, tag + " log_prob")
    bar(got[1], want[1], tag + " value_loss"), bar(got[2], want[2], tag + " entropy_loss"), bar(g_value, gv, tag + " d/d value")
    if B == 1 and normalize:
        # torch.std of one element is NaN and the reference's A2C has no `len > 1` guard (a2c.py:155-156): the policy loss, the loss
        # and every gradient that passes through the advantage are NaN in the fp64 statement, and in the kernel
        assert np.isnan(want[0]) and np.isnan(want[3]) and np.isnan(gm).all() and np.isnan(gl).all()
        assert np.isnan(got[0]) and np.isnan(got[3]) and bool(th.isnan(g_mean).all()) and bool(th.isnan(g_ls).all())
        return
    bar(got[0], want[0], tag + " policy_loss"), bar(got[3], want[3], tag + " loss")
    bar(g_mean, gm, tag + " d/d mean"), bar(g_ls, gl, tag + " d/d log_std")


@pytest.mark.parametrize("B,A", [(12, 2), (300, 4)])
def test_loss_constant_advantages_with_normalisation(ops, B, A):
    case = loss_case(B, A, seed=5, constant_adv=True)  # std = 0: the normalised advantages are 0 / 1e-8 = 0
    want, gm, gv, gl, _ = a2c_loss_f64(*case, True, 0.01, 0.5)
    scal, g_mean, g_value, g_ls, _ = run_loss(ops, case, True)
    assert float(scal[0]) == 0.0 and float(g_mean.abs().max()) == 0.0 and np.abs(gm).max() == 0.0 and want[0] == 0.0
    bar(g_value, gv, "constant advantages d/d value"), bar(g_ls, gl, "constant advantages d/d log_std")
    bar(scal.cpu().numpy()[1:], want[1:], "constant advantages scalars")
    scal2, *_ = run_loss(ops, case, True)
    assert th.equal(scal2, scal)  # deterministic


def test_loss_reads_strided_means_and_needs_no_optional_output(ops):
    B, A = 70, 2
    mean, log_std, actions, values, adv, returns = loss_case(B, A, seed=9)
    wide = th.zeros(B, 4, device=DEV)
    wide[:, :A] = dev(mean)
    g_mean, g_value, g_ls, ws = th.empty(B, A, device=DEV), th.empty(B, device=DEV), th.empty(A, device=DEV), ops.new_ppo_workspace(DEV)
    ops.a2c_loss(wide[:, :A], dev(log_std), dev(actions), dev(values), dev(adv), dev(returns), False, 0.01, 0.5, g_mean, g_value, g_ls, ws)
    _, gm, gv, gl, _ = a2c_loss_f64(mean, log_std, actions, values, adv, returns, False, 0.01, 0.5)
    bar(g_mean, gm, "strided mean d/d mean"), bar(g_value, gv, "strided mean d/d value"), bar(g_ls, gl, "strided mean d/d log_std")


# ---- RMSprop -----------------------------------------------------------------------------------------------------------------
def device_norm(g):
    """||g||_2 as cstr_grad_clip_f32 / cstr_rmsprop_f32 sum it: min(ceil(n / 256), 64) workgroups of 256 threads, every thread adds
    its float32 squares to an f64 accumulator in grid-stride order, a halving tree per workgroup, the workgroups in order."""
    n = g.size
    grid = min(-(-n // 256), 64)
    stride = grid * 256
    sq = np.zeros(-(-n // stride) * stride, np.float64)
    sq[:n] = (g * g).astype(np.float32)
    acc = np.zeros((grid, 256), np.float64)
    for chunk in sq.reshape(-1, grid, 256):
        acc = acc + chunk
    o = 128
    while o > 0:
        acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
        o >>= 1
    s = 0.0
    for b in range(grid):
        s = s + acc[b, 0]
    return np.float32(np.sqrt(s))


def clip_coef(norm, max_norm):
    return np.minimum(np.float32(max_norm) / (norm + np.float32(1e-6)), np.float32(1.0))


def rmsprop_case(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    grads = [(10.0 ** rng.uniform(-8, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(3)]  # spanning 1e-8 .. 1
    return w, grads


@pytest.mark.parametrize("mode", ["engaged", "not_engaged", "off"])
@pytest.mark.parametrize("n", [1, 7, 1030, 9001])  # below one vector, a scalar tail, more than one workgroup
def test_rmsprop_is_bit_identical_to_the_numpy_statement(ops, n, mode):
    lr, alpha, eps = 7e-4, 0.99, 1e-5
    w, grads = rmsprop_case(n, seed=n)
    sq = np.zeros(n, np.float32)
    param, square_avg, lr_dev = dev(w), dev(sq), th.tensor([lr], dtype=th.float64, device=DEV)
    ws, out = ops.new_ppo_workspace(DEV), th.full((1,), -1.0, device=DEV)
    for k, g in enumerate(grads):  # three consecutive steps: the second and third meet a non-zero square_avg
        norm = device_norm(g)
        max_norm = {"engaged": 0.25 * float(norm), "not_engaged": 4.0 * float(norm) + 1.0, "off": 0.0 if k else None}[mode]
        coef = np.float32(1.0) if mode == "off" else clip_coef(norm, max_norm)
        assert (coef < 1) == (mode == "engaged")
        grad = dev(g)
        if mode == "off":
            ops.rmsprop(param, grad, square_avg, lr_dev, alpha, eps, max_norm)  # no workspace, no norm_out
        else:
            ops.rmsprop(param, grad, square_avg, lr_dev, alpha, eps, max_norm, ws, out)
            bar(out, [np.sqrt((g.astype(np.float64) ** 2).sum())], f"rmsprop n={n} {mode} step {k} norm_out")
            assert float(out) == float(norm)
        w, g_clipped, sq = rmsprop_numpy(w, g, sq, lr, alpha, eps, coef)
        np.testing.assert_array_equal(param.cpu().numpy(), w, err_msg=f"param, step {k}")
        np.testing.assert_array_equal(square_avg.cpu().numpy(), sq, err_msg=f"square_avg, step {k}")
        np.testing.assert_array_equal(grad.cpu().numpy(), g_clipped, err_msg=f"grad, step {k}")  # written back clipped; untouched when off
    if mode == "off":
        assert float(out) == -1.0


@pytest.mark.parametrize("n", [7, 9001])
def test_fused_clip_and_step_equals_grad_clip_then_the_unclipped_step(ops, n):
    lr, alpha, eps = 7e-4, 0.99, 1e-5
    w, grads = rmsprop_case(n, seed=100 + n)
    lr_dev = th.tensor([lr], dtype=th.float64, device=DEV)
    pa, sa, pb, sb = dev(w), th.zeros(n, device=DEV), dev(w), th.zeros(n, device=DEV)
    ws, na, nb = ops.new_ppo_workspace(DEV), th.zeros(1, device=DEV), th.zeros(1, device=DEV)
    for g in grads:
        max_norm = 0.3 * float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        ga, gb = dev(g), dev(g)
        ops.rmsprop(pa, ga, sa, lr_dev, alpha, eps, max_norm, ws, na)
        ops.grad_clip(gb, max_norm, ws, nb)
        ops.rmsprop(pb, gb, sb, lr_dev, alpha, eps, None)
        assert th.equal(pa, pb) and th.equal(sa, sb) and th.equal(ga, gb) and th.equal(na, nb)
    assert not th.equal(pa, dev(w))


def test_flat_rmsprop_state_dict_round_trips_through_torch(ops):
    from core.common.arena import FlatRMSprop, ParamArena

    gen = th.Generator().manual_seed(3)
    shapes = [(5, 3), (7,), (2, 4)]

    def params():
        g = th.Generator().manual_seed(4)
        return [th.nn.Parameter(th.rand(*s, generator=g) * 2 - 1) for s in shapes]

    ps = params()
    arena = ParamArena(ps, DEV)
    opt = FlatRMSprop(arena, lr=1e-2, alpha=0.99, eps=1e-5, weight_decay=0)
    assert opt.state_dict()["state"] == {} and opt.step_count == 0
    ws = ops.new_ppo_workspace(DEV)
    grads = [[th.randn(*s, generator=gen) for s in shapes] for _ in range(3)]

    def set_grads(plist, gs):
        for p, g in zip(plist, gs):
            if p.grad is None:
                p.grad = g.to(p.device).clone()
            else:
                p.grad.copy_(g)

    set_grads(ps, grads[0]), opt.step(max_norm=0.5, workspace=ws)
    set_grads(ps, grads[1]), opt.step()
    sd = opt.state_dict()
    assert list(sd["param_groups"][0].keys()) == ["lr", "momentum", "alpha", "eps", "centered", "weight_decay", "capturable", "foreach",
                                                  "maximize", "differentiable", "params"]
    assert set(sd["state"][0].keys()) == {"step", "square_avg"} and float(sd["state"][1]["step"]) == 2.0 and opt.step_count == 2
    # into torch.optim.RMSprop over clones of the parameters ...
    clones = [th.nn.Parameter(p.detach().clone()) for p in ps]
    topt = th.optim.RMSprop(clones, lr=1e-2, alpha=0.99, eps=1e-5, weight_decay=0)
    topt.load_state_dict(sd)
    for c, p in zip(clones, ps):
        o = arena.offset_of[id(p)]
        assert th.equal(topt.state[c]["square_avg"], opt.square_avg[o:o + p.numel()].view(p.shape))
    # ... and back into a fresh FlatRMSprop
    ps2 = params()
    arena2 = ParamArena(ps2, DEV)
    with th.no_grad():
        arena2.flat.copy_(arena.flat)
    opt2 = FlatRMSprop(arena2, lr=5e-3, alpha=0.99, eps=1e-5)
    opt2.load_state_dict(topt.state_dict())
    assert th.equal(opt2.square_avg, opt.square_avg) and opt2.step_count == 2 and opt2.param_groups[0]["lr"] == 1e-2
    assert float(opt2.lr_dev) == 1e-2
    # the next step from all three agrees: the two flat ones bit for bit, torch's own kernels within twice the CPU measurement of
    # the NumPy statement against ATen (tests/test_a2c_abi.py: square_avg 2.4e-7 relative, weights 6e-8 absolute, |w| <= 1.5)
    set_grads(ps, grads[2]), set_grads(ps2, grads[2]), set_grads(clones, grads[2])
    opt.step(), opt2.step(), topt.step()
    assert th.equal(arena.flat, arena2.flat) and th.equal(opt.square_avg, opt2.square_avg)
    for c, p in zip(clones, ps):
        o = arena.offset_of[id(p)]
        sq_t, sq_f = topt.state[c]["square_avg"].double(), opt.square_avg[o:o + p.numel()].view(p.shape).double()
        assert float(((sq_t - sq_f).abs() / sq_t).max()) <= 2 * 2.4e-7
        assert float((c.detach() - p.detach()).abs().max()) <= 2 * 6e-8 and float(p.detach().abs().max()) <= 1.5
    bad = topt.state_dict()
    bad["state"] = {i: dict(st, momentum_buffer=th.zeros(1)) for i, st in bad["state"].items()}
    with pytest.raises(ValueError, match="momentum"):
        opt2.load_state_dict(bad)
    with pytest.raises(ValueError, match="no weight decay"):
        FlatRMSprop(arena2, momentum=0.9)


# ---- the classes against the reference's fixtures ------------------------------------------------------------------------------------
def make_model(g, prefix="before", n_steps=None, **kw):
    from core.a2c import A2C
    from core.common.vec_env import CSTRVecEnv

    model = A2C("MlpPolicy", CSTRVecEnv(int(g["n_envs"]), device=DEV), seed=int(g["seed"]), n_steps=int(g["n_steps"]),
                learning_rate=float(g["learning_rate"]), ent_coef=float(g["ent_coef"]),
                policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]]), device=DEV, **kw)
    with th.no_grad():
        for k, v in model.policy.state_dict().items():
            v.copy_(th.as_tensor(g[f"{prefix}/policy/{k}"]))
    return model


def storage_order(g, pre, it, name):
    """The fixture's per-row record is in the order of get(None): row k is flat index perm[k] = env * T + step (swap_and_flatten).
    Back into the buffer's storage order, row step * N + env."""
    perm, T, N = g[f"{pre}it{it}/permutation"], int(g["n_steps"]), int(g["n_envs"])
    out = np.empty(T * N, np.float32)
    out[(perm % T) * N + perm // T] = g[f"{pre}it{it}/{name}"]
    return out


def rollout_arrays(g, pre, it):
    return {f: g[f"{pre}it{it}/rollout/{f}"] if f"{pre}it{it}/rollout/{f}" in g.files else g[f"it{it}/rollout/{f}"] for f in ROLLOUT_FIELDS}


def check_step(model, g, pre, it, path, logger=False):
    """the bars of tests/test_ppo.py::check_train"""
    label = {"fused": "a2c_fused", "rocblas": "a2c_rocblas", "torch": "a2c_aten"}[path]
    cap = model.last_train_capture
    want_v, want_lp = storage_order(g, pre, it, "values"), storage_order(g, pre, it, "log_prob")
    want_s = g[f"{pre}it{it}/scalars"].astype(np.float64)
    assert rel_err(cap["values"].cpu().numpy(), want_v, float(np.abs(want_v).mean())) < 1e-5, (it, "values")
    assert q_err(cap["log_prob"].cpu().numpy(), want_lp, label) < 1e-5, (it, "log_prob")
    got = cap["scalars"].cpu().numpy().astype(np.float64)
    for i in range(4):
        print(f"STEP {pre}it{it} {path} scalar {i}: got {got[i]:.9g} want {want_s[i]:.9g}")
        assert abs(got[i] - want_s[i]) <= 1e-5 * max(abs(want_s[i]), 1.0), (it, i, got[i], want_s[i])
    gn = rel_err(cap["grad_norm"].cpu().numpy(), g[f"{pre}it{it}/grad_norm"])
    print(f"STEP {pre}it{it} {path} grad_norm rel {gn:.3g}")
    assert gn < 5e-5, (it, "grad_norm")
    assert model._n_updates == int(g[f"{pre}it{it}/n_updates"]) and model.policy.optimizer.step_count == int(g[f"{pre}it{it}/optimizer_steps"])
    p = f"{pre}it{it}/"
    # RMSprop turns a gradient error d into at most lr / eps * d on a weight. The fixtures' own distance (the reference's f32 on the
    # CPU) from an fp64 restatement of the same two steps is at most 0.10 of check_weights' bar, so the bar stays as it is.
    check_weights(model, {k[len(p):]: g[k] for k in g.files if k.startswith(p + "after/")}, "after", ["policy"])
    if logger:
        logged = model.logger.resolved()
        want = dict(zip([str(k) for k in g[f"{p}logged_keys"]], g[f"{p}logged_values"]))
        assert set(want) == {"train/n_updates", "train/explained_variance", "train/entropy_loss", "train/policy_loss", "train/value_loss",
                             "train/std", "train/learning_rate"}
        assert set(want) <= set(logged), set(want) - set(logged)
        for key, w in want.items():
            assert abs(float(logged[key]) - w) <= 1e-5 * max(abs(w), 1.0), (key, logged[key], w)


def run_two_iterations(g, path, monkeypatch, pre="", logger=False, **kw):
    from core.common import fused
    from core.common.buffers import RolloutBuffer

    if path == "rocblas":  # the kernel path with every GEMM left to PyTorch-ROCm / rocBLAS (CSTR_FUSED_LINEAR=0)
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    model = make_model(g, **kw)
    if path == "torch":
        model.fused_learner = False
    assert model.fused_learner == (path != "torch")
    model.debug_capture = True
    total = int(g["iterations"]) * int(g["n_envs"]) * int(g["n_steps"])
    for it in range(int(g["iterations"])):
        model.rollout_buffer = RolloutBuffer.from_arrays(model.observation_space, model.action_space, DEV, gamma=model.gamma,
                                                         gae_lambda=model.gae_lambda, **rollout_arrays(g, pre, it))
        model.rollout_buffer.forced_permutations = [g[f"{pre}it{it}/permutation"]]
        model._update_current_progress_remaining((it + 1) * int(g["n_envs"]) * int(g["n_steps"]), total)
        model.train()
        assert not model.rollout_buffer.forced_permutations  # consumed on either path
        check_step(model, g, pre, it, path, logger=logger)
    return model


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("name", ["small", "default"])
def test_train_teacher_forced_two_iterations(golden, name, path, monkeypatch):
    from core.common.arena import FlatRMSprop

    g = golden(f"a2c_train_kat_{name}.npz")
    model = run_two_iterations(g, path, monkeypatch, logger=name == "small")
    assert isinstance(model.policy.optimizer, FlatRMSprop) and model.policy.flat_optimizers() == [model.policy.optimizer]
    if name == "small":  # the optimiser state in torch's layout against the reference's
        sd = model.policy.optimizer.state_dict()
        for i, (k, _) in enumerate(model.policy.named_parameters()):
            want = g[f"it1/opt/square_avg/{k}"]
            got = sd["state"][i]["square_avg"].cpu().numpy()
            assert float(np.abs(got - want).max()) <= 1e-4 * float(np.abs(want).max()), k


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("variant", ["norm", "noclip", "adam"])
def test_train_teacher_forced_variants(golden, variant, path, monkeypatch):
    from core.common.arena import FlatAdam, FlatRMSprop

    g = golden("a2c_train_kat_variants.npz")
    kw = {"norm": dict(normalize_advantage=True), "noclip": dict(max_grad_norm=float(g["noclip/max_grad_norm"])), "adam": dict(use_rms_prop=False)}[variant]
    model = run_two_iterations(g, path, monkeypatch, pre=variant + "/", **kw)
    assert isinstance(model.policy.optimizer, FlatAdam if variant == "adam" else FlatRMSprop)
    if variant == "adam":
        assert model.policy.optimizer.param_groups[0]["eps"] == 1e-5


def test_device_rollout_and_train_reproduce_the_first_iteration(golden):
    """collect_rollouts on the device (the `before/` weights, the initial observations and step counters injected after
    _setup_learn's reset, the recorded Normal draws forced) followed by train() on the buffer it filled, in place."""
    g = golden("a2c_train_kat_small.npz")
    model = make_model(g)
    assert model.fused_learner and model._device_rollout()
    n, T = int(g["n_envs"]), int(g["n_steps"])
    _, cb = model._setup_learn(2 * n * T, None)
    model.env.set_state(g["init_obs"], g["init_steps"])
    model._fast.eps_queue = [th.as_tensor(e) for e in g["it0/eps"]]
    assert model.collect_rollouts(model.env, cb, model.rollout_buffer, T)
    rb = model.rollout_buffer
    assert rb.full and not model._fast.eps_queue and g["it0/timeouts"].sum() >= 1
    np.testing.assert_array_equal(rb.episode_starts.cpu().numpy(), g["it0/rollout/episode_starts"])
    for f in ("observations", "actions", "values", "log_probs", "rewards", "advantages", "returns"):
        want = g[f"it0/rollout/{f}"]
        err = float(np.abs(getattr(rb, f).cpu().numpy().reshape(want.shape) - want).max() / np.abs(want).max())
        assert err < 1e-5, (f, err)
    model.debug_capture = True
    model._update_current_progress_remaining(n * T, 2 * n * T)
    before = rb.permutation_rng.get_state()[1].copy()
    model.train()
    np.testing.assert_array_equal(rb.permutation_rng.get_state()[1], before)  # the algorithm's own RandomState: the draw is skipped
    check_step(model, g, "", 0, "fused")


def test_in_place_evaluation_agrees_with_get_none(golden, monkeypatch):
    """The same step two ways: the kernel path on the buffer in place (no gather launch) and the torch statements over get(None) with
    the reference's recorded permutation."""
    from core.common import hip_ops
    from core.common.buffers import RolloutBuffer

    g = golden("a2c_train_kat_small.npz")
    caps, gathers = {}, []
    gather = hip_ops.ppo_gather
    monkeypatch.setattr(hip_ops, "ppo_gather", lambda *a: (gathers.append(1), gather(*a))[1])
    for how in ("in_place", "torch"):
        model = make_model(g)
        model.debug_capture = True
        if how == "torch":
            model.fused_learner = False
        model.rollout_buffer = RolloutBuffer.from_arrays(model.observation_space, model.action_space, DEV, gamma=model.gamma,
                                                         gae_lambda=model.gae_lambda, **rollout_arrays(g, "", 0))
        model.rollout_buffer.forced_permutations = [g["it0/permutation"]]
        del gathers[:]
        model.train()
        assert len(gathers) == (0 if how == "in_place" else 1)  # no gather launch in place
        check_step(model, g, "", 0, "torch" if how == "torch" else "fused")
        caps[how] = model.last_train_capture
    a, b = caps["in_place"], caps["torch"]
    va, vb = a["values"].cpu().numpy(), b["values"].cpu().numpy()
    assert rel_err(va, vb, float(np.abs(vb).mean())) < 1e-5
    assert q_err(a["log_prob"].cpu().numpy(), b["log_prob"].cpu().numpy(), "a2c_aten") < 1e-5
    for x, y in zip(a["scalars"].tolist(), b["scalars"].tolist()):
        assert abs(x - y) <= 1e-5 * max(abs(y), 1.0)
    assert rel_err(a["grad_norm"].cpu().numpy(), b["grad_norm"].cpu().numpy()) < 5e-5


def host_vec_env(n):
    """A VecEnv that is not device-resident (NumPy in, NumPy out) around a CSTRVecEnv: learn() takes the reference's NumPy rollout
    loop and the rollout buffer draws its permutations from NumPy's global stream."""
    from core.common.vec_env import CSTRVecEnv, VecEnv

    class HostVecEnv(VecEnv):
        def __init__(self):
            self.inner = CSTRVecEnv(n, device=DEV)
            super().__init__(n, self.inner.observation_space, self.inner.action_space)

        def seed(self, seed=None):
            return self.inner.seed(seed)

        def reset(self):
            return self.inner.reset()

        def step_async(self, actions):
            self.inner.step_async(actions)

        def step_wait(self):
            return self.inner.step_wait()

    return HostVecEnv()


def test_global_numpy_stream_moves_as_in_the_reference():
    from core.a2c import A2C

    env = host_vec_env(4)
    model = A2C("MlpPolicy", env, seed=3, device=DEV)
    assert model._denv is None and model.fused_learner
    _, cb = model._setup_learn(40, None)
    assert model.collect_rollouts(env, cb, model.rollout_buffer, model.n_steps) and not model._device_rollout()
    assert model.rollout_buffer.permutation_rng is None
    for fused_path in (True, False):
        model.fused_learner = fused_path
        np.random.seed(77)
        model.train()
        got = np.random.get_state()
        np.random.seed(77)
        np.random.permutation(20)  # one permutation(T * N) per train(): buffers.py:483 under a2c.py:144
        want = np.random.get_state()
        assert got[2] == want[2] and np.array_equal(got[1], want[1]), fused_path
    assert model._n_updates == 2 and all(bool(th.isfinite(p).all()) for p in model.policy.parameters())


def test_save_load_round_trip(golden, tmp_path):
    import zipfile

    from core.a2c import A2C
    from core.common.arena import FlatRMSprop
    from core.common.vec_env import CSTRVecEnv

    g = golden("a2c_train_kat_small.npz")
    model = make_model(g, normalize_advantage=True, rms_prop_eps=2e-5)
    model.learn(3 * int(g["n_envs"] * g["n_steps"]))
    path = str(tmp_path / "a2c_model.zip")
    model.save(path)
    assert {"data", "policy.pth", "policy.optimizer.pth"} <= set(zipfile.ZipFile(path).namelist())  # the SB3 layout
    # the optimiser state in torch's layout: it loads into a torch.optim.RMSprop over the same parameters
    from core.common.save_util import load_from_zip_file

    _, params, _ = load_from_zip_file(path)
    sd = params["policy.optimizer"]
    assert set(sd["state"][0]) == {"step", "square_avg"} and float(sd["state"][0]["step"]) == 3.0
    assert sd["param_groups"][0]["alpha"] == 0.99 and sd["param_groups"][0]["eps"] == 2e-5 and sd["param_groups"][0]["momentum"] == 0
    th.optim.RMSprop([th.nn.Parameter(p.detach().clone()) for p in model.policy.parameters()], lr=1.0).load_state_dict(sd)
    loaded = A2C.load(path, env=CSTRVecEnv(int(g["n_envs"]), device=DEV), device=DEV)
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    assert isinstance(loaded.policy.optimizer, FlatRMSprop) and loaded.fused_learner
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count == 3
    assert th.equal(loaded.policy.optimizer.square_avg, model.policy.optimizer.square_avg)
    assert (loaded.n_steps, loaded.normalize_advantage, loaded.rms_prop_eps, loaded.use_rms_prop, loaded.gae_lambda) == (5, True, 2e-5, True, 1.0)
    assert loaded.policy.optimizer.param_groups[0]["eps"] == 2e-5 and loaded.policy_kwargs["net_arch"] == [32, 32]
    assert loaded.num_timesteps == model.num_timesteps and loaded._n_updates == model._n_updates == 3
    obs = np.random.default_rng(0).uniform(-1, 1, (5, 4)).astype(np.float32)
    np.testing.assert_array_equal(model.predict(obs, deterministic=True)[0], loaded.predict(obs, deterministic=True)[0])
    # a checkpoint whose optimiser state was written by torch.optim.RMSprop itself (the reference's policy.optimizer.pth)
    ref = th.optim.RMSprop([th.nn.Parameter(p.detach().cpu().clone()) for p in model.policy.parameters()], lr=3e-3, alpha=0.99, eps=1e-5)
    for p in ref.param_groups[0]["params"]:
        p.grad = th.ones_like(p)
    ref.step()
    loaded.set_parameters({"policy": model.policy.state_dict(), "policy.optimizer": ref.state_dict()})
    assert loaded.policy.optimizer.step_count == 1 and abs(float(loaded.policy.optimizer.square_avg.max()) - 0.01) < 1e-9


def test_logger_keys_and_refusals():
    from core.a2c import A2C
    from core.common import distributed as dist_util
    from core.common.vec_env import CSTRVecEnv, VecNormalize

    env = CSTRVecEnv(8, device=DEV)
    model = A2C("MlpPolicy", env, seed=3, device=DEV)
    model.learn(8 * 5 * 4, log_interval=2)
    keys = set(model.logger.last_dump) | set(model.logger.resolved())
    for key in ("train/n_updates", "train/explained_variance", "train/entropy_loss", "train/policy_loss", "train/value_loss", "train/std",
                "train/learning_rate", "time/iterations", "time/fps", "time/time_elapsed", "time/total_timesteps"):
        assert key in keys, key
    assert not any(k.startswith("train/clip") or k == "train/approx_kl" for k in keys) and model._n_updates == 4
    with pytest.raises(NotImplementedError, match="hipGraph"):
        model.enable_graph_capture(True)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        A2C("MlpPolicy", VecNormalize(CSTRVecEnv(4, device=DEV)), device=DEV)
    with pytest.raises(ValueError, match="does not support gSDE"):
        A2C("MlpPolicy", env, use_sde=True, device=DEV)
    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            A2C("MlpPolicy", env, device=DEV)
    finally:
        dist_util.rank_world = orig


def test_optimiser_routing():
    from core.a2c import A2C
    from core.common.arena import FlatAdam, FlatRMSprop
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO

    # PPO with RMSprop keeps the stock torch optimiser and the torch-statement path
    ppo = PPO("MlpPolicy", CSTRVecEnv(4, device=DEV), n_steps=8, batch_size=16, n_epochs=1, seed=1, device=DEV,
              policy_kwargs=dict(optimizer_class=th.optim.RMSprop, optimizer_kwargs=dict(alpha=0.99, eps=1e-5, weight_decay=0)))
    assert not ppo.fused_learner and type(ppo.policy.optimizer) is th.optim.RMSprop and ppo.policy.flat_optimizers() == []
    env = CSTRVecEnv(4, device=DEV)
    assert isinstance(A2C("MlpPolicy", env, device=DEV).policy.optimizer, FlatRMSprop)
    assert isinstance(A2C("MlpPolicy", env, use_rms_prop=False, device=DEV).policy.optimizer, FlatAdam)
    # RMSprop outside the flat kernel's form: the stock optimiser, the torch statements
    for kwargs in (dict(momentum=0.9), dict(centered=True), dict(weight_decay=1e-4)):
        other = A2C("MlpPolicy", env, seed=1, device=DEV, policy_kwargs=dict(optimizer_class=th.optim.RMSprop, optimizer_kwargs=kwargs))
        assert not other.fused_learner and type(other.policy.optimizer) is th.optim.RMSprop, kwargs
        with pytest.raises(ValueError, match="no kernel path"):
            other.fused_learner = True
    other.learn(4 * 5 * 2)
    assert other._n_updates == 2 and all(bool(th.isfinite(p).all()) for p in other.policy.parameters())


def test_it_learns():
    from core.a2c import A2C
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv

    def score(model):
        env = CSTRVecEnv(8, device=DEV)
        env.seed(1000)
        return evaluate_policy(model, env, n_eval_episodes=8, deterministic=True)[0]

    # 300 iterations of 16 steps: with the class defaults (n_steps 5, lr 7e-4, log_std 0) the reference itself, run on the CPU for
    # 400 iterations on 32 envs, improved on one seed of two; with these settings it went from -309 to -57 / -152 / -56 on three seeds
    model = A2C("MlpPolicy", CSTRVecEnv(32, device=DEV), learning_rate=1e-3, n_steps=16, gae_lambda=0.95, seed=0, device=DEV,
                policy_kwargs=dict(log_std_init=-1.0))
    before = score(model)
    model.learn(32 * 16 * 300)
    after = score(model)
    print(f"A2C evaluate_policy before {before:.1f}, after {after:.1f}")
    assert np.isfinite(after) and after > before
    assert model.fused_learner and model._n_updates == 300 == model.policy.optimizer.step_count
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
