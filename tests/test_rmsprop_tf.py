"""GPU checks of RMSpropTFLike on the HIP path.

The kernel (cstr_rmsprop_tf_f32, csrc/cstr_a2c.hip) bit for bit against the NumPy float32 statement kept in
tests/test_rmsprop_tf_abi.py, in six forms, with the clip engaged, not engaged and off, over three steps with the learning rate changed
in HBM; the folded clip + step against cstr_grad_clip_f32 followed by the unclipped call; NaN propagation; sentinel padding behind
every arena; FlatRMSpropTFLike's state_dict against the class; two teacher-forced train() steps against fixtures written by the
unmodified reference (tests/golden/a2c_tflike_train_kat_*.npz, tools/refharness/gen_golden.py --only rmsprop_tf) on the kernel path,
with CSTR_FUSED_LINEAR=0 and on the torch-statement path; routing, the launch count, checkpoints and a short learning run."""
import numpy as np
import pytest
import torch as th

from _sentinel_bufs import Bufs
from test_a2c import DEV, check_step, clip_coef, dev, device_norm, rmsprop_case, rollout_arrays
from test_rmsprop_tf_abi import CPU_DISTANCE, FORMS, new_state, rmsprop_tf_numpy

pytestmark = pytest.mark.gpu
STATE = ("square_avg", "momentum_buffer", "grad_avg")


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


def launch(ops, kw, st, grad, lr_dev, max_norm=None, ws=None, out=None):
    """st: {"param", "square_avg"[, "momentum_buffer"][, "grad_avg"]} of device tensors, as the form has them"""
    ops.rmsprop_tf(st["param"], grad, st["square_avg"], lr_dev, kw.get("alpha", 0.99), kw.get("eps", 1e-8), kw.get("weight_decay", 0.0),
                   kw.get("momentum", 0.0), st.get("momentum_buffer"), st.get("grad_avg"), max_norm, ws, out)


def padded_state(bufs, host):
    """host: (w, sq, buf, ga) NumPy arrays or None -> the device state, every arena followed by sentinel padding"""
    return {name: bufs.put(name, a) for name, a in zip(("param",) + STATE, host) if a is not None}


def assert_state(st, host, what):
    for name, a in zip(("param",) + STATE, host):
        assert (a is None) == (name not in st), name
        if a is not None:
            np.testing.assert_array_equal(st[name].cpu().numpy(), a, err_msg=f"{name}, {what}")


# ---- the kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 9001])  # the scalar tail alone, one float4, body + tail, several workgroups
def test_kernel_is_bit_identical_to_the_numpy_statement(ops, n, form):
    kw = FORMS[form]
    lrs = (7e-4, 7e-4, 3e-3)  # changed in HBM between the second and the third step
    for mode in ("engaged", "not_engaged", "off"):
        w, grads = rmsprop_case(n, seed=n)
        host = (w,) + new_state(n, kw)
        first, second = Bufs(), Bufs()  # the same launches on two sets of buffers: the second is bit-identical to the first
        sa, sb = padded_state(first, host), padded_state(second, host)
        lr_dev = th.tensor([lrs[0]], dtype=th.float64, device=DEV)
        ws, out, ref_norm = ops.new_ppo_workspace(DEV), th.full((1,), -1.0, device=DEV), th.zeros(1, device=DEV)
        for k, g in enumerate(grads):
            if lrs[k] != float(lr_dev):
                lr_dev.fill_(lrs[k])
            norm = device_norm(g)
            max_norm = {"engaged": 0.25 * float(norm), "not_engaged": 4.0 * float(norm) + 1.0, "off": 0.0 if k else None}[mode]
            coef = np.float32(1.0) if mode == "off" else clip_coef(norm, max_norm)
            assert (coef < 1) == (mode == "engaged")
            ga, gb = first.put("grad", g), second.put("grad", g)
            if mode == "off":
                launch(ops, kw, sa, ga, lr_dev, max_norm), launch(ops, kw, sb, gb, lr_dev, max_norm)  # no workspace, no norm_out
            else:
                launch(ops, kw, sa, ga, lr_dev, max_norm, ws, out), launch(ops, kw, sb, gb, lr_dev, max_norm, ws, out)
                ops.grad_clip(dev(g), max_norm, ws, ref_norm)
                assert float(out) == float(norm) and th.equal(out, ref_norm)  # cstr_grad_clip_f32's norm
            w_, g_clipped, sq, buf, gavg = rmsprop_tf_numpy(host[0], g, *host[1:], lrs[k], coef=coef, **kw)
            host = (w_, sq, buf, gavg)
            what = f"n={n} {form} {mode} step {k}"
            assert_state(sa, host, what), assert_state(sb, host, what + " (second launch)")
            # written back clipped, before weight decay; untouched when the clip is off
            np.testing.assert_array_equal(ga.cpu().numpy(), g_clipped, err_msg="grad, " + what)
            np.testing.assert_array_equal(gb.cpu().numpy(), g_clipped, err_msg="grad, " + what)
            first.check(), second.check()
        if mode == "off":
            assert float(out) == -1.0
        assert not np.array_equal(host[0], w) and np.isfinite(host[0]).all()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [5, 9001])
def test_folded_clip_equals_grad_clip_then_the_unclipped_step(ops, n, form):
    kw = FORMS[form]
    w, grads = rmsprop_case(n, seed=100 + n)
    host = (w,) + new_state(n, kw)
    sa, sb = padded_state(Bufs(), host), padded_state(Bufs(), host)
    lr_dev = th.tensor([7e-4], dtype=th.float64, device=DEV)
    ws, na, nb = ops.new_ppo_workspace(DEV), th.zeros(1, device=DEV), th.zeros(1, device=DEV)
    for g in grads:
        max_norm = 0.3 * float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        ga, gb = dev(g), dev(g)
        launch(ops, kw, sa, ga, lr_dev, max_norm, ws, na)
        ops.grad_clip(gb, max_norm, ws, nb)
        launch(ops, kw, sb, gb, lr_dev, None)
        assert th.equal(ga, gb) and th.equal(na, nb) and all(th.equal(sa[k], sb[k]) for k in sa)
    assert not th.equal(sa["param"], dev(w))


@pytest.mark.parametrize("form", list(FORMS))
def test_a_nan_gradient_element_spreads_as_in_the_statement(ops, form):
    kw, n = FORMS[form], 1030
    w, grads = rmsprop_case(n, seed=7)
    g = grads[0]
    g[[2, 517, n - 1]] = np.nan  # in the float4 body of two workgroups and in the scalar tail
    host = (w,) + new_state(n, kw)
    bufs = Bufs()
    st, grad = padded_state(bufs, host), bufs.put("grad", g)
    launch(ops, kw, st, grad, th.tensor([7e-4], dtype=th.float64, device=DEV))
    w_, _, sq, buf, gavg = rmsprop_tf_numpy(host[0], g, *host[1:], 7e-4, **kw)
    assert np.isnan(w_).sum() == 3 and np.isnan(sq).sum() == 3  # those elements alone
    assert_state(st, (w_, sq, buf, gavg), form)  # assert_array_equal: NaNs in the same places, everything else bit for bit
    bufs.check()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_centred_form_gives_nan_where_the_variance_estimate_rounds_below_minus_eps(ops, momentum):
    """square_avg - grad_avg^2 + eps < 0 (a state no sequence of steps from ones reaches, set by hand): NaN on both sides"""
    kw = dict(centered=True, eps=1e-5, **({"momentum": momentum} if momentum else {}))
    n = 9
    w = np.linspace(-1, 1, n).astype(np.float32)
    sq, ga = np.full(n, 1e-4, np.float32), np.full(n, 0.5, np.float32)
    sq[::2] = 1.0  # every other element stays regular
    host = (w, sq, np.zeros(n, np.float32) if momentum else None, ga)
    bufs = Bufs()
    st, grad = padded_state(bufs, host), bufs.put("grad", np.full(n, 1e-3, np.float32))
    launch(ops, kw, st, grad, th.tensor([1e-2], dtype=th.float64, device=DEV))
    w_, _, sq_, buf_, ga_ = rmsprop_tf_numpy(w, np.full(n, 1e-3, np.float32), sq, host[2], ga, 1e-2, **kw)
    assert np.isnan(w_[1::2]).all() and np.isfinite(w_[::2]).all() and np.isfinite(sq_).all() and np.isfinite(ga_).all()
    assert_state(st, (w_, sq_, buf_, ga_), "negative variance estimate")
    bufs.check()


# ---- FlatRMSpropTFLike -------------------------------------------------------------------------------------------------------
SHAPES = [(5, 3), (7,), (2, 4)]


def new_params(device="cpu"):
    g = th.Generator().manual_seed(4)
    return [th.nn.Parameter((th.rand(*s, generator=g) * 2 - 1).to(device)) for s in SHAPES]


def new_grads(seed):
    rng = np.random.default_rng(seed)  # the magnitudes of the CPU measurement: 1e-8 .. 1, either sign
    return [th.as_tensor((10.0 ** rng.uniform(-8, 0, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32)) for s in SHAPES]


def set_grads(plist, gs):
    for p, g in zip(plist, gs):
        if p.grad is None:
            p.grad = g.to(p.device).clone()
        else:
            p.grad.copy_(g)


def flat_state(opt, arena, p, key):
    o = arena.offset_of[id(p)]
    buf = {"square_avg": opt.square_avg, "momentum_buffer": opt.momentum_buf, "grad_avg": opt.grad_avg}[key]
    return buf[o:o + p.numel()].view(p.shape)


@pytest.mark.parametrize("form", list(FORMS))
def test_flat_optimiser_state_dict_round_trips_through_the_class(ops, form):
    from core.common.arena import FlatRMSpropTFLike, ParamArena
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    kw = FORMS[form]
    keys = [k for k in STATE if k == "square_avg" or (k == "momentum_buffer" and kw.get("momentum")) or (k == "grad_avg" and kw.get("centered"))]
    ps = new_params()
    arena = ParamArena(ps, DEV)
    opt = FlatRMSpropTFLike(arena, lr=1e-2, **kw)
    assert opt.state_dict()["state"] == {} and opt.step_count == 0 and bool((opt.square_avg == 1).all())
    assert (opt.momentum_buf is not None) == bool(kw.get("momentum")) and (opt.grad_avg is not None) == bool(kw.get("centered"))
    ws = ops.new_ppo_workspace(DEV)
    set_grads(ps, new_grads(0)), opt.step(max_norm=0.5, workspace=ws)
    set_grads(ps, new_grads(1)), opt.step()
    sd = opt.state_dict()
    assert list(sd["param_groups"][0]) == ["lr", "momentum", "alpha", "eps", "centered", "weight_decay", "params"]
    assert sd["param_groups"][0]["params"] == [0, 1, 2] and opt.step_count == 2
    assert all(set(sd["state"][i]) == {"step", *keys} and type(sd["state"][i]["step"]) is int and sd["state"][i]["step"] == 2 for i in range(3))
    # into the class over CPU clones of the parameters ...
    clones = [th.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    topt = RMSpropTFLike(clones, lr=1e-2, **kw)
    topt.load_state_dict(sd)
    for c, p in zip(clones, ps):
        assert set(topt.state[c]) == {"step", *keys} and topt.state[c]["step"] == 2
        for key in keys:
            assert th.equal(topt.state[c][key], flat_state(opt, arena, p, key).cpu()), key
    # ... and back into a fresh flat optimiser, with int and with string keys
    for as_str in (False, True):
        ps2 = new_params()
        arena2 = ParamArena(ps2, DEV)
        with th.no_grad():
            arena2.flat.copy_(arena.flat)
        opt2 = FlatRMSpropTFLike(arena2, lr=5e-3, **kw)
        back = topt.state_dict()
        if as_str:
            back = dict(back, state={str(i): st for i, st in back["state"].items()})
        opt2.load_state_dict(back)
        assert opt2.step_count == 2 and opt2.param_groups[0]["lr"] == 1e-2 and float(opt2.lr_dev) == 1e-2
        for key in keys:
            assert all(th.equal(flat_state(opt2, arena2, q, key), flat_state(opt, arena, p, key)) for p, q in zip(ps, ps2)), key
    # one further step of all three: the flat ones bit for bit, the class within twice the CPU measurement of the NumPy statement
    # against it (tests/test_rmsprop_tf_abi.py CPU_DISTANCE; the magnitudes here are inside those of the measurement)
    g3 = new_grads(2)
    set_grads(ps, g3), set_grads(ps2, g3), set_grads(clones, g3)
    opt.step(), opt2.step(), topt.step()
    assert th.equal(arena.flat, arena2.flat) and opt.step_count == 3
    for c, p in zip(clones, ps):
        st = topt.state[c]
        sq_t, sq_f = st["square_avg"].double(), flat_state(opt, arena, p, "square_avg").cpu().double()
        d = dict(square_avg=float(((sq_t - sq_f).abs() / sq_t).max()), param=float((c.detach() - p.detach().cpu()).abs().max()))
        for key in keys[1:]:
            d[key] = float((st[key] - flat_state(opt, arena, p, key).cpu()).abs().max())
        print(f"FLAT vs class {form} {tuple(p.shape)}: " + ", ".join(f"{k} {v:.3g}" for k, v in d.items()))
        for key, v in d.items():
            assert v <= 2 * CPU_DISTANCE[key], (form, key, v)
        assert float(p.detach().abs().max()) <= 1.6
    with pytest.raises(ValueError, match="Invalid momentum value"):
        FlatRMSpropTFLike(arena2, momentum=-1.0)


def test_flat_optimiser_load_state_dict_refusals(ops):
    from core.common.arena import FlatRMSpropTFLike, ParamArena
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    def class_state(**kw):
        ps = new_params()
        topt = RMSpropTFLike(ps, lr=1e-2, **kw)
        set_grads(ps, new_grads(0)), topt.step()
        return topt.state_dict()

    plain, full = class_state(), class_state(momentum=0.9, centered=True)
    new = lambda **kw: FlatRMSpropTFLike(ParamArena(new_params(), DEV), lr=1e-2, **kw)  # noqa: E731
    for kw, sd, word in ((dict(momentum=0.9), plain, "momentum_buffer"), (dict(centered=True), plain, "grad_avg"),  # a buffer the form needs
                         ({}, full, "does not keep"), (dict(momentum=0.9), full, "grad_avg"), (dict(centered=True), full, "momentum_buffer")):
        opt = new(**kw)
        before = opt.square_avg.clone()
        with pytest.raises(ValueError, match=word):
            opt.load_state_dict(sd)
        assert th.equal(opt.square_avg, before) and opt.step_count == 0  # refused before anything was written
    uneven = class_state()
    uneven["state"][1] = dict(uneven["state"][1], step=5)
    with pytest.raises(ValueError, match="one common step count"):
        new().load_state_dict(uneven)
    ok = new(momentum=0.9, centered=True)
    ok.load_state_dict(full)
    assert ok.step_count == 1 and float(ok.square_avg.min()) < 1.0


# ---- the class against the reference's fixtures ------------------------------------------------------------------------------------
def optimiser_kwargs(g):
    kw = {k.split("/")[1]: float(g[k]) for k in g.files if k.startswith("optimizer_kwargs/")}
    if "centered" in kw:
        kw["centered"] = bool(kw["centered"])
    return kw


def make_model(g, **kw):
    from core.a2c import A2C
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike
    from core.common.vec_env import CSTRVecEnv

    model = A2C("MlpPolicy", CSTRVecEnv(int(g["n_envs"]), device=DEV), seed=int(g["seed"]), n_steps=int(g["n_steps"]),
                learning_rate=float(g["learning_rate"]), ent_coef=float(g["ent_coef"]), device=DEV,
                policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]], optimizer_class=RMSpropTFLike, optimizer_kwargs=optimiser_kwargs(g)), **kw)
    with th.no_grad():
        for k, v in model.policy.state_dict().items():
            v.copy_(th.as_tensor(g[f"before/policy/{k}"]))
    return model


@pytest.mark.parametrize("name,path", [("small", "fused"), ("small", "rocblas"), ("small", "torch"), ("variants", "fused"), ("variants", "torch")])
def test_train_teacher_forced_two_iterations(golden, name, path, monkeypatch):
    """check_step is tests/test_a2c.py's, check_weights unwidened: with square_avg starting at ones avg is about 1, so a gradient error d
    moves a weight by about lr * d, far better conditioned than torch.optim.RMSprop's lr / eps * d whose fixtures keep the same bar."""
    from core.common import fused
    from core.common.arena import FlatRMSpropTFLike
    from core.common.buffers import RolloutBuffer

    g = golden(f"a2c_tflike_train_kat_{name}.npz")
    if path == "rocblas":  # the kernel path with every GEMM left to PyTorch-ROCm / rocBLAS (CSTR_FUSED_LINEAR=0)
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    model = make_model(g)
    opt = model.policy.optimizer
    assert isinstance(opt, FlatRMSpropTFLike) and model.policy.flat_optimizers() == [opt] and model.fused_learner
    assert (opt.momentum_buf is not None, opt.grad_avg is not None) == ((True, True) if name == "variants" else (False, False))
    if path == "torch":
        model.fused_learner = False
    model.debug_capture = True
    total = int(g["iterations"]) * int(g["n_envs"]) * int(g["n_steps"])
    for it in range(int(g["iterations"])):
        model.rollout_buffer = RolloutBuffer.from_arrays(model.observation_space, model.action_space, DEV, gamma=model.gamma,
                                                         gae_lambda=model.gae_lambda, **rollout_arrays(g, "", it))
        model.rollout_buffer.forced_permutations = [g[f"it{it}/permutation"]]
        model._update_current_progress_remaining((it + 1) * int(g["n_envs"]) * int(g["n_steps"]), total)
        model.train()
        assert not model.rollout_buffer.forced_permutations
        check_step(model, g, "", it, path, logger=name == "small")
        # the optimiser state in the class's layout against the reference's, at the bar tests/test_a2c.py sets for square_avg
        sd = opt.state_dict()
        for i, (k, _) in enumerate(model.policy.named_parameters()):
            for key in [key for key in STATE if f"it{it}/opt/{key}/{k}" in g.files]:
                want, got = g[f"it{it}/opt/{key}/{k}"], sd["state"][i][key].cpu().numpy()
                assert float(np.abs(got - want).max()) <= 1e-4 * float(np.abs(want).max()), (it, key, k)
            assert set(sd["state"][i]) == {"step"} | {key for key in STATE if f"it{it}/opt/{key}/{k}" in g.files}


# ---- routing, launch count, checkpoints ------------------------------------------------------------------------------------------
def tf_a2c(env, okw=None, policy_kwargs=None, **kw):
    from core.a2c import A2C
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    pk = dict(policy_kwargs or {}, optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5) if okw is None else okw)
    return A2C("MlpPolicy", env, device=DEV, policy_kwargs=pk, **kw)


def abi_calls_of_one_train(model):
    from core import _native as nv

    model.learn(model.n_envs * model.n_steps)  # one rollout, one train(): buffers and workspaces exist, the buffer is full
    before = nv.ABI_CALLS[0]
    model.train()
    return nv.ABI_CALLS[0] - before


def test_routing_and_launch_count():
    from core.a2c import A2C
    from core.common.arena import FlatRMSprop, FlatRMSpropTFLike
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike
    from core.common.vec_env import CSTRVecEnv
    from core.ppo import PPO
    from core.sac import SAC

    env = CSTRVecEnv(4, device=DEV)
    model = tf_a2c(env, seed=1)
    opt = model.policy.optimizer
    assert isinstance(opt, FlatRMSpropTFLike) and model.fused_learner and opt.param_groups[0]["eps"] == 1e-5 and opt.param_groups[0]["lr"] == 7e-4
    assert model.policy_kwargs["optimizer_class"] is RMSpropTFLike and model.policy_kwargs["optimizer_kwargs"] == dict(eps=1e-5)  # not rewritten
    default = A2C("MlpPolicy", env, seed=1, device=DEV)
    assert isinstance(default.policy.optimizer, FlatRMSprop)
    calls, calls_default = abi_calls_of_one_train(model), abi_calls_of_one_train(default)
    print(f"ABI calls of one train(): RMSpropTFLike {calls}, default {calls_default}")
    assert calls == calls_default and opt.step_count == 2
    for okw in (dict(momentum=0.9), dict(centered=True), dict(weight_decay=1e-4), dict(alpha=0.95, eps=1e-6, momentum=0.5, centered=True, weight_decay=1e-3)):
        other = tf_a2c(env, okw, seed=1)  # every form stays flat, at the same launch count
        assert other.fused_learner and isinstance(other.policy.optimizer, FlatRMSpropTFLike), okw
        assert abi_calls_of_one_train(other) == calls_default, okw
        assert all(bool(th.isfinite(p).all()) for p in other.policy.parameters())
    # a keyword the flat form does not know falls to the class, which refuses it as torch.optim classes do
    with pytest.raises(TypeError, match="foreach"):
        tf_a2c(env, dict(foreach=True))
    # PPO and SAC run the class itself on the arena's parameter views
    ppo = PPO("MlpPolicy", CSTRVecEnv(4, device=DEV), n_steps=8, batch_size=16, n_epochs=1, seed=1, device=DEV,
              policy_kwargs=dict(optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5)))
    assert not ppo.fused_learner and type(ppo.policy.optimizer) is RMSpropTFLike and ppo.policy.flat_optimizers() == []
    ppo.learn(64)
    assert ppo._n_updates == 2 and all(bool(th.isfinite(p).all()) for p in ppo.policy.parameters())
    assert all(type(st["step"]) is int and st["step"] == 4 for st in ppo.policy.optimizer.state.values())
    sac = SAC("MlpPolicy", CSTRVecEnv(4, device=DEV), seed=1, device=DEV, batch_size=16, buffer_size=256, learning_starts=16,
              policy_kwargs=dict(net_arch=[32, 32], optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5)))
    assert type(sac.actor.optimizer) is RMSpropTFLike and type(sac.critic.optimizer) is RMSpropTFLike
    sac.learn(48)
    assert sac._n_updates > 0 and all(bool(th.isfinite(p).all()) for p in sac.policy.parameters())


@pytest.mark.parametrize("okw", [dict(eps=1e-5), dict(eps=1e-5, momentum=0.9, centered=True, weight_decay=1e-3)])
def test_save_load_round_trip(okw, tmp_path):
    import zipfile

    from core.a2c import A2C
    from core.common.arena import FlatRMSpropTFLike
    from core.common.save_util import load_from_zip_file
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike
    from core.common.vec_env import CSTRVecEnv

    model = tf_a2c(CSTRVecEnv(4, device=DEV), okw, seed=2, learning_rate=3e-3)
    model.learn(3 * 4 * 5)
    path = str(tmp_path / "a2c_tflike.zip")
    model.save(path)
    assert {"data", "policy.pth", "policy.optimizer.pth"} <= set(zipfile.ZipFile(path).namelist())
    data, params, _ = load_from_zip_file(path)
    assert data["policy_kwargs"] == dict(optimizer_class=RMSpropTFLike, optimizer_kwargs=okw)
    # policy.optimizer.pth is the class's own state_dict: it loads into the class over the same parameters
    sd = params["policy.optimizer"]
    keys = {"step", "square_avg"} | ({"momentum_buffer", "grad_avg"} if "momentum" in okw else set())
    assert set(sd["state"][0]) == keys and type(sd["state"][0]["step"]) is int and sd["state"][0]["step"] == 3
    clones = [th.nn.Parameter(p.detach().cpu().clone()) for p in model.policy.parameters()]
    topt = RMSpropTFLike(clones, lr=1.0)
    topt.load_state_dict(sd)
    g0 = topt.param_groups[0]
    assert (g0["lr"], g0["eps"], g0["momentum"], g0["centered"]) == (3e-3, 1e-5, okw.get("momentum", 0), okw.get("centered", False))
    loaded = A2C.load(path, env=CSTRVecEnv(4, device=DEV), device=DEV)
    lopt, mopt = loaded.policy.optimizer, model.policy.optimizer
    assert isinstance(lopt, FlatRMSpropTFLike) and loaded.fused_learner and lopt.step_count == mopt.step_count == 3
    assert loaded.policy_kwargs["optimizer_class"] is RMSpropTFLike and loaded.policy_kwargs["optimizer_kwargs"] == okw
    assert {k: lopt.defaults[k] for k in okw} == okw

    def same_state():  # per parameter: the arena's padding between tensors holds no state
        sa, sb = lopt.state_dict()["state"], mopt.state_dict()["state"]
        return len(sa) == len(sb) > 0 and all(set(sa[i]) == set(sb[i]) == keys and sa[i]["step"] == sb[i]["step"] and
                                              all(th.equal(sa[i][k], sb[i][k]) for k in keys - {"step"}) for i in sa)

    assert same_state()
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    # the next train() on the same rollout is bit-identical to the unsaved model's
    loaded.rollout_buffer = model.rollout_buffer
    loaded._current_progress_remaining = model._current_progress_remaining
    model.train(), loaded.train()
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    assert same_state() and lopt.step_count == 4


def test_it_learns_with_the_tf_like_optimiser():
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv

    def score(model):
        env = CSTRVecEnv(8, device=DEV)
        env.seed(1000)
        return evaluate_policy(model, env, n_eval_episodes=8, deterministic=True)[0]

    # The settings and the criterion of tests/test_a2c.py::test_it_learns (300 iterations of 16 steps on 32 envs, lr 1e-3, gae_lambda
    # 0.95, log_std_init -1) with optimizer_class=RMSpropTFLike, eps 1e-5. The reference itself, run on the CPU with these settings
    # (tools/refharness/a2c_tflike_learning.py), improved on all three seeds, but slowly: with square_avg starting at ones the step is
    # about lr * g, not lr * g / |g|: -309.0 -> -306.8 (seed 0), -308.0 -> -307.1 (seed 1), -309.5 -> -307.0 (seed 2).
    model = tf_a2c(CSTRVecEnv(32, device=DEV), policy_kwargs=dict(log_std_init=-1.0), learning_rate=1e-3, n_steps=16, gae_lambda=0.95, seed=0)
    before = score(model)
    model.learn(32 * 16 * 300)
    after = score(model)
    print(f"A2C + RMSpropTFLike evaluate_policy before {before:.1f}, after {after:.1f}")
    assert np.isfinite(after) and after > before
    assert model.fused_learner and model._n_updates == 300 == model.policy.optimizer.step_count
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
