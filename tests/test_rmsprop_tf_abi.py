"""CPU-side checks of RMSpropTFLike: the public class (core.common.sb2_compat.rmsprop_tf_like, the reference's module path) has the
reference's constructor, messages, `__setstate__` defaults and state keys and reproduces three steps of the unmodified reference's
class in six forms (tests/golden/rmsprop_tf_kat.npz, tools/refharness/gen_golden.py --only rmsprop_tf); the NumPy float32 statement of
the step that csrc/cstr_a2c.hip follows (kept here, imported by tests/test_rmsprop_tf.py) is compared with the class on the CPU;
cstr_rmsprop_tf_f32 is exported and rejects bad arguments on the host (nothing is dereferenced or launched)."""
import ctypes as C
import inspect
import pickle

import numpy as np
import pytest
import torch as th

from core import _native as nv
from test_a2c_abi import BAD, P, f32, f64, i64, null, off

FORMS = {"plain": {}, "a2c": dict(eps=1e-5), "momentum": dict(momentum=0.9), "centered": dict(centered=True),
         "centered_momentum": dict(centered=True, momentum=0.9), "weight_decay": dict(weight_decay=1e-2)}
STATE = ("square_avg", "momentum_buffer", "grad_avg")

# The NumPy statement against the class on the CPU (test_numpy_statement_against_the_class_on_the_cpu): the worst distance over the six
# forms and three steps, measured on the CPU of the development machine with torch 2.10 before the assertion was written; twice these
# figures are asserted, there and wherever a flat kernel step is compared with a step of the class (tests/test_rmsprop_tf.py).
# square_avg relative; weights (|w| <= 1.6), momentum_buffer (|buf| <= 2.8) and grad_avg (|ga| <= 0.03) absolute.
# Measured: square_avg 6.14e-8 (half an ulp of a value near one) in every form; weights 1.19e-7 (one ulp at |w| > 1) with momentum, 0
# without; momentum_buffer 1.19e-7; grad_avg 1.86e-9.
CPU_DISTANCE = dict(square_avg=6.14e-8, param=1.19e-7, momentum_buffer=1.19e-7, grad_avg=1.86e-9)


def rmsprop_tf_numpy(param, grad, square_avg, momentum_buf, grad_avg, lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0,
                     centered=False, coef=np.float32(1.0)):
    """RMSpropTFLike's step with every operation rounded to float32, in the order of include/cstr_rl_hip.h (cstr_rmsprop_tf_f32).
    Returns (param, clipped grad, square_avg, momentum_buf, grad_avg); the two optional arrays pass through as None. lr / alpha / eps /
    weight_decay / momentum are Python floats, coef a float32."""
    one = np.float32
    assert param.dtype == grad.dtype == square_avg.dtype == np.float32
    assert (momentum_buf is not None) == (momentum > 0) and (grad_avg is not None) == bool(centered)
    with np.errstate(invalid="ignore"):
        g = grad * one(coef)
        gd = g + one(weight_decay) * param if weight_decay != 0 else g
        sq = square_avg * one(alpha) + (one(1.0 - alpha) * gd) * gd
        if centered:
            grad_avg = grad_avg * one(alpha) + one(1.0 - alpha) * gd
            avg = np.sqrt((sq - grad_avg * grad_avg) + one(eps))
        else:
            avg = np.sqrt(sq + one(eps))
        if momentum > 0:
            momentum_buf = momentum_buf * one(momentum) + gd / avg
            param = param + one(-lr) * momentum_buf
        else:
            param = param + (one(-lr) * gd) / avg
    return param, g, sq, momentum_buf, grad_avg


def new_state(n, kw):
    """(square_avg = ones, momentum_buf or None, grad_avg or None) of a form"""
    return (np.ones(n, np.float32), np.zeros(n, np.float32) if kw.get("momentum", 0) > 0 else None,
            np.zeros(n, np.float32) if kw.get("centered") else None)


def test_import_path_signature_and_messages():
    import core.common.sb2_compat as pkg
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    assert pkg.RMSpropTFLike is RMSpropTFLike and issubclass(RMSpropTFLike, th.optim.Optimizer)
    assert (RMSpropTFLike.__module__, RMSpropTFLike.__qualname__) == ("core.common.sb2_compat.rmsprop_tf_like", "RMSpropTFLike")
    assert pickle.loads(pickle.dumps(dict(optimizer_class=RMSpropTFLike)))["optimizer_class"] is RMSpropTFLike
    sig = inspect.signature(RMSpropTFLike.__init__).parameters
    assert list(sig) == ["self", "params", "lr", "alpha", "eps", "weight_decay", "momentum", "centered"]
    assert {k: sig[k].default for k in list(sig)[2:]} == dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False)
    assert list(inspect.signature(RMSpropTFLike.step).parameters) == ["self", "closure"]
    p = [th.nn.Parameter(th.zeros(3))]
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate: -1.0"), (dict(eps=-1e-3), "Invalid epsilon value: -0.001"),
                    (dict(momentum=-0.5), "Invalid momentum value: -0.5"), (dict(weight_decay=-2.0), "Invalid weight_decay value: -2.0"),
                    (dict(alpha=-0.1), "Invalid alpha value: -0.1")):
        with pytest.raises(ValueError) as e:
            RMSpropTFLike(p, **kw)
        assert str(e.value) == msg
    opt = RMSpropTFLike(p)
    assert opt.defaults == dict(lr=1e-2, momentum=0, alpha=0.99, eps=1e-8, centered=False, weight_decay=0)
    state = opt.__getstate__()
    for g in state["param_groups"]:
        del g["momentum"], g["centered"]
    opt.__setstate__(state)
    assert opt.param_groups[0]["momentum"] == 0 and opt.param_groups[0]["centered"] is False


def test_state_keys_ones_and_the_sparse_refusal():
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    for form, kw in FORMS.items():
        p, q = th.nn.Parameter(th.full((2, 3), 0.5)), th.nn.Parameter(th.zeros(4))  # q never gets a gradient
        opt = RMSpropTFLike([p, q], lr=0.0, **kw)  # lr 0: the parameter stays, the state moves
        p.grad = th.zeros(2, 3)
        assert opt.step() is None and opt.step(lambda: 1.25) == 1.25
        st = opt.state[p]
        want = {"step", "square_avg"} | ({"momentum_buffer"} if kw.get("momentum") else set()) | ({"grad_avg"} if kw.get("centered") else set())
        assert set(st) == want and type(st["step"]) is int and st["step"] == 2 and q not in opt.state, form
        if form != "weight_decay":  # a zero gradient: ones * alpha * alpha, so the average started at ones
            np.testing.assert_array_equal(st["square_avg"].numpy(), np.full((2, 3), np.float32(1.0) * np.float32(0.99) * np.float32(0.99)))
        assert th.equal(p.detach(), th.full((2, 3), 0.5))
        assert list(opt.state_dict()["param_groups"][0]) == ["lr", "momentum", "alpha", "eps", "centered", "weight_decay", "params"]
    p = th.nn.Parameter(th.zeros(4))
    p.grad = th.zeros(4).to_sparse()
    with pytest.raises(RuntimeError, match="RMSpropTF does not support sparse gradients"):
        RMSpropTFLike([p]).step()


@pytest.mark.parametrize("form", list(FORMS))
def test_class_reproduces_the_reference_fixture(golden, form):
    """Within 2 ulp of every f32 value after each of three steps (the class issues the reference's ATen calls: bit-equal on the same
    torch build)."""
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    g = golden("rmsprop_tf_kat.npz")
    assert [str(f) for f in g["forms"]] == list(FORMS) and g["sizes"].tolist() == [257, 1024] and int(g["steps"]) == 3
    kw = FORMS[form]
    for key in ("lr", "alpha", "eps", "weight_decay", "momentum"):
        assert float(g[f"{form}/{key}"]) == dict(dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0), **kw)[key]
    assert bool(g[f"{form}/centered"]) == bool(kw.get("centered", False))
    ps = [th.nn.Parameter(th.tensor(g[f"param0/w{i}"])) for i in range(2)]
    opt = RMSpropTFLike(ps, **kw)
    for k in range(3):
        for i, p in enumerate(ps):
            p.grad = th.tensor(g[f"grad{k}/w{i}"])
        opt.step()
        for i, p in enumerate(ps):
            st = opt.state[p]
            assert st["step"] == k + 1
            for key, got in [("param", p.detach())] + [(key, st[key]) for key in STATE if key in st]:
                want = g[f"{form}/step{k}/{key}/w{i}"]
                ulps = float(np.max(np.abs(got.numpy().astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)))
                print(f"KAT {form} step {k} {key}/w{i}: {ulps:.2f} ulp")
                assert ulps <= 2.0, (form, k, key, i, ulps)
            assert all((key in st) == (f"{form}/step{k}/{key}/w{i}" in g.files) for key in STATE)
    assert float(np.abs(ps[1].detach().numpy() - g["param0/w1"]).max()) > 1e-3  # the steps moved the weights


def statement_case(n=100_000, seed=0):
    rng = np.random.default_rng(seed)
    w0 = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    grads = [(10.0 ** rng.uniform(-8, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(3)]
    return w0, grads


def distances(state_np, p, st):
    """{tensor: distance} of the NumPy statement's state from the class's, in CPU_DISTANCE's measures"""
    w, sq, buf, ga = state_np
    want_sq = st["square_avg"].numpy().reshape(-1)
    d = dict(square_avg=float(np.max(np.abs(sq - want_sq) / want_sq)), param=float(np.max(np.abs(w - p.detach().numpy().reshape(-1)))))
    if buf is not None:
        d["momentum_buffer"] = float(np.max(np.abs(buf - st["momentum_buffer"].numpy().reshape(-1))))
    if ga is not None:
        d["grad_avg"] = float(np.max(np.abs(ga - st["grad_avg"].numpy().reshape(-1))))
    return d


@pytest.mark.parametrize("form", list(FORMS))
def test_numpy_statement_against_the_class_on_the_cpu(form):
    """Three steps on 1e5 elements, gradients spanning 1e-8 .. 1. The float32 statement is not bit-equal to ATen's CPU kernels, which
    contract differently (a vectorised add(alpha=) may fuse where the statement rounds twice); CPU_DISTANCE holds what was measured,
    twice that is asserted per state tensor."""
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    kw, lr = FORMS[form], 7e-4
    w0, grads = statement_case()
    p = th.nn.Parameter(th.tensor(w0))
    opt = RMSpropTFLike([p], lr=lr, **kw)
    w = w0.copy()
    sq, buf, ga = new_state(w.size, kw)
    for k, g in enumerate(grads):
        p.grad = th.tensor(g)
        opt.step()
        w, _, sq, buf, ga = rmsprop_tf_numpy(w, g, sq, buf, ga, lr, **kw)
        d = distances((w, sq, buf, ga), p, opt.state[p])
        print(f"RMSpropTFLike NumPy vs ATen {form} step {k}: " + ", ".join(f"{key} {v:.3g}" for key, v in d.items()))
        for key, v in d.items():
            assert v <= 2 * CPU_DISTANCE[key], (form, k, key, v)
    assert float(np.abs(w - w0).max()) > 1e-4 and float(np.abs(w).max()) <= 1.6
    if buf is not None:
        assert float(np.abs(buf).max()) <= 2.8
    if ga is not None:
        assert float(np.abs(ga).max()) <= 0.03


def test_symbol_exported_and_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    assert "cstr_rmsprop_tf_f32" in nv.SYMBOLS and hasattr(lib, "cstr_rmsprop_tf_f32") and lib.cstr_abi_version() == 5  # additive

    def step(param=P(0), grad=P(1), sq=P(2), buf=null, ga=null, lr=P(5), alpha=0.99, eps=1e-5, wd=0.0, mom=0.0, mx=0.5, ws=P(6), out=null,
             n=1000):
        return lib.cstr_rmsprop_tf_f32(param, grad, sq, buf, ga, lr, f64(alpha), f64(eps), f64(wd), f64(mom), f32(mx), ws, out, i64(n), null)

    full = dict(buf=P(3), ga=P(4), mom=0.9)  # the centred form with momentum: all five arenas
    assert step(param=null) == BAD and step(grad=null) == BAD and step(sq=null) == BAD and step(lr=null) == BAD
    assert step(n=0) == BAD and step(n=-1) == BAD and step(n=0, **full) == BAD
    for name, k in (("param", 0), ("grad", 1), ("sq", 2), ("buf", 3), ("ga", 4)):  # float4 accesses: 16-byte alignment of every arena
        assert step(**dict(full, **{name: off(P(k), 4)})) == BAD and step(**dict(full, **{name: off(P(k), 8)})) == BAD, name
    names = ("param", "grad", "sq", "buf", "ga")
    for a in range(5):  # any two of the five arenas overlapping: the same address, and the last 16 bytes of the other
        for b in range(5):
            if a != b:
                assert step(**dict(full, **{names[a]: P(b)})) == BAD, (names[a], names[b])
                assert step(**dict(full, **{names[a]: off(P(b), 4000 - 16)})) == BAD, (names[a], names[b])
    assert step(ga=P(0)) == BAD and step(ga=P(2)) == BAD                       # ... in the centred form without momentum as well
    assert step(alpha=-0.1) == BAD and step(eps=-1.0) == BAD and step(wd=-1e-2) == BAD and step(mom=-0.9, buf=P(3)) == BAD
    assert step(alpha=float("nan")) == BAD and step(eps=float("nan")) == BAD and step(wd=float("nan")) == BAD
    assert step(mom=float("nan"), buf=P(3)) == BAD and step(mx=float("nan")) == BAD
    assert step(buf=P(3), mom=0.0) == BAD                                        # a momentum buffer without momentum ...
    assert step(buf=null, mom=0.9) == BAD                                        # ... and momentum without its buffer
    assert step(mx=0.5, ws=null) == BAD and step(mx=0.5, ws=null, **full) == BAD  # the clip needs the workspace ...
    assert step(mx=0.0, ws=null, param=null) == BAD                              # ... the unclipped step does not, but validates the rest
    assert step(mx=0.0, ws=null, n=0, **full) == BAD
    assert step(ws=off(P(6), 4)) == BAD and step(lr=off(P(5), 4)) == BAD and step(out=off(P(7), 2)) == BAD
    for k in range(5):  # the workspace, norm_out or lr over an arena
        assert step(ws=P(k), **full) == BAD and step(out=P(k), **full) == BAD and step(lr=P(k), **full) == BAD, k
    assert step(out=P(6)) == BAD and step(lr=P(6)) == BAD


def test_hip_ops_wrapper_and_routing_on_the_host():
    from core.common import arena, hip_ops
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    z = th.zeros(8)
    with pytest.raises(ValueError, match="No CPU fallback|device"):
        hip_ops.rmsprop_tf(z, z.clone(), z.clone(), th.zeros(1, dtype=th.float64))
    sig = inspect.signature(arena.FlatRMSpropTFLike.__init__).parameters
    assert list(sig) == ["self", "arena", "lr", "alpha", "eps", "weight_decay", "momentum", "centered"]
    step = inspect.signature(arena.FlatRMSpropTFLike.step).parameters
    assert [step[k].default for k in ("closure", "max_norm", "workspace", "norm_out")] == [None] * 4
    for name in ("zero_grad", "sync_lr", "step", "step_count", "state_dict", "load_state_dict"):
        assert hasattr(arena.FlatRMSpropTFLike, name), name
    assert arena.RMSpropTFLike is RMSpropTFLike


def test_a2c_leaves_the_callers_optimiser_class_alone():
    from core.a2c import A2C
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike
    from test_a2c_abi import make_policy

    own = dict(optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5))
    assert A2C._rewrite_policy_kwargs(dict(own), True, 1e-5) == own and A2C._rewrite_policy_kwargs(dict(own), False, 1e-5) == own
    pol = make_policy(**own)
    assert pol.optimizer_class is RMSpropTFLike and pol.optimizer_kwargs == dict(eps=1e-5)


def test_the_class_in_policy_kwargs_is_stored_by_name():
    """`data` is JSON, nothing is pickled: the class goes in as its name and comes back through a table of known names"""
    import json

    from core.common.save_util import data_to_json, json_to_data
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    pk = dict(net_arch=[32, 32], optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5, momentum=0.9, centered=True))
    text = data_to_json(dict(policy_kwargs=pk, n_steps=5))
    assert json.loads(text)["policy_kwargs"]["optimizer_class"] == {":class:": "core.common.sb2_compat.rmsprop_tf_like.RMSpropTFLike"}
    assert json_to_data(text) == dict(policy_kwargs=pk, n_steps=5)
    assert "policy_kwargs" not in json.loads(data_to_json(dict(policy_kwargs=dict(optimizer_class=th.optim.SGD))))  # as before: skipped
    for name in ("os.system", "torch.optim.rmsprop.RMSprop"):  # a name outside the table is an error, never an import
        with pytest.raises(ValueError, match="not one of"):
            json_to_data(json.dumps(dict(policy_kwargs=dict(optimizer_class={":class:": name}))))


def test_fixtures_hold_what_the_gpu_tests_rely_on(golden):
    import os

    from conftest import GOLDEN

    for name, extra in (("small", set()), ("variants", {"momentum_buffer", "grad_avg"})):
        g = golden(f"a2c_tflike_train_kat_{name}.npz")
        assert int(g["iterations"]) == 2 and str(g["optimizer"]) == "RMSpropTFLike" and float(g["optimizer_kwargs/eps"]) == 1e-5
        assert (int(g["n_envs"]), int(g["n_steps"]), float(g["learning_rate"]), float(g["ent_coef"])) == (4, 5, 3e-3, 0.01)
        for k in range(2):
            assert float(g[f"it{k}/grad_norm"]) > float(g["max_grad_norm"]) == 0.5  # the clip is engaged in both steps
            assert int(g[f"it{k}/timeouts"].sum()) >= 1 and int(g[f"it{k}/optimizer_steps"]) == k + 1 == int(g[f"it{k}/n_updates"])
            assert {key.split("/")[2] for key in g.files if key.startswith(f"it{k}/opt/")} == {"square_avg"} | extra
        assert float(g["it0/opt/square_avg/log_std"].min()) > 0.9  # started at ones
        assert os.path.getsize(os.path.join(GOLDEN, f"a2c_tflike_train_kat_{name}.npz")) < 100 * 1024
    v = golden("a2c_tflike_train_kat_variants.npz")
    assert float(v["optimizer_kwargs/momentum"]) == 0.9 and float(v["optimizer_kwargs/centered"]) == 1.0
    assert sorted(golden("a2c_tflike_train_kat_small.npz").files) == sorted(
        list(golden("a2c_train_kat_small.npz").files) + ["optimizer_kwargs/eps"])  # the layout of a2c_train_kat_small.npz
    assert os.path.getsize(os.path.join(GOLDEN, "rmsprop_tf_kat.npz")) < 300 * 1024
