"""TQC's two loss launches (csrc/cstr_tqc.hip) on the MI355X against the fp64 restatement of tests/_tqc_reference.py on the same
float32 inputs. Bar: the project's kernel-against-fp64 bar, |got - want| <= 2e-6 |want| + 1e-7 max|want| over the tensor, for gz,
target_out, gz_pi, g_logp, z_pi_mean and every scalar; no element is excluded (the launches work in float64, the only rounding is the
final float32 store). Each case prints its worst error / bar before it asserts. Outputs sit behind sentinels (tests/_sentinel_bufs.py):
nothing beyond a buffer is written, everything inside is, and a relaunch gives the same bits."""
import numpy as np
import pytest
import torch as th

import _tqc_reference as ref
from _sentinel_bufs import Bufs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 12345.678
# (G, Nq, k): one atom; the class defaults; nothing dropped; all but one atom per critic dropped; five critics (M = 125); odd sizes;
# M = 256, the cap; M = 64 and 65, either side of one wave
CASES = [(1, 1, 0), (2, 25, 2), (2, 25, 0), (2, 25, 24), (5, 25, 2), (3, 13, 1), (16, 16, 3), (2, 32, 1), (5, 13, 1)]
BATCHES = [1, 3, 65, 255, 256, 257]


def _d(a):
    return th.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(th.int32)


def _ratio(got, want) -> float:
    """max |got - want| / (2e-6 |want| + 1e-7 max|want|): the bar is 1"""
    got, want = np.asarray(got.cpu().numpy() if isinstance(got, th.Tensor) else got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bar = 2e-6 * np.abs(want) + 1e-7 * float(np.abs(want).max())
    err = np.abs(got - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300))))


SUM0, MSUM0 = 1.5, (-2.5, 0.25)


def _run_critic(inp, k, leave_out=(), alpha=False, twice=False):
    """one launch (two with `twice`) into sentinel-padded outputs -> {name: clone}"""
    from core.common import hip_ops

    G, B, Nq = inp["z"].shape
    shapes = dict(gz=(G, B, Nq), loss_out=(1,), loss_sum=(1,), target_out=(B, ref.n_keep(G, Nq, k)), means_out=(2,), means_sum=(2,))
    bufs = Bufs()
    outs = {n: (None if n in leave_out else bufs.new(n, *s)) for n, s in shapes.items()}
    if outs["loss_sum"] is not None:
        outs["loss_sum"].fill_(SUM0)
    if outs["means_sum"] is not None:
        outs["means_sum"].copy_(th.tensor(MSUM0, device=DEV))
    ws_all = th.full((3 * B + 8,), SENT, dtype=th.float64, device=DEV)
    part, ent_coef = None, _d([inp["alpha"]])
    if alpha:
        part = dict(log_alpha=_d([inp["log_alpha"]]), logp_pi=_d(inp["logp"]), target_entropy=inp["target_entropy"], grad_out=bufs.new("a_grad", 1),
                    ent_coef_out=bufs.new("a_ent_coef", 1), loss_out=bufs.new("a_loss", 1), loss_sum=bufs.put("a_loss_sum", [SUM0]),
                    ent_coef_sum=bufs.put("a_ent_coef_sum", [SUM0]))
        ent_coef = None
    args = (_d(inp["z"]), _d(inp["z_next"]), _d(inp["next_logp"]), _d(inp["rew"]), _d(inp["done"]), ent_coef, inp["gamma"], k)
    gz = outs.pop("gz")
    for _ in range(2 if twice else 1):
        hip_ops.tqc_critic_loss(*args, gz, ws_all[:3 * B], alpha=part, **outs)
    outs["gz"] = gz
    sums = ("loss_sum", "means_sum", "a_loss_sum", "a_ent_coef_sum")
    bufs.check(written=[n for n in bufs.flat if n not in sums])
    assert bool((ws_all[3 * B:] == SENT).all()) and not bool((ws_all[:3 * B] == SENT).any())
    got = {n: v.clone() for n, v in outs.items() if v is not None}
    if alpha:
        got.update({n: part[n].clone() for n in ("grad_out", "ent_coef_out")}, a_loss=part["loss_out"].clone(), a_loss_sum=part["loss_sum"].clone(),
                   a_ent_coef_sum=part["ent_coef_sum"].clone())
    return got


def _check_critic(got, inp, k, label, alpha_value=None):
    a = inp["alpha"] if alpha_value is None else alpha_value
    want = ref.critic_loss(inp["z"], inp["z_next"], inp["next_logp"], inp["rew"], inp["done"], a, inp["gamma"], k)
    r = dict(gz=_ratio(got["gz"], want["gz"]), y=_ratio(got["target_out"], want["y"]), loss=_ratio(got["loss_out"], [want["loss"]]),
             target_mean=_ratio(got["means_out"][0:1], [want["target_mean"]]), atom_mean=_ratio(got["means_out"][1:2], [want["atom_mean"]]))
    line = f"{label}: worst error / bar " + " ".join(f"{n} {v:.3f}" for n, v in r.items())
    print(line)
    assert all(v <= 1.0 for v in r.values()), line
    assert bool((got["target_out"][:, 1:] >= got["target_out"][:, :-1]).all()), f"{label}: target_out is not ascending"
    f32 = np.float32
    assert float(got["loss_sum"]) == float(f32(SUM0) + f32(float(got["loss_out"])))  # one float32 addition
    for i in range(2):
        assert float(got["means_sum"][i]) == float(f32(MSUM0[i]) + f32(float(got["means_out"][i])))
    return want


@pytest.mark.parametrize("B", BATCHES)
def test_critic_loss_against_fp64(B):
    for G, Nq, k in CASES:
        # both atom sizes; where the fp64 reference holds B * M * n_keep > 1e7 terms (M = 256 at the three large batches), one of them
        for scale in ((1.0, 300.0) if B * G * Nq < 30000 else (300.0,) if B % 2 else (1.0,)):
            inp = ref.loss_inputs(B, G, Nq, seed=B * 131 + G * 17 + Nq + k, scale=scale)
            got = _run_critic(inp, k)
            _check_critic(got, inp, k, f"critic B{B} G{G} Nq{Nq} k{k} |z|~{scale:g}")
        again = _run_critic(inp, k)  # a relaunch: the same bits
        assert all(th.equal(_bits(got[n]), _bits(again[n])) for n in got), [n for n in got if not th.equal(_bits(got[n]), _bits(again[n]))]


@pytest.mark.parametrize("mode", ["done", "ties", "edges"])
def test_critic_loss_input_patterns(mode):
    """every done = 1 (y = r in every slot); every target atom tied at least G-fold (exactly n_keep kept: target_out is fully written and
    equals the sorted row's head); delta exactly 0 and exactly +-1 (the Huber branch point and the indicator's)"""
    for B in (3, 65):
        for G, Nq, k in CASES:
            inp = ref.loss_inputs(B, G, Nq, seed=7 + G + Nq, scale=1.0, mode=mode)
            got = _run_critic(inp, k)
            want = _check_critic(got, inp, k, f"critic {mode} B{B} G{G} Nq{Nq} k{k}")
            if mode == "done":
                assert th.equal(got["target_out"], _d(inp["rew"]).reshape(B, 1).expand(B, ref.n_keep(G, Nq, k)))
            if mode == "edges":  # y = r and z = r + {-1, 0, 1}: every Huber term is 0 or 0.5, every derivative 0 or +-1
                np.testing.assert_array_equal(got["target_out"].cpu().numpy().astype(np.float64), want["y"])
                delta = want["y"][:, None, None, :] - inp["z"].astype(np.float64).transpose(1, 0, 2)[:, :, :, None]
                assert set(np.unique(delta)) <= {-1.0, 0.0, 1.0}


def test_critic_loss_sum_form_called_twice_and_the_alpha_part():
    for G, Nq, k in ((2, 25, 2), (5, 13, 1)):
        inp = ref.loss_inputs(65, G, Nq, seed=3)
        once, twice = _run_critic(inp, k), _run_critic(inp, k, twice=True)
        f32 = np.float32
        assert float(twice["loss_sum"]) == float(f32(f32(SUM0) + f32(float(once["loss_out"]))) + f32(float(once["loss_out"])))
        assert all(th.equal(_bits(once[n]), _bits(twice[n])) for n in ("gz", "loss_out", "target_out", "means_out"))
        # SAC's entropy-coefficient part riding along: alpha = exp(log_alpha) feeds the targets
        got = _run_critic(inp, k, alpha=True)
        ap = ref.alpha_part(inp["log_alpha"], inp["logp"], inp["target_entropy"])
        _check_critic(got, inp, k, f"critic with the alpha part G{G} Nq{Nq} k{k}", alpha_value=ap["ent_coef"])
        r = dict(grad=_ratio(got["grad_out"], [ap["grad"]]), ent_coef=_ratio(got["ent_coef_out"], [ap["ent_coef"]]), loss=_ratio(got["a_loss"], [ap["loss"]]))
        print("alpha part: worst error / bar " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), r
        assert float(got["a_loss_sum"]) == float(f32(SUM0) + f32(float(got["a_loss"])))
        assert float(got["a_ent_coef_sum"]) == float(f32(SUM0) + f32(float(got["ent_coef_out"])))


def test_critic_optional_outputs_left_out_in_turn():
    inp = ref.loss_inputs(65, 3, 13, seed=5)
    full = _run_critic(inp, 1)
    for group in (("loss_out",), ("loss_sum",), ("target_out",), ("means_out",), ("means_sum",), ("loss_out", "loss_sum", "target_out", "means_out", "means_sum")):
        part = _run_critic(inp, 1, leave_out=group)
        assert set(part) == set(full) - set(group)
        assert all(th.equal(_bits(part[n]), _bits(full[n])) for n in part), group


def _run_actor(inp, leave_out=(), twice=False):
    from core.common import hip_ops

    G, B, Nq = inp["z_pi"].shape
    shapes = dict(gz_pi=(G, B, Nq), g_logp=(B,), loss_out=(1,), loss_sum=(1,), z_pi_mean=(B,))
    bufs = Bufs()
    outs = {n: (None if n in leave_out else bufs.new(n, *s)) for n, s in shapes.items()}
    if outs["loss_sum"] is not None:
        outs["loss_sum"].fill_(SUM0)
    for _ in range(2 if twice else 1):
        hip_ops.tqc_actor_loss(_d(inp["z_pi"]), _d(inp["logp"]), _d([inp["alpha"]]), **outs)
    bufs.check(written=[n for n in outs if outs[n] is not None and n != "loss_sum"])
    return {n: v.clone() for n, v in outs.items() if v is not None}


@pytest.mark.parametrize("B", BATCHES)
def test_actor_loss_against_fp64(B):
    for G, Nq, _ in CASES:
        for scale in (1.0, 300.0):
            inp = ref.loss_inputs(B, G, Nq, seed=B * 7 + G + Nq, scale=scale)
            got = _run_actor(inp)
            want = ref.actor_loss(inp["z_pi"], inp["logp"], inp["alpha"])
            r = {n: _ratio(got[n], want[n]) for n in ("gz_pi", "g_logp", "z_pi_mean")}
            r["loss"] = _ratio(got["loss_out"], [want["loss"]])
            line = f"actor B{B} G{G} Nq{Nq} |z|~{scale:g}: worst error / bar " + " ".join(f"{n} {v:.3f}" for n, v in r.items())
            print(line)
            assert all(v <= 1.0 for v in r.values()), line
            assert float(got["loss_sum"]) == float(np.float32(SUM0) + np.float32(float(got["loss_out"])))
        again = _run_actor(inp)
        assert all(th.equal(_bits(got[n]), _bits(again[n])) for n in got)
    twice = _run_actor(inp, twice=True)
    assert float(twice["loss_sum"]) == float(np.float32(np.float32(SUM0) + np.float32(float(got["loss_out"]))) + np.float32(float(got["loss_out"])))
    for group in (("loss_out",), ("loss_sum",), ("z_pi_mean",), ("loss_out", "loss_sum", "z_pi_mean")):
        part = _run_actor(inp, leave_out=group)
        assert set(part) == set(got) - set(group) and all(th.equal(_bits(part[n]), _bits(got[n])) for n in part), group


def test_supported_limits_and_bad_arguments():
    from core import _native as nv
    from core.common import hip_ops

    sup = hip_ops.tqc_supported
    assert sup(1, 1, 0) and sup(2, 25, 2) and sup(16, 16, 3) and sup(16, 16, 15) and sup(2, 128, 0)
    # just beyond each limit: critics, atoms, drops
    assert not sup(0, 25, 0) and not sup(17, 15, 0) and not sup(16, 17, 0) and not sup(2, 129, 0) and not sup(2, 25, 25) and not sup(2, 25, -1)
    z = lambda *s: th.zeros(*s, device=DEV)  # noqa: E731
    ok = lambda: dict(z=z(2, 8, 25), z_next=z(2, 8, 25), next_logp=z(8), rew=z(8, 1), done=z(8, 1), ent_coef=z(1), gamma=0.99, drop_per_net=2,  # noqa: E731
                      gz=z(2, 8, 25), ws=th.zeros(24, dtype=th.float64, device=DEV))
    hip_ops.tqc_critic_loss(**ok())
    for key, bad, msg in (("z_next", z(2, 8, 24), "z_next"), ("gz", z(2, 9, 25), "gz"), ("z", z(2, 8, 25).cpu(), "z"), ("z", z(2, 8, 50)[:, :, ::2], "z"),
                          ("next_logp", z(7), "next_logp"), ("rew", z(8).double(), "rew"), ("ws", z(24), "ws"), ("ws", th.zeros(23, dtype=th.float64, device=DEV), "ws"),
                          ("ent_coef", None, "ent_coef"), ("ent_coef", z(2), "ent_coef")):
        kw = ok()
        kw[key] = bad
        with pytest.raises(ValueError, match=msg):
            hip_ops.tqc_critic_loss(**kw)
    with pytest.raises(ValueError, match="target_out"):
        hip_ops.tqc_critic_loss(**ok(), target_out=z(8, 50))  # n_keep is 46
    for kw in (dict(drop_per_net=25), dict(drop_per_net=-1), dict(gamma=-0.5)):
        with pytest.raises(nv.NativeError, match="bad argument"):
            hip_ops.tqc_critic_loss(**dict(ok(), **kw))
    big = dict(ok(), z=z(2, 8, 129), z_next=z(2, 8, 129), gz=z(2, 8, 129))
    with pytest.raises(nv.NativeError, match="unsupported"):
        hip_ops.tqc_critic_loss(**big)
    same = ok()
    same["gz"] = same["z"]  # an output on an input
    with pytest.raises(nv.NativeError, match="bad argument"):
        hip_ops.tqc_critic_loss(**same)
    aok = lambda: dict(z_pi=z(2, 8, 25), logp=z(8), ent_coef=z(1), gz_pi=z(2, 8, 25), g_logp=z(8))  # noqa: E731
    hip_ops.tqc_actor_loss(**aok())
    for key, bad, msg in (("gz_pi", z(2, 8, 24), "gz_pi"), ("logp", z(9), "logp"), ("g_logp", z(8, 2)[:, 0], "g_logp"), ("ent_coef", z(2), "ent_coef")):
        kw = aok()
        kw[key] = bad
        with pytest.raises(ValueError, match=msg):
            hip_ops.tqc_actor_loss(**kw)
    with pytest.raises(nv.NativeError, match="unsupported"):
        hip_ops.tqc_actor_loss(**dict(aok(), z_pi=z(17, 8, 2), gz_pi=z(17, 8, 2)))
    th.cuda.synchronize()
