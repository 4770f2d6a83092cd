"""QR-DQN's two entry points (csrc/cstr_qrdqn.hip) on the MI355X against the fp64 restatement of tests/_qrdqn_reference.py on the same
float32 inputs. Bar: the project's kernel-against-fp64 bar (tests/test_tqc_abi.py's), |got - want| <= 2e-6 |want| + 1e-7 max|want| over
the tensor, for gz (dense: the zeros off the taken action must be exact zeros), cur_out, target_out, loss_out, w_mean and b_mean; no
element is excluded (the launches work in float64, the only rounding is the final float32 store). next_index_out must be equal. Each
case prints its worst error / bar before it asserts. Outputs sit behind sentinels (tests/_sentinel_bufs.py): nothing beyond a buffer
is written, everything inside is, and a relaunch gives the same bits."""
import numpy as np
import pytest
import torch as th

import _qrdqn_reference as ref
from _sentinel_bufs import Bufs, SENT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WS_SENT, IDX_SENT = -6.0221407612345e23, -7
# (K, Nq): one atom on the smallest face; a small odd pair; Nq = 64 and 65, either side of one wave; the class defaults (M = 25, Nq =
# 200: four waves of quantiles); the widest face (M = 256 lanes of actions) with few atoms, and with the cap of 256
SHAPES = [(2, 1), (3, 8), (4, 64), (4, 65), (5, 200), (16, 25), (16, 256)]
BATCHES = [1, 3, 65, 257]
SUM0 = 1.5


def _d(a):
    return th.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(th.int32) if t.dtype == th.float32 else t


def _ratio(got, want) -> float:
    """max |got - want| / (2e-6 |want| + 1e-7 max|want|): the bar is 1"""
    got, want = np.asarray(got.cpu().numpy() if isinstance(got, th.Tensor) else got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bar = 2e-6 * np.abs(want) + 1e-7 * float(np.abs(want).max())
    err = np.abs(got - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300))))


def _run(inp, K, leave_out=(), twice=False, pad=0):
    """one call (two with `twice`) into sentinel-padded outputs -> {name: clone}; pad: extra floats behind every row of z, z_next, gz"""
    from core.common import hip_ops

    B, NM = inp["z"].shape
    Nq = NM // (K * K)
    bufs = Bufs()
    gz_wide = bufs.new("gz", B, NM + pad)
    shapes = dict(loss_out=(1,), loss_sum=(1,), cur_out=(B, Nq), target_out=(B, Nq))
    outs = {n: (None if n in leave_out else bufs.new(n, *s)) for n, s in shapes.items()}
    if outs["loss_sum"] is not None:
        outs["loss_sum"].fill_(SUM0)
    idx_all = th.full((B + 8,), IDX_SENT, dtype=th.int64, device=DEV)
    outs["next_index_out"] = None if "next_index_out" in leave_out else idx_all[:B]
    ws_all = th.full((B + 8,), WS_SENT, dtype=th.float64, device=DEV)
    wide = lambda a: _d(np.pad(a, ((0, 0), (0, pad)), constant_values=777.0))[:, :NM]  # noqa: E731
    args = (wide(inp["z"]), wide(inp["z_next"]), _d(inp["valve"]), _d(inp["rew"]), _d(inp["done"]), inp["gamma"], K, Nq)
    for _ in range(2 if twice else 1):
        hip_ops.qrdqn_loss(*args, gz_wide[:, :NM], ws_all[:B], **outs)
    bufs.check(written=[n for n in bufs.flat if n not in ("loss_sum", "gz")])
    assert not bool((gz_wide[:, :NM] == SENT).any()) and bool((gz_wide[:, NM:] == SENT).all())  # the row is written, the gap behind it is not
    assert bool((ws_all[B:] == WS_SENT).all()) and not bool((ws_all[:B] == WS_SENT).any())
    assert bool((idx_all[B:] == IDX_SENT).all()) and ("next_index_out" in leave_out) == bool((idx_all[:B] == IDX_SENT).all())
    got = {n: v.clone() for n, v in outs.items() if v is not None}
    got["gz"] = gz_wide[:, :NM].clone()
    return got


def _check(got, inp, K, label):
    want = ref.loss_step(inp["z"], inp["z_next"], inp["valve"], inp["rew"], inp["done"], inp["gamma"], K)
    B, NM = inp["z"].shape
    M = K * K
    r = dict(gz=_ratio(got["gz"], want["gz"]), cur=_ratio(got["cur_out"], want["cur"]), y=_ratio(got["target_out"], want["y"]),
             loss=_ratio(got["loss_out"], [want["loss"]]))
    line = f"{label}: worst error / bar " + " ".join(f"{n} {v:.3f}" for n, v in r.items())
    print(line)
    assert all(v <= 1.0 for v in r.values()), line
    np.testing.assert_array_equal(got["next_index_out"].cpu().numpy(), want["next_index"], err_msg=label)
    off = np.ones((B, NM // M, M), bool)
    off[np.arange(B), :, inp["index"]] = False
    g = got["gz"].cpu().numpy().reshape(B, NM // M, M)
    assert (g[off] == 0).all() and not np.signbit(g[off]).any(), f"{label}: gz off the taken action is not +0"
    assert float(got["loss_sum"]) == float(np.float32(SUM0) + np.float32(float(got["loss_out"])))  # one float32 addition
    return want


@pytest.mark.parametrize("B", BATCHES)
def test_loss_against_fp64(B):
    for K, Nq in SHAPES:
        if (K, Nq) == (16, 256) and B not in (1, 65):
            continue
        for scale in (1.0, 300.0):
            inp = ref.loss_inputs(B, K, Nq, seed=B * 131 + K * 17 + Nq, scale=scale)
            got = _run(inp, K)
            _check(got, inp, K, f"loss B{B} K{K} Nq{Nq} |z|~{scale:g}")
        again = _run(inp, K)  # a relaunch: the same bits
        assert all(th.equal(_bits(got[n]), _bits(again[n])) for n in got), [n for n in got if not th.equal(_bits(got[n]), _bits(again[n]))]


def test_loss_with_padded_rows():
    """ldz = ldn = Nq * M + 4: the four floats behind every row are neither read (777 there would show) nor written"""
    for B, K, Nq in ((65, 3, 8), (3, 5, 200)):
        inp = ref.loss_inputs(B, K, Nq, seed=11)
        flat, padded = _run(inp, K), _run(inp, K, pad=4)
        _check(padded, inp, K, f"loss padded B{B} K{K} Nq{Nq}")
        assert all(th.equal(_bits(flat[n]), _bits(padded[n])) for n in flat)


@pytest.mark.parametrize("mode", ["random", "done", "edges", "ties"])
def test_loss_input_patterns(mode):
    """every done = 1 (y = r in every slot); delta exactly 0 and exactly +-1 (the Huber branch point and the indicator's); two actions
    tied at the top of the next state's atom sums (the first wins)"""
    for B in (3, 65):
        for K, Nq in SHAPES[:-1]:
            inp = ref.loss_inputs(B, K, Nq, seed=7 + K + Nq, mode=mode)
            got = _run(inp, K)
            want = _check(got, inp, K, f"loss {mode} B{B} K{K} Nq{Nq}")
            if mode == "done":
                assert th.equal(got["target_out"], _d(inp["rew"]).reshape(B, 1).expand(B, Nq))
            if mode == "edges":  # y = r and z = r + {-1, 0, 1}: every Huber term is 0 or 0.5, every derivative 0 or +-1
                np.testing.assert_array_equal(got["target_out"].cpu().numpy().astype(np.float64), want["y"])
                assert set(np.unique(want["y"][:, None, :] - want["cur"][:, :, None])) <= {-1.0, 0.0, 1.0}
            if mode == "ties":
                assert bool((got["next_index_out"] == 1).all())


def test_a_nan_in_a_next_atom_reaches_the_targets_and_the_loss():
    B, K, Nq = 65, 3, 8
    M = K * K
    inp = ref.loss_inputs(B, K, Nq, seed=3)
    zn = inp["z_next"].reshape(B, Nq, M)
    zn[7, 5, 4], inp["done"][7] = np.nan, 0.0  # its sum is a NaN: action 4 is the greedy one, atom 5 of the targets a NaN
    zn[9, 0, 2], inp["done"][9] = np.nan, 1.0  # (1 - done) * gamma = 0, and 0 * NaN is still NaN
    got = _run(inp, K)
    want = ref.loss_step(inp["z"], inp["z_next"], inp["valve"], inp["rew"], inp["done"], inp["gamma"], K)
    idx, y, g = got["next_index_out"].cpu().numpy(), got["target_out"].cpu().numpy(), got["gz"].cpu().numpy().reshape(B, Nq, M)
    assert idx[7] == 4 and idx[9] == 2 and np.array_equal(idx, want["next_index"])
    assert np.isnan(y[7, 5]) and np.isnan(y[9, 0]) and np.isnan(y).sum() == 2 and np.array_equal(np.isnan(y), np.isnan(want["y"]))
    assert np.isnan(float(got["loss_out"])) and np.isnan(want["loss"])
    for b in (7, 9):  # every current atom of the row meets the NaN target
        assert np.isnan(g[b, :, inp["index"][b]]).all()
    assert np.isnan(g).sum() == 2 * Nq
    ok = np.ones(B, bool)
    ok[[7, 9]] = False
    assert _ratio(g[ok].reshape(-1), want["gz_closed"].reshape(B, Nq, M)[ok].reshape(-1)) <= 1.0 and _ratio(y[ok], want["y"][ok]) <= 1.0


def test_loss_sum_form_called_twice_and_optional_outputs_left_out_in_turn():
    inp = ref.loss_inputs(65, 5, 13, seed=5)
    full, twice = _run(inp, 5), _run(inp, 5, twice=True)
    f32 = np.float32
    assert float(twice["loss_sum"]) == float(f32(f32(SUM0) + f32(float(full["loss_out"]))) + f32(float(full["loss_out"])))
    assert all(th.equal(_bits(full[n]), _bits(twice[n])) for n in full if n != "loss_sum")
    everything = ("loss_out", "loss_sum", "cur_out", "target_out", "next_index_out")
    for group in tuple((n,) for n in everything) + (everything,):
        part = _run(inp, 5, leave_out=group)
        assert set(part) == set(full) - set(group)
        assert all(th.equal(_bits(part[n]), _bits(full[n])) for n in part), group


@pytest.mark.parametrize("H", [4, 64, 66])
def test_fold_head_against_fp64(H):
    from core.common import hip_ops

    for K, Nq in SHAPES:
        M = K * K
        rng = np.random.default_rng(K * 1000 + Nq + H)
        for scale in (1.0, 300.0):
            w = np.ascontiguousarray(rng.normal(0.0, 1.0, (Nq * M, H)) * scale + (scale if scale > 1 else 0.0), np.float32)
            b = np.ascontiguousarray(rng.normal(0.0, 1.0, Nq * M) * scale, np.float32)
            bufs = Bufs()
            w_mean, b_mean = bufs.new("w_mean", M, H), bufs.new("b_mean", M)
            wd, bd = _d(w), _d(b)
            hip_ops.qrdqn_fold_head(wd, bd, M, w_mean, b_mean)
            bufs.check(written=("w_mean", "b_mean"))
            snap = bufs.snapshot()
            want_w, want_b = ref.folded_head(w, b, Nq, M)
            r = dict(w_mean=_ratio(w_mean, want_w), b_mean=_ratio(b_mean, want_b))
            line = f"fold K{K} Nq{Nq} H{H} |w|~{scale:g}: worst error / bar " + " ".join(f"{n} {v:.3f}" for n, v in r.items())
            print(line)
            assert all(v <= 1.0 for v in r.values()), line
            hip_ops.qrdqn_fold_head(wd, bd, M, w_mean, b_mean)
            bufs.check(written=("w_mean", "b_mean"))
            bufs.same_as(snap)
    # no cap on the atom count: 300 atoms, beyond the loss launch's 256
    w, b = np.ascontiguousarray(rng.normal(size=(300 * 9, H)), np.float32), np.ascontiguousarray(rng.normal(size=300 * 9), np.float32)
    w_mean, b_mean = th.zeros(9, H, device=DEV), th.zeros(9, device=DEV)
    hip_ops.qrdqn_fold_head(_d(w), _d(b), 9, w_mean, b_mean)
    want_w, want_b = ref.folded_head(w, b, 300, 9)
    assert _ratio(w_mean, want_w) <= 1.0 and _ratio(b_mean, want_b) <= 1.0


def test_supported_limits_and_bad_arguments():
    from core import _native as nv
    from core.common import hip_ops

    sup = hip_ops.qrdqn_supported
    assert sup(4, 2, 1) and sup(9, 3, 8) and sup(25, 5, 200) and sup(256, 16, 256)
    # just beyond each limit: atoms, levels, a face that is no square
    assert not sup(4, 2, 0) and not sup(4, 2, 257) and not sup(1, 1, 8) and not sup(289, 17, 8) and not sup(10, 3, 8)
    z = lambda *s: th.zeros(*s, device=DEV)  # noqa: E731
    ok = lambda: dict(z=z(8, 72), z_next=z(8, 72), valve=z(8, 2), reward=z(8, 1), done=z(8, 1), gamma=0.99, levels=3, n_quantiles=8,  # noqa: E731
                      gz=z(8, 72), ws=th.zeros(8, dtype=th.float64, device=DEV))
    hip_ops.qrdqn_loss(**ok())
    for key, bad, msg in (("z_next", z(8, 71), "z_next"), ("gz", z(9, 72), "gz"), ("gz", z(8, 80)[:, :72], "row stride"), ("z", z(8, 72).cpu(), "z"),
                          ("z", z(8, 144)[:, ::2], "z"), ("valve", z(8, 3), "valve"), ("reward", z(7), "reward"), ("done", z(8).double(), "done"),
                          ("ws", z(8), "ws"), ("ws", th.zeros(9, dtype=th.float64, device=DEV), "ws"), ("n_quantiles", 7, "columns"),
                          ("levels", 4, "columns")):
        kw = ok()
        kw[key] = bad
        with pytest.raises(ValueError, match=msg):
            hip_ops.qrdqn_loss(**kw)
    for name, bad in (("cur_out", z(8, 7)), ("target_out", z(9, 8)), ("loss_out", z(2))):
        with pytest.raises(ValueError, match=name):
            hip_ops.qrdqn_loss(**ok(), **{name: bad})
    with pytest.raises(ValueError, match="next_index_out"):
        hip_ops.qrdqn_loss(**ok(), next_index_out=th.zeros(8, dtype=th.int32, device=DEV))
    for kw in (dict(gamma=-0.5), dict(gamma=float("nan")), dict(valve=z(17)[1:].view(8, 2))):  # the last: a valve pair off its 8-byte boundary
        with pytest.raises(nv.NativeError, match="bad argument"):
            hip_ops.qrdqn_loss(**dict(ok(), **kw))
    big = dict(ok(), z=z(8, 257 * 9), z_next=z(8, 257 * 9), gz=z(8, 257 * 9), n_quantiles=257)
    with pytest.raises(nv.NativeError, match="unsupported"):
        hip_ops.qrdqn_loss(**big)
    same = ok()
    same["gz"] = same["z"]  # an output on an input
    with pytest.raises(nv.NativeError, match="bad argument"):
        hip_ops.qrdqn_loss(**same)
    fok = lambda: dict(weight=z(72, 16), bias=z(72), n_actions=9, w_mean=z(9, 16), b_mean=z(9))  # noqa: E731
    hip_ops.qrdqn_fold_head(**fok())
    for key, bad, msg in (("weight", z(70, 16), "weight"), ("bias", z(71), "bias"), ("w_mean", z(9, 15), "w_mean"), ("b_mean", z(8), "b_mean"),
                          ("weight", z(72, 32)[:, ::2], "weight"), ("n_actions", 0, "weight")):
        kw = fok()
        kw[key] = bad
        with pytest.raises(ValueError, match=msg):
            hip_ops.qrdqn_fold_head(**kw)
    head = z(72 + 9, 16)
    with pytest.raises(nv.NativeError, match="bad argument"):
        hip_ops.qrdqn_fold_head(**dict(fok(), weight=head[:72], w_mean=head[63:72]))  # the folded head on the rows it is folded from
    th.cuda.synchronize()
