"""The LSTM sequence entry points and RecurrentPPO's construction, host side: exports, every refusal before a launch. CPU only."""
import ctypes as C

import numpy as np
import pytest

BAD, UNS = -1, -2
R, S, K, H = 8, 2, 4, 16


def _call(which="fwd", **kw):
    """cstr_lstm_seq_fwd_f32 / _bwd_f32 on disjoint fake addresses (never dereferenced: every call here is refused on the host)"""
    from core import _native as nv

    seg = np.ascontiguousarray(kw.pop("seg", [(0, 3, 0), (3, 5, 1)]), dtype=np.int32)
    a = dict(rows=R, state_rows=S, n_seg=len(seg), k=K, h=H)
    names = ("x", "es", "w_ih", "w_hh", "b_ih", "b_hh", "sh", "sc", "segd", "out", "hn", "cn", "gates", "cseq", "hprev", "dout", "dgates", "dh0", "dc0")
    p = {n: 0x10000000 + i * 0x1000000 for i, n in enumerate(names)}
    a.update(p)
    a.update(kw)
    v, i64 = C.c_void_p, C.c_int64
    segh = seg.ctypes.data_as(v) if a.get("segh", 1) else v(None)
    if which == "fwd":
        return nv.lib().cstr_lstm_seq_fwd_f32(v(a["x"]), v(a["es"]), i64(a["rows"]), v(a["w_ih"]), v(a["w_hh"]), v(a["b_ih"]), v(a["b_hh"]), v(a["sh"]),
                                              v(a["sc"]), i64(a["state_rows"]), segh, v(a["segd"]), i64(a["n_seg"]), v(a["out"]), v(a["hn"]), v(a["cn"]),
                                              v(a["gates"]), v(a["cseq"]), v(a["hprev"]), i64(a["k"]), i64(a["h"]), C.c_int(0), v(None))
    return nv.lib().cstr_lstm_seq_bwd_f32(v(a["dout"]), v(a["gates"]), v(a["cseq"]), v(a["sc"]), i64(a["state_rows"]), v(a["es"]), i64(a["rows"]),
                                          v(a["w_hh"]), segh, v(a["segd"]), i64(a["n_seg"]), v(a["dgates"]), v(a["dh0"]), v(a["dc0"]), i64(a["h"]),
                                          C.c_int(0), v(None))


def test_exports_and_support_table():
    from core import _native as nv
    from core.common import hip_ops

    for sym in ("cstr_lstm_supported", "cstr_lstm_resident", "cstr_lstm_seq_fwd_f32", "cstr_lstm_seq_bwd_f32"):
        assert sym in nv.SYMBOLS and hasattr(nv.lib(), sym)
    ok = hip_ops.lstm_supported
    assert ok(4, 16) and ok(7, 256) and not ok(4, 24) and not ok(4, 272) and not ok(0, 16) and not ok(4, 0)
    res = hip_ops.lstm_resident  # weight_hh beside the tiles in 160 KB: the forward up to H = 80, the backward up to H = 96
    assert res(4, 80) and not res(4, 96) and res(4, 96, True) and not res(4, 112, True) and not res(4, 24)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_refusals_before_any_launch(which):
    assert _call(which, h=24) == UNS and _call(which, h=272) == UNS and _call(which, h=0) == BAD
    required = ("x", "es", "w_ih", "w_hh", "b_ih", "b_hh", "sh", "sc", "segd", "hn", "cn") if which == "fwd" else (
        "dout", "gates", "cseq", "sc", "es", "w_hh", "segd", "dgates", "dh0", "dc0")
    for name in required:
        assert _call(which, **{name: 0}) == BAD, name
    assert _call(which, segh=0) == BAD and _call(which, rows=0) == BAD and _call(which, n_seg=0) == BAD and _call(which, state_rows=0) == BAD
    out = "hn" if which == "fwd" else "dh0"
    assert _call(which, **{out: 0x10000000 + 5 * 0x1000000 if which == "fwd" else 0x10000000 + 3 * 0x1000000}) == BAD  # an output on an input
    assert _call(which, **{out: 0x10000002}) == BAD                                                                 # off a 4-byte boundary
    assert _call(which, **({"cn": 0x10000000 + 10 * 0x1000000 + 4} if which == "fwd" else {"dc0": 0x10000000 + 17 * 0x1000000 + 4})) == BAD  # two outputs
    for seg in ([(0, 3, 0), (3, 6, 1)], [(0, 0, 0)], [(-1, 2, 0)], [(0, 3, 2)], [(0, 3, -1)], [(3, 5, 0), (0, 3, 1)], [(0, 4, 0), (3, 5, 1)]):
        assert _call(which, seg=seg) == BAD, seg  # leaves the rows, empty, negative, state row outside, out of order, a shared row
    if which == "fwd":
        assert _call(k=0) == BAD and _call(k=257) == UNS
        assert _call(gates=0) == BAD and _call(out=0) == BAD                              # part of the training-mode outputs
        assert _call(w_hh=0x10000000 + 3 * 0x1000000 + 4) == BAD                          # weight_hh off its 16-byte boundary


def test_construction_refusals():
    import core

    with pytest.raises(ValueError, match="n_lstm_layers"):
        core.RecurrentPPO("MlpLstmPolicy", None, policy_kwargs=dict(n_lstm_layers=2))
    with pytest.raises(ValueError, match="gSDE"):
        core.RecurrentPPO("MlpLstmPolicy", None, use_sde=True)
