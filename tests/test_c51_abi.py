"""C51's entry points (csrc/cstr_c51.hip) and construction, host side: exports, the support table, every refusal before a launch.
CPU only: the calls run on fake addresses that are never dereferenced, since each one is refused on the host."""
import ctypes as C

import pytest

BAD, UNS = -1, -2
NAMES = ("h", "w", "bias", "q", "z", "z_next", "valve", "reward", "done", "gz", "loss_out", "m_out", "next_index_out", "ws")
ADDR = {n: 0x10000000 + i * 0x1000000 for i, n in enumerate(NAMES)}


def _head(**kw):
    from core import _native as nv

    a = dict(ADDR, n=8, ldh=8, ldq=4, m=4, levels=2, atoms=5, hid=8, v_min=-10.0, v_max=10.0)
    a.update(kw)
    v, i64 = C.c_void_p, C.c_int64
    return nv.lib().cstr_c51_head_q_f32(v(a["h"]), i64(a["ldh"]), v(a["w"]), v(a["bias"]), i64(a["n"]), C.c_int(a["m"]), C.c_int(a["levels"]),
                                        C.c_int(a["atoms"]), i64(a["hid"]), C.c_double(a["v_min"]), C.c_double(a["v_max"]), v(a["q"]),
                                        i64(a["ldq"]), v(None))


def _loss(**kw):
    from core import _native as nv

    a = dict(ADDR, batch=8, ldz=20, ldn=20, m=4, levels=2, atoms=5, gamma=0.99, v_min=-10.0, v_max=10.0)
    a.update(kw)
    v, i64 = C.c_void_p, C.c_int64
    return nv.lib().cstr_c51_loss_f32(v(a["z"]), i64(a["ldz"]), v(a["z_next"]), i64(a["ldn"]), v(a["valve"]), v(a["reward"]), v(a["done"]),
                                      C.c_double(a["gamma"]), C.c_double(a["v_min"]), C.c_double(a["v_max"]), i64(a["batch"]), C.c_int(a["m"]),
                                      C.c_int(a["levels"]), C.c_int(a["atoms"]), v(a["gz"]), v(a["loss_out"]), v(None), v(a["m_out"]), v(None),
                                      v(a["next_index_out"]), v(None), v(a["ws"]), v(None))


def test_exports_and_support_table():
    import core
    from core import _native as nv
    from core.common import hip_ops

    for sym in ("cstr_c51_supported", "cstr_c51_head_q_f32", "cstr_c51_loss_f32"):
        assert sym in nv.SYMBOLS and hasattr(nv.lib(), sym)
    ok = hip_ops.c51_supported
    assert [ok(4, 2, n) for n in (1, 2, 256, 257)] == [False, True, True, False]
    assert [ok(4, 2, 51, h) for h in (0, 4, 6, 512, 516)] == [False, True, False, True, False]
    assert [ok(k * k, k, 51) for k in (1, 2, 16, 17)] == [False, True, True, False] and not ok(10, 3, 51)
    assert core.C51 is core.c51.C51 and "C51" in core.__all__


INF, NAN = float("inf"), float("nan")
SUPPORT = [dict(v_max=-10.0), dict(v_min=10.0), dict(v_max=INF), dict(v_min=-INF), dict(v_min=NAN)]


@pytest.mark.parametrize("kw,rc", [(dict(**{n: 0}), BAD) for n in ("h", "w", "bias", "q")] + [(k, BAD) for k in SUPPORT] + [
    (dict(n=0), BAD), (dict(hid=0), BAD), (dict(atoms=0), BAD), (dict(ldh=7), BAD), (dict(ldq=3), BAD),
    (dict(h=ADDR["h"] + 2), BAD), (dict(w=ADDR["w"] + 8), BAD), (dict(q=ADDR["w"] + 64), BAD),  # off 4 / 16 bytes; q on an input
    (dict(atoms=1), UNS), (dict(atoms=257), UNS), (dict(hid=6, ldh=6), UNS), (dict(hid=516, ldh=516), UNS), (dict(m=5, ldq=5), UNS),
    (dict(n=(1 << 30) + 1), UNS)])
def test_head_refusals_before_any_launch(kw, rc):
    assert _head(**kw) == rc


@pytest.mark.parametrize("kw,rc", [(dict(**{n: 0}), BAD) for n in ("z", "z_next", "valve", "reward", "done", "gz", "ws")] + [(k, BAD) for k in SUPPORT] + [
    (dict(batch=0), BAD), (dict(atoms=0), BAD), (dict(ldz=19), BAD), (dict(ldn=19), BAD), (dict(gamma=-0.5), BAD), (dict(gamma=NAN), BAD),
    (dict(ws=ADDR["ws"] + 4), BAD), (dict(next_index_out=ADDR["next_index_out"] + 4), BAD), (dict(valve=ADDR["valve"] + 4), BAD),
    (dict(gz=ADDR["z"]), BAD), (dict(m_out=ADDR["loss_out"]), BAD),  # an output on an input; two outputs on each other
    (dict(atoms=1, ldz=4, ldn=4), UNS), (dict(atoms=257, ldz=1028, ldn=1028), UNS), (dict(m=5, ldz=25, ldn=25), UNS),
    (dict(batch=16385), UNS)])
def test_loss_refusals_before_any_launch(kw, rc):
    assert _loss(**kw) == rc


@pytest.mark.parametrize("kw,match", [(dict(policy_kwargs=dict(n_atoms=1)), "n_atoms"), (dict(v_min=1.0, v_max=1.0), "v_min"),
                                      (dict(v_max=INF), "v_min")])
def test_construction_refusals(kw, match):
    import core

    with pytest.raises(ValueError, match=match):
        core.C51("MlpPolicy", None, **kw)
