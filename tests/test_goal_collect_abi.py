"""CPU-side checks of the goal face's fused collect step (cstr_goal_collect_step_f32, csrc/cstr_her.hip): the symbol is exported, every
argument the entry point refuses is refused on the host (fake, never dereferenced device addresses: nothing is launched),
`hip_ops.goal_collect_step` refuses CPU tensors, and `HerReplayBuffer.note_fused_add` is the host bookkeeping of a fused add."""
import ctypes as C

import numpy as np
import pytest

from core import _native as nv

i64, f32, u64 = C.c_int64, C.c_float, C.c_uint64
null = C.c_void_p(None)
BAD, UNSUP = -1, -2
ROWS, N = 12, 64


def P(k: int) -> C.c_void_p:
    """the k-th of a set of fake, well separated, 256-byte-aligned device addresses (never dereferenced)"""
    return C.c_void_p(0x1000000 * (k + 1))


def off(p: C.c_void_p, nbytes: int) -> C.c_void_p:
    return C.c_void_p(p.value + nbytes)


def ring(obs=P(20), nxt=P(21), act=P(22), rew=P(23), done=P(24), tout=P(25), rows=ROWS, n=N, d=4, a=2):
    return nv.Ring(obs.value, nxt.value, act.value, rew.value, done.value, tout.value, rows, n, d, a)


def her(goal=P(30), start=P(31), length=P(32), cur=P(33), valid=P(34), bits=P(35)):
    return nv.Her(goal.value, start.value, length.value, cur.value, valid.value, bits.value)


def collect(coef=None, integ=0, d=4, r=None, h=None, ctl=P(40), obs=P(0), rows=P(1), st=P(2), pcg=P(3), init=null, tgt=P(4), ep=null,
            glo=0.1, ghi=0.4, pol=P(5), squashed=1, lo=(-1.0, -1.0), hi=(1.0, 1.0), noise=null, rew=P(7), done=P(8), tout=P(9), nxt=P(10),
            ret=P(11), stats=P(12), rng=null, adv=0):
    coef = C.byref(nv.default_coef()) if coef is None else coef
    r = C.byref(ring()) if r is None else (null if r is null else C.byref(r))
    h = C.byref(her()) if h is None else (null if h is null else C.byref(h))
    lo = null if lo is None else (f32 * 2)(*lo)
    hi = null if hi is None else (f32 * 2)(*hi)
    return nv.lib().cstr_goal_collect_step_f32(coef, integ, d, r, h, ctl, obs, rows, st, pcg, init, tgt, ep, u64(0), i64(0), f32(glo), f32(ghi), pol,
                                               squashed, lo, hi, noise, rew, done, tout, nxt, ret, stats, rng, u64(adv), null)


def test_symbol_declared_and_exported():
    lib = nv.lib()
    assert "cstr_goal_collect_step_f32" in nv.SYMBOLS and hasattr(lib, "cstr_goal_collect_step_f32")
    assert lib.cstr_abi_version() == 5  # additive


def test_null_required_pointers():
    """Each case changes ONE argument of a well-formed call (which is never sent: it would launch)."""
    for name in ("coef", "ctl", "obs", "rows", "st", "pcg", "tgt", "pol"):
        assert collect(**{name: null}) == BAD, name
    assert collect(r=null) == BAD and collect(h=null) == BAD
    assert collect(lo=None) == BAD and collect(hi=None) == BAD
    for name in ("obs", "nxt", "act", "rew", "done", "tout"):
        assert collect(r=ring(**{name: null})) == BAD, name
    for name in ("goal", "start", "length", "cur", "valid", "bits"):
        assert collect(h=her(**{name: null})) == BAD, name


def test_sizes_and_shapes():
    assert collect(r=ring(n=0)) == BAD and collect(r=ring(n=-3)) == BAD and collect(r=ring(rows=0)) == BAD
    assert collect(r=ring(d=8)) == UNSUP and collect(r=ring(d=8, a=4)) == UNSUP and collect(r=ring(d=6)) == UNSUP and collect(r=ring(a=4)) == UNSUP
    assert collect(d=8) == UNSUP and collect(d=6) == UNSUP
    assert collect(squashed=2) == UNSUP and collect(squashed=3) == UNSUP  # bit 1: the multi-agent action chain
    assert collect(integ=2) == UNSUP and collect(integ=-1) == UNSUP
    assert collect(r=ring(rows=nv.HER_MAX_ROWS + 1)) == UNSUP and collect(r=ring(n=nv.HER_MAX_ENVS + 1, rows=1)) == UNSUP
    assert collect(r=ring(rows=8192, n=1 << 18)) == UNSUP  # 2^31 transitions
    assert collect(lo=(1.0, -1.0), hi=(1.0, 1.0)) == BAD and collect(lo=(-1.0, 2.0), hi=(1.0, 1.0)) == BAD  # empty action interval
    assert collect(ep=P(13), glo=0.4, ghi=0.1) == BAD


def test_statistics_go_together():
    assert collect(ret=null) == BAD and collect(stats=null) == BAD


def test_misaligned_rows():
    assert collect(obs=off(P(0), 8)) == BAD and collect(rows=off(P(1), 4)) == BAD and collect(pol=off(P(5), 4)) == BAD
    assert collect(noise=off(P(6), 4)) == BAD and collect(pcg=off(P(3), 8)) == BAD and collect(nxt=off(P(10), 4)) == BAD
    assert collect(st=off(P(2), 2)) == BAD and collect(tgt=off(P(4), 2)) == BAD and collect(ep=off(P(13), 2)) == BAD
    assert collect(rew=off(P(7), 2)) == BAD and collect(done=off(P(8), 2)) == BAD and collect(tout=off(P(9), 2)) == BAD
    assert collect(ret=off(P(11), 2)) == BAD and collect(stats=off(P(12), 4)) == BAD and collect(ctl=off(P(40), 4)) == BAD
    assert collect(init=off(P(14), 4)) == BAD and collect(rng=off(P(15), 4)) == BAD
    assert collect(r=ring(obs=off(P(20), 8))) == BAD and collect(r=ring(act=off(P(22), 4))) == BAD and collect(h=her(bits=off(P(35), 4))) == BAD
    assert collect(h=her(start=off(P(31), 2))) == BAD


def test_overlaps():
    # an output on an input, on the env state or on the flat rows
    assert collect(rew=P(5)) == BAD and collect(done=off(P(5), 8 * (N - 1))) == BAD and collect(nxt=P(0)) == BAD and collect(nxt=off(P(1), 24 * 3)) == BAD
    assert collect(tout=P(2)) == BAD and collect(ret=P(4)) == BAD and collect(rew=off(P(3), 32 * N - 4)) == BAD
    assert collect(noise=P(6), rew=off(P(6), 8)) == BAD
    # the env state on the flat rows
    assert collect(rows=off(P(0), 16 * 32)) == BAD
    # outputs on each other
    assert collect(done=P(7)) == BAD and collect(tout=P(8)) == BAD and collect(ret=P(9)) == BAD and collect(rew=off(P(10), 24)) == BAD
    assert collect(stats=off(P(11), 4 * N - 8)) == BAD
    # the ring and the side arrays on the rows, the state and the outputs
    assert collect(rows=off(P(20), 16 * 5)) == BAD and collect(nxt=off(P(21), 16 * 35)) == BAD and collect(pol=off(P(22), 8)) == BAD
    assert collect(rew=P(23)) == BAD and collect(obs=off(P(30), 64)) == BAD and collect(done=off(P(32), 4 * ROWS * N - 4)) == BAD
    assert collect(tout=P(33)) == BAD and collect(ret=P(34)) == BAD and collect(stats=P(35)) == BAD
    # the control words
    assert collect(rng=P(40)) == BAD and collect(rng=off(P(12), 16)) == BAD and collect(ctl=off(P(12), 0)) == BAD


def test_hip_ops_refuses_cpu_tensors():
    import torch as th

    from core.common import hip_ops

    class Fake:
        n_envs, rows = 3, 4

    n = 3
    z = lambda *s, dt=th.float32: th.zeros(*s, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="must live in HBM"):
        hip_ops.goal_collect_step(nv.default_coef(), "euler", Fake(), Fake(), z(n, 4), z(n, 6), z(n, dt=th.int32), z(n, 4, dt=th.int64), z(n),
                                  z(n, 2), 1, [-1, -1], [1, 1])
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        hip_ops.goal_collect_step(nv.default_coef(), "euler", Fake(), Fake(), np.zeros((n, 4), np.float32), z(n, 6), z(n, dt=th.int32),
                                  z(n, 4, dt=th.int64), z(n), z(n, 2), 1, [-1, -1], [1, 1])


def test_note_fused_add_counts():
    """`note_fused_add` is `add_device`'s host bookkeeping without the launch: `_adds`, and `pos` / `full` through it."""
    from core.her import HerReplayBuffer

    rb = HerReplayBuffer.__new__(HerReplayBuffer)  # no device memory: the bookkeeping is host state
    rb.buffer_size, rb._adds = 3, 0
    seen = []
    for _ in range(7):
        rb.note_fused_add()
        seen.append((rb._adds, rb.pos, rb.full))
    assert seen == [(1, 1, False), (2, 2, False), (3, 0, True), (4, 1, True), (5, 2, True), (6, 0, True), (7, 1, True)]
