"""Host-side checks of the prioritized-replay ABI (no GPU): the exported symbols, the tree layout of a capacity, and the refusals every
entry point makes before it enqueues anything."""
import ctypes as C

import pytest

PER_SYMBOLS = ("cstr_per_tree_layout", "cstr_per_rebuild_f64", "cstr_per_add_f64", "cstr_per_sample_f32", "cstr_per_update_f64",
               "cstr_dqn_loss_weighted_f32")
BADARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def nv():
    from core import _native

    _native.lib()
    return _native


def layout(nv, capacity):
    t = nv.PerTree()
    rc = nv.lib().cstr_per_tree_layout(C.c_int64(capacity), C.byref(t))
    return rc, t


def test_symbols_and_constants(nv):
    lib = nv.lib()
    assert all(s in nv.SYMBOLS and hasattr(lib, s) for s in PER_SYMBOLS) and lib.cstr_abi_version() == 5  # additive
    assert (nv.PER_MAX_LEVELS, nv.PER_CTL_WORDS, nv.PER_MAX_BATCH, nv.PER_MAX_CAPACITY) == (6, 8, 1024, 1 << 30)


@pytest.mark.parametrize("capacity,counts", [(1, [1, 1]), (15, [15, 1]), (64, [64, 1]), (65, [65, 2, 1]), (4160, [4160, 65, 2, 1]),
                                             (1 << 20, [1 << 20, 1 << 14, 256, 4, 1]), (1 << 30, [1 << 30, 1 << 24, 1 << 18, 4096, 64, 1])])
def test_layout(nv, capacity, counts):
    rc, t = layout(nv, capacity)
    assert rc == 0 and t.n_levels == len(counts) and list(t.count)[:t.n_levels] == counts
    offsets, off = [], 0
    for n in counts:  # every level starts behind the previous one padded to a multiple of 64
        offsets.append(off)
        off += -(-n // 64) * 64
    assert list(t.offset)[:t.n_levels] == offsets and t.words == off


def test_refusals_come_before_any_launch(nv):
    lib = nv.lib()
    assert layout(nv, 0)[0] == BADARG and layout(nv, (1 << 30) + 1)[0] == UNSUPPORTED
    _, t = layout(nv, 65)
    buf = (C.c_double * 512)()  # host memory: every call below must return before it would touch it
    p = C.cast(buf, C.c_void_p)
    assert lib.cstr_per_rebuild_f64(C.byref(t), None) == BADARG  # node is NULL
    t.node = p.value
    bent = nv.PerTree.from_buffer_copy(t)
    bent.offset[1] = 64  # not the layout of its capacity
    assert lib.cstr_per_rebuild_f64(C.byref(bent), None) == BADARG
    ctl = C.c_void_p(p.value + 3072)
    assert lib.cstr_per_add_f64(C.byref(t), ctl, C.c_int64(5), C.c_int64(12), ctl, C.c_double(0.6), None) == BADARG  # 5 * 12 != 65
    assert lib.cstr_per_add_f64(C.byref(t), ctl, C.c_int64(5), C.c_int64(13), C.c_void_p(p.value + 3200), C.c_double(-0.1), None) == BADARG
    idx, td = C.c_void_p(p.value + 3328), C.c_void_p(p.value + 3584)
    upd = lambda b, alpha, minp, ctl_=ctl: lib.cstr_per_update_f64(C.byref(t), ctl_, idx, td, C.c_int64(b), C.c_double(alpha),  # noqa: E731
                                                                   C.c_double(minp), None)
    assert upd(1025, 0.6, 1e-6) == UNSUPPORTED and upd(0, 0.6, 1e-6) == BADARG and upd(8, 0.6, 0.0) == BADARG
    assert upd(8, float("nan"), 1e-6) == BADARG and upd(8, 0.6, 1e-6, C.c_void_p(p.value + 8)) == BADARG  # per_ctl inside the tree
    assert lib.cstr_dqn_loss_weighted_f32(p, C.c_int64(4), p, C.c_int64(4), p, p, p, None, C.c_float(0.99), C.c_int64(2), C.c_int(4), C.c_int(2),
                                          p, p, None, None, None, p, p, None) == BADARG  # no weights


def test_buffer_argument_checks():
    from core.common.buffers import PrioritizedReplayBuffer
    from core.common.spaces import Box

    spaces = (Box(-1, 1, (4,)), Box(-1, 1, (2,)))
    for kw in (dict(alpha=-0.1), dict(beta=1.5), dict(beta=-0.1), dict(final_beta=2.0), dict(min_priority=0.0)):
        with pytest.raises(ValueError):
            PrioritizedReplayBuffer(64, *spaces, device="cpu", **kw)
