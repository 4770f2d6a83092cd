"""The guarded buffers of the kernel-level GPU tests (tests/_sentinel_bufs.py: GuardedBufs) on the CPU: every one of its checks
fires on the fault it is there for, for every element type, and `misalign` places the payload where it says."""
import numpy as np
import pytest
import torch as th

from _sentinel_bufs import PAD, SENTINELS, GuardedBufs

DTYPES = [th.float32, th.float64, th.int32, th.int64, "uint64"]


def _bufs(dtype, misalign=0):
    b = GuardedBufs("cpu")
    out = b.new("out", 5, 3, dtype=dtype, misalign=misalign)
    cols = b.new_cols("cols", 4, 9, 2, 3, dtype=dtype, misalign=misalign)
    ro = b.put_ro("ro", np.arange(7), dtype=dtype, misalign=misalign)
    out.fill_(1)
    cols.fill_(2)
    return b, out, cols, ro


def _block(b, name):
    return b.bufs[name][0]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_clean_launch_passes(dtype):
    b, out, cols, ro = _bufs(dtype)
    b.check(written=("out", "cols"))
    snap = b.snapshot()
    b.same_as(snap)
    assert ro.tolist() == list(range(7)) and tuple(cols.shape) == (4, 3) and cols.stride(0) == 9


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", ["out", "cols", "ro"])
def test_a_write_in_front_of_the_payload_is_seen(dtype, name):
    b, *_ = _bufs(dtype)
    f, mask, _ = b.bufs[name]
    first = int(mask.nonzero()[0])
    assert first >= PAD
    for at in (first - 1, first - PAD):  # the nearest and the farthest element of the front band
        f[at] = 0
        with pytest.raises(AssertionError, match="in front of"):
            b.check()
        f[at] = SENTINELS[f.dtype]
    b.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", ["out", "cols", "ro"])
def test_a_write_behind_the_payload_is_seen(dtype, name):
    b, *_ = _bufs(dtype)
    f, mask, _ = b.bufs[name]
    last = int(mask.nonzero()[-1]) + 1
    assert f.numel() - last >= PAD
    for at in (last, last + PAD - 1):
        f[at] = 0
        with pytest.raises(AssertionError, match="behind"):
            b.check()
        f[at] = SENTINELS[f.dtype]
    b.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_write_to_a_gap_column_is_seen(dtype):
    b, _, cols, _ = _bufs(dtype)
    whole = cols.as_strided((4, 9), (9, 1), cols.storage_offset() - 2)
    for r, c in ((0, 5), (1, 1), (2, 8), (3, 0)):  # right behind the block, right in front of it, the row's last and first column
        whole[r, c] = 0
        with pytest.raises(AssertionError, match="gap column"):
            b.check()
        whole[r, c] = SENTINELS[whole.dtype]
    b.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_tail_overrun_inside_a_pack_is_seen(dtype):
    b = GuardedBufs("cpu")
    a0, a1, a2 = b.new_pack("arenas", [5, 1, 7], dtype=dtype)
    assert a0.data_ptr() % 16 == 0 and a1.data_ptr() % 16 == 0 and a2.data_ptr() % 16 == 0
    for a in (a0, a1, a2):
        a.fill_(1)
    b.check(written=("arenas",))
    f = _block(b, "arenas")
    first = b.span["arenas"][0]
    for at in (first + 5, first + 5 + PAD - 1):  # right behind the first arena, right in front of the second
        f[at] = 0
        with pytest.raises(AssertionError, match="between two arenas"):
            b.check()
        f[at] = SENTINELS[f.dtype]
    a1[0] = SENTINELS[f.dtype]
    with pytest.raises(AssertionError, match="elements left unwritten"):
        b.check(written=("arenas",))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_changed_read_only_input_is_seen(dtype):
    b, _, _, ro = _bufs(dtype)
    ro[3] = 99
    with pytest.raises(AssertionError, match="read-only"):
        b.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_unwritten_output_element_is_seen(dtype):
    b = GuardedBufs("cpu")
    out, cols = b.new("out", 5, 3, dtype=dtype), b.new_cols("cols", 4, 9, 2, 3, dtype=dtype)
    out.fill_(1)
    cols.fill_(1)
    b.check(written=("out", "cols"))
    out[4, 2] = SENTINELS[out.dtype]
    with pytest.raises(AssertionError, match="out: elements left unwritten"):
        b.check(written=("out", "cols"))
    out.fill_(1)
    cols[3, 2] = SENTINELS[out.dtype]
    with pytest.raises(AssertionError, match="cols: elements left unwritten"):
        b.check(written=("out", "cols"))
    b.check(written=("out",))  # only the named outputs are asked


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_differing_second_launch_is_seen(dtype):
    b, out, cols, _ = _bufs(dtype)
    snap = b.snapshot()
    out[0, 0] = 3
    with pytest.raises(AssertionError, match="out: the second launch differs"):
        b.same_as(snap)
    b.same_as(snap, skip=("out",))
    cols[1, 1] = 3
    with pytest.raises(AssertionError, match="cols: the second launch differs"):
        b.same_as(snap, skip=("out",))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5])
def test_misalign_places_the_payload(dtype, k):
    b = GuardedBufs("cpu")
    item = 8 if dtype == "uint64" else th.empty((), dtype=dtype).element_size()
    t = b.new("t", 6, dtype=dtype, misalign=k)
    c = b.new_cols("c", 3, 8, 4, 2, dtype=dtype, misalign=k)
    r = b.put_ro("r", np.arange(4), dtype=dtype, misalign=k)
    assert t.data_ptr() % 256 == k * item and r.data_ptr() % 256 == k * item
    assert c.data_ptr() % 256 == (k + 4) * item  # the block starts k elements behind the boundary, the payload 4 columns further
    assert t.data_ptr() % 16 == (k * item) % 16
    if item == 4:  # float32 / int32: k = 1 is 4-byte but neither 8- nor 16-byte aligned, k = 2 is 8-byte but not 16-byte aligned
        assert {1: (4, 4), 2: (8, 0), 3: (12, 4), 4: (0, 0)}.get(k, (t.data_ptr() % 16, t.data_ptr() % 8)) == (t.data_ptr() % 16, t.data_ptr() % 8)
    t.fill_(1)
    c.fill_(1)
    b.check(written=("t", "c"))
    f, mask, _ = b.bufs["t"]  # the bands moved with the payload
    first = int(mask.nonzero()[0])
    assert first >= PAD and f.numel() - (first + 6) >= PAD and f[first:first + 6].data_ptr() == t.data_ptr()
