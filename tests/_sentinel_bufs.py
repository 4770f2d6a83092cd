"""Sentinel-padded device buffers of the kernel-level GPU tests (tests/test_chain_kernels.py, tests/test_rowkernels.py): every output
buffer is filled with a sentinel and followed by 64 sentinel floats; after a launch the padding must be untouched, the named outputs
fully written, and a second launch must leave the same bits.
GuardedBufs (tests/test_perlayer_guards.py, tests/test_flat_env_guards.py, tests/test_vecnorm_shapes.py; its own checks are shown to fire
in tests/test_sentinel_bufs.py) adds a band IN FRONT of every buffer, integer and float64 buffers, payloads off their 16-byte boundary,
column blocks of wider matrices, read-only inputs and several arenas in one block."""
import numpy as np
import torch as th

DEV = "cuda:0"
SENT = float(np.float32(12345.678))
PAD = 64


class Bufs:
    """output buffers: sentinel-filled, 64 sentinel floats behind the end"""

    def __init__(self):
        self.flat = {}

    def new(self, name, *shape):
        n = int(np.prod(shape))
        f = th.full((n + PAD,), SENT, dtype=th.float32, device=DEV)
        self.flat[name] = (f, n)
        return f[:n].view(*shape)

    def put(self, name, a):
        """an in / out buffer: the given values, the sentinel padding behind them"""
        a = th.as_tensor(np.ascontiguousarray(a)) if not isinstance(a, th.Tensor) else a
        t = self.new(name, *a.shape)
        t.copy_(a.to(DEV, th.float32))
        return t

    def check(self, written=()):
        th.cuda.synchronize()
        for name, (f, n) in self.flat.items():
            assert bool((f[n:] == SENT).all()), f"{name}: the padding behind the buffer was written"
        for name in written:
            f, n = self.flat[name]
            assert not bool((f[:n] == SENT).any()), f"{name}: elements left unwritten"

    def snapshot(self):
        return {name: f.clone() for name, (f, _) in self.flat.items()}

    def same_as(self, snap, skip=()):
        for name, (f, _) in self.flat.items():
            if name not in skip:
                assert th.equal(f, snap[name]), f"{name}: the second launch differs from the first"


# one sentinel per element type: values a correct kernel of this project cannot produce (the float ones are exactly representable
# nowhere near any test's data; the integer ones are the bit pattern 0xA5A5...)
SENTINELS = {th.float32: SENT, th.float64: -6.0221407612345e23, th.int32: -1515870811, th.int64: -6510615555426900571}
ALIGN = 256  # bytes: `misalign` counts elements from such a boundary


class GuardedBufs:
    """Buffers with PAD sentinel elements IN FRONT OF and BEHIND the payload, for float32 / float64 / int32 / int64 ("uint64" = its bits
    in an int64 tensor), a payload that starts `misalign` elements behind a 256-byte boundary, and [rows][ld] blocks of which only the
    columns [c0, c0 + n) are payload (the gap columns hold the sentinel and are checked like the padding). check(): everything that
    is not payload still holds the sentinel, read-only inputs (put_ro) hold the bits they were given, the named outputs hold no
    sentinel any more; snapshot() / same_as(): a second launch leaves the same bits."""

    def __init__(self, device=None):
        self.device = DEV if device is None else device
        self.bufs = {}  # name -> (whole block, payload mask over the block, read-only copy or None)
        self.span = {}  # name -> (first payload element, one past the last, payload contiguous) of the block

    def _block(self, name, n_span, dtype, misalign):
        if dtype == "uint64":
            dtype = th.int64
        assert name not in self.bufs and dtype in SENTINELS and misalign >= 0
        item = th.empty((), dtype=dtype).element_size()
        f = th.full((2 * PAD + ALIGN // item + misalign + n_span,), SENTINELS[dtype], dtype=dtype, device=self.device)
        first = PAD  # the first element at or behind PAD that sits on a 256-byte boundary
        while (f.data_ptr() + first * item) % ALIGN:
            first += 1
        return f, first + misalign

    def new(self, name, *shape, dtype=th.float32, misalign=0):
        """an output: sentinel-filled payload of the given shape"""
        n = int(np.prod(shape))
        f, p = self._block(name, n, dtype, misalign)
        mask = th.zeros(f.numel(), dtype=th.bool, device=self.device)
        mask[p:p + n] = True
        self.bufs[name], self.span[name] = (f, mask, None), (p, p + n, True)
        return f[p:p + n].view(*shape)

    def new_cols(self, name, rows, ld, c0, n, dtype=th.float32, misalign=0):
        """an output that is the column block [:, c0:c0 + n] of a [rows][ld] matrix; the other columns are gaps"""
        assert 0 <= c0 and c0 + n <= ld
        f, p = self._block(name, rows * ld, dtype, misalign)
        whole = f[p:p + rows * ld].view(rows, ld)
        mask = th.zeros(f.numel(), dtype=th.bool, device=self.device)
        mask[p:p + rows * ld].view(rows, ld)[:, c0:c0 + n] = True
        self.bufs[name], self.span[name] = (f, mask, None), (p + c0, p + (rows - 1) * ld + c0 + n, False)
        return whole[:, c0:c0 + n]

    def new_pack(self, name, sizes, dtype=th.float32, misalign=0):
        """several flat arenas back to back in ONE block, PAD sentinel elements (rounded up so that every arena starts on the same 16-byte
        phase) between them: the tail overrun of one arena lands in the front band of the next"""
        item = 8 if dtype == "uint64" else th.empty((), dtype=dtype).element_size()
        offs, o = [], 0
        for n in sizes:
            offs.append(o)
            o += n + PAD + (-n) % (16 // item)
        span = offs[-1] + sizes[-1]
        f, p = self._block(name, span, dtype, misalign)
        mask = th.zeros(f.numel(), dtype=th.bool, device=self.device)
        for o, n in zip(offs, sizes):
            mask[p + o:p + o + n] = True
        self.bufs[name], self.span[name] = (f, mask, None), (p, p + span, False)
        return [f[p + o:p + o + n] for o, n in zip(offs, sizes)]

    def _fill(self, t, a):
        a = th.as_tensor(np.ascontiguousarray(a)) if not isinstance(a, th.Tensor) else a
        t.copy_(a.to(self.device, t.dtype))
        return t

    def put(self, name, a, dtype=th.float32, misalign=0):
        """an in / out buffer: the given values, guarded on both sides"""
        return self._fill(self.new(name, *tuple(a.shape), dtype=dtype, misalign=misalign), a)

    def put_cols(self, name, a, ld, c0, dtype=th.float32, misalign=0):
        """an in / out column block of a wider matrix"""
        return self._fill(self.new_cols(name, a.shape[0], ld, c0, a.shape[1], dtype=dtype, misalign=misalign), a)

    def freeze(self, name):
        f, mask, _ = self.bufs[name]
        self.bufs[name] = (f, mask, f.clone())

    def put_ro(self, name, a, dtype=th.float32, misalign=0):
        """a read-only input: check() wants it bit-identical to what was put"""
        t = self.put(name, a, dtype=dtype, misalign=misalign)
        self.freeze(name)
        return t

    def put_ro_cols(self, name, a, ld, c0, dtype=th.float32, misalign=0):
        t = self.put_cols(name, a, ld, c0, dtype=dtype, misalign=misalign)
        self.freeze(name)
        return t

    def check(self, written=()):
        if str(self.device).startswith("cuda"):
            th.cuda.synchronize()
        for name, (f, mask, ro) in self.bufs.items():
            sent = SENTINELS[f.dtype]
            first, last, contiguous = self.span[name]
            assert bool((f[:first] == sent).all()), f"{name}: the padding in front of the buffer was written"
            assert bool((f[last:] == sent).all()), f"{name}: the padding behind the buffer was written"
            assert contiguous or bool((f[first:last][~mask[first:last]] == sent).all()), f"{name}: a gap column (or the band between two arenas) was written"
            if ro is not None:
                assert th.equal(f, ro), f"{name}: a read-only input was changed"
        for name in written:
            f, mask, _ = self.bufs[name]
            first, last, contiguous = self.span[name]
            payload = f[first:last] if contiguous else f[mask]
            assert not bool((payload == SENTINELS[f.dtype]).any()), f"{name}: elements left unwritten"

    def snapshot(self):
        return {name: f.clone() for name, (f, _, _) in self.bufs.items()}

    def same_as(self, snap, skip=()):
        for name, (f, _, _) in self.bufs.items():
            if name not in skip:
                assert th.equal(f, snap[name]), f"{name}: the second launch differs from the first"
