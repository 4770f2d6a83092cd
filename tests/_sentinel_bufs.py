"""Sentinel-padded device buffers of the kernel-level GPU tests (tests/test_chain_kernels.py, tests/test_rowkernels.py): every output
buffer is filled with a sentinel and followed by 64 sentinel floats; after a launch the padding must be untouched, the named outputs
fully written, and a second launch must leave the same bits."""
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
