"""The lean dW / db + Adam kernel against the kernel it replaced (cstr_linear_bwd_weight_adam_sets_f32, csrc/cstr_mlp.hip).

Both write the same bits: the lean kernel changes where the slice boundaries and a set's operands come from, which wave updates which
element of a tile and which tile body a workgroup runs, never the arithmetic of an element. Every case runs the launch twice from
identical inputs, once per setting of cstr_wgrad_adam_lean, and compares every buffer the launch may write byte for byte: dW, db, the
parameters, both moments, own targets, the tile-major shadow, the flat Adam segment and the polyak run -- each with 64 sentinel floats
behind it that must survive. tests/test_chain_kernels.py::test_linear_bwd_weight_adam_sets is the fp64 statement of the launch; this
module only ties the two kernels together, at the smallest shapes at which each body, the slice lookup and the tile walk can go wrong.
The body selection itself (cstr_wgrad_adam_tile_body) is a host function and is checked without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import _chain_reference as R

DEV = "cuda:0"
SENT = float(np.float32(12345.678))
PAD = 64
FULL, KNARROW, NNARROW, GENERIC = 0, 1, 2, 3


def body_of(m, n, k, tile_n, tile_k):
    """the rule of include/cstr_rl_hip.h, restated"""
    if m != 256 or n * k >= 1 << 28:
        return GENERIC
    n_full, k_full = 16 * tile_n + 16 <= n, 16 * tile_k + 16 <= k
    if n_full and k_full:
        return FULL
    if k <= 16 and n_full:
        return KNARROW
    if n <= 16 and k_full:
        return NNARROW
    return GENERIC


def bodies(lib, m, n, k):
    f = lib.cstr_wgrad_adam_tile_body
    f.argtypes, f.restype = [C.c_int64] * 5, C.c_int
    got = {(tn, tk): f(m, n, k, tn, tk) for tn in range((n + 15) // 16) for tk in range((k + 15) // 16)}
    assert got == {(tn, tk): body_of(m, n, k, tn, tk) for tn, tk in got}, (m, n, k)
    return got


def test_body_selection():
    """SAC's two launches at the class defaults (batch 256, [256, 256], 4 observations, 2 actions) run lean bodies only; TD3's and MADDPG's
    [400, 300] run the generic body exactly on the tiles that are ragged in the 300-wide dimension; other batch sizes run it everywhere"""
    from core import _native

    lib = _native.lib()
    sac_critic, sac_actor = [(256, 6), (256, 256), (1, 256)] * 2, [(256, 4), (256, 256), (4, 256)]
    for n, k in sac_critic + sac_actor:
        assert GENERIC not in bodies(lib, 256, n, k).values(), (n, k)
    assert set(bodies(lib, 256, 256, 6).values()) == {KNARROW} and set(bodies(lib, 256, 256, 4).values()) == {KNARROW}
    assert set(bodies(lib, 256, 256, 256).values()) == {FULL}
    assert set(bodies(lib, 256, 1, 256).values()) == {NNARROW} and set(bodies(lib, 256, 4, 256).values()) == {NNARROW}
    # TD3 / MADDPG, [400, 300]: first layers (critic input 6 or the joint 12, actor input 4), hidden layer, heads
    for k in (4, 6, 12):
        assert set(bodies(lib, 256, 400, k).values()) == {KNARROW}
    hidden = bodies(lib, 256, 300, 400)
    assert all(b == (GENERIC if tn == 18 else FULL) for (tn, tk), b in hidden.items()) and len(hidden) == 19 * 25
    for n in (1, 2):
        head = bodies(lib, 256, n, 300)
        assert all(b == (GENERIC if tk == 18 else NNARROW) for (tn, tk), b in head.items()) and len(head) == 19
    assert bodies(lib, 256, 20, 36) == {(0, 0): FULL, (0, 1): FULL, (0, 2): GENERIC, (1, 0): GENERIC, (1, 1): GENERIC, (1, 2): GENERIC}
    assert set(bodies(lib, 256, 4, 6).values()) == {GENERIC}  # narrow both ways
    for m in (48, 64, 255, 257, 512):
        assert set(bodies(lib, m, 32, 48).values()) == {GENERIC}
    f = lib.cstr_wgrad_adam_tile_body
    assert f(256, 16, 16, 1, 0) == -1 and f(256, 16, 16, 0, 1) == -1 and f(0, 16, 16, 0, 0) == -1  # no such tile
    assert lib.cstr_wgrad_adam_lean(-1) == 1  # the lean kernel is the default


# ---- the two kernels on the same operands -----------------------------------------------------------------------------------------
class Opt:
    """what linear_bwd_weight_adam_sets and chain_root read of a FlatAdam"""

    def __init__(self, ops, lr, betas, eps, grad_scale, step):
        self.ctl = th.zeros(4, dtype=th.int64, device=DEV)
        self.lr_dev = th.tensor([lr], dtype=th.float64, device=DEV)
        self.param_groups, self.grad_scale = [dict(betas=betas, eps=eps)], grad_scale
        ops.set_adam_step(self.ctl, step, *betas)


HYPER = [dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, step=3), dict(lr=7e-3, betas=(0.8, 0.99), eps=1e-6, grad_scale=0.125, step=7)]
TAU = 0.005


def S(m, n, k, ldx=None, shadow=False, target=False, opt=0):
    return dict(m=m, n=n, k=k, ldx=ldx or k, shadow=shadow, target=target, opt=opt)


class Launch:
    """one launch's operands from a seed: every buffer the launch may write is sentinel-padded and kept by name"""

    def __init__(self, ops, specs, seed, flat_adam=False, polyak=False, advance=False):
        rng = np.random.default_rng(seed)
        self.ops, self.bufs, self.written = ops, {}, []
        self.opts = [Opt(ops, **h) for h in HYPER]
        self.sets = []
        for j, s in enumerate(specs):
            m, n, k = s["m"], s["n"], s["k"]
            dz = self.const(rng.standard_normal((m, n)) * 0.1)
            x = self.const(rng.standard_normal((m, s["ldx"])))[:, :k]
            quad = {}
            for p, shape in (("w", (n, k)), ("b", (n,))):
                quad[p] = (self.put(f"{p}{j}", rng.standard_normal(shape) * 0.3), self.new(f"d{p}{j}", shape),
                           self.put(f"{p}_m{j}", rng.standard_normal(shape) * 1e-3), self.put(f"{p}_v{j}", rng.uniform(0, 1, shape) * 1e-5))
                self.written.append(f"d{p}{j}")
            shadow = None
            if s["shadow"]:
                shadow = self.new(f"shadow{j}", (ops.swizzled_numel(n, k),))
                ops.policy_swizzle(quad["w"][0], shadow)  # as FlatAdam.add_weight_shadow leaves it
            own = (self.put(f"t_w{j}", rng.standard_normal((n, k))), self.put(f"t_b{j}", rng.standard_normal((n,))), TAU) if s["target"] else None
            self.sets.append((dz, x, quad["w"], quad["b"], s["opt"], shadow, own))
        self.flat = []
        if flat_adam:  # an Adam range on optimiser 0's control words, as SAC's entropy coefficient rides
            g = self.const(rng.standard_normal(37) * 0.01)
            p, mm, vv = self.put("flat_p", rng.standard_normal(37)), self.put("flat_m", rng.standard_normal(37) * 1e-3), self.put("flat_v", rng.uniform(0, 1, 37) * 1e-5)
            h = HYPER[0]
            self.flat.append((p, g, mm, vv, self.opts[0].ctl, self.opts[0].lr_dev, *h["betas"], h["eps"], h["grad_scale"]))
        if polyak:
            self.flat.append(("polyak", self.const(rng.standard_normal(1030)), self.put("polyak_t", rng.standard_normal(1030)), TAU))
        if advance:  # state["step"] += 1 of both optimisers by the loss workgroup of a chain root, as on the training path
            self.advance()

    def const(self, a):
        return th.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)

    def new(self, name, shape):
        n = int(np.prod(shape))
        f = th.full((n + PAD,), SENT, dtype=th.float32, device=DEV)
        self.bufs[name] = (f, n)
        return f[:n].view(*shape)

    def put(self, name, a):
        t = self.new(name, np.shape(a))
        t.copy_(self.const(a))
        return t

    def advance(self):
        ops, binp = self.ops, R.q_bwd_case(0)
        bw = [[self.const(net[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")] for net in binp["nets"]]
        bh1, bh2, bq = [self.const(v) for v in binp["h1"]], [self.const(v) for v in binp["h2"]], [self.const(v) for v in binp["q_part"]]
        root = ops.chain_root("td", 16, bq, [w[5] for w in bw], bq[0].shape[0], gamma=0.97, scale=1.0, rew=self.const(binp["rew"]),
                              done=self.const(binp["done"]), adam_advance=self.opts)
        nets = [ops.chain_net(((bw[g][0], bw[g][1]), (bw[g][2], bw[g][3]), (bw[g][4].view(-1), bw[g][5])), None, bh1[g], bh2[g]) for g in range(2)]
        ops.q_chain_bwd(nets, root, 6, 4, 16, 16, 1, dz2=th.empty(2, 16, 16, device=DEV), dz1=th.empty(2, 16, 16, device=DEV))
        th.cuda.synchronize()
        assert [int(o.ctl[0]) for o in self.opts] == [h["step"] + 1 for h in HYPER]

    def run(self, lib, lean):
        ctl = [o.ctl.clone() for o in self.opts]
        before = {name: f.clone() for name, (f, _) in self.bufs.items() if name[0] in "wb" and name[1].isdigit()}
        was = lib.cstr_wgrad_adam_lean(1 if lean else 0)
        try:
            self.ops.linear_bwd_weight_adam_sets(self.sets, self.opts, self.flat)
            th.cuda.synchronize()
        finally:
            lib.cstr_wgrad_adam_lean(was)
        for name, (f, n) in self.bufs.items():
            assert bool((f[n:] == SENT).all()), f"{name}: the padding behind the buffer was written (lean = {lean})"
        for name in self.written:
            f, n = self.bufs[name]
            assert not bool((f[:n] == SENT).any()), f"{name}: elements left unwritten (lean = {lean})"
        assert all(th.equal(a, o.ctl) for a, o in zip(ctl, self.opts))  # control words are read, never written
        for name, t in before.items():  # the weights and biases have taken their step (a step below half an ulp is possible, not common)
            n = self.bufs[name][1]
            assert float((t[:n] != self.bufs[name][0][:n]).float().mean()) > 0.99, f"{name}: elements left at their old value (lean = {lean})"
        return {name: f.cpu().numpy().copy() for name, (f, _) in self.bufs.items()}


def both(specs, **kw):
    from core import _native
    from core.common import hip_ops

    lib = _native.lib()
    out = [Launch(hip_ops, specs, 1234, **kw).run(lib, lean) for lean in (False, True)]
    assert out[0].keys() == out[1].keys() and len(out[0]) >= 8 * len(specs)
    for name in out[0]:
        a, b = out[0][name], out[1][name]
        assert a.tobytes() == b.tobytes(), f"{name}: {int((a.view(np.int32) != b.view(np.int32)).sum())} of {a.size} words differ between the two kernels"


ALL = [S(256, 16, 16), S(256, 32, 48, opt=1, target=True), S(256, 16, 6, ldx=8, target=True), S(256, 16, 4, ldx=6, shadow=True, opt=1), S(256, 1, 16),
       S(256, 4, 32, opt=1), S(256, 20, 36, shadow=True), S(48, 16, 16, opt=1)]
CASES = {
    "full_16x16": [S(256, 16, 16)],
    "full_32x48": [S(256, 32, 48)],  # six tiles: the k-major tile walk, the wave <-> row-register mapping
    "k_narrow_16x6": [S(256, 16, 6, ldx=8)],
    "k_narrow_16x4_shadow": [S(256, 16, 4, ldx=6, shadow=True)],
    "n_narrow_1x16": [S(256, 1, 16)],
    "n_narrow_4x32": [S(256, 4, 32)],
    "ragged_20x36": [S(256, 20, 36)],  # tiles (0, 0) and (0, 1) are whole, the other four take the generic body
    "rows_48": [S(48, 16, 16)],  # not the lean bodies' row count
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_one_set(case):
    both(CASES[case])


@pytest.mark.gpu
def test_all_in_one_launch():
    """every shape above in one launch, two optimisers with different hyper-parameters pre-advanced through a chain root, an own-target
    soft update on one full and one narrow set, a flat Adam segment of 37 elements and a polyak run of 1,030"""
    both(ALL, flat_adam=True, polyak=True, advance=True)


@pytest.mark.gpu
def test_many_slices():
    """16 sets + 2 flat segments = 18 slices: boundaries in every preloaded head word the launch can use but the last"""
    specs = [S(256, 16, 16, opt=j & 1) if j % 4 == 0 else S(256, 16, 6, ldx=8) if j % 4 == 1 else S(256, 1, 16, opt=1) if j % 4 == 2 else S(256, 20, 36, target=True)
             for j in range(16)]
    both(specs, flat_adam=True, polyak=True)
