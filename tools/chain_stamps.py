#!/usr/bin/env python3
"""Per-phase timeline of the chain kernels from in-kernel s_memtime stamps (diagnostic build: `make -C .../csrc diag`, run with
CSTR_LIB_PATH=tools/ab/libcstr_rl_hip_diag.so). Stamps per wave: 0 entry | 1 prologue done (before the first barrier) | 2 past it |
3 panel ready (layer 1 / dz2 recomputed, past the barrier) | 4 MFMAs done | 5 split-K combined | 6 partials reduced (past the last
barrier) | 7 stores issued. Prints the median over workgroups (and the slowest workgroup) of each phase end, in ns after the launch's
earliest stamp of the same XCD-agnostic per-workgroup origin (stamp 0 of the workgroup's first wave).

FIN=1 (library built with `make diag DIAG_EXTRA=-DCSTR_QFWD_FIN_STAMPS`): the 4-network Q forward stamps its pending head's finalisation instead
of phases 3 - 5 -- 3 partial sums arrived | 4 action written to xs | 5 log-prob done -- and this prints them per role and per kind of
workgroup (column group 0 stores, the others do not): the median workgroup's ticks after its own entry, on the finalising wave."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("CSTR_LIB_PATH", os.path.join(ROOT, "tools", "ab", "libcstr_rl_hip_diag.so"))
for p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from core import _native as nv  # noqa: E402
from core.common.vec_env import CSTRVecEnv  # noqa: E402
from core.sac import SAC  # noqa: E402
from tools.chain_probe import chain_launches  # noqa: E402

KERNEL_OF = dict(sac_actor_chain_fwd=0, q_chain_fwd_4nets=1, q_chain_bwd_td=2, q_chain_fwd_2nets=1, q_chain_bwd_actor=2, sac_actor_chain_bwd=3)
NAMES = ["entry", "prologue", "barrier1", "panel", "mfma", "combine", "partials", "stores"]
FIN_NAMES = {1: "prologue", 3: "head_partials", 4: "action_in_xs", 5: "logp_done", 2: "barrier1", 6: "last_barrier", 7: "stores"}
ROLE_NAMES = ["STORE_PI", "PLAIN", "NEXT_STORE", "NEXT"]


def fin_report(st, rowgroups):
    """st [workgroups][4 waves][8 stamps] of the 4-network launch, grid (column groups, row groups, 4 networks)"""
    gx = st.shape[0] // (4 * rowgroups)
    wg = np.arange(st.shape[0])
    z, x = wg // (gx * rowgroups), wg % gx
    t0 = st[:, :, 0].min(axis=1)
    out = {}
    for role in range(4):
        for kind, sel in (("colgroup0", x == 0), ("others", x > 0)):
            row = {}
            for i, nm in FIN_NAMES.items():
                v = st[:, :, i] - t0[:, None]
                fresh = (st[:, :, i] >= st[:, :, 0]) & (st[:, :, i] <= st[:, :, 7])  # a slot this launch did not write keeps an older stamp
                v = np.where(fresh, v, -1).max(axis=1)[sel & (z == role)]  # the workgroup's last wave that stamped it
                v = v[v >= 0]
                if v.size:
                    row[nm] = int(np.median(v))
            out[f"{ROLE_NAMES[role]}/{kind}"] = row
            print(f"{ROLE_NAMES[role]:10s} {kind:9s}", row)
    return out

if __name__ == "__main__":
    B = 256
    arch = [int(v) for v in os.environ.get("ARCH", "256,256").split(",")]
    model = SAC("MlpPolicy", CSTRVecEnv(4096), seed=0, batch_size=B, policy_kwargs=dict(net_arch=arch))
    model.learn(4096 * 4)
    fns = chain_launches(model, B)
    lib = nv.lib()
    lib.cstr_diag_chain_stamps.argtypes = [C.c_void_p, C.c_int64]
    words = 4 * 1024 * 4 * 8
    buf = (C.c_uint64 * words)()
    out = {}
    ghz = 0.1  # s_memtime on gfx950 ticks at 100 MHz
    for name, (fn, _) in fns.items():
        for _ in range(5):
            fn()
        # a different kernel in between, like in the iteration's graph (cold operands)
        th.cuda.synchronize()
        fn()
        th.cuda.synchronize()
        assert lib.cstr_diag_chain_stamps(buf, words) == 0
        st = np.frombuffer(buf, dtype=np.uint64).reshape(4, 1024, 4, 8)[KERNEL_OF[name]].astype(np.int64)
        live = st[:, 0, 0] > 0
        st = st[live]
        t0 = st[:, :, 0].min(axis=1)  # the workgroup's own entry
        launch0 = st[:, :, 0].min()
        rel = (st - t0[:, None, None]) / ghz
        row = {}
        fin = os.environ.get("FIN") == "1" and name == "q_chain_fwd_4nets"
        for i, nm in enumerate(NAMES):
            if fin and i in (3, 4, 5):  # these slots hold the finalisation's stamps: fin_report
                continue
            v = rel[:, :, i].max(axis=1)  # the workgroup's last wave
            v = v[(st[:, :, i].max(axis=1) > 0)]
            if v.size:
                row[nm] = dict(median_ns=int(np.median(v)), max_ns=int(v.max()))
        if fin:
            row["fin_ticks"] = fin_report(st, B // 16)
        row["entry_spread_ns"] = int((t0.max() - launch0) / ghz)
        row["workgroups"] = int(live.sum())
        out[name] = row
        print(name, {k: (int(v["median_ns"] / 10) if isinstance(v, dict) else v) for k, v in row.items() if k not in ("entry_spread_ns", "fin_ticks")})
    tag = "" if arch == [256, 256] else "_" + "x".join(str(v) for v in arch)
    tag += os.environ.get("TAG", "")
    json.dump(out, open(os.path.join(ROOT, "gpurun_out", f"r03_chain_phase_stamps{tag}.json"), "w"), indent=1)
