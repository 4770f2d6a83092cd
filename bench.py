#!/usr/bin/env python3
"""bench.py -- env-steps/sec of SAC on 4096 vectorised two-series CSTR envs per GPU (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

N > 1 runs N ranks, one per GPU, over RCCL. Either the caller starts them (torch.distributed.run: WORLD_SIZE / RANK /
LOCAL_RANK / MASTER_* in the environment), or -- plain `python bench.py --gpus N` -- this file does: the parent, BEFORE
any GPU call, starts N fresh child processes of itself with that environment, relays rank 0's single JSON line and exits
non-zero unless the job really ran N ranks (`n_gpus`, `rccl_world`, `allreduce_checksum` on the line prove it).

A "step" is ONE iteration of `core.SAC("MlpPolicy", env).learn()` with the class-default HYPER-PARAMETERS
(reference: core/common/off_policy_algorithm.py:331-351): one vec-step of 4096 envs (policy network + sampling + env step
+ ring row + the replay index draw in one launch) followed by one gradient step (gather inside the first layer behind
the sample, MLP forward/backward on hand-written f32-MFMA kernels [the rocBLAS/PyTorch-ROCm variant is reported beside
it], HIP td-target + losses, flat Adam launches, HIP polyak). The launches are replayed from a captured hipGraph with
EIGHT iterations recorded per graph: `model.enable_graph_capture(True, unroll=8)` -- an opt-in of this stack, `learn()`
alone launches eagerly and CSTR_GRAPH_UNROLL defaults to 1; the host bookkeeping (episode statistics, lazily read loss
means) of those eight iterations runs after the replay. `config.hip_graph` / `config.graph_unroll` say so on the line and
`unroll1_variant` is the same run with one iteration per graph. Inputs are resident in HBM
before the timed region. The timed region is exactly K steps, bracketed by a barrier + torch.cuda.synchronize() on both
sides; the MAX over ranks is reported and `ms_per_step` is that duration / K.
The run FAILS (non-zero exit) if hipGraph replay was requested but the timed iterations ran eagerly.

--dump-outputs DIR writes, after the timed steps, what the last timed step left for a caller of learn() (rank 0): every
tensor of the policy's state_dict (actor, critics, target networks), SAC's log entropy coefficient, the envs' observations
and the replay-ring row that step wrote, as DIR/<name>.npy (float32, well under 64 MB). The seeds are fixed, so the same
arguments give the same inputs from run to run and two builds can be compared output for output.

A plain run does only what the headline needs (set-up, warm-up, the K timed steps, --dump-outputs, the line). --full adds
the extra objects below (each still subject to --no-roofline / --no-variant / --no-cpu-baseline):
  roofline      the dominant kernel OF THE REPLAYED GRAPH: `rollout_step_kernel` (policy network + collect step of all
                envs + replay index draw in one launch). Matrix-core bound: the policy network's algorithmic FLOPs per
                launch / its launch duration (HIP events on the launch stream, graph-replayed back-to-back launches right
                after the timed region) against the dense f32 MFMA peak. `hbm` inside it: the same launch against the HBM
                roofline (104 B per env-step, SURVEY 8d, + the weights once) -- meaningless at this size and printed for
                that reason. `traffic` = HBM bytes per launch from the committed rocprofv3 PMC passes (`traffic_source`).
  roofline_collect / roofline_stream   the fused collect kernel alone (the launch of the eager path and of MADDPG) at the
                workload size and at N = 2^22 envs (436 MB per launch: its bandwidth-bound regime).
  roofline_mfma the stand-alone whole-policy launch (`policy_rows_fwd_kernel`) with the rollout launch under `as_launched`.
  roofline_iteration  the WHOLE iteration: algorithmic bytes (2.09 MB) and FLOPs / ms_per_step against both
                peaks, launches per iteration and the mean launch interval -- the iteration is launch-latency-bound.
  kernels       per-kernel average launch duration / algorithmic GB/s for the other HIP kernels of the step
  td3_variant / maddpg_variant   BASELINE configs 3 and 5 (TD3 class defaults, 4096 envs; MADDPG, 4 agents on the 8-obs /
                4-act twin-train env, 1024 envs), same loop, short runs on rank 0.
  cpu_baseline  the oracle port (C env step + ring add + MT19937 sampler with OpenMP, torch-CPU SAC step)
                timed on this box's host cores on a bounded sample of the same workload (rank 0, N=1 only): all-cores
                leg (`value`) and a single-thread leg, CPU model string from /proc/cpuinfo.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3  # dense f32-input MFMA, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s measured achievable)
# the reference's own Python on CPU, measured in the survey container (8 cores, no GPU; SURVEY 6 / BASELINE.md 2): unmodified
# reference SAC("MlpPolicy").learn() on DummyVecEnv(4096 x TwoSeriesCSTREnv), class defaults. It cannot travel to the GPU box.
REFERENCE_PYTHON_ENV_STEPS_PER_S = 4.2e3


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)  # >= 2000 vec-steps after 200 warm-up (0.4 s of GPU time)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--algo", default="sac", choices=["sac", "td3", "maddpg"])
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--obs-dim", type=int, default=4, choices=[4, 8])
    ap.add_argument("--integrator", default="euler", choices=["euler", "rk4"])
    ap.add_argument("--graph", type=int, default=int(os.environ.get("CSTR_BENCH_GRAPH", "1")))
    ap.add_argument("--graph-unroll", type=int, default=int(os.environ.get("CSTR_GRAPH_UNROLL", "8")),
                    help="iterations recorded per hipGraph on one GPU: the ~9 us the GPU idles between two graph launches "
                         "(tools/graph_timeline.sh) is paid once per replay; the same launches in the same order")
    ap.add_argument("--blas", default=os.environ.get("CSTR_BLAS", "rocblas"), choices=["rocblas", "hipblaslt", "default"])
    ap.add_argument("--tunable", type=int, default=int(os.environ.get("CSTR_BENCH_TUNABLE", "0")))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-variant", action="store_true", help="skip the secondary north_star-shaped run (obs 8, RK4)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--full", action="store_true", help="also run the rooflines, per-kernel timings, variants, CPU baseline and "
                                                        "reference comparison (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy")
    return ap.parse_args()


def host_cores() -> int:
    """CPU share of this process: min(affinity, cgroup quota); the GPU box reports all 256 host threads in
    os.cpu_count() but a 1-GPU job owns 16 of them (oversubscribing OpenMP/torch wrecks the CPU baseline)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return int(os.environ.get("CSTR_CPU_CORES", min(n, 16)))


def event_time_us(fn, n_launch, stream, in_graph=False):
    """Average duration of `fn` (one kernel launch) over n_launch back-to-back launches, HIP events on the launch stream.
    in_graph: the launches are captured into one hipGraph and the replay is timed -- for microsecond kernels the host's
    launch gap (~10 us per ctypes call) would otherwise dominate; this is also how the training loop issues them."""
    for _ in range(5):
        fn()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    if in_graph:
        th.cuda.synchronize()
        side = th.cuda.Stream()
        side.wait_stream(th.cuda.current_stream())
        g = th.cuda.CUDAGraph()
        import gc

        gc.collect()  # a collection that frees device memory in the middle of a capture aborts the process
        gc.disable()
        try:
            with th.cuda.stream(side):
                g.capture_begin(capture_error_mode="thread_local")
                for _ in range(n_launch):
                    fn()
                g.capture_end()
        finally:
            gc.enable()
        th.cuda.current_stream().wait_stream(side)
        g.replay()
        stream.synchronize()
        e0.record(stream)
        g.replay()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_launch
    stream.synchronize()
    e0.record(stream)
    for _ in range(n_launch):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n_launch


def roofline_collect(n_envs, obs_dim, integrator, n_launch):
    """Fused collect kernel alone on its own synthetic state (the training state is untouched): C in U[0.05,0.45],
    T in U[280,380] normalised, policy output U[-1,1]."""
    from core import _native as nv
    from core.common import hip_ops

    dev = th.device("cuda", th.cuda.current_device())
    g = th.Generator(device=dev).manual_seed(1)
    lo = th.tensor([0.0, 273.15, 0.0, 273.15], device=dev)
    hi = th.tensor([0.7, 400.0, 0.7, 400.0], device=dev)
    u = th.rand(n_envs, 4, device=dev, generator=g)
    raw = th.stack([0.05 + 0.4 * u[:, 0], 280 + 100 * u[:, 1], 0.05 + 0.4 * u[:, 2], 280 + 100 * u[:, 3]], dim=1)
    obs4 = 2.0 * (raw - lo) / (hi - lo) - 1.0
    obs = (obs4 if obs_dim == 4 else th.cat([obs4, raw], dim=1)).contiguous()
    steps = th.zeros(n_envs, dtype=th.int32, device=dev)
    pcg = th.randint(1, 2**62, (n_envs, 4), dtype=th.int64, device=dev, generator=g) | 1
    ring = hip_ops.DeviceRing(2, n_envs, obs_dim, 2, dev)
    pol = (th.rand(n_envs, 2, device=dev, generator=g) * 2 - 1).contiguous()
    coef = nv.default_coef()
    stream = th.cuda.current_stream()

    def launch():
        hip_ops.collect_step(coef, integrator, ring, obs, steps, pol, True, [-1, -1], [1, 1], pcg_state=pcg)

    us = event_time_us(launch, n_launch, stream, in_graph=n_envs <= 65536)
    bytes_per_env = 2 * (2 * 4 * obs_dim + 8 + 12)  # 104 B (D=4) / 168 B (D=8): SURVEY 8d
    alg = bytes_per_env * n_envs
    gbs = alg / us / 1e3
    return dict(bound="hbm", kernel="collect_step_kernel", achieved=round(gbs, 2), peak=HBM_PEAK_GBS, unit="GB/s",
                frac=round(gbs / HBM_PEAK_GBS, 5), traffic=pmc_traffic(n_envs, obs_dim, integrator), launch_us=round(us, 3),
                n_envs=n_envs, algorithmic_bytes_per_launch=alg)


def pmc_traffic(n_envs, obs_dim, integrator):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/r01_collect_pmc.json: separate
    FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 FETCH correction) -- counters cannot be read from inside the bench."""
    if obs_dim != 4 or integrator != "euler":
        return None
    try:
        with open(os.path.join(ROOT, "profiles", "r01_collect_pmc.json")) as fh:
            return json.load(fh)["collect_step_kernel<4,0>"][str(n_envs)]["traffic_bytes"]
    except (OSError, KeyError, ValueError):
        return None


def other_kernels(model, batch):
    """Average launch time of the remaining hand-written kernels at the workload's sizes."""
    from core.common import hip_ops

    stream = th.cuda.current_stream()
    pol = model.policy
    out = {}
    n = pol.critic_arena.numel
    tgt = pol.critic_target_arena.flat.clone()
    us = event_time_us(lambda: hip_ops.polyak(pol.critic_arena.flat, tgt, 0.005), 200, stream, in_graph=True)
    out["polyak_kernel"] = dict(launch_us=round(us, 3), n_params=n, gbs=round(12 * n / us / 1e3, 2))
    p, g = pol.critic_arena.flat.clone(), th.randn_like(pol.critic_arena.flat)
    m, v = th.zeros_like(p), th.zeros_like(p)
    ctl = hip_ops.new_adam_ctl(p.device)
    lr = th.tensor([3e-4], dtype=th.float64, device=p.device)
    us = event_time_us(lambda: hip_ops.adam(p, g, m, v, ctl, lr), 200, stream, in_graph=True)
    out["adam_kernel"] = dict(launch_us=round(us, 3), n_params=n, gbs=round(28 * n / us / 1e3, 2))
    # the same two kernels in their bandwidth-bound regime (2^25 parameters: 403 MB / 940 MB of traffic per launch)
    nbig = 1 << 25
    pb, tb = th.randn(nbig, device=p.device), th.randn(nbig, device=p.device)
    us = event_time_us(lambda: hip_ops.polyak(pb, tb, 0.005), 20, stream)
    out["polyak_kernel_stream"] = dict(launch_us=round(us, 2), n_params=nbig, gbs=round(12 * nbig / us / 1e3, 1), frac=round(12 * nbig / us / 1e3 / HBM_PEAK_GBS, 4))
    mb, vb = th.zeros(nbig, device=p.device), th.zeros(nbig, device=p.device)
    us = event_time_us(lambda: hip_ops.adam(pb, tb, mb, vb, ctl, lr), 20, stream)
    out["adam_kernel_stream"] = dict(launch_us=round(us, 2), n_params=nbig, gbs=round(28 * nbig / us / 1e3, 1), frac=round(28 * nbig / us / 1e3 / HBM_PEAK_GBS, 4))
    del pb, tb, mb, vb
    rb = model.replay_buffer
    b = rb.alloc_batch(batch)
    mt = th.zeros(628, dtype=th.int32, device=p.device)
    hip_ops.mt19937_seed(mt, 1)
    us = event_time_us(lambda: hip_ops.replay_sample(rb.ring, mt, batch, b.observations, b.actions, b.next_observations,
                                                     b.dones, b.rewards), 200, stream, in_graph=True)
    d = rb.obs_shape[0]
    out["replay_sample_kernel"] = dict(launch_us=round(us, 3), batch=batch, gbs=round(2 * batch * (8 * d + 20) / us / 1e3, 3))
    q = th.randn(batch, 1, device=p.device)
    o = th.empty_like(q)
    ent = th.ones(1, device=p.device)
    us = event_time_us(lambda: hip_ops.td_target_min(q, q, q, q, q, ent, 0.99, o), 200, stream, in_graph=True)
    out["td_target_min_kernel"] = dict(launch_us=round(us, 3), batch=batch, gbs=round(24 * batch / us / 1e3, 3))
    # the MFMA Linear kernels at the learners' hidden-layer shape (batch x 256 x 256): latency-bound, a few per cent of the
    # f32 matrix-core peak (157.3 TFLOP/s: v_mfma_f32_16x16x4_f32 at 64 FLOP/clk/SIMD, MI355X_MICROARCH.md)
    h = 256
    x, w, bias = th.randn(batch, h, device=p.device), th.randn(h, h, device=p.device) / 16, th.zeros(h, device=p.device)
    gz, y = th.randn(batch, h, device=p.device), th.relu(th.randn(batch, h, device=p.device))
    dw, db = th.empty(h, h, device=p.device), th.empty(h, device=p.device)
    flops = 2.0 * batch * h * h
    for name, fn in (("linear_act_fwd_kernel", lambda: hip_ops.linear_act_fwd(x, w, bias, 1)),
                     ("linear_bwd_input_kernel", lambda: hip_ops.linear_bwd_input(gz, w, y, 1)),
                     ("linear_bwd_weight_kernel", lambda: hip_ops.linear_bwd_weight(gz, x, dw, db))):
        us = event_time_us(fn, 200, stream, in_graph=True)
        out[name] = dict(launch_us=round(us, 3), shape=[batch, h, h], bound="mfma", tflops=round(flops / us / 1e6, 2),
                         frac=round(flops / us / 1e6 / F32_MFMA_PEAK_TFLOPS, 4))
    # the rollout's whole policy network in one launch (the longest kernel of the iteration): n_envs rows, obs -> 256 -> 256 -> 2A
    n_rows, k0, a = rb.n_envs, rb.obs_shape[0], rb.action_dim
    xo = th.randn(n_rows, k0, device=p.device)
    w1, b1 = th.randn(h, k0, device=p.device) / 2, th.zeros(h, device=p.device)
    w3, b3 = th.randn(2 * a, h, device=p.device) / 16, th.zeros(2 * a, device=p.device)
    act_out, ctl = th.empty(n_rows, a, device=p.device), hip_ops.new_rng_ctl(1, p.device)
    w_tiles = hip_ops.policy_swizzle(w)  # the product path reads the tile-major copy of the hidden layer (FlatAdam.add_weight_shadow)
    # as the training loop launches it: tile-major W2 copy, Philox offset advanced by the collect launch that consumes the actions
    # (cstr_collect_step_rng_f32) instead of a 256-workgroup ticket of its own; `launch_us_self_advancing` = the stand-alone form
    us = event_time_us(lambda: hip_ops.policy_rows_fwd(xo, w1, b1, w, bias, w3, b3, 1, 0, 0, act_out, rng_ctl=ctl, w2_swz=w_tiles,
                                                       defer_rng_advance=True), 200, stream, in_graph=True)
    us_self = event_time_us(lambda: hip_ops.policy_rows_fwd(xo, w1, b1, w, bias, w3, b3, 1, 0, 0, act_out, rng_ctl=ctl, w2_swz=w_tiles), 200,
                            stream, in_graph=True)
    flops = 2.0 * n_rows * (k0 * h + h * h + h * 2 * a)
    out["policy_rows_fwd_kernel"] = dict(launch_us=round(us, 3), launch_us_self_advancing=round(us_self, 3), shape=[n_rows, k0, h, h, 2 * a], bound="mfma",
                                         tflops=round(flops / us / 1e6, 2), frac=round(flops / us / 1e6 / F32_MFMA_PEAK_TFLOPS, 4))
    # what the captured iteration really launches: the SAME network + the collect step of all envs + the replay index draw in one
    # launch (cstr_rollout_step_f32), then the gather launch (cstr_replay_gather_packed_f32) -- against the three launches they replace
    if k0 in (4, 8) and a == 2:
        from core import _native as nv

        ring = hip_ops.DeviceRing(8, n_rows, k0, a, p.device)
        env_obs = (th.rand(n_rows, k0, device=p.device) * 2 - 1).contiguous()
        steps = th.zeros(n_rows, dtype=th.int32, device=p.device)
        pcg = th.randint(1, 2 ** 62, (n_rows, 4), device=p.device, dtype=th.int64)
        idx = th.zeros(2, batch, dtype=th.int32, device=p.device)
        coef, lo, hi = nv.default_coef(max_steps=1 << 30), [-1.0] * a, [1.0] * a
        pbk = rb.alloc_packed_batch(batch)
        integ = "euler" if k0 == 4 else "rk4"

        def rollout():
            hip_ops.rollout_step(env_obs, w1, b1, w, bias, w3, b3, 1, 0, 0, w_tiles, ctl, coef, integ, ring, env_obs, steps, 1, lo, hi,
                                 pcg_state=pcg, mt_state=mt, sample_idx=idx)

        def gather():
            hip_ops.replay_gather_packed(ring, idx, batch, pbk.x_data, pbk.x_next, pbk.x_pi, pbk.samples.dones, pbk.samples.rewards,
                                         advance_ring=True, rng_advance=(ctl, n_rows))

        def separate():
            hip_ops.policy_rows_fwd(env_obs, w1, b1, w, bias, w3, b3, 1, 0, 0, act_out, rng_ctl=ctl, w2_swz=w_tiles, defer_rng_advance=True)
            hip_ops.collect_step(coef, integ, ring, env_obs, steps, act_out, 1, lo, hi, pcg_state=pcg, rng_advance=(ctl, n_rows))
            hip_ops.replay_sample_packed(ring, mt, batch, pbk.x_data, pbk.x_next, pbk.x_pi, pbk.samples.dones, pbk.samples.rewards)

        rollout(), gather()
        us_r = event_time_us(rollout, 100, stream, in_graph=True)
        us_rg = event_time_us(lambda: (rollout(), gather()), 100, stream, in_graph=True)
        us_sep = event_time_us(separate, 100, stream, in_graph=True)
        out["rollout_step_kernel"] = dict(launch_us=round(us_r, 3), with_gather_launch_us=round(us_rg, 3), three_separate_launches_us=round(us_sep, 3),
                                          shape=[n_rows, k0, h, h, 2 * a], bound="mfma", tflops=round(flops / us_r / 1e6, 2),
                                          frac=round(flops / us_r / 1e6 / F32_MFMA_PEAK_TFLOPS, 4),
                                          note="policy network (the MFMA work priced here) + fused collect step of all envs + replay index draw")
    # the SAC gradient step's row-chain launches (csrc/cstr_chain.hip) as the replayed graph issues them, back to back in a graph
    try:
        from tools.chain_probe import chain_launches

        if type(model).__name__ == "SAC" and model._chain_for(batch) is not None:
            for name, (fn, fl) in chain_launches(model, batch).items():
                fn()
                us = event_time_us(fn, 200, stream, in_graph=True)
                out[name] = dict(launch_us=round(us, 3), bound="mfma", tflops=round(fl / us / 1e6, 2), frac=round(fl / us / 1e6 / F32_MFMA_PEAK_TFLOPS, 4),
                                 note="back-to-back graph replays of ONE launch; in the iteration's graph it follows a different kernel (fresh operands): "
                                      "profiles/r03_sac_graph_timeline.json")
    except Exception as exc:  # noqa: BLE001 -- a microbenchmark must never fail the headline line
        out["chain_kernels_error"] = repr(exc)
    return out


def cpu_model() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform

    return platform.processor() or platform.machine()


def cpu_baseline(n_envs, batch, seconds):
    """All-cores leg (`value`) and single-thread leg of the oracle port, each a bounded sample."""
    multi = cpu_baseline_leg(n_envs, batch, seconds, host_cores())
    single = cpu_baseline_leg(n_envs, batch, max(3.0, seconds / 2), 1)
    multi["cpu_model"] = cpu_model()
    multi["single_thread"] = dict(value=single["value"], unit=single["unit"], cores=1, sample=single["sample"],
                                  env_only_value=single["env_only_value"], ms_per_iteration=single["ms_per_iteration"])
    return multi


def cpu_baseline_leg(n_envs, batch, seconds, cores):
    """Oracle port of one learn() iteration on the host cores: C env step + ring add (OpenMP over envs), C MT19937
    sampler + gather, torch-CPU actor forward and SAC gradient step (oracle/sac_cpu.py). Bounded sample."""
    from oracle import cstr_oracle as orc
    from oracle import sac_cpu

    th.set_num_threads(cores)
    rng = np.random.default_rng(0)
    rows = max(1_000_000 // n_envs, 1)
    ring = orc.ReplayRing(rows, n_envs, 4, 2)
    obs = rng.uniform(-0.5, 0.5, (n_envs, 4)).astype(np.float32)
    steps = np.zeros(n_envs, np.int32)
    reset = rng.uniform(-0.5, 0.5, (n_envs, 4)).astype(np.float32)
    learner = sac_cpu.SacCpu(sac_cpu.init_params(4, 2, [256, 256], seed=0))
    mt = orc.MT19937(n_envs - 1)
    low, high = np.array([-1, -1], np.float32), np.array([1, 1], np.float32)

    def iteration():
        nonlocal obs, steps
        a = learner.act(th.from_numpy(obs)).numpy()
        buf_a, env_a = orc.action_scale_chain(a, True, low, high)
        nxt, after, rew, done, tout, steps = orc.vec_step(obs, env_a, steps, reset, n_threads=cores)
        ring.add(obs, nxt, buf_a, rew, done, tout)
        obs = after
        (o, ac, no, d, r), _ = ring.sample(mt, batch)
        learner.train_step(*(th.from_numpy(x) for x in (o, ac, no, d, r)))

    for _ in range(3):
        iteration()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        iteration()
        n += 1
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    k = 50 if cores > 1 else 10
    orc.collect_loop(ring, obs.copy(), np.zeros((n_envs, 2), np.float32), steps.copy(), reset, k, cores)
    env_only = k * n_envs / (time.perf_counter() - t1)
    return dict(value=round(n * n_envs / dt, 1), unit="env-steps/s", cores=cores, kind="port",
                sample=f"{n} learn() iterations of {n_envs} envs + 1 gradient step (batch {batch}) in {dt:.1f} s: C oracle env step/ring/"
                       f"MT19937 sampler (OpenMP, {cores} threads) + torch-CPU SAC step ({cores} threads)",
                env_only_value=round(env_only, 1), ms_per_iteration=round(1e3 * dt / n, 3))


def variant_run(n_envs: int, device: str, graph: bool, obs_dim: int = 8, integrator: str = "rk4", mlp_on_rocblas: bool = False,
                algo: str = "sac", unroll: int = 8, warm: int = 30, steps: int = 160) -> dict:
    """The same loop as the headline on another configuration (rank 0, one GPU, short run):
      * north_star-literal SAC: 8-dim state + batched RK4 (the reference: 4-dim obs, forward Euler), obs =
        [normalised | raw]; and "MLP forward/backward on PyTorch-ROCm": every GEMM left to rocBLAS (CSTR_FUSED_LINEAR=0)
        instead of the hand-written f32-MFMA kernels (DESIGN D8);
      * BASELINE config 3: TD3 class defaults on the same 4096 envs (two graphs: the delayed policy update);
      * BASELINE config 5: MADDPG, 4 agents (one per reactor) on the 8-obs / 4-act twin-train env (two reactor trains side by side
        per env), 1024 envs, class-default nets [400, 300];
      * the headline configuration with ONE iteration per hipGraph (`unroll=1`)."""
    from core.common import fused
    from core.common.callbacks import NoopCallback
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC
    from core.td3 import TD3

    fused_before = fused.USE_FUSED_LINEAR
    if mlp_on_rocblas:
        fused.USE_FUSED_LINEAR = False
    steps = -(-steps // (2 * unroll)) * (2 * unroll)  # whole graphs of both policy-delay phases
    if algo == "maddpg":
        from core.maddpg import MADDPG

        env = CSTRVecEnv(n_envs, obs_dim=8, twin=True, integrator=integrator, device=device)
        model = MADDPG(4, "MlpPolicy", env, [[0, 1], [2, 3], [4, 5], [6, 7]], [[0], [1], [2], [3]], learning_rate_list=[1e-3] * 4,
                       seed=0, device=device)
        what = f"4 agents, {n_envs} envs, twin-train env: obs 8 / act 4, {integrator}, nets [400,300], ring {model.replay_buffer.buffer_size}x{n_envs}"
    else:
        env = CSTRVecEnv(n_envs, obs_dim=obs_dim, integrator=integrator, device=device)
        model = (SAC if algo == "sac" else TD3)("MlpPolicy", env, seed=0, device=device)
        what = f"{n_envs} envs, obs {obs_dim} / act 2, {integrator}" + (", every MLP GEMM on PyTorch-ROCm (rocBLAS)" if mlp_on_rocblas else "")
    _, cb = model._setup_learn((warm + steps) * n_envs, NoopCallback(), True, "bench", False)
    model.enable_graph_capture(graph, unroll=unroll)

    def run_steps(k):  # learn()'s while loop for exactly k vec-steps (a replayed graph may cover several: never past the target)
        target = model.num_timesteps + k * n_envs
        model._total_timesteps = target
        while model.num_timesteps < target:
            model._learn_iteration(cb, None)
        assert model.num_timesteps == target

    run_steps(warm)
    if graph:  # until a whole call of the timed shape replays (every policy-delay phase's graph recorded), untimed
        for _ in range(40):
            before = model.graph_status()["eager_iterations"]
            run_steps(2 * unroll)
            if model.graph_status()["eager_iterations"] == before or not model._graph_enabled:
                break
    st0 = model.graph_status()
    th.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(steps)
    th.cuda.synchronize()
    dt = time.perf_counter() - t0
    st1 = model.graph_status()
    fused.USE_FUSED_LINEAR = fused_before
    launches = st1["abi_launches_per_iteration"]
    return dict(workload=f"{algo.upper()} class defaults, {what}, batch 256", steps=steps,
                value=round(steps * n_envs / dt, 1), unit="env-steps/s", ms_per_step=round(1e3 * dt / steps, 4), graph_unroll=unroll if graph else 0,
                eager_iterations_in_timed_region=st1["eager_iterations"] - st0["eager_iterations"],
                launches_per_iteration=round(sum(launches.values()) / max(len(launches), 1), 2) if launches else None)


def iteration_model(algo: str, n_envs: int, obs_dim: int, act_dim: int, batch: int, hidden=(256, 256), n_critic_params: int = 0) -> dict:
    """Algorithmic bytes and FLOPs of one SAC iteration (2 FLOP per multiply-add, biases / activations / losses not counted).
    bytes: env step + ring row 2 x (8 D + 4 A + 12) per env-step; sampler gather B x that (read + write); TD target 6 x 4 B per
    sample; soft update 12 B per critic parameter. FLOPs: rollout policy N rows; actor forward on 2B rows (obs and next_obs); four
    Q networks forward on B rows; the two critics' backward (dX + dW ~ 2 x forward); actor loss: two Q networks forward + dX on B
    rows, actor backward (dX + dW) on B rows."""
    d, a, (h1, h2) = obs_dim, act_dim, hidden
    row = 2 * 4 * d + 4 * a + 12
    by = dict(env_and_ring=2 * row * n_envs, sampler=2 * batch * row, td_target=24 * batch, soft_update=12 * n_critic_params)
    actor = 2.0 * (d * h1 + h1 * h2 + h2 * 2 * a)
    q = 2.0 * ((d + a) * h1 + h1 * h2 + h2)
    fl = dict(rollout_policy=actor * n_envs, actor_fwd_2B=actor * 2 * batch, critics_and_targets_fwd=4 * q * batch, critics_bwd=2 * 2 * q * batch,
              actor_loss_critics_fwd_dx=2 * 2 * q * batch, actor_bwd=2 * actor * batch)
    return dict(bytes=by, bytes_total=sum(by.values()), flops=fl, flops_total=sum(fl.values()))


def dump_outputs(model, env, out_dir: str) -> None:
    """What the last timed step left for a caller of learn(), as out_dir/<name>.npy (float32): the policy's state_dict
    (actor, critics, targets), SAC's log entropy coefficient, the envs' observations and the replay-ring row that step wrote."""
    th.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    arrays = {f"policy.{k}": v for k, v in model.policy.state_dict().items() if v.is_floating_point()}
    if getattr(model, "log_ent_coef", None) is not None:
        arrays["log_ent_coef"] = model.log_ent_coef
    arrays["env_obs"] = env.obs
    ring = model.replay_buffer.ring
    row = (int(ring.ctl[0]) - 1) % ring.rows  # ring_ctl = {pos, full, ticket, adds}: pos is the next row to write
    for name in ("observations", "next_observations", "actions", "rewards", "dones"):
        arrays[f"ring_last_row.{name}"] = getattr(ring, name)[row]
    total = 0
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        total += a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)
    assert total <= 64 << 20, f"--dump-outputs wrote {total} bytes (limit 64 MB)"


def launch_ranks(args) -> int:
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes of this file (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set), relay rank 0's JSON line, return non-zero unless every rank exited 0 and the line says n_gpus == N.
    Nothing here touches the GPU (`torch.cuda.device_count()` only counts devices) and nothing re-execs this process."""
    import socket
    import subprocess
    import tempfile

    n = args.gpus
    single = os.environ.get("CSTR_BENCH_SINGLE_DEVICE") == "1"  # rehearsal: N ranks on cuda:0 (gloo transport)
    have = th.cuda.device_count()
    if not single and have < n:
        print(f"bench.py: --gpus {n} but this node exposes {have} GPU(s); refusing to report a {n}-GPU number", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
               OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"), CSTR_BENCH_SPAWNED="1")
    limit = float(os.environ.get("CSTR_BENCH_LAUNCH_TIMEOUT_S", "1500"))  # wall clock for the whole job
    out0 = tempfile.TemporaryFile()  # rank 0's stdout (ONE line) -- a file, so that nobody blocks on a full pipe while we poll
    procs = []
    for r in range(n):
        renv = dict(env, RANK=str(r), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(n))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=renv,
                                      stdout=out0 if r == 0 else sys.stderr, start_new_session=True))
    # poll ALL children: the first rank that dies (bad device, out of memory, an exception during start-up) would otherwise leave
    # the others waiting in the rendezvous / a collective until the backend's timeout. These are fresh children of this
    # (GPU-free) parent: terminating them is an ordinary signal, nothing is re-exec'ed.
    t0, failed = time.monotonic(), None
    while True:
        codes = [p.poll() for p in procs]
        bad = [r for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            failed = f"rank {bad[0]} exited with code {codes[bad[0]]}"
        elif time.monotonic() - t0 > limit:
            failed = f"no result after {limit:.0f} s"
        if failed or all(c == 0 for c in codes):
            break
        time.sleep(0.05)
    if failed:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        t1 = time.monotonic()
        while any(p.poll() is None for p in procs) and time.monotonic() - t1 < 10:
            time.sleep(0.05)
        for p in procs:
            if p.poll() is None:
                p.kill()
        codes = [p.wait() for p in procs]
        print(f"bench.py: {failed}; siblings terminated; rank exit codes {codes}", file=sys.stderr)
        return 1
    out0.seek(0)
    out0 = out0.read()
    lines = [ln for ln in out0.decode().splitlines() if ln.strip().startswith("{")]
    if any(codes) or len(lines) != 1:
        print(f"bench.py: rank exit codes {codes}, {len(lines)} JSON line(s) from rank 0", file=sys.stderr)
        return 1
    rec = json.loads(lines[0])
    if rec.get("n_gpus") != n or rec.get("rccl_world") != n:
        print(f"bench.py: asked for {n} ranks, the job ran n_gpus={rec.get('n_gpus')} rccl_world={rec.get('rccl_world')}", file=sys.stderr)
        return 1
    sys.stdout.write(lines[0] + "\n")
    sys.stdout.flush()
    return 0


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args))
    # stdout carries exactly ONE line, the JSON result: libraries that print to fd 1 (RCCL's version banner on rank 0) go to stderr
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    from core.common import distributed as dist_util

    # rehearsal knobs (a 1-GPU box): CSTR_DIST_BACKEND=gloo + CSTR_BENCH_SINGLE_DEVICE=1 run N ranks on cuda:0 over gloo, which
    # exercises this file's multi-rank path (RCCL refuses two ranks on one device); the driver's real runs use neither
    if os.environ.get("CSTR_BENCH_FAIL_RANK") == os.environ.get("RANK", "0") and "WORLD_SIZE" in os.environ:
        # test knob (tests/test_bench_contract.py): this rank dies during start-up, before the rendezvous
        print(f"[bench] rank {os.environ.get('RANK')}: injected start-up failure (CSTR_BENCH_FAIL_RANK)", file=sys.stderr)
        raise SystemExit(7)
    rank, local_rank, world = dist_util.init_from_env(os.environ.get("CSTR_DIST_BACKEND"))
    if os.environ.get("CSTR_BENCH_SINGLE_DEVICE") == "1":
        local_rank = 0
    if world > 1:
        print(f"[bench] rank {rank}/{world} on cuda:{local_rank} ok ({th.distributed.get_backend()} process group up)", file=sys.stderr, flush=True)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: refusing to label a {world}-rank run as {args.gpus} GPUs")
    assert th.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    th.cuda.set_device(local_rank)
    from core import _native as nv
    from core.common.callbacks import NoopCallback
    from core.common.vec_env import CSTRVecEnv
    from core.sac import SAC
    from core.td3 import TD3

    nv.lib()
    from core.common import blas

    blas.configure(args.blas)
    N, B = args.n_envs, 256
    if args.algo == "maddpg":  # BASELINE config 5: 4 agents (one per reactor) on the twin-train 8-obs / 4-act env
        from core.maddpg import MADDPG

        env = CSTRVecEnv(N, obs_dim=8, twin=True, integrator=args.integrator, device=f"cuda:{local_rank}")
        model = MADDPG(4, "MlpPolicy", env, [[0, 1], [2, 3], [4, 5], [6, 7]], [[0], [1], [2], [3]], learning_rate_list=[1e-3] * 4,
                       seed=0, device=f"cuda:{local_rank}")
    else:
        env = CSTRVecEnv(N, obs_dim=args.obs_dim, integrator=args.integrator, device=f"cuda:{local_rank}")
        cls = SAC if args.algo == "sac" else TD3
        model = cls("MlpPolicy", env, seed=0, device=f"cuda:{local_rank}")  # class defaults: buffer 1e6 -> 244 rows x 4096
    if os.environ.get("CSTR_BENCH_FORCE_DP") == "1" and world == 1:
        # rehearsal knob (a 1-GPU box): the N > 1 launch structure -- graph segments with an RCCL all-reduce on each gradient
        # arena between them -- in a world of one rank: measures what segmentation + the process group's enqueue cost
        th.distributed.init_process_group("nccl", init_method="tcp://127.0.0.1:29533", rank=0, world_size=1,
                                          device_id=th.device("cuda", local_rank))
        dist_util.is_distributed = lambda: True
        model._force_segment_boundaries = True
        if os.environ.get("CSTR_GRAPH_COLLECTIVES", "auto") == "auto":
            model._graph_collectives = dist_util.graph_collectives_ok(model.device)  # the start-up trial itself
            print(f"[bench] collectives inside the graph: {model._graph_collectives}", file=sys.stderr)
    env_obs_dim, env_act_dim, ring_rows = env.obs_dim, env.act_dim, model.replay_buffer.buffer_size
    total = (args.warmup + args.steps) * N
    _, callback = model._setup_learn(total, NoopCallback(), True, "bench", False)
    use_graph = bool(args.graph)  # world > 1: graph segments with the RCCL all-reduces between them
    model.enable_graph_capture(use_graph, unroll=args.graph_unroll)  # world > 1: multi-iteration graphs only with in-graph collectives
    if os.environ.get("CSTR_BENCH_BREAK_CAPTURE") == "1":  # test knob (tests/test_bench_contract.py): the recorded body raises
        body = model._graph_body

        def broken_body():
            body()
            if th.cuda.is_current_stream_capturing():
                raise RuntimeError("injected capture failure (CSTR_BENCH_BREAK_CAPTURE)")

        model._graph_body = broken_body
    if args.tunable:  # development: record / eager-tune every GEMM shape (input of tools/tune_gemms.py)
        th.cuda.tunable.enable(True)
        th.cuda.tunable.tuning_enable(True)
        th.cuda.tunable.set_filename(os.path.join(ROOT, "gpurun_out", "tunableop_results.csv"))

    def run_steps(k):  # exactly OffPolicyAlgorithm.learn()'s while loop, for k vec-steps (one call may replay several)
        target = model.num_timesteps + k * N
        model._total_timesteps = target  # learn(total_timesteps): unrolled graphs never run past it
        while model.num_timesteps < target:
            model._learn_iteration(callback, None)
        assert model.num_timesteps == target

    def barrier():
        th.cuda.synchronize()
        if world > 1:
            th.distributed.barrier()
        th.cuda.synchronize()

    def agreed_max(x: float) -> float:  # MAX over ranks (every rank takes the same decisions from it)
        if world == 1:
            return x
        t = th.tensor([x], dtype=th.float64, device=model.device)
        th.distributed.all_reduce(t, op=th.distributed.ReduceOp.MAX)
        return float(t)

    run_steps(args.warmup)
    # --warmup is honoured as given; if hipGraph replay was requested and the graphs of every phase are not recorded yet
    # (3 side-stream iterations + the capture per phase; TD3 / MADDPG have two phases) keep warming up, untimed and reported
    prewarm = 0
    if use_graph:
        # every graph the timed region can need: `unroll`-iteration graphs (one per policy-delay phase) and, when K is not a multiple
        # of the unroll factor, the unroll / 2, unroll / 4, ... 1-iteration ones for the tail -- run both call shapes until a whole call replays
        dp = world > 1 or getattr(model, "_force_segment_boundaries", False)
        u = model.graph_unroll if (not dp or model._collectives_in_graph()) else 1
        # (an odd call length flips the policy-delay phase a call starts in: two clean calls in a row cover both)
        for k in ([2 * u] if args.steps % u == 0 else [2 * u, 2 * u + args.steps % u]):
            clean = 0
            for _ in range(40):
                before = model.graph_status()["eager_iterations"]
                run_steps(k)
                prewarm += k
                clean = clean + 1 if model.graph_status()["eager_iterations"] == before else 0
                if not model._graph_enabled or clean >= (2 if k % 2 else 1):
                    break
    st0 = model.graph_status()
    barrier()
    t0 = time.perf_counter()
    run_steps(args.steps)
    host_dt = time.perf_counter() - t0  # host time to ENQUEUE the K steps (before the closing synchronize): ~ ms_per_step means host-bound
    barrier()
    dt = agreed_max(time.perf_counter() - t0)  # seconds per K steps
    timed_steps = args.steps
    st1 = model.graph_status()
    graph_replays = st1["replays"] - st0["replays"]
    eager_in_timed = st1["eager_iterations"] - st0["eager_iterations"]
    if args.dump_outputs and rank == 0:
        dump_outputs(model, env, args.dump_outputs)
    # proof of the rank count: a summing all-reduce on the job's backend, and the weights of every rank after training
    checksum = dict(expected=world * (world + 1) // 2, got=rank + 1, backend="none")
    weights_identical = None
    if world > 1:
        t = th.tensor([float(rank + 1)], dtype=th.float64, device=model.device)
        th.distributed.all_reduce(t)
        checksum.update(got=int(t), backend=th.distributed.get_backend())
        flats = [p.detach().reshape(-1) for p in model.policy.parameters()]
        if getattr(model, "log_ent_coef", None) is not None:
            flats.append(model.log_ent_coef.detach().reshape(-1))
        h = th.stack([f.double().sum() for f in flats] + [f.double().abs().sum() for f in flats])
        hmax, hmin = h.clone(), h.clone()
        th.distributed.all_reduce(hmax, op=th.distributed.ReduceOp.MAX)
        th.distributed.all_reduce(hmin, op=th.distributed.ReduceOp.MIN)
        weights_identical = bool(th.equal(hmax, hmin))
    value = args.steps * N * world / dt
    rccl_world = th.distributed.get_world_size() if th.distributed.is_initialized() else 1
    line = {
        "metric": "env-steps/sec (SAC, two-series CSTR, 4096 vec-envs) at 1/2/4/8 GPUs" if args.algo == "sac" else
                  f"env-steps/sec ({args.algo.upper()}, two-series CSTR, {N} vec-envs)",
        "value": round(value, 1), "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic", "rccl_world": rccl_world, "allreduce_checksum": checksum,
        "weights_identical_across_ranks": weights_identical, "graph_collectives": st1["graph_collectives"],
        "host_enqueue_ms_per_step": round(1e3 * host_dt / args.steps, 4),
        "timed_steps_total": timed_steps, "timed_seconds_total": round(dt, 6),
        "graph_prewarm_steps": prewarm, "hip_graph_active": st1["active"], "hip_graph_replays_in_timed_region": graph_replays,
        "eager_iterations_in_timed_region": eager_in_timed, "hip_graph_error": st1["error"],
        "config": {"workload": f"{args.algo.upper()} MlpPolicy class defaults on {N} vectorised two-series CSTR envs per GPU "
                               f"(obs {env_obs_dim}/act {env_act_dim}{' twin-train env, 4 agents' if args.algo == 'maddpg' else ''}, {args.integrator}, batch 256, "
                               f"ring {ring_rows}x{N}, 1 gradient step per vec-step; hipGraph replay, {args.graph_unroll} iterations per graph)",
                   "n_envs_per_gpu": N, "global_batch": B * world, "parallelism": f"dp{world}", "hip_graph": bool(st1["active"]), "hip_graph_requested": use_graph, "hip_graph_segments": st1["segments_per_graph"], "graph_unroll": (model.graph_unroll if (world == 1 and not getattr(model, "_force_segment_boundaries", False)) or st1["graph_collectives"] == "in-graph" else 1) if use_graph else 0, "blas": args.blas,
                   "n_updates": model._n_updates},
    }
    if rank == 0:
        launches = st1["abi_launches_per_iteration"]
        n_launch = round(sum(launches.values()) / max(len(launches), 1), 2) if launches else None
        if args.full:
            line["reference_python_env_steps_per_s"] = {
                "value": REFERENCE_PYTHON_ENV_STEPS_PER_S, "provenance": "unmodified reference SAC.learn() on DummyVecEnv(4096), survey "
                "container, 8 CPU cores, no GPU (SURVEY 6 / BASELINE.md 2); not re-measurable here (the reference is not part of this "
                "repository)", "cross_machine_ratio": round(value / REFERENCE_PYTHON_ENV_STEPS_PER_S, 1)}
        if args.full and not args.no_roofline and args.algo != "maddpg":
            rc = roofline_collect(N, args.obs_dim, args.integrator, 500)
            rc["note"] = ("the fused collect kernel ALONE (the eager path's and MADDPG's launch; inside captured SAC / TD3 iterations it is "
                          "part of rollout_step_kernel): 4096 envs x 104 B = 426 KB per launch, cache-resident and launch-latency-bound; "
                          "roofline_stream is the bandwidth-bound regime of the same kernel")
            rc["traffic_source"] = "profiles/r01_collect_pmc.json (committed rocprofv3 --pmc passes; not measured in this run)"
            line["roofline_collect"] = rc
            line["roofline_stream"] = roofline_collect(1 << 22, args.obs_dim, args.integrator, 30)
            line["roofline_stream"]["traffic_source"] = rc["traffic_source"]
            line["kernels"] = other_kernels(model, B)
            pk = line["kernels"]["policy_rows_fwd_kernel"]  # the stand-alone whole-policy launch (eager path, MADDPG)
            bench_shape = pk["shape"] == [4096, 4, 256, 256, 4]

            def committed_traffic(fname, *keys):  # HBM bytes per launch from the committed PMC passes, bench shape only
                if not bench_shape:
                    return None, None
                for rnd in ("r03", "r02"):
                    try:
                        with open(os.path.join(ROOT, "profiles", f"{rnd}_{fname}")) as fh:
                            v = json.load(fh)
                        for k in keys:
                            v = v[k]
                        return v, f"profiles/{rnd}_{fname} (committed rocprofv3 --pmc passes: FETCH_SIZE x 2 on gfx950 + WRITE_SIZE; not measured in this run)"
                    except (OSError, KeyError, ValueError, TypeError):
                        continue
                return None, None

            traffic, tsrc = committed_traffic("policy_pmc.json", "policy_rows_fwd_kernel", "4096", "traffic_bytes")
            line["roofline_mfma"] = dict(bound="mfma", kernel="policy_rows_fwd_kernel", achieved=pk["tflops"], peak=F32_MFMA_PEAK_TFLOPS,
                                         unit="TFLOP/s", frac=pk["frac"], traffic=traffic, traffic_source=tsrc, launch_us=pk["launch_us"], shape=pk["shape"],
                                         note="the stand-alone whole-policy launch (not in the replayed SAC / TD3 graph; MADDPG's and the eager path's launch)")
            rk = line["kernels"].get("rollout_step_kernel")
            if rk is not None:  # THE dominant kernel of the replayed graph: the same matrix work + the env step + the index draw
                rtraffic, rsrc = committed_traffic("rollout_pmc.json", "traffic_bytes")
                n_rows, k0, h1, h2, a2 = rk["shape"]
                flops = 2.0 * n_rows * (k0 * h1 + h1 * h2 + h2 * a2)
                w_bytes = 4 * (k0 * h1 + h1 + h1 * h2 + h2 + h2 * a2 + a2)
                env_bytes = n_rows * 2 * (2 * 4 * k0 + 4 * (a2 // 2) + 12)
                alg_bytes = env_bytes + w_bytes
                gbs = alg_bytes / rk["launch_us"] / 1e3
                line["roofline"] = dict(
                    bound="mfma", kernel="rollout_step_kernel", achieved=rk["tflops"], peak=F32_MFMA_PEAK_TFLOPS, unit="TFLOP/s", frac=rk["frac"],
                    traffic=rtraffic, traffic_source=rsrc, launch_us=rk["launch_us"], shape=rk["shape"], flops_per_launch=flops,
                    hbm=dict(algorithmic_bytes_per_launch=alg_bytes, env_and_ring_bytes=env_bytes, weight_bytes=w_bytes, achieved=round(gbs, 2),
                             peak=HBM_PEAK_GBS, unit="GB/s", frac=round(gbs / HBM_PEAK_GBS, 5),
                             traffic_over_algorithmic=None if rtraffic is None else round(rtraffic / alg_bytes, 2),
                             note="104 B per env-step (SURVEY 8d) + the policy weights once; at 4096 envs the launch is matrix-core / latency "
                                  "bound, the HBM fraction is printed only to say so"),
                    note="dominant kernel of the replayed graph: policy network (the MFMA work priced here) + fused collect step of all envs + "
                         "replay index draw in ONE launch; duration = HIP events around graph-replayed back-to-back launches on the launch stream")
                line["roofline_mfma"]["as_launched"] = dict(kernel="rollout_step_kernel", achieved=rk["tflops"], frac=rk["frac"], launch_us=rk["launch_us"],
                                                            traffic=rtraffic, traffic_source=rsrc)
            else:
                line["roofline"] = rc
        if args.full and args.algo == "sac":
            n_crit = sum(p.numel() for p in model.critic.parameters())
            im = iteration_model("sac", N, args.obs_dim, 2, B, (256, 256), n_crit)
            ms = line["ms_per_step"]
            gbs, tfl = im["bytes_total"] / ms / 1e6, im["flops_total"] / ms / 1e9
            line["roofline_iteration"] = dict(
                algorithmic_bytes=im["bytes_total"], bytes_by_part=im["bytes"], achieved_gbs=round(gbs, 2), hbm_peak_gbs=HBM_PEAK_GBS,
                hbm_frac=round(gbs / HBM_PEAK_GBS, 5), algorithmic_flops=im["flops_total"], flops_by_part=im["flops"], achieved_tflops=round(tfl, 2),
                mfma_f32_peak_tflops=F32_MFMA_PEAK_TFLOPS, mfma_frac=round(tfl / F32_MFMA_PEAK_TFLOPS, 4), launches_per_iteration=n_launch,
                mean_launch_interval_us=None if not n_launch else round(1e3 * ms / n_launch, 3),
                note="whole iteration / ms_per_step: launch-latency-bound (a chain of dependent sub-10-us launches), far from either roofline; "
                     "launches = C-ABI launches recorded into the graph per iteration (rocprofv3 cross-check: tools/count_launches.sh)")
        line["config"]["launches_per_iteration"] = n_launch
        if args.full and world == 1 and not args.no_variant and args.algo == "sac" and (args.obs_dim, args.integrator) == (4, "euler"):
            del model, env
            dev = f"cuda:{local_rank}"
            u = args.graph_unroll
            line["north_star_variant"] = variant_run(N, dev, use_graph, unroll=u)
            line["mlp_on_pytorch_rocm_variant"] = variant_run(N, dev, use_graph, 4, "euler", mlp_on_rocblas=True, unroll=u)
            line["unroll1_variant"] = variant_run(N, dev, use_graph, 4, "euler", unroll=1, steps=320)
            line["td3_variant"] = variant_run(N, dev, use_graph, 4, "euler", algo="td3", unroll=u, warm=40, steps=320)
            line["maddpg_variant"] = variant_run(1024, dev, use_graph, 8, "euler", algo="maddpg", unroll=u, warm=40, steps=160)
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(N, B, args.cpu_seconds)
            line["speedup_vs_cpu_port"] = round(value / line["cpu_baseline"]["value"], 2)
        os.write(result_fd, (json.dumps(line) + "\n").encode())
    if world > 1:
        th.distributed.barrier()
    if th.distributed.is_initialized():
        th.distributed.destroy_process_group()
    problems = []
    if use_graph and (not st1["active"] or eager_in_timed or graph_replays != timed_steps):
        problems.append(f"hipGraph replay requested but the timed region ran {eager_in_timed} eager / {graph_replays} replayed of {timed_steps} "
                        f"iterations (capture error: {st1['error']})")
    if checksum["got"] != checksum["expected"]:
        problems.append(f"all-reduce checksum {checksum}")
    if weights_identical is False:
        problems.append("weights differ between ranks after training")
    if world > 1 and os.environ.get("CSTR_DIST_BACKEND") is None and checksum["backend"] != "nccl":
        problems.append(f"multi-GPU run on backend {checksum['backend']!r}, not RCCL")
    if problems:
        print("bench.py: INVALID RUN -- " + "; ".join(problems), file=sys.stderr)
        raise SystemExit(3)


if __name__ == "__main__":
    main()
