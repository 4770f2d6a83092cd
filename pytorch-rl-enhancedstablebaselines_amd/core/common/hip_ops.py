"""Torch-tensor front end of the C ABI (include/cstr_rl_hip.h).

Every wrapper validates shape / dtype / device / contiguity on the host before the launch (a
mis-shaped operand must never reach a hand-written kernel), passes raw device pointers and the
current HIP stream, and raises on a non-zero return code. Nothing here computes on the CPU.
"""
import ctypes as C
import math
from typing import Optional

import torch as th

from core import _native as nv
from core._native import INTEGRATORS, check, ptr, stream_ptr


def _chk(t: th.Tensor, name: str, shape, dtype) -> th.Tensor:
    if not isinstance(t, th.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live in HBM (device tensor); got device {t.device}. No CPU fallback exists.")
    if t.device.index != th.cuda.current_device():  # a pointer from another GPU must never reach a launch on this one
        raise ValueError(f"{name}: lives on {t.device}, the current device is cuda:{th.cuda.current_device()}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


LAYOUTS = ((4, 2), (8, 2), (8, 4))


def _opt(t: Optional[th.Tensor], name, shape, dtype):
    return None if t is None else _chk(t, name, shape, dtype)


class DeviceRing:
    """cstr_ring_t + ring_ctl over torch tensors (HBM). Field arrays have the reference's shapes
    (core/common/buffers.py:212-234): [rows, n_envs, D] / [rows, n_envs, A] / [rows, n_envs]."""

    def __init__(self, rows: int, n_envs: int, obs_dim: int, act_dim: int, device):
        if (obs_dim, act_dim) not in LAYOUTS:
            raise ValueError(f"DeviceRing supports (obs_dim, act_dim) in (4,2), (8,2), (8,4) (CSTR layouts), got {obs_dim}/{act_dim}")
        z = lambda *s: th.zeros(*s, dtype=th.float32, device=device)  # noqa: E731
        self.observations, self.next_observations = z(rows, n_envs, obs_dim), z(rows, n_envs, obs_dim)
        self.actions = z(rows, n_envs, act_dim)
        self.rewards, self.dones, self.timeouts = z(rows, n_envs), z(rows, n_envs), z(rows, n_envs)
        self.ctl = th.zeros(nv.RING_CTL_WORDS, dtype=th.int64, device=device)  # {pos, full, ticket, adds}
        self.rows, self.n_envs, self.obs_dim, self.act_dim = rows, n_envs, obs_dim, act_dim
        self.c = nv.Ring(self.observations.data_ptr(), self.next_observations.data_ptr(), self.actions.data_ptr(),
                         self.rewards.data_ptr(), self.dones.data_ptr(), self.timeouts.data_ptr(), rows, n_envs,
                         obs_dim, act_dim)


def vec_step(coef, integrator: str, obs, act, step_count, reset_obs, next_obs, obs_after, reward, done, timeout):
    n, d = obs.shape
    a = act.shape[-1]
    if (d, a) not in LAYOUTS:
        raise ValueError(f"(obs_dim, act_dim) = {(d, a)} is not a CSTR layout {LAYOUTS}")
    _chk(obs, "obs", (n, d), th.float32), _chk(act, "act", (n, a), th.float32)
    _chk(step_count, "step_count", (n,), th.int32), _chk(reset_obs, "reset_obs", (n, d), th.float32)
    _chk(next_obs, "next_obs", (n, d), th.float32), _chk(obs_after, "obs_after", (n, d), th.float32)
    for t, nm in ((reward, "reward"), (done, "done"), (timeout, "timeout")):
        _chk(t, nm, (n,), th.float32)
    check(nv.lib().cstr_vec_step_f32(C.byref(coef), C.c_int(INTEGRATORS[integrator]), C.c_int(d), C.c_int(a), ptr(obs), ptr(act),
                                     ptr(step_count), ptr(reset_obs), ptr(next_obs), ptr(obs_after), ptr(reward),
                                     ptr(done), ptr(timeout), C.c_int64(n), stream_ptr()), "cstr_vec_step_f32")


def reset_draw(pcg_state, mask, obs_out, act_dim: int = 2, static_init=None):
    n, d = obs_out.shape
    if (d, act_dim) not in LAYOUTS:
        raise ValueError(f"(obs_dim, act_dim) = {(d, act_dim)} is not a CSTR layout {LAYOUTS}")
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64), _chk(obs_out, "obs_out", (n, d), th.float32)
    _opt(mask, "mask", (n,), th.uint8)
    _opt(static_init, "static_init", (n, 8 if act_dim == 4 else 4), th.float64)
    check(nv.lib().cstr_reset_draw_f32(ptr(pcg_state), ptr(mask), ptr(static_init), C.c_int(d), C.c_int(act_dim), ptr(obs_out),
                                       C.c_int64(n), stream_ptr()), "cstr_reset_draw_f32")


def replay_add(ring: DeviceRing, obs, next_obs, act, rew, done, timeout):
    n, d, a = ring.n_envs, ring.obs_dim, ring.act_dim
    _chk(obs, "obs", (n, d), th.float32), _chk(next_obs, "next_obs", (n, d), th.float32), _chk(act, "act", (n, a), th.float32)
    for t, nm in ((rew, "rew"), (done, "done"), (timeout, "timeout")):
        _chk(t, nm, (n,), th.float32)
    check(nv.lib().cstr_replay_add_f32(C.byref(ring.c), ptr(ring.ctl), ptr(obs), ptr(next_obs), ptr(act), ptr(rew),
                                       ptr(done), ptr(timeout), stream_ptr()), "cstr_replay_add_f32")


def collect_step(coef, integrator: str, ring: DeviceRing, env_obs, step_count, policy_out, squashed, act_low,
                 act_high, noise=None, reset_obs=None, pcg_state=None, reward_out=None, done_out=None, ep_return=None,
                 ep_stats=None, static_init=None, rng_advance=None):
    """`rng_advance` = (rng_ctl, count) or None: the Philox control block of the policy launch that produced `policy_out` with
    `defer_rng_advance=True`; this launch's last workgroup advances its offset by `count` (cstr_collect_step_rng_f32)."""
    n, d, a = ring.n_envs, ring.obs_dim, ring.act_dim
    _chk(env_obs, "env_obs", (n, d), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(policy_out, "policy_out", (n, a), th.float32)
    _opt(noise, "noise", (n, a), th.float32), _opt(reset_obs, "reset_obs", (n, d), th.float32)
    _opt(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64)
    _opt(static_init, "static_init", (n, 8 if a == 4 else 4), th.float64)
    if static_init is not None and pcg_state is None:
        raise ValueError("static_init (init_mode='static') needs the per-env pcg_state reset source")
    _opt(reward_out, "reward_out", (n,), th.float32), _opt(done_out, "done_out", (n,), th.float32)
    _opt(ep_return, "ep_return", (n,), th.float32), _opt(ep_stats, "ep_stats", (4,), th.float64)
    if (ep_return is None) != (ep_stats is None):
        raise ValueError("ep_return and ep_stats go together")
    if (reset_obs is None) == (pcg_state is None):
        raise ValueError("collect_step needs exactly one reset source: reset_obs or pcg_state")
    if len(act_low) != a or len(act_high) != a:
        raise ValueError(f"act_low/act_high need {a} entries")
    lo = (C.c_float * a)(*[float(v) for v in act_low])
    hi = (C.c_float * a)(*[float(v) for v in act_high])
    rng_ctl, rng_count = rng_advance if rng_advance is not None else (None, 0)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_collect_step_rng_f32(C.byref(coef), C.c_int(INTEGRATORS[integrator]), C.byref(ring.c), ptr(ring.ctl),
                                             ptr(env_obs), ptr(step_count), ptr(policy_out), C.c_int(int(squashed)), lo, hi,
                                             ptr(noise), ptr(reset_obs), ptr(pcg_state), ptr(static_init), ptr(reward_out), ptr(done_out),
                                             ptr(ep_return), ptr(ep_stats), ptr(rng_ctl), C.c_uint64(int(rng_count)), stream_ptr()),
          "cstr_collect_step_rng_f32")


def mt19937_seed(mt_state, seed: int):
    _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32)
    check(nv.lib().cstr_mt19937_seed(ptr(mt_state), C.c_uint32(seed & 0xFFFFFFFF), stream_ptr()), "cstr_mt19937_seed")


def mt19937_normal(mt_state, loc, scale, out):
    """`out.shape[0]` consecutive np.random.normal(loc, scale).astype(float32) from the device legacy stream
    (reference: core/common/noise.py:44-45, :141-142); out [n, len(loc)] f32."""
    _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32)
    loc, scale = [float(v) for v in loc], [float(v) for v in scale]
    period = len(loc)
    if len(scale) != period or not 1 <= period <= nv.MAX_NOISE_PERIOD:
        raise ValueError(f"loc / scale must have the same length in [1, {nv.MAX_NOISE_PERIOD}]")
    if any(not v >= 0.0 for v in scale):
        raise ValueError("scale < 0")  # numpy's message
    if out.dtype not in (th.float32, th.float64):
        raise ValueError(f"out: dtype {out.dtype}, expected float32 or float64")
    _chk(out, "out", (out.shape[0], period), out.dtype)
    fn = nv.lib().cstr_mt19937_normal_f32 if out.dtype == th.float32 else nv.lib().cstr_mt19937_normal_f64
    check(fn(ptr(mt_state), (C.c_double * period)(*loc), (C.c_double * period)(*scale), C.c_int32(period), ptr(out),
             C.c_int64(out.numel()), stream_ptr()), "cstr_mt19937_normal")


def replay_sample(ring: DeviceRing, mt_state, batch: int, out_obs, out_act, out_next_obs, out_done, out_rew,
                  out_row_idx=None, out_env_idx=None):
    d, a = ring.obs_dim, ring.act_dim
    _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32)
    _chk(out_obs, "out_obs", (batch, d), th.float32), _chk(out_next_obs, "out_next_obs", (batch, d), th.float32)
    _chk(out_act, "out_act", (batch, a), th.float32)
    _chk(out_done, "out_done", (batch, 1), th.float32), _chk(out_rew, "out_rew", (batch, 1), th.float32)
    _opt(out_row_idx, "out_row_idx", (batch,), th.int64), _opt(out_env_idx, "out_env_idx", (batch,), th.int64)
    if not 0 < batch <= nv.MAX_SAMPLE_BATCH:
        raise ValueError(f"batch_size must be in [1, {nv.MAX_SAMPLE_BATCH}], got {batch}")
    check(nv.lib().cstr_replay_sample_mt19937_f32(C.byref(ring.c), ptr(ring.ctl), ptr(mt_state), C.c_int64(batch),
                                                  ptr(out_obs), ptr(out_act), ptr(out_next_obs), ptr(out_done),
                                                  ptr(out_rew), ptr(out_row_idx), ptr(out_env_idx), stream_ptr()),
          "cstr_replay_sample_mt19937_f32")


def vecnorm_init(vn_state):
    _chk(vn_state, "vn_state", (nv.VECNORM_STATE_WORDS,), th.float64)
    check(nv.lib().cstr_vecnorm_init_f64(ptr(vn_state), stream_ptr()), "cstr_vecnorm_init_f64")


def vecnorm_step(cfg, vn_state, returns, obs, reward, done, norm_obs_out=None, norm_reward_out=None):
    """VecNormalize.step_wait / reset (reward=None) on raw device tensors (reference: vec_normalize.py:174-204, :291-307)."""
    n, d = obs.shape
    if d != cfg.obs_dim:
        raise ValueError(f"obs has {d} columns, VecNormalize was built for {cfg.obs_dim}")
    _chk(vn_state, "vn_state", (nv.VECNORM_STATE_WORDS,), th.float64), _chk(returns, "returns", (n,), th.float64)
    _chk(obs, "obs", (n, d), th.float32)
    _opt(reward, "reward", (n,), th.float32), _opt(done, "done", (n,), th.float32)
    _opt(norm_obs_out, "norm_obs_out", (n, d), th.float32), _opt(norm_reward_out, "norm_reward_out", (n,), th.float32)
    if norm_obs_out is not None and norm_obs_out.data_ptr() == obs.data_ptr():
        raise ValueError("norm_obs_out must not alias obs (the raw observation stays available as get_original_obs)")
    if reward is None and (done is not None or norm_reward_out is not None):
        raise ValueError("the reset form (reward=None) takes neither done nor norm_reward_out")
    check(nv.lib().cstr_vecnorm_step_f64(C.byref(cfg), ptr(vn_state), ptr(returns), ptr(obs), ptr(reward), ptr(done),
                                         ptr(norm_obs_out), ptr(norm_reward_out), C.c_int64(n), stream_ptr()), "cstr_vecnorm_step_f64")


def vecnorm_apply(cfg, vn_state, obs, next_obs, reward):
    """normalize_obs / normalize_reward of a sampled batch, in place (reference: buffers.py:143-155, :312-323)."""
    _chk(vn_state, "vn_state", (nv.VECNORM_STATE_WORDS,), th.float64)
    ref = next((t for t in (obs, next_obs, reward) if t is not None), None)
    if ref is None:
        raise ValueError("nothing to normalise")
    b = ref.shape[0]
    _opt(obs, "obs", (b, cfg.obs_dim), th.float32), _opt(next_obs, "next_obs", (b, cfg.obs_dim), th.float32)
    if reward is not None and reward.numel() != b:
        raise ValueError(f"reward has {reward.numel()} entries, batch is {b}")
    _opt(reward, "reward", tuple(reward.shape) if reward is not None else (), th.float32)
    check(nv.lib().cstr_vecnorm_apply_f32(C.byref(cfg), ptr(vn_state), ptr(obs), ptr(next_obs), ptr(reward), C.c_int64(b),
                                          stream_ptr()), "cstr_vecnorm_apply_f32")


def replay_sample_packed(ring: DeviceRing, mt_state, batch: int, x_data, x_next, x_pi, out_done, out_rew, out_row_idx=None,
                         out_env_idx=None):
    """ReplayBuffer.sample gathered straight into the critic-input rows (obs | act), (next_obs | .), (obs | .)."""
    w = ring.obs_dim + ring.act_dim
    _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32)
    _chk(x_data, "x_data", (batch, w), th.float32), _chk(x_next, "x_next", (batch, w), th.float32), _opt(x_pi, "x_pi", (batch, w), th.float32)
    _chk(out_done, "out_done", (batch, 1), th.float32), _chk(out_rew, "out_rew", (batch, 1), th.float32)
    _opt(out_row_idx, "out_row_idx", (batch,), th.int64), _opt(out_env_idx, "out_env_idx", (batch,), th.int64)
    if not 0 < batch <= nv.MAX_SAMPLE_BATCH:
        raise ValueError(f"batch_size must be in [1, {nv.MAX_SAMPLE_BATCH}], got {batch}")
    check(nv.lib().cstr_replay_sample_packed_mt19937_f32(C.byref(ring.c), ptr(ring.ctl), ptr(mt_state), C.c_int64(batch), ptr(x_data),
                                                         ptr(x_next), ptr(x_pi), ptr(out_done), ptr(out_rew), ptr(out_row_idx),
                                                         ptr(out_env_idx), stream_ptr()), "cstr_replay_sample_packed_mt19937_f32")


def replay_gather_packed(ring: DeviceRing, sample_idx, batch: int, x_data, x_next, x_pi, out_done, out_rew, out_row_idx=None,
                         out_env_idx=None, advance_ring: bool = False, rng_advance=None):
    """The gather of `replay_sample_packed` for index pairs drawn by `rollout_step` (sample_idx int32 [2, batch]), plus the control-word
    updates that launch left to this one: ReplayBuffer.add's epilogue (`advance_ring`) and `rng_advance` = (rng_ctl, count)."""
    w = ring.obs_dim + ring.act_dim
    _chk(sample_idx, "sample_idx", (2, batch), th.int32)
    _chk(x_data, "x_data", (batch, w), th.float32), _chk(x_next, "x_next", (batch, w), th.float32), _opt(x_pi, "x_pi", (batch, w), th.float32)
    _chk(out_done, "out_done", (batch, 1), th.float32), _chk(out_rew, "out_rew", (batch, 1), th.float32)
    _opt(out_row_idx, "out_row_idx", (batch,), th.int64), _opt(out_env_idx, "out_env_idx", (batch,), th.int64)
    if not 0 < batch <= nv.MAX_SAMPLE_BATCH:
        raise ValueError(f"batch_size must be in [1, {nv.MAX_SAMPLE_BATCH}], got {batch}")
    rng_ctl, rng_count = rng_advance if rng_advance is not None else (None, 0)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_replay_gather_packed_f32(C.byref(ring.c), ptr(ring.ctl), C.c_int(1 if advance_ring else 0), ptr(rng_ctl),
                                                 C.c_uint64(int(rng_count)), ptr(sample_idx), C.c_int64(batch), ptr(x_data), ptr(x_next),
                                                 ptr(x_pi), ptr(out_done), ptr(out_rew), ptr(out_row_idx), ptr(out_env_idx), stream_ptr()),
          "cstr_replay_gather_packed_f32")


def linear_act_fwd_gather(ring: DeviceRing, sample_idx, batch: int, both: bool, weight, bias, act: int, x_data, x_next, x_pi, out_done,
                          out_rew, advance_ring: bool = False, rng_advance=None, out=None):
    """`replay_gather_packed` fused into the first Linear layer behind it (cstr_linear_act_fwd_gather_f32): y = act(x W^T + b) with
    x = the sampled observations (rows [0, B)) and next observations (rows [B, 2B)) for `both`, else the B next observations; the
    packed batch is written for the later launches and the control words are advanced like `replay_gather_packed` does."""
    d, w = ring.obs_dim, ring.obs_dim + ring.act_dim
    n = weight.shape[0]
    m = 2 * batch if both else batch
    _chk(sample_idx, "sample_idx", (2, batch), th.int32), _chk(weight, "weight", (n, d), th.float32), _chk(bias, "bias", (n,), th.float32)
    _chk(x_data, "x_data", (batch, w), th.float32), _chk(x_next, "x_next", (batch, w), th.float32), _opt(x_pi, "x_pi", (batch, w), th.float32)
    _chk(out_done, "out_done", (batch, 1), th.float32), _chk(out_rew, "out_rew", (batch, 1), th.float32)
    if not 0 < batch <= nv.MAX_SAMPLE_BATCH:
        raise ValueError(f"batch_size must be in [1, {nv.MAX_SAMPLE_BATCH}], got {batch}")
    if out is None:
        out = th.empty(m, n, dtype=th.float32, device=weight.device)
    _chk(out, "out", (m, n), th.float32)
    rng_ctl, rng_count = rng_advance if rng_advance is not None else (None, 0)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_linear_act_fwd_gather_f32(C.byref(ring.c), ptr(ring.ctl), C.c_int(1 if advance_ring else 0), ptr(rng_ctl),
                                                  C.c_uint64(int(rng_count)), ptr(sample_idx), C.c_int64(batch), C.c_int(1 if both else 0),
                                                  ptr(weight), ptr(bias), C.c_int(act), ptr(out), C.c_int64(n), ptr(x_data), ptr(x_next),
                                                  ptr(x_pi), ptr(out_done), ptr(out_rew), stream_ptr()), "cstr_linear_act_fwd_gather_f32")
    return out


def td_target_min(q1, q2, logp, rew, done, ent_coef, gamma: float, out):
    n = q1.numel()
    for t, nm in ((q1, "q1"), (q2, "q2"), (rew, "rew"), (done, "done"), (out, "out")):
        if t.numel() != n:
            raise ValueError(f"{nm}: numel {t.numel()} != {n}")
        _chk(t, nm, t.shape, th.float32)
    if (logp is None) != (ent_coef is None):
        raise ValueError("logp and ent_coef go together (SAC) or are both None (TD3)")
    if logp is not None:
        _chk(logp, "logp", logp.shape, th.float32), _chk(ent_coef, "ent_coef", ent_coef.shape, th.float32)
        if logp.numel() != n or ent_coef.numel() != 1:
            raise ValueError("logp must have n elements and ent_coef exactly one")
    check(nv.lib().cstr_td_target_min_f32(ptr(q1), ptr(q2), ptr(logp), ptr(rew), ptr(done), ptr(ent_coef),
                                          C.c_float(gamma), ptr(out), C.c_int64(n), stream_ptr()), "cstr_td_target_min_f32")


def polyak(param_flat, target_flat, tau: float):
    n = param_flat.numel()
    _chk(param_flat, "param_flat", (n,), th.float32), _chk(target_flat, "target_flat", (n,), th.float32)
    check(nv.lib().cstr_polyak_f32(ptr(param_flat), ptr(target_flat), C.c_double(tau), C.c_int64(n), stream_ptr()),
          "cstr_polyak_f32")


def new_adam_ctl(device, step: int = 0, beta1: float = 0.9, beta2: float = 0.999) -> th.Tensor:
    """adam_ctl = {step, ticket, beta1^step, beta2^step} (the two powers stored as f64 bit patterns in the int64 tensor)."""
    ctl = th.zeros(nv.ADAM_CTL_WORDS, dtype=th.int64, device=device)
    set_adam_step(ctl, step, beta1, beta2)
    return ctl


def set_adam_step(ctl: th.Tensor, step: int, beta1: float = 0.9, beta2: float = 0.999) -> None:
    host = th.zeros(nv.ADAM_CTL_WORDS, dtype=th.int64)
    host[0] = int(step)
    host.view(th.float64)[2] = float(beta1) ** int(step)
    host.view(th.float64)[3] = float(beta2) ** int(step)
    ctl.copy_(host)


def adam(param, grad, exp_avg, exp_avg_sq, adam_ctl, lr_dev, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, nm, (n,), th.float32)
    _chk(adam_ctl, "adam_ctl", (nv.ADAM_CTL_WORDS,), th.int64), _chk(lr_dev, "lr", (1,), th.float64)
    check(nv.lib().cstr_adam_f32(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ptr(adam_ctl), ptr(lr_dev),
                                 C.c_double(beta1), C.c_double(beta2), C.c_double(eps), C.c_float(grad_scale),
                                 C.c_int64(n), stream_ptr()), "cstr_adam_f32")


def _adam_segments(segments):
    """ctypes array of cstr_adam_seg_t from adam_multi's segment tuples."""
    segs = list(segments)
    arr = (nv.AdamSeg * max(len(segs), 1))()
    _fill_adam_segments(arr, segs)
    return arr, len(segs)


def adam_multi(segments):
    """Several flat-arena updates in one launch; `segments` = iterable of adam()'s positional argument tuples (optionally
    followed by a shadow = (tile-major copy tensor, begin, n, k) or None: see policy_swizzle, and by own_target = (target tensor,
    tau): the soft update of THESE parameters' target in the same pass), or ("polyak", source, target, tau) for a soft target
    update of parameters no segment changes (<= 4 segments, mutually independent)."""
    segs = list(segments)
    arr = (nv.AdamSeg * len(segs))()
    _fill_adam_segments(arr, segs)
    check(nv.lib().cstr_adam_multi_f32(arr, C.c_int(len(segs)), stream_ptr()), "cstr_adam_multi_f32")


def _fill_adam_segments(arr, segs) -> None:
    for i, seg in enumerate(segs):
        if seg[0] == "polyak":
            _, source, target, tau = seg
            n = source.numel()
            _chk(source, "source", (n,), th.float32), _chk(target, "target", (n,), th.float32)
            arr[i] = nv.AdamSeg(target.data_ptr(), None, None, None, None, None, 0.0, 0.0, 0.0, 1.0, n, source.data_ptr(), float(tau),
                                None, 0, 0, 0, None)
            continue
        param, grad, exp_avg, exp_avg_sq, adam_ctl, lr_dev, beta1, beta2, eps, grad_scale = seg[:10]
        shadow = seg[10] if len(seg) > 10 else None
        n = param.numel()
        for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            _chk(t, nm, (n,), th.float32)
        _chk(adam_ctl, "adam_ctl", (nv.ADAM_CTL_WORDS,), th.int64), _chk(lr_dev, "lr", (1,), th.float64)
        sh = (None, 0, 0, 0)
        if shadow is not None:
            t, begin, rows, cols = shadow
            if _f32c(t, "shadow").numel() != swizzled_numel(rows, cols) or begin % 4 or cols % 4 or begin + rows * cols > n:
                raise ValueError("shadow: wrong size or position")
            sh = (t.data_ptr(), begin, rows, cols)
        own, tau = (None, 0.0)
        if len(seg) > 11 and seg[11] is not None:
            own, tau = seg[11]
            _chk(own, "own_target", (n,), th.float32)
        arr[i] = nv.AdamSeg(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), adam_ctl.data_ptr(),
                            lr_dev.data_ptr(), beta1, beta2, eps, grad_scale, n, None, float(tau), *sh, None if own is None else own.data_ptr())


# ---- learner glue around the GEMMs (csrc/cstr_mlp.hip) ------------------------------------------------------------
ACT = {"none": 0, "relu": 1, "tanh": 2}


def _f32c(t, name):
    if not (isinstance(t, th.Tensor) and t.is_cuda and t.dtype == th.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: needs a contiguous float32 device tensor")
    return t


def _gmn(t):
    """[m, n] -> (1, m, n); [G, m, n] -> (G, m, n)"""
    if t.dim() == 2:
        return (1, t.shape[0], t.shape[1])
    if t.dim() == 3:
        return tuple(t.shape)
    raise ValueError(f"expected a 2-D or 3-D tensor, got shape {tuple(t.shape)}")


def bias_act_fwd_(y, bias, act: int):
    g, m, n = _gmn(y)
    _f32c(y, "y"), _f32c(bias, "bias")
    if bias.numel() != g * n:
        raise ValueError(f"bias has {bias.numel()} elements, expected {g * n}")
    check(nv.lib().cstr_bias_act_fwd_f32(ptr(y), ptr(bias), C.c_int(act), C.c_int64(g), C.c_int64(m), C.c_int64(n), stream_ptr()),
          "cstr_bias_act_fwd_f32")
    return y


def bias_act_bwd(gy, y, act: int, gz, gbias):
    g, m, n = _gmn(gy)
    _f32c(gy, "gy"), _chk(gz, "gz", gy.shape, th.float32)
    if act != 0:
        _chk(y, "y", gy.shape, th.float32)
    if gbias is not None:
        _f32c(gbias, "gbias")
        if gbias.numel() != g * n:
            raise ValueError(f"gbias has {gbias.numel()} elements, expected {g * n}")
    check(nv.lib().cstr_bias_act_bwd_f32(ptr(gy), ptr(y), C.c_int(act), ptr(gz), ptr(gbias), C.c_int64(g), C.c_int64(m), C.c_int64(n),
                                         stream_ptr()), "cstr_bias_act_bwd_f32")


def bias_act_bwd_rows(gy, y, act: int, gz, gbias=None):
    """`bias_act_bwd` for one group whose gy / y may be column blocks of wider row-major matrices (row-strided views); gz is a
    contiguous [M, N] tensor."""
    m, n = gz.shape
    _chk(gz, "gz", (m, n), th.float32)
    ldg = _rows(gy, "gy", m, n)
    ldy = _rows(y, "y", m, n) if act != 0 else n
    if gbias is not None and _f32c(gbias, "gbias").numel() != n:
        raise ValueError(f"gbias has {gbias.numel()} elements, expected {n}")
    check(nv.lib().cstr_bias_act_bwd_rows_f32(ptr(gy), C.c_int64(ldg), ptr(y if act != 0 else None), C.c_int64(ldy), C.c_int(act), ptr(gz),
                                              ptr(gbias), C.c_int64(m), C.c_int64(n), stream_ptr()), "cstr_bias_act_bwd_rows_f32")
    return gz


def new_rng_ctl(seed: int, device) -> th.Tensor:
    """{seed, offset, ticket, -, sub-tickets[8], -} of the in-kernel Philox stream (cstr_gaussian_head_fwd_f32), int64 bit patterns"""
    return th.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF] + [0] * (nv.RNG_CTL_WORDS - 1), dtype=th.int64).to(device)


def gaussian_head_fwd_(params, bias, eps, rng_ctl, action, logp):
    """params [B, 2A] += bias in place; action [B, A] (row-strided view allowed) = tanh(mean + std * eps); eps is drawn in
    the kernel when rng_ctl is given (and stored for the backward), read otherwise."""
    b, a2 = params.shape
    a = a2 // 2
    _chk(params, "params", (b, 2 * a), th.float32), _chk(eps, "eps", (b, a), th.float32)
    if bias is not None:
        _chk(bias, "bias", (2 * a,), th.float32)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64), _opt(logp, "logp", (b,), th.float32)
    stride = _rows(action, "action", b, a)
    if a > nv.MAX_HEAD_ACT:
        raise ValueError(f"gaussian head supports up to {nv.MAX_HEAD_ACT} action dimensions, got {a}")
    check(nv.lib().cstr_gaussian_head_fwd_f32(ptr(params), ptr(bias), ptr(eps), ptr(rng_ctl), ptr(action), C.c_int64(stride), ptr(logp),
                                              C.c_int64(b), C.c_int(a), stream_ptr()), "cstr_gaussian_head_fwd_f32")


def gaussian_head_gemm_fwd(hidden, weight, bias, params, eps, rng_ctl, action, logp):
    """gaussian_head_fwd_ with the head's Linear inside: params [B, 2A] = hidden @ weight^T + bias is an OUTPUT."""
    b, k = hidden.shape
    a2 = weight.shape[0]
    a = a2 // 2
    if not (hidden.is_cuda and hidden.dtype == th.float32 and hidden.stride(1) == 1):
        raise ValueError("hidden: needs a float32 device matrix with unit column stride")
    _chk(weight, "weight", (a2, k), th.float32), _chk(bias, "bias", (a2,), th.float32)
    _chk(params, "params", (b, a2), th.float32), _chk(eps, "eps", (b, a), th.float32)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64), _opt(logp, "logp", (b,), th.float32)
    stride = _rows(action, "action", b, a)
    check(nv.lib().cstr_gaussian_head_gemm_fwd_f32(ptr(hidden), C.c_int64(hidden.stride(0)), ptr(weight), ptr(bias), ptr(params), ptr(eps),
                                                   ptr(rng_ctl), ptr(action), C.c_int64(stride), ptr(logp), C.c_int64(b), C.c_int(a),
                                                   C.c_int64(k), stream_ptr()), "cstr_gaussian_head_gemm_fwd_f32")


def gaussian_head_bwd(g_action, g_logp, action, params, eps, g_params, g_bias):
    b, a2 = params.shape
    a = a2 // 2
    _chk(params, "params", (b, 2 * a), th.float32), _chk(eps, "eps", (b, a), th.float32), _chk(g_params, "g_params", (b, 2 * a), th.float32)
    _opt(g_logp, "g_logp", (b,), th.float32), _opt(g_bias, "g_bias", (2 * a,), th.float32)
    stride = _rows(action, "action", b, a)
    ga_stride = 0 if g_action is None else _rows(g_action, "g_action", b, a)
    check(nv.lib().cstr_gaussian_head_bwd_f32(ptr(g_action), C.c_int64(ga_stride), ptr(g_logp), ptr(action), C.c_int64(stride),
                                              ptr(params), ptr(eps), ptr(g_params), ptr(g_bias), C.c_int64(b), C.c_int(a), stream_ptr()),
          "cstr_gaussian_head_bwd_f32")


def gaussian_head_bwd_input(g_action, g_logp, action, params, eps, weight, hidden, act: int, g_params, dz):
    """g_params (as gaussian_head_bwd) and dz = (g_params @ weight) * act'(hidden) in one launch; weight [2A, H], hidden [B, H]."""
    b, a2 = params.shape
    a = a2 // 2
    h = weight.shape[1]
    _chk(params, "params", (b, 2 * a), th.float32), _chk(eps, "eps", (b, a), th.float32), _chk(g_params, "g_params", (b, 2 * a), th.float32)
    _chk(weight, "weight", (2 * a, h), th.float32), _chk(dz, "dz", (b, h), th.float32), _opt(g_logp, "g_logp", (b,), th.float32)
    stride = _rows(action, "action", b, a)
    ga_stride = 0 if g_action is None else _rows(g_action, "g_action", b, a)
    ldh = _rows(hidden, "hidden", b, h)
    check(nv.lib().cstr_gaussian_head_bwd_input_f32(ptr(g_action), C.c_int64(ga_stride), ptr(g_logp), ptr(action), C.c_int64(stride),
                                                    ptr(params), ptr(eps), ptr(weight), ptr(hidden), C.c_int64(ldh), C.c_int(act),
                                                    ptr(g_params), ptr(dz), C.c_int64(b), C.c_int(a), C.c_int64(h), stream_ptr()),
          "cstr_gaussian_head_bwd_input_f32")
    return dz


POLICY_LDS_FLOATS = 16 * 1024  # 64 KB


def swizzled_numel(n: int, k: int) -> int:
    return -(-n // 16) * -(-k // 16) * 256


def policy_swizzle(w, out=None):
    """Tile-major copy of a weight matrix [N, K] (K % 4 == 0) for the policy kernel's matrix-core operand loads
    (cstr_policy_swizzle_f32): a wave's load then reads 1 KB of consecutive bytes."""
    n, k = w.shape
    _chk(w, "w", (n, k), th.float32)
    if out is None:
        out = th.empty(swizzled_numel(n, k), dtype=th.float32, device=w.device)
    _chk(out, "out", (swizzled_numel(n, k),), th.float32)
    check(nv.lib().cstr_policy_swizzle_f32(ptr(w), C.c_int64(n), C.c_int64(k), ptr(out), stream_ptr()), "cstr_policy_swizzle_f32")
    return out


def policy_rows_supported(k0: int, h1: int, h2: int, n_out: int) -> bool:
    return (k0 <= 256 and h1 % 4 == 0 and h2 % 4 == 0 and 16 * (h1 + h2 + 8) <= POLICY_LDS_FLOATS
            and n_out <= 2 * nv.MAX_HEAD_ACT)


def policy_rows_fwd(x, w1, b1, w2, b2, w3, b3, act: int, head: int, out_act: int, action, eps=None, rng_ctl=None, logp=None, w2_swz=None,
                    defer_rng_advance: bool = False):
    """A two-hidden-layer policy network + action head for all rows of x in ONE launch, inference only (cstr_policy_rows_fwd_f32).
    head 0: squashed-Gaussian sample (w3 [2A, H2]; noise from `eps` [M, A] or the Philox stream `rng_ctl`; optional `logp`);
    head 1: deterministic out_act(h2 @ w3^T + b3). `action` [M, A] may be a column block of a wider row-major matrix.
    `defer_rng_advance`: the launch leaves the stream offset alone -- the caller advances it by M before the next consumer
    (collect_step(..., rng_advance=(rng_ctl, M)) does it in the collect kernel's last-workgroup epilogue)."""
    m, k0 = x.shape
    h1, h2, n_out = w1.shape[0], w2.shape[0], w3.shape[0]
    a = n_out // 2 if head == 0 else n_out
    if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError("x: needs a float32 device matrix with unit column stride")
    _chk(w1, "w1", (h1, k0), th.float32), _chk(b1, "b1", (h1,), th.float32), _chk(w2, "w2", (h2, h1), th.float32)
    _chk(b2, "b2", (h2,), th.float32), _chk(w3, "w3", (n_out, h2), th.float32), _chk(b3, "b3", (n_out,), th.float32)
    _opt(eps, "eps", (m, a), th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64), _opt(logp, "logp", (m,), th.float32)
    stride = _rows(action, "action", m, a)
    if w2_swz is not None:
        _chk(w2_swz, "w2_swz", (swizzled_numel(h2, h1),), th.float32)
    net = nv.PolicyMlp(k0, h1, h2, a, act, head, out_act, 1 if (defer_rng_advance and rng_ctl is not None) else 0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                       b3.data_ptr(), None if w2_swz is None else w2_swz.data_ptr())
    check(nv.lib().cstr_policy_rows_fwd_f32(C.byref(net), ptr(x), C.c_int64(max(x.stride(0), k0)), ptr(eps), ptr(rng_ctl), ptr(action),
                                            C.c_int64(stride), ptr(logp), C.c_int64(m), stream_ptr()), "cstr_policy_rows_fwd_f32")
    return action


EVAL_LDS_BYTES = 64 * 1024


def eval_episodes_supported(k0: int, h1: int, h2: int, n_out: int, head: int, act_dim: int) -> bool:
    """cstr_eval_episodes_f32 takes the network shapes of cstr_policy_rows_fwd_f32 on a CSTR layout's observation rows."""
    lds = 4 * (16 * (16 * -(-h1 // 16) + 4 + 16 * -(-h2 // 16) + 4) + 8 * 16 * 8 + 2 * 16 * 8)
    return ((k0, act_dim) in LAYOUTS and n_out == (2 * act_dim if head == 0 else act_dim) and policy_rows_supported(k0, h1, h2, n_out)
            and lds <= EVAL_LDS_BYTES)


def eval_episodes(w1, b1, w2, b2, w3, b3, act: int, head: int, out_act: int, w2_swz, coef, integrator: str, env_obs, step_count, pcg_state,
                  squashed: bool, act_low, act_high, targets, max_vec_steps: int, static_init=None):
    """Whole evaluation episodes in ONE launch (cstr_eval_episodes_f32): env i runs `targets[i]` episodes with the policy network's
    deterministic action (head 0: the squashed Gaussian's mode, head 1: the deterministic actor) from the state in `env_obs` /
    `step_count` / `pcg_state`, which the launch advances. `targets`: a host sequence of non-negative ints. Returns
    (ep_return float64 [N, max(targets)], ep_len int32 [N, max(targets)], ep_done int32 [N]) in HBM; slots at and beyond targets[i]
    keep the value the buffers were allocated with (zero). Raises RuntimeError if `max_vec_steps` ended the launch before every env
    had met its target (ep_done < targets)."""
    import numpy as np

    n, d = env_obs.shape
    h1, h2, n_out = w1.shape[0], w2.shape[0], w3.shape[0]
    a = n_out // 2 if head == 0 else n_out
    if (d, a) not in LAYOUTS:
        raise ValueError(f"(obs_dim, act_dim) = {(d, a)} is not a CSTR layout {LAYOUTS}")
    _chk(env_obs, "env_obs", (n, d), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64)
    _opt(static_init, "static_init", (n, 8 if a == 4 else 4), th.float64)
    _chk(w1, "w1", (h1, d), th.float32), _chk(b1, "b1", (h1,), th.float32), _chk(w2, "w2", (h2, h1), th.float32)
    _chk(b2, "b2", (h2,), th.float32), _chk(w3, "w3", (n_out, h2), th.float32), _chk(b3, "b3", (n_out,), th.float32)
    if w2_swz is not None:
        _chk(w2_swz, "w2_swz", (swizzled_numel(h2, h1),), th.float32)
    if len(act_low) != a or len(act_high) != a:
        raise ValueError(f"act_low/act_high need {a} entries")
    tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int32))
    if tg.shape != (n,):
        raise ValueError(f"targets: shape {tg.shape}, expected {(n,)}")
    if tg.min() < 0:
        raise ValueError("targets must be non-negative")
    stride = int(tg.max())
    ep_return = th.zeros(n, stride, dtype=th.float64, device=env_obs.device)
    ep_len = th.zeros(n, stride, dtype=th.int32, device=env_obs.device)
    ep_done = th.zeros(n, dtype=th.int32, device=env_obs.device)
    eval_episodes_into(w1, b1, w2, b2, w3, b3, act, head, out_act, w2_swz, coef, integrator, env_obs, step_count, pcg_state, squashed,
                       act_low, act_high, tg, max_vec_steps, ep_return, ep_len, ep_done, static_init)
    short = (ep_done.cpu().numpy() < tg).nonzero()[0]  # the one read-back this wrapper does: a run cut short must not pass for a result
    if short.size:
        raise RuntimeError(f"cstr_eval_episodes_f32: max_vec_steps={int(max_vec_steps)} ended the launch before envs {short.tolist()} had "
                           f"run their episodes (counted {ep_done.cpu().numpy()[short].tolist()}, wanted {tg[short].tolist()})")
    return ep_return, ep_len, ep_done


def eval_episodes_into(w1, b1, w2, b2, w3, b3, act, head, out_act, w2_swz, coef, integrator, env_obs, step_count, pcg_state, squashed,
                       act_low, act_high, targets, max_vec_steps, ep_return, ep_len, ep_done, static_init=None):
    """`eval_episodes` into caller-owned result buffers; nothing is checked beyond what the entry point itself checks. `targets`: a
    contiguous int32 NumPy array that the CALLER keeps alive and unmodified until the stream has passed the launch (the entry point
    copies it to the device asynchronously): hold a reference until one of the results has been read back."""
    n, d = env_obs.shape
    n_out = w3.shape[0]
    a = n_out // 2 if head == 0 else n_out
    lo = (C.c_float * a)(*[float(v) for v in act_low])
    hi = (C.c_float * a)(*[float(v) for v in act_high])
    net = nv.PolicyMlp(d, w1.shape[0], w2.shape[0], a, act, head, out_act, 0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                       w3.data_ptr(), b3.data_ptr(), None if w2_swz is None else w2_swz.data_ptr())
    check(nv.lib().cstr_eval_episodes_f32(C.byref(net), C.byref(coef), C.c_int(INTEGRATORS[integrator]), C.c_int(d), ptr(env_obs),
                                          ptr(step_count), ptr(pcg_state), ptr(static_init), C.c_int(1 if squashed else 0), lo, hi,
                                          targets.ctypes.data_as(C.c_void_p), C.c_int64(n), C.c_int64(int(max_vec_steps)), ptr(ep_return),
                                          ptr(ep_len), ptr(ep_done), stream_ptr()), "cstr_eval_episodes_f32")


def collect_episodes_supported(k0: int, h1: int, h2: int, n_out: int, head: int, act_dim: int) -> bool:
    """cstr_collect_episodes_f32 takes what cstr_eval_episodes_f32 takes, on the (4, 2) layout only."""
    return (k0, act_dim) == LAYOUTS[0] and eval_episodes_supported(k0, h1, h2, n_out, head, act_dim)


def collect_episodes(w1, b1, w2, b2, w3, b3, act: int, head: int, out_act: int, w2_swz, coef, integrator: str, env_obs, step_count, pcg_state,
                     squashed: bool, act_low, act_high, ring: DeviceRing, n_steps: int, row0: int = 0, explore_prob: float = 0.0, seed: int = 0,
                     index_offset: int = 0, step_offset: int = 0, ep_stride: int = 0, static_init=None, record_explored: bool = False):
    """A policy rolled out into ring rows `row0 .. row0 + n_steps - 1` in ONE launch (cstr_collect_episodes_f32): every env runs `n_steps`
    vec-steps with the network's deterministic action or, with probability `explore_prob` per (env, step), a uniform draw over the action
    space from the Philox stream (`seed`, counter = (index_offset + env, step_offset + step, COLLECT_TAG)); the rows are those of
    `collect_step` (terminal next observation, done = timeout). The env state in `env_obs` / `step_count` / `pcg_state` advances; the
    ring's control words are not touched. Returns (ep_return float64 [N, ep_stride], ep_len int32 [N, ep_stride], ep_done int32 [N]) in
    HBM -- episodes of an env beyond `ep_stride` are counted in ep_done, not stored -- and, with `record_explored`, the uint8 flags
    [ring rows, N] behind them (rows outside the launch's stay 0)."""
    n, d = env_obs.shape
    h1, h2, n_out = w1.shape[0], w2.shape[0], w3.shape[0]
    a = n_out // 2 if head == 0 else n_out
    if (d, a) != LAYOUTS[0]:
        raise ValueError(f"(obs_dim, act_dim) = {(d, a)}: collect_episodes covers the {LAYOUTS[0]} layout")
    if (ring.n_envs, ring.obs_dim, ring.act_dim) != (n, d, a):
        raise ValueError(f"ring is ({ring.n_envs}, {ring.obs_dim}, {ring.act_dim}), the env ({n}, {d}, {a})")
    n_steps, row0, ep_stride = int(n_steps), int(row0), int(ep_stride)
    if n_steps <= 0 or row0 < 0 or row0 + n_steps > ring.rows:
        raise ValueError(f"rows {row0} .. {row0 + n_steps - 1} do not lie in a ring of {ring.rows} rows")
    if not 0.0 <= float(explore_prob) <= 1.0:
        raise ValueError(f"explore_prob = {explore_prob} is not a probability")
    if ep_stride < 0 or step_offset < 0 or step_offset + n_steps > 1 << 32:
        raise ValueError("ep_stride and step_offset must be non-negative, step_offset + n_steps at most 2^32")
    _chk(env_obs, "env_obs", (n, d), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64)
    _opt(static_init, "static_init", (n, 4), th.float64)
    _chk(w1, "w1", (h1, d), th.float32), _chk(b1, "b1", (h1,), th.float32), _chk(w2, "w2", (h2, h1), th.float32)
    _chk(b2, "b2", (h2,), th.float32), _chk(w3, "w3", (n_out, h2), th.float32), _chk(b3, "b3", (n_out,), th.float32)
    if w2_swz is not None:
        _chk(w2_swz, "w2_swz", (swizzled_numel(h2, h1),), th.float32)
    _chk(ring.observations, "ring.observations", (ring.rows, n, d), th.float32), _chk(ring.next_observations, "ring.next_observations", (ring.rows, n, d), th.float32)
    _chk(ring.actions, "ring.actions", (ring.rows, n, a), th.float32)
    for t, nm in ((ring.rewards, "ring.rewards"), (ring.dones, "ring.dones"), (ring.timeouts, "ring.timeouts")):
        _chk(t, nm, (ring.rows, n), th.float32)
    if len(act_low) != a or len(act_high) != a:
        raise ValueError(f"act_low/act_high need {a} entries")
    dev = env_obs.device
    ep_return = th.zeros(n, ep_stride, dtype=th.float64, device=dev)
    ep_len = th.zeros(n, ep_stride, dtype=th.int32, device=dev)
    ep_done = th.zeros(n, dtype=th.int32, device=dev)
    explored = th.zeros(ring.rows, n, dtype=th.uint8, device=dev) if record_explored else None
    collect_episodes_into(w1, b1, w2, b2, w3, b3, act, head, out_act, w2_swz, coef, integrator, env_obs, step_count, pcg_state, squashed, act_low,
                          act_high, ring, n_steps, row0, explore_prob, seed, index_offset, step_offset, ep_return, ep_len, ep_stride, ep_done,
                          explored, static_init)
    return (ep_return, ep_len, ep_done) + ((explored,) if record_explored else ())


def collect_episodes_into(w1, b1, w2, b2, w3, b3, act, head, out_act, w2_swz, coef, integrator, env_obs, step_count, pcg_state, squashed, act_low,
                          act_high, ring, n_steps, row0, explore_prob, seed, index_offset, step_offset, ep_return, ep_len, ep_stride, ep_done,
                          explored=None, static_init=None):
    """`collect_episodes` into caller-owned result buffers; nothing is checked beyond what the entry point itself checks."""
    n, d = env_obs.shape
    n_out = w3.shape[0]
    a = n_out // 2 if head == 0 else n_out
    lo = (C.c_float * a)(*[float(v) for v in act_low])
    hi = (C.c_float * a)(*[float(v) for v in act_high])
    net = nv.PolicyMlp(d, w1.shape[0], w2.shape[0], a, act, head, out_act, 0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                       w3.data_ptr(), b3.data_ptr(), None if w2_swz is None else w2_swz.data_ptr())
    check(nv.lib().cstr_collect_episodes_f32(C.byref(net), C.byref(coef), C.c_int(INTEGRATORS[integrator]), C.c_int(d), ptr(env_obs),
                                             ptr(step_count), ptr(pcg_state), ptr(static_init), C.c_int(1 if squashed else 0), lo, hi,
                                             C.byref(ring.c), C.c_int64(int(row0)), C.c_int64(n), C.c_int64(int(n_steps)),
                                             C.c_float(float(explore_prob)), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_int64(int(index_offset)),
                                             C.c_int64(int(step_offset)), ptr(ep_return), ptr(ep_len), C.c_int64(int(ep_stride)), ptr(ep_done),
                                             ptr(explored), stream_ptr()), "cstr_collect_episodes_f32")


def rollout_step_supported(k0: int, h1: int, h2: int, n_out: int, has_swizzled_w2: bool) -> bool:
    """cstr_rollout_step_f32 covers the pipelined policy kernel with a one-chunk first layer (see the header)."""
    return has_swizzled_w2 and k0 <= 16 and k0 % 4 == 0 and h1 <= 512 and h2 <= 512 and policy_rows_supported(k0, h1, h2, n_out)


def rollout_step(x, w1, b1, w2, b2, w3, b3, act: int, head: int, out_act: int, w2_swz, rng_ctl, coef, integrator: str, ring: DeviceRing,
                 env_obs, step_count, squashed, act_low, act_high, noise=None, reset_obs=None, pcg_state=None, static_init=None,
                 reward_out=None, done_out=None, ep_return=None, ep_stats=None, action_out=None, mt_state=None, sample_idx=None):
    """One vec-step in ONE launch (cstr_rollout_step_f32): policy network + sampling on x [N, k0], the fused collect step of
    `collect_step` with the action kept in registers, and -- when `mt_state` / `sample_idx` int32 [2, batch] are given -- the replay
    index draw of the gradient step behind it. Writes NO control word: follow it with `replay_gather_packed(advance_ring=True,
    rng_advance=(rng_ctl, N))`."""
    n, d, a = ring.n_envs, ring.obs_dim, ring.act_dim
    k0 = x.shape[1]
    h1, h2, n_out = w1.shape[0], w2.shape[0], w3.shape[0]
    if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and x.shape[0] == n and x.stride(1) == 1):
        raise ValueError("x: needs a float32 device matrix [n_envs, k0] with unit column stride")
    if (n_out // 2 if head == 0 else n_out) != a:
        raise ValueError(f"policy head width {n_out} does not match the ring's act_dim {a}")
    _chk(w1, "w1", (h1, k0), th.float32), _chk(b1, "b1", (h1,), th.float32), _chk(w2, "w2", (h2, h1), th.float32)
    _chk(b2, "b2", (h2,), th.float32), _chk(w3, "w3", (n_out, h2), th.float32), _chk(b3, "b3", (n_out,), th.float32)
    _chk(w2_swz, "w2_swz", (swizzled_numel(h2, h1),), th.float32)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    _chk(env_obs, "env_obs", (n, d), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _opt(noise, "noise", (n, a), th.float32), _opt(reset_obs, "reset_obs", (n, d), th.float32)
    _opt(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64)
    _opt(static_init, "static_init", (n, 8 if a == 4 else 4), th.float64)
    _opt(reward_out, "reward_out", (n,), th.float32), _opt(done_out, "done_out", (n,), th.float32)
    _opt(ep_return, "ep_return", (n,), th.float32), _opt(ep_stats, "ep_stats", (4,), th.float64)
    _opt(action_out, "action_out", (n, a), th.float32)
    if (ep_return is None) != (ep_stats is None):
        raise ValueError("ep_return and ep_stats go together")
    if (reset_obs is None) == (pcg_state is None):
        raise ValueError("rollout_step needs exactly one reset source: reset_obs or pcg_state")
    if len(act_low) != a or len(act_high) != a:
        raise ValueError(f"act_low/act_high need {a} entries")
    if (mt_state is None) != (sample_idx is None):
        raise ValueError("mt_state and sample_idx go together")
    batch = 0
    if mt_state is not None:
        _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32)
        batch = sample_idx.shape[1] if sample_idx.dim() == 2 else -1
        _chk(sample_idx, "sample_idx", (2, batch), th.int32)
    lo = (C.c_float * a)(*[float(v) for v in act_low])
    hi = (C.c_float * a)(*[float(v) for v in act_high])
    net = nv.PolicyMlp(k0, h1, h2, a, act, head, out_act, 1, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                       b3.data_ptr(), w2_swz.data_ptr())
    check(nv.lib().cstr_rollout_step_f32(C.byref(net), ptr(x), C.c_int64(max(x.stride(0), k0)), ptr(rng_ctl), C.byref(coef),
                                         C.c_int(INTEGRATORS[integrator]), C.byref(ring.c), ptr(ring.ctl), ptr(env_obs), ptr(step_count),
                                         C.c_int(int(squashed)), lo, hi, ptr(noise), ptr(reset_obs), ptr(pcg_state), ptr(static_init),
                                         ptr(reward_out), ptr(done_out), ptr(ep_return), ptr(ep_stats), ptr(action_out), ptr(mt_state),
                                         C.c_int64(batch), ptr(sample_idx), stream_ptr()), "cstr_rollout_step_f32")


def linear_act_fwd(x, weight, bias, act: int, out=None):
    """y = act(x @ W^T + b) in one launch (f32 matrix cores). x [M, K] or [G, M, K] with unit inner stride (rows / groups may
    be strided, a stride-0 group dimension shares the input), weight [N, K] / [G, N, K], bias [N] / [G, N] contiguous."""
    if x.dim() == 2:
        g, (m, k), gs, ldx = 1, x.shape, 0, x.stride(0)
        n = weight.shape[0]
        shape = (m, n)
    else:
        g, m, k = x.shape
        gs, ldx = x.stride(0), x.stride(1)
        n = weight.shape[1]
        shape = (g, m, n)
    if not (x.is_cuda and x.dtype == th.float32 and x.stride(-1) == 1 and ldx >= k):
        raise ValueError("x: needs a float32 device tensor with unit inner stride")
    if m == 1:
        ldx = max(ldx, k)
    _f32c(weight, "weight"), _f32c(bias, "bias")
    if weight.numel() != g * n * k or bias.numel() != g * n:
        raise ValueError(f"weight / bias do not match x {tuple(x.shape)}: {tuple(weight.shape)}, {tuple(bias.shape)}")
    y = th.empty(shape, dtype=th.float32, device=x.device) if out is None else _chk(out, "out", shape, th.float32)
    check(nv.lib().cstr_linear_act_fwd_f32(ptr(x), C.c_int64(gs), C.c_int64(ldx), ptr(weight), ptr(bias), C.c_int(act), ptr(y),
                                           C.c_int64(g), C.c_int64(m), C.c_int64(n), C.c_int64(k), stream_ptr()), "cstr_linear_act_fwd_f32")
    return y


def linear_act_fwd_sets(sets, act: int):
    """Several independent Linear + bias + activation layers of ONE shape in one launch. `sets`: [(x [M, K] (row-strided ok),
    weight [N, K], bias [N], y [M, N] (row-strided ok: e.g. a column block of the joint action))]."""
    sets = list(sets)
    if not 0 < len(sets) <= nv.MAX_LINEAR_SETS:
        raise ValueError(f"1..{nv.MAX_LINEAR_SETS} sets, got {len(sets)}")
    m, k = sets[0][0].shape
    n = sets[0][1].shape[0]
    arr = (nv.LinearSet * len(sets))()
    for i, (x, w, b, y) in enumerate(sets):
        for t, nm, shape in ((x, "x", (m, k)), (y, "y", (m, n))):
            if not (t.is_cuda and t.dtype == th.float32 and tuple(t.shape) == shape and t.stride(1) == 1):
                raise ValueError(f"{nm}[{i}]: needs a float32 device matrix {shape} with unit column stride")
        _chk(w, f"weight[{i}]", (n, k), th.float32), _chk(b, f"bias[{i}]", (n,), th.float32)
        arr[i] = nv.LinearSet(x.data_ptr(), max(x.stride(0), k), w.data_ptr(), b.data_ptr(), y.data_ptr(), max(y.stride(0), n))
    check(nv.lib().cstr_linear_act_fwd_sets_f32(arr, C.c_int(len(sets)), C.c_int(act), C.c_int64(m), C.c_int64(n), C.c_int64(k),
                                                stream_ptr()), "cstr_linear_act_fwd_sets_f32")


def linear_bwd_input(gz, weight, y, act: int, sum_groups: bool = False):
    """dz = (gz @ W) * act'(y): a Linear's input gradient fused with the activation gradient of the layer below (whose output
    y is this layer's input). gz [M, N] / [G, M, N], weight [N, K] / [G, N, K] contiguous. sum_groups: the G groups share one
    input, the result is the [M, K] sum over groups."""
    g, m, n = _gmn(gz)
    k = weight.shape[-1]
    _f32c(gz, "gz"), _f32c(weight, "weight")
    if weight.numel() != g * n * k:
        raise ValueError(f"weight {tuple(weight.shape)} does not match gz {tuple(gz.shape)}")
    shape = (m, k) if (gz.dim() == 2 or sum_groups) else (g, m, k)
    if act != 0:
        _chk(y, "y", shape, th.float32)
    dz = th.empty(shape, dtype=th.float32, device=gz.device)
    check(nv.lib().cstr_linear_bwd_input_f32(ptr(gz), ptr(weight), ptr(y if act != 0 else None), C.c_int(act), ptr(dz), C.c_int64(g),
                                             C.c_int(int(sum_groups)), C.c_int64(m), C.c_int64(n), C.c_int64(k), stream_ptr()),
          "cstr_linear_bwd_input_f32")
    return dz


def linear_bwd_weight(dz, x, dw, db=None):
    """dw = dz^T @ x and (optionally) db = column sums of dz in one launch. dz [M, N] / [G, M, N] contiguous; x [M, K] /
    [G, M, K] with unit inner stride (rows / groups may be strided, stride-0 groups share the input); dw, db: contiguous
    views of the gradient arena."""
    g, m, n = _gmn(dz)
    k = x.shape[-1]
    _f32c(dz, "dz"), _f32c(dw, "dw")
    if x.dim() == 2:
        gs, ldx = 0, x.stride(0)
    else:
        gs, ldx = x.stride(0), x.stride(1)
    if not (x.is_cuda and x.dtype == th.float32 and x.stride(-1) == 1 and x.shape[-2] == m):
        raise ValueError("x: needs a float32 device tensor with unit inner stride and as many rows as dz")
    if m == 1:
        ldx = max(ldx, k)
    if dw.numel() != g * n * k:
        raise ValueError(f"dw has {dw.numel()} elements, expected {g * n * k}")
    if db is not None and _f32c(db, "db").numel() != g * n:
        raise ValueError(f"db has {db.numel()} elements, expected {g * n}")
    check(nv.lib().cstr_linear_bwd_weight_f32(ptr(dz), ptr(x), C.c_int64(gs), C.c_int64(ldx), ptr(dw), ptr(db), C.c_int64(g),
                                              C.c_int64(m), C.c_int64(n), C.c_int64(k), stream_ptr()), "cstr_linear_bwd_weight_f32")


def linear_bwd_weight_sets(sets):
    """`linear_bwd_weight` for several independent (2-D) Linears of any shapes in one launch. `sets`: [(dz [M, N], x [M, K]
    (row-strided ok), dw [N, K] view, db [N] view or None)]."""
    sets = list(sets)
    if not 0 < len(sets) <= nv.MAX_LINEAR_SETS:
        raise ValueError(f"1..{nv.MAX_LINEAR_SETS} sets, got {len(sets)}")
    arr = (nv.WgradSet * len(sets))()
    for i, (dz, x, dw, db) in enumerate(sets):
        if dz.dim() != 2:
            raise ValueError(f"dz[{i}]: needs a matrix")
        m, n = dz.shape
        k = x.shape[-1]
        _f32c(dz, f"dz[{i}]"), _f32c(dw, f"dw[{i}]")
        if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == m):
            raise ValueError(f"x[{i}]: needs a float32 device matrix with unit inner stride and as many rows as dz")
        if dw.numel() != n * k or (db is not None and _f32c(db, f"db[{i}]").numel() != n):
            raise ValueError(f"dw / db[{i}] do not match dz {tuple(dz.shape)} and x {tuple(x.shape)}")
        arr[i] = nv.WgradSet(dz.data_ptr(), x.data_ptr(), max(x.stride(0), k), dw.data_ptr(), None if db is None else db.data_ptr(),
                             m, n, k)
    check(nv.lib().cstr_linear_bwd_weight_sets_f32(arr, C.c_int(len(sets)), stream_ptr()), "cstr_linear_bwd_weight_sets_f32")


def target_smooth(action, noise, rng_ctl, sigma: float, clip: float, out):
    """out = clamp(action + clamp(noise, -clip, clip), -1, 1); noise given ([B, A], already scaled) or drawn (rng_ctl)."""
    b, a = action.shape
    _chk(action, "action", (b, a), th.float32), _opt(noise, "noise", (b, a), th.float32)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    if (noise is None) == (rng_ctl is None):
        raise ValueError("target_smooth needs exactly one noise source: a noise tensor or rng_ctl")
    stride = _rows(out, "out", b, a)
    check(nv.lib().cstr_target_smooth_f32(ptr(action), ptr(noise), ptr(rng_ctl), C.c_float(sigma), C.c_float(clip), ptr(out),
                                          C.c_int64(stride), C.c_int64(b), C.c_int(a), stream_ptr()), "cstr_target_smooth_f32")
    return out


def linear_smooth_supported(m: int, n: int, k: int) -> bool:
    return n <= 16 and k > 32 and m <= 32768


def linear_smooth_fwd(x, weight, bias, act: int, noise, rng_ctl, sigma: float, clip: float, out):
    """`linear_act_fwd` followed by `target_smooth` in ONE launch (cstr_linear_smooth_fwd_f32): out [M, N] (may be a column block of a
    wider row-major matrix) = clamp(act(x W^T + b) + clamp(noise | sigma N(0, 1) from rng_ctl, -clip, clip), -1, 1)."""
    m, k = x.shape
    n = weight.shape[0]
    if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError("x: needs a float32 device matrix with unit column stride")
    _chk(weight, "weight", (n, k), th.float32), _chk(bias, "bias", (n,), th.float32)
    _opt(noise, "noise", (m, n), th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    if (noise is None) == (rng_ctl is None):
        raise ValueError("exactly one noise source: noise or rng_ctl")
    stride = _rows(out, "out", m, n)
    check(nv.lib().cstr_linear_smooth_fwd_f32(ptr(x), C.c_int64(max(x.stride(0), k)), ptr(weight), ptr(bias), C.c_int(act), ptr(noise),
                                              ptr(rng_ctl), C.c_float(sigma), C.c_float(clip), ptr(out), C.c_int64(stride), C.c_int64(m),
                                              C.c_int64(n), C.c_int64(k), stream_ptr()), "cstr_linear_smooth_fwd_f32")
    return out


def hidden_head_fwd_(z, b1, act: int, w2, b2, q):
    """y = act(z + b1) in place on z [G, m, k] (or [m, k]); q [G, m, 1] = y . w2 + b2 (a Q network's scalar head)."""
    g, m, k = _gmn(z)
    for t, nm, numel in ((z, "z", g * m * k), (b1, "b1", g * k), (w2, "w2", g * k), (b2, "b2", g), (q, "q", g * m)):
        if _f32c(t, nm).numel() != numel:
            raise ValueError(f"{nm} has {t.numel()} elements, expected {numel}")
    check(nv.lib().cstr_hidden_head_fwd_f32(ptr(z), ptr(b1), C.c_int(act), ptr(w2), ptr(b2), ptr(q), C.c_int64(g), C.c_int64(m),
                                            C.c_int64(k), stream_ptr()), "cstr_hidden_head_fwd_f32")
    return q


def hidden_head_bwd(gq, y, act: int, w2, dz, gb1=None, gw2=None, gb2=None):
    """dz = gq * w2 * act'(y); with parameter gradients: gb1 = sum_m dz, gw2 = sum_m gq * y, gb2 = sum_m gq."""
    g, m, k = _gmn(y)
    _chk(dz, "dz", y.shape, th.float32)
    for t, nm, numel in ((gq, "gq", g * m), (y, "y", g * m * k), (w2, "w2", g * k)):
        if _f32c(t, nm).numel() != numel:
            raise ValueError(f"{nm} has {t.numel()} elements, expected {numel}")
    grads = (gb1, gw2, gb2)
    if any(t is None for t in grads) != all(t is None for t in grads):
        raise ValueError("gb1, gw2 and gb2 go together")
    if gb1 is not None:
        for t, nm, numel in ((gb1, "gb1", g * k), (gw2, "gw2", g * k), (gb2, "gb2", g)):
            if _f32c(t, nm).numel() != numel:
                raise ValueError(f"{nm} has {t.numel()} elements, expected {numel}")
    check(nv.lib().cstr_hidden_head_bwd_f32(ptr(gq), ptr(y), C.c_int(act), ptr(w2), ptr(dz), ptr(gb1), ptr(gw2), ptr(gb2),
                                            C.c_int64(g), C.c_int64(m), C.c_int64(k), stream_ptr()), "cstr_hidden_head_bwd_f32")


def hidden_head_bwd_root(root: dict, y, act: int, w2, dz, gb1=None, gw2=None, gb2=None):
    """`hidden_head_bwd` for the twin Q networks with the loss root inside (cstr_hidden_head_bwd_root_f32): `root` =
    dict(mode="td", q1_t, q2_t, next_logp | None, rew, done, ent_coef | None, gamma, scale, q1, q2, target_out | None, loss_out | None,
    loss_sum | None, alpha | None) -- the arguments of `td_twin_q_loss` -- or dict(mode="sac_actor", logp, q1, q2, ent_coef, g_logp,
    loss_out | None, loss_sum | None) -- those of `sac_actor_loss` --, or dict(mode="neg_mean", q1, loss_out | None, loss_sum | None): the
    deterministic actors' -mean(Q1) through the FIRST Q network alone (y [1, m, k])."""
    g, m, k = _gmn(y)
    if g != (1 if root["mode"] == "neg_mean" else 2):
        raise ValueError("the loss-root form is built for the twin Q networks (2 groups; mode 'neg_mean': the first one alone)")
    _chk(dz, "dz", y.shape, th.float32)
    for t, nm, numel in ((y, "y", g * m * k), (w2, "w2", g * k)):
        if _f32c(t, nm).numel() != numel:
            raise ValueError(f"{nm} has {t.numel()} elements, expected {numel}")
    grads = (gb1, gw2, gb2)
    if any(t is None for t in grads) != all(t is None for t in grads):
        raise ValueError("gb1, gw2 and gb2 go together")
    if gb1 is not None:
        for t, nm, numel in ((gb1, "gb1", g * k), (gw2, "gw2", g * k), (gb2, "gb2", g)):
            if _f32c(t, nm).numel() != numel:
                raise ValueError(f"{nm} has {t.numel()} elements, expected {numel}")
    p = lambda key, n=m: None if root.get(key) is None else _vec(root[key], key, n).data_ptr()  # noqa: E731
    part = nv.AlphaPart()
    if root["mode"] == "td":
        alpha = root.get("alpha")
        if alpha is not None:
            _vec(alpha["logp_pi"], "logp_pi", m)
            for nm in ("log_alpha", "grad_out", "ent_coef_out"):
                _vec(alpha[nm], nm, 1)
            part = nv.AlphaPart(alpha["log_alpha"].data_ptr(), alpha["logp_pi"].data_ptr(), float(alpha["target_entropy"]),
                                alpha["grad_out"].data_ptr(), alpha["ent_coef_out"].data_ptr(),
                                *(None if alpha.get(kk) is None else alpha[kk].data_ptr() for kk in ("loss_out", "loss_sum", "ent_coef_sum")))
        rt = nv.HeadRoot(1, m, float(root["gamma"]), float(root["scale"]), p("q1_t"), p("q2_t"), p("next_logp"), p("rew"), p("done"),
                         None if alpha is not None else p("ent_coef", 1), p("q1"), p("q2"), p("target_out"), None, None,
                         p("loss_out", 1), p("loss_sum", 1), part)
    elif root["mode"] == "sac_actor":
        rt = nv.HeadRoot(2, m, 0.0, 0.0, None, None, None, None, None, p("ent_coef", 1), p("q1"), p("q2"), None, p("logp"), p("g_logp"),
                         p("loss_out", 1), p("loss_sum", 1), part)
    elif root["mode"] == "neg_mean":  # neg_mean_loss's arguments: loss = -mean(q1)
        rt = nv.HeadRoot(3, m, 0.0, 0.0, None, None, None, None, None, None, p("q1"), None, None, None, None, p("loss_out", 1), p("loss_sum", 1),
                         part)
    else:
        raise ValueError(f"unknown loss root {root['mode']!r}")
    check(nv.lib().cstr_hidden_head_bwd_root_f32(C.byref(rt), ptr(y), C.c_int(act), ptr(w2), ptr(dz), ptr(gb1), ptr(gw2), ptr(gb2),
                                                 C.c_int64(m), C.c_int64(k), stream_ptr()), "cstr_hidden_head_bwd_root_f32")


def _rows(t, name, b, a):
    """A [b, a] float32 device matrix whose rows may be strided (a column slice of a wider row-major matrix)."""
    if not (isinstance(t, th.Tensor) and t.is_cuda and t.dtype == th.float32 and tuple(t.shape) == (b, a) and t.stride(1) == 1
            and t.stride(0) >= a):
        raise ValueError(f"{name}: needs a float32 device matrix [{b}, {a}] with unit column stride")
    return t.stride(0)


def squashed_gaussian_fwd(mean, log_std_raw, eps, action, logp):
    b, a = mean.shape
    stride = _rows(mean, "mean", b, a)
    if _rows(log_std_raw, "log_std_raw", b, a) != stride:
        raise ValueError("mean and log_std_raw must share their row stride")
    _chk(eps, "eps", (b, a), th.float32), _chk(action, "action", (b, a), th.float32)
    _opt(logp, "logp", (b,), th.float32)
    check(nv.lib().cstr_squashed_gaussian_fwd_f32(ptr(mean), ptr(log_std_raw), ptr(eps), ptr(action), ptr(logp), C.c_int64(b),
                                                  C.c_int(a), C.c_int(stride), stream_ptr()), "cstr_squashed_gaussian_fwd_f32")


def squashed_gaussian_bwd(g_action, g_logp, action, log_std_raw, eps, g_mean, g_log_std_raw):
    b, a = action.shape
    _chk(action, "action", (b, a), th.float32), _chk(eps, "eps", (b, a), th.float32)
    stride = _rows(log_std_raw, "log_std_raw", b, a)
    if _rows(g_mean, "g_mean", b, a) != stride or _rows(g_log_std_raw, "g_log_std_raw", b, a) != stride:
        raise ValueError("g_mean / g_log_std_raw must have log_std_raw's row stride")
    ga_stride = a if g_action is None else _rows(g_action, "g_action", b, a)
    if g_logp is not None and (g_logp.numel() != b or not g_logp.is_contiguous() or g_logp.dtype != th.float32):
        raise ValueError("g_logp must be a contiguous float32 tensor with batch elements")
    check(nv.lib().cstr_squashed_gaussian_bwd_f32(ptr(g_action), ptr(g_logp), ptr(action), ptr(log_std_raw), ptr(eps), ptr(g_mean),
                                                  ptr(g_log_std_raw), C.c_int64(b), C.c_int(a), C.c_int(stride), C.c_int(ga_stride),
                                                  stream_ptr()), "cstr_squashed_gaussian_bwd_f32")


def _vec(t, name, n):
    if not (isinstance(t, th.Tensor) and t.is_cuda and t.dtype == th.float32 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{name}: needs a contiguous float32 device tensor with {n} elements")
    return t


def sac_alpha(log_alpha, logp, target_entropy: float, grad_out, ent_coef_out, loss_sum=None, ent_coef_sum=None, loss_out=None):
    b = logp.numel()
    _vec(logp, "logp", b)
    for t, nm in ((log_alpha, "log_alpha"), (grad_out, "grad_out"), (ent_coef_out, "ent_coef_out")):
        _vec(t, nm, 1)
    check(nv.lib().cstr_sac_alpha_f32(ptr(log_alpha), ptr(logp), C.c_float(target_entropy), ptr(grad_out), ptr(ent_coef_out),
                                      ptr(loss_out), ptr(loss_sum), ptr(ent_coef_sum), C.c_int64(b), stream_ptr()), "cstr_sac_alpha_f32")


def twin_q_loss(q1, q2, target, scale: float, gq1, gq2, loss_out=None, loss_sum=None):
    b = q1.numel()
    for t, nm in ((q1, "q1"), (q2, "q2"), (target, "target"), (gq1, "gq1"), (gq2, "gq2")):
        _vec(t, nm, b)
    check(nv.lib().cstr_twin_q_loss_f32(ptr(q1), ptr(q2), ptr(target), C.c_float(scale), ptr(gq1), ptr(gq2), ptr(loss_out),
                                        ptr(loss_sum), C.c_int64(b), stream_ptr()), "cstr_twin_q_loss_f32")


def td_twin_q_loss(q1_t, q2_t, next_logp, rew, done, ent_coef, gamma: float, q1, q2, scale: float, target_out, gq1, gq2,
                   loss_out=None, loss_sum=None, alpha=None):
    """`td_target_min` + `twin_q_loss` (+ `sac_alpha`) in one launch. `alpha` = None or a dict(log_alpha, logp_pi,
    target_entropy, grad_out, ent_coef_out, loss_out=None, loss_sum=None, ent_coef_sum=None): SAC's entropy-coefficient loss
    rides along and the target uses exp(log_alpha) (`ent_coef` is ignored then)."""
    b = q1.numel()
    for t, nm in ((q1_t, "q1_t"), (q2_t, "q2_t"), (rew, "rew"), (done, "done"), (q1, "q1"), (q2, "q2"), (gq1, "gq1"), (gq2, "gq2")):
        _vec(t, nm, b)
    if next_logp is not None:
        _vec(next_logp, "next_logp", b)
        if alpha is None:
            if ent_coef is None:
                raise ValueError("next_logp needs ent_coef or the alpha part")
            _vec(ent_coef, "ent_coef", 1)
    if target_out is not None:
        _vec(target_out, "target_out", b)
    part = None
    if alpha is not None:
        _vec(alpha["logp_pi"], "logp_pi", b)
        for nm in ("log_alpha", "grad_out", "ent_coef_out"):
            _vec(alpha[nm], nm, 1)
        part = nv.AlphaPart(alpha["log_alpha"].data_ptr(), alpha["logp_pi"].data_ptr(), float(alpha["target_entropy"]),
                            alpha["grad_out"].data_ptr(), alpha["ent_coef_out"].data_ptr(),
                            *(None if alpha.get(k) is None else alpha[k].data_ptr() for k in ("loss_out", "loss_sum", "ent_coef_sum")))
    check(nv.lib().cstr_td_twin_q_loss_f32(ptr(q1_t), ptr(q2_t), ptr(next_logp), ptr(rew), ptr(done),
                                           ptr(None if alpha is not None else ent_coef), C.c_float(gamma), ptr(q1), ptr(q2),
                                           C.c_float(scale), ptr(target_out), ptr(gq1), ptr(gq2), ptr(loss_out), ptr(loss_sum),
                                           None if part is None else C.byref(part), C.c_int64(b), stream_ptr()),
          "cstr_td_twin_q_loss_f32")


def sac_actor_loss(logp, q1, q2, ent_coef, g_logp, gq1, gq2, loss_out=None, loss_sum=None):
    b = logp.numel()
    for t, nm in ((logp, "logp"), (q1, "q1"), (q2, "q2"), (g_logp, "g_logp"), (gq1, "gq1"), (gq2, "gq2")):
        _vec(t, nm, b)
    _vec(ent_coef, "ent_coef", 1)
    check(nv.lib().cstr_sac_actor_loss_f32(ptr(logp), ptr(q1), ptr(q2), ptr(ent_coef), ptr(g_logp), ptr(gq1), ptr(gq2),
                                           ptr(loss_out), ptr(loss_sum), C.c_int64(b), stream_ptr()), "cstr_sac_actor_loss_f32")


def _critic_rows(q, name, b):
    """(base pointer, row stride in elements, N) of N critics' Q values over a batch of b: a stacked tensor [N, b] / [N, b, 1] whose rows
    are contiguous (a `fused.QOut` is taken by its `.stacked` tensor), or a sequence of N contiguous [b] / [b, 1] tensors that lie
    equally spaced in memory (one tensor for N = 1)."""
    stacked = getattr(q, "stacked", None)
    if stacked is not None:
        q = stacked
    if isinstance(q, th.Tensor):
        if not (q.is_cuda and q.dtype == th.float32 and q.dim() in (2, 3) and q.shape[1] == b and (q.dim() == 2 or q.shape[2] == 1)):
            raise ValueError(f"{name}: needs a float32 device tensor [N, {b}] or [N, {b}, 1], got {tuple(q.shape)} {q.dtype} on {q.device}")
        if q.stride(1) != 1 or (q.shape[0] > 1 and q.stride(0) < b):
            raise ValueError(f"{name}: every critic's row must be contiguous and the rows must not overlap")
        n, rows = q.shape[0], [q.data_ptr() + 4 * i * q.stride(0) for i in range(q.shape[0])]
    else:
        ts = list(q)
        for i, t in enumerate(ts):
            _vec(t, f"{name}[{i}]", b)
        n, rows = len(ts), [t.data_ptr() for t in ts]
    if not 1 <= n <= nv.MAX_ENS_CRITICS:
        raise ValueError(f"{name}: {n} critics; the ensemble loss heads take 1..{nv.MAX_ENS_CRITICS}")
    stride = (rows[1] - rows[0]) // 4 if n > 1 else b
    if n > 1 and (stride < b or any(r != rows[0] + 4 * i * stride for i, r in enumerate(rows))):
        raise ValueError(f"{name}: the critics' rows must lie equally spaced in one allocation (a stacked [N, B, 1] output)")
    return rows[0], stride, n


def td_ens_q_loss(q_t, next_logp, rew, done, ent_coef, gamma: float, q, scale: float, target_out, gq, loss_out=None, loss_sum=None,
                  alpha=None):
    """`td_twin_q_loss` for N critics (cstr_td_ens_q_loss_f32): q_t / q = the target critics' / the critics' Q values (stacked [N, B, 1],
    a `fused.QOut`, or N equally spaced [B, 1] views), gq [N, B, 1] contiguous. At N = 2 bit-identical to `td_twin_q_loss`."""
    b = rew.numel()
    qt_ptr, qt_stride, n = _critic_rows(q_t, "q_t", b)
    q_ptr, q_stride, n_q = _critic_rows(q, "q", b)
    if n_q != n:
        raise ValueError(f"q_t has {n} critics, q has {n_q}")
    _vec(gq, "gq", n * b)  # [N, B, 1] contiguous
    for t, nm in ((rew, "rew"), (done, "done")):
        _vec(t, nm, b)
    if next_logp is not None:
        _vec(next_logp, "next_logp", b)
        if alpha is None:
            if ent_coef is None:
                raise ValueError("next_logp needs ent_coef or the alpha part")
            _vec(ent_coef, "ent_coef", 1)
    if target_out is not None:
        _vec(target_out, "target_out", b)
    part = None
    if alpha is not None:
        _vec(alpha["logp_pi"], "logp_pi", b)
        for nm in ("log_alpha", "grad_out", "ent_coef_out"):
            _vec(alpha[nm], nm, 1)
        part = nv.AlphaPart(alpha["log_alpha"].data_ptr(), alpha["logp_pi"].data_ptr(), float(alpha["target_entropy"]),
                            alpha["grad_out"].data_ptr(), alpha["ent_coef_out"].data_ptr(),
                            *(None if alpha.get(k) is None else alpha[k].data_ptr() for k in ("loss_out", "loss_sum", "ent_coef_sum")))
    check(nv.lib().cstr_td_ens_q_loss_f32(C.c_void_p(qt_ptr), C.c_int64(qt_stride), ptr(next_logp), ptr(rew), ptr(done),
                                          ptr(None if alpha is not None else ent_coef), C.c_float(gamma), C.c_void_p(q_ptr),
                                          C.c_int64(q_stride), C.c_float(scale), ptr(target_out), ptr(gq), ptr(loss_out), ptr(loss_sum),
                                          None if part is None else C.byref(part), C.c_int(n), C.c_int64(b), stream_ptr()),
          "cstr_td_ens_q_loss_f32")


def sac_actor_ens_loss(logp, q, ent_coef, g_logp, gq, loss_out=None, loss_sum=None):
    """`sac_actor_loss` for N critics (cstr_sac_actor_ens_loss_f32): loss = mean(ent_coef * logp - min_i q_i); q as in `td_ens_q_loss`,
    gq [N, B, 1] contiguous. At N = 2 bit-identical to `sac_actor_loss`."""
    b = logp.numel()
    q_ptr, q_stride, n = _critic_rows(q, "q", b)
    _vec(gq, "gq", n * b)  # [N, B, 1] contiguous
    _vec(logp, "logp", b), _vec(g_logp, "g_logp", b), _vec(ent_coef, "ent_coef", 1)
    check(nv.lib().cstr_sac_actor_ens_loss_f32(ptr(logp), C.c_void_p(q_ptr), C.c_int64(q_stride), ptr(ent_coef), ptr(g_logp), ptr(gq),
                                               ptr(loss_out), ptr(loss_sum), C.c_int(n), C.c_int64(b), stream_ptr()),
          "cstr_sac_actor_ens_loss_f32")


# ---- gSDE (csrc/cstr_sde.hip, include/cstr_rl_hip.h "gSDE") ------------------------------------------------------------------
def _sde_dims(log_std, act_dim: int):
    if log_std.dim() != 2 or log_std.shape[1] not in (1, act_dim):
        raise ValueError(f"log_std: needs [L, {act_dim}] or [L, 1], got {tuple(log_std.shape)}")
    L = log_std.shape[0]
    if not 1 <= act_dim <= nv.MAX_HEAD_ACT or not 1 <= L <= nv.SDE_MAX_LATENT:
        raise ValueError(f"gSDE head: latent width {L} / action dim {act_dim} out of range (<= {nv.SDE_MAX_LATENT} / <= {nv.MAX_HEAD_ACT})")
    _chk(log_std, "log_std", tuple(log_std.shape), th.float32)
    return L, log_std.shape[1]


def sde_draw(log_std, act_dim: int, use_expln: bool, z, mats, std_out=None, rng_ctl=None, z_keep: Optional[int] = None):
    """mats [n, L, A] = z * get_std(log_std) (cstr_sde_draw_f32); z [n, L, A] is drawn from `rng_ctl`'s Philox stream (whose offset
    the launch advances on the device) when given and read otherwise; a drawn z is stored for the first `z_keep` matrices (default:
    all); std_out [L, A] optional."""
    L, cols = _sde_dims(log_std, act_dim)
    n = mats.shape[0]
    _chk(mats, "mats", (n, L, act_dim), th.float32), _chk(z, "z", (n, L, act_dim), th.float32)
    _opt(std_out, "std_out", (L, act_dim), th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_sde_draw_f32(ptr(log_std), C.c_int(cols), C.c_int(L), C.c_int(act_dim), C.c_int(int(use_expln)), C.c_int64(n),
                                     ptr(std_out), ptr(z), C.c_int64(n if z_keep is None else z_keep), ptr(mats), ptr(rng_ctl),
                                     stream_ptr()), "cstr_sde_draw_f32")


def _sde_mats(mats, b: int, L: int, a: int):
    """(pointer owner, row stride of the matrices): [L, A] = one shared matrix, [B, L, A] = one per row, None = the mode."""
    if mats is None:
        return None, 0
    if mats.dim() == 2:
        return _chk(mats, "mats", (L, a), th.float32), 0
    return _chk(mats, "mats", (b, L, a), th.float32), L * a


def sde_head_fwd(h, w_mu, b_mu, clip_mean: float, mats, std_mat, action, logp=None, aux=None):
    """The gSDE head forward (cstr_sde_head_fwd_f32) from the latent h [B, L] (row stride allowed): action [B, A] (row-strided view
    allowed) = tanh(Hardtanh(h W^T + b) + h M); logp [B] and aux [B, 2A] optional. mats: see `_sde_mats`."""
    b, L = h.shape
    a = w_mu.shape[0]
    if h.stride(1) != 1 or h.stride(0) < L or not h.is_cuda or h.dtype != th.float32:
        raise ValueError("h: needs a float32 device matrix with unit column stride")
    _chk(w_mu, "w_mu", (a, L), th.float32), _chk(b_mu, "b_mu", (a,), th.float32), _chk(std_mat, "std_mat", (L, a), th.float32)
    m, ms = _sde_mats(mats, b, L, a)
    stride = _rows(action, "action", b, a)
    _opt(logp, "logp", (b,), th.float32), _opt(aux, "aux", (b, 2 * a), th.float32)
    check(nv.lib().cstr_sde_head_fwd_f32(ptr(h), C.c_int64(h.stride(0)), C.c_int64(b), C.c_int(L), C.c_int(a), ptr(w_mu), ptr(b_mu),
                                         C.c_float(clip_mean), ptr(m), C.c_int64(ms), ptr(std_mat), ptr(action), C.c_int64(stride), ptr(logp),
                                         ptr(aux), stream_ptr()), "cstr_sde_head_fwd_f32")


def sde_head_bwd(g_action, g_logp, action, aux, h, w_mu, clip_mean: float, mats, std_mat, below_act: int, g_pre, g_x, g_var, dh=None):
    """Per-row gradients of the gSDE head (cstr_sde_head_bwd_f32): g_pre / g_x / g_var [B, A] and dh [B, L] (times the activation
    gradient `below_act` of the layer that produced h)."""
    b, L = h.shape
    a = w_mu.shape[0]
    if h.stride(1) != 1 or h.stride(0) < L:
        raise ValueError("h: needs unit column stride")
    gs = _rows(g_action, "g_action", b, a) if g_action is not None else 0
    _opt(g_logp, "g_logp", (b,), th.float32)
    astr = _rows(action, "action", b, a)
    _chk(aux, "aux", (b, 2 * a), th.float32), _chk(w_mu, "w_mu", (a, L), th.float32), _chk(std_mat, "std_mat", (L, a), th.float32)
    m, ms = _sde_mats(mats, b, L, a)
    for t, nm in ((g_pre, "g_pre"), (g_x, "g_x"), (g_var, "g_var")):
        _opt(t, nm, (b, a), th.float32)
    _opt(dh, "dh", (b, L), th.float32)
    check(nv.lib().cstr_sde_head_bwd_f32(ptr(g_action), C.c_int64(gs), ptr(g_logp), ptr(action), C.c_int64(astr), ptr(aux), ptr(h),
                                         C.c_int64(h.stride(0)), C.c_int64(b), C.c_int(L), C.c_int(a), ptr(w_mu), C.c_float(clip_mean), ptr(m),
                                         C.c_int64(ms), ptr(std_mat), C.c_int(below_act), ptr(g_pre), ptr(g_x), ptr(g_var), ptr(dh),
                                         stream_ptr()), "cstr_sde_head_bwd_f32")


def sde_param_grad(h, g_pre, g_x, g_var, z, std_mat, log_std, use_expln: bool, dw_mu=None, db_mu=None, dlog_std=None):
    """dW_mu [A, L], db_mu [A] and d log_std (log_std's shape) of a batch, reduced in one launch (cstr_sde_param_grad_f32); z [L, A] is
    the shared matrix's standard-normal draw (None: no noise term)."""
    b, L = h.shape
    a = g_pre.shape[1]
    if h.stride(1) != 1 or h.stride(0) < L:
        raise ValueError("h: needs unit column stride")
    _, cols = _sde_dims(log_std, a)
    for t, nm in ((g_pre, "g_pre"), (g_x, "g_x"), (g_var, "g_var")):
        _chk(t, nm, (b, a), th.float32)
    _opt(z, "z", (L, a), th.float32), _chk(std_mat, "std_mat", (L, a), th.float32)
    _opt(dw_mu, "dw_mu", (a, L), th.float32), _opt(db_mu, "db_mu", (a,), th.float32), _opt(dlog_std, "dlog_std", (L, cols), th.float32)
    check(nv.lib().cstr_sde_param_grad_f32(ptr(h), C.c_int64(h.stride(0)), C.c_int64(b), C.c_int(L), C.c_int(a), ptr(g_pre), ptr(g_x),
                                           ptr(g_var), ptr(z), ptr(std_mat), ptr(log_std), C.c_int(cols), C.c_int(int(use_expln)),
                                           ptr(dw_mu), ptr(db_mu), ptr(dlog_std), stream_ptr()), "cstr_sde_param_grad_f32")


# ---- BCQ (csrc/cstr_bcq.hip; reference core/bcq/bcq.py:137-213, core/bcq/policies.py) ------------------------------------------------
def bcq_supported(latent: int, act_dim: int, samples: int = 1) -> bool:
    """Widths the BCQ kernels take (cstr_bcq_*: CSTR_E_UNSUPPORTED beyond them)."""
    return 0 < latent <= nv.BCQ_MAX_LATENT and 0 < act_dim <= nv.BCQ_MAX_ACT and 0 < samples <= nv.BCQ_MAX_SAMPLES


def _one_noise(noise, rng_ctl, shape, what: str):
    if (noise is None) == (rng_ctl is None):
        raise ValueError(f"{what} needs exactly one noise source: a noise tensor or rng_ctl")
    _opt(noise, "noise", shape, th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)


def bcq_latent_fwd(params, obs, eps, rng_ctl, xdec, std_out, eps_out=None):
    """xdec [B, D + L] = [obs | mean + exp(clamp(log_std_raw, -4, 15)) * eps] from params [B, 2L] = [mean | log_std_raw]; eps [B, L] is
    read, or drawn (rng_ctl) and stored in eps_out; std_out [B, L] (policies.py:76-85)."""
    b, l2 = params.shape
    L = l2 // 2
    d = obs.shape[1]
    _chk(params, "params", (b, 2 * L), th.float32), _chk(xdec, "xdec", (b, d + L), th.float32), _chk(std_out, "std_out", (b, L), th.float32)
    ldo = _rows(obs, "obs", b, d)
    _one_noise(eps, rng_ctl, (b, L), "bcq_latent_fwd")
    _opt(eps_out, "eps_out", (b, L), th.float32)
    if rng_ctl is not None and eps_out is None:
        raise ValueError("bcq_latent_fwd: drawn noise needs eps_out")
    check(nv.lib().cstr_bcq_latent_fwd_f32(ptr(params), C.c_int64(2 * L), ptr(obs), C.c_int64(ldo), ptr(eps), ptr(rng_ctl), ptr(xdec),
                                           C.c_int64(d + L), ptr(std_out), ptr(eps_out), C.c_int64(b), C.c_int(d), C.c_int(L), stream_ptr()),
          "cstr_bcq_latent_fwd_f32")
    return xdec


def bcq_vae_loss(recon, act, params, std, g_recon=None, g_mean=None, g_std=None, loss_out=None, loss_sum=None):
    """mse(recon, act) + 0.5 * (-0.5 * mean(1 + log(std^2) - mean^2 - std^2)) (bcq.py:145-149): the logged scalar and the gradients
    w.r.t. recon and, for the KL term, mean / std."""
    b, a = recon.shape
    L = std.shape[1]
    ldr, lda = _rows(recon, "recon", b, a), _rows(act, "act", b, a)
    _chk(params, "params", (b, 2 * L), th.float32), _chk(std, "std", (b, L), th.float32)
    _opt(g_recon, "g_recon", (b, a), th.float32), _opt(g_mean, "g_mean", (b, L), th.float32), _opt(g_std, "g_std", (b, L), th.float32)
    for t, nm in ((loss_out, "loss_out"), (loss_sum, "loss_sum")):
        if t is not None:
            _vec(t, nm, 1)
    check(nv.lib().cstr_bcq_vae_loss_f32(ptr(recon), C.c_int64(ldr), ptr(act), C.c_int64(lda), ptr(params), C.c_int64(2 * L), ptr(std),
                                         C.c_int64(b), C.c_int(a), C.c_int(L), ptr(g_recon), ptr(g_mean), ptr(g_std), ptr(loss_out),
                                         ptr(loss_sum), stream_ptr()), "cstr_bcq_vae_loss_f32")


def bcq_latent_bwd(g_z, g_mean_kl, g_std_kl, params, std, eps, g_params):
    """g_params [B, 2L] = [g_z + g_mean_kl | (g_z * eps + g_std_kl) * std masked by the clamp]; g_z may be the latent columns of the
    decoder input's gradient (row-strided view)."""
    b, L = std.shape
    _chk(params, "params", (b, 2 * L), th.float32), _chk(std, "std", (b, L), th.float32), _chk(eps, "eps", (b, L), th.float32)
    _chk(g_params, "g_params", (b, 2 * L), th.float32)
    ldg = L if g_z is None else _rows(g_z, "g_z", b, L)
    _opt(g_mean_kl, "g_mean_kl", (b, L), th.float32), _opt(g_std_kl, "g_std_kl", (b, L), th.float32)
    check(nv.lib().cstr_bcq_latent_bwd_f32(ptr(g_z), C.c_int64(ldg), ptr(g_mean_kl), ptr(g_std_kl), ptr(params), C.c_int64(2 * L), ptr(std),
                                           ptr(eps), ptr(g_params), C.c_int64(b), C.c_int(L), stream_ptr()), "cstr_bcq_latent_bwd_f32")
    return g_params


def bcq_expand(state, samples: int, noise, rng_ctl, xdec, xa=None, xb=None, clip: float = 0.5):
    """xdec [n S, D + L] row r = [state[r % n] | clamp(noise, -clip, clip)] (noise [n S, L] raw, or drawn from rng_ctl); the first D
    columns of xa / xb [n S, >= D] (the perturbation net's and the critics' inputs) receive state[r % n] too (policies.py:122-124)."""
    if (noise is None) == (rng_ctl is None):
        raise ValueError("bcq_expand needs exactly one noise source: a noise tensor or rng_ctl")
    n, d = state.shape
    lds = _rows(state, "state", n, d)
    rows = n * samples
    if xdec.dim() != 2 or xdec.shape[1] <= d:
        raise ValueError("xdec: needs [n * samples, obs_dim + latent]")
    L = xdec.shape[1] - d
    _chk(xdec, "xdec", (rows, d + L), th.float32)
    _one_noise(noise, rng_ctl, (rows, L), "bcq_expand")
    lds_x = []
    for t, nm in ((xa, "xa"), (xb, "xb")):
        if t is not None and (t.dim() != 2 or t.shape[1] < d):
            raise ValueError(f"{nm}: needs at least obs_dim columns")
        lds_x.append(0 if t is None else _rows(t, nm, rows, t.shape[1]))
    check(nv.lib().cstr_bcq_expand_f32(ptr(state), C.c_int64(lds), C.c_int64(n), C.c_int(samples), C.c_int(d), C.c_int(L), ptr(noise),
                                       ptr(rng_ctl), C.c_float(clip), ptr(xdec), C.c_int64(d + L), ptr(xa), C.c_int64(lds_x[0]), ptr(xb),
                                       C.c_int64(lds_x[1]), stream_ptr()), "cstr_bcq_expand_f32")
    return xdec


def bcq_perturb_fwd(a_vae, p, max_perturbation: float, out):
    """out = clamp(a_vae + p * max_perturbation, -1, 1) (policies.py:165-166); a_vae / out may be column blocks of wider buffers."""
    rows, a = p.shape
    lda, ldp, ldo = _rows(a_vae, "a_vae", rows, a), _rows(p, "p", rows, a), _rows(out, "out", rows, a)
    check(nv.lib().cstr_bcq_perturb_fwd_f32(ptr(a_vae), C.c_int64(lda), ptr(p), C.c_int64(ldp), C.c_float(max_perturbation), ptr(out),
                                            C.c_int64(ldo), C.c_int64(rows), C.c_int(a), stream_ptr()), "cstr_bcq_perturb_fwd_f32")
    return out


def bcq_perturb_bwd(g_out, a_vae, p, max_perturbation: float, g_p):
    """g_p [rows, A] = g_out * max_perturbation where -1 <= a_vae + p * max_perturbation <= 1, else 0."""
    rows, a = p.shape
    ldg, lda, ldp = _rows(g_out, "g_out", rows, a), _rows(a_vae, "a_vae", rows, a), _rows(p, "p", rows, a)
    _chk(g_p, "g_p", (rows, a), th.float32)
    check(nv.lib().cstr_bcq_perturb_bwd_f32(ptr(g_out), C.c_int64(ldg), ptr(a_vae), C.c_int64(lda), ptr(p), C.c_int64(ldp),
                                            C.c_float(max_perturbation), ptr(g_p), C.c_int64(rows), C.c_int(a), stream_ptr()),
          "cstr_bcq_perturb_bwd_f32")
    return g_p


def bcq_target(q, n_states: int, samples: int, reference_grouping: bool, rew, done, gamma: float, target_out, max_q_out=None):
    """q [N, n S, 1] or [N, n S] (contiguous): min over the N critics per row, max over groups of S rows -- the reference's grouping
    (S consecutive flat rows, bcq.py:171-172) or the state's own candidates (rows i + n s) -- and the TD target (bcq.py:173)."""
    nq = q.shape[0]
    rows = n_states * samples
    if not (isinstance(q, th.Tensor) and q.is_cuda and q.dtype == th.float32 and q.is_contiguous() and q.numel() == nq * rows):
        raise ValueError(f"q: needs a contiguous float32 device tensor [N, {rows}(, 1)]")
    if target_out is not None:
        _vec(target_out, "target_out", n_states), _vec(rew, "rew", n_states), _vec(done, "done", n_states)
    if max_q_out is not None:
        _vec(max_q_out, "max_q_out", n_states)
    check(nv.lib().cstr_bcq_target_f32(ptr(q), C.c_int64(rows), C.c_int(nq), C.c_int64(n_states), C.c_int(samples),
                                       C.c_int(0 if reference_grouping else 1), ptr(rew), ptr(done), C.c_float(gamma), ptr(target_out),
                                       ptr(max_q_out), stream_ptr()), "cstr_bcq_target_f32")
    return target_out


def bcq_select(q1, cand, n_states: int, samples: int, index_out, action_out):
    """Per state the row (i + n s) of its largest q1 (first maximum wins, as argmax) and that row of cand [n S, A] (policies.py:429-435)."""
    rows = n_states * samples
    _vec(q1, "q1", rows)
    a = cand.shape[1]
    ldc = _rows(cand, "cand", rows, a)
    _opt(index_out, "index_out", (n_states,), th.int64), _chk(action_out, "action_out", (n_states, a), th.float32)
    check(nv.lib().cstr_bcq_select_f32(ptr(q1), ptr(cand), C.c_int64(ldc), C.c_int64(n_states), C.c_int(samples), C.c_int(a), ptr(index_out),
                                       ptr(action_out), stream_ptr()), "cstr_bcq_select_f32")
    return action_out


def neg_mean_loss(q, gq, loss_out=None, loss_sum=None):
    b = q.numel()
    _vec(q, "q", b), _vec(gq, "gq", b)
    check(nv.lib().cstr_neg_mean_loss_f32(ptr(q), ptr(gq), ptr(loss_out), ptr(loss_sum), C.c_int64(b), stream_ptr()),
          "cstr_neg_mean_loss_f32")


# ---- TD3+BC (csrc/cstr_td3bc.hip) ---------------------------------------------------------------------------------------------------
def td3bc_supported(batch: int, act_dim: int) -> bool:
    return 0 < batch <= nv.TD3BC_MAX_BATCH and 0 < act_dim <= nv.TD3BC_MAX_ACT


def td3bc_actor_loss(q, pi, act, alpha: float, gq, loss_out=None, loss_sum=None, aux=None):
    """TD3+BC's actor loss -lam * mean(q) + mean((pi - act)^2), lam = alpha / mean|q| (a constant), as a backward root
    (cstr_td3bc_actor_loss_f32): gq = -lam / B; aux [3] = {lam, -lam * mean(q), the second term}. pi / act [B, A] may be column
    blocks of wider row-major matrices."""
    b = q.numel()
    _vec(q, "q", b), _vec(gq, "gq", b)
    if pi.dim() != 2 or pi.shape[0] != b:
        raise ValueError(f"pi: needs a [{b}, A] matrix, got shape {tuple(pi.shape)}")
    a = pi.shape[1]
    ldpi, ldact = _rows(pi, "pi", b, a), _rows(act, "act", b, a)
    if aux is not None:
        _vec(aux, "aux", 3)
    for t, nm in ((loss_out, "loss_out"), (loss_sum, "loss_sum")):
        if t is not None:
            _vec(t, nm, 1)
    check(nv.lib().cstr_td3bc_actor_loss_f32(ptr(q), ptr(pi), C.c_int64(ldpi), ptr(act), C.c_int64(ldact), C.c_float(alpha), ptr(gq),
                                             ptr(loss_out), ptr(loss_sum), ptr(aux), C.c_int64(b), C.c_int(a), stream_ptr()),
          "cstr_td3bc_actor_loss_f32")


def td3bc_act_bwd_rows(gy, y, act, coef: float, act_kind: int, gz):
    """gz = (gy + coef * (y - act)) * act'(y) (cstr_td3bc_act_bwd_rows_f32): `bias_act_bwd_rows` with the behaviour-cloning gradient
    added where the incoming gradient is read; gy / y / act may be column blocks of wider row-major matrices, gz is contiguous."""
    m, n = gz.shape
    _chk(gz, "gz", (m, n), th.float32)
    ldg, ldy, lda = _rows(gy, "gy", m, n), _rows(y, "y", m, n), _rows(act, "act", m, n)
    check(nv.lib().cstr_td3bc_act_bwd_rows_f32(ptr(gy), C.c_int64(ldg), ptr(y), C.c_int64(ldy), ptr(act), C.c_int64(lda), C.c_float(coef),
                                               C.c_int(act_kind), ptr(gz), C.c_int64(m), C.c_int64(n), stream_ptr()),
          "cstr_td3bc_act_bwd_rows_f32")
    return gz


# ---- CQL (csrc/cstr_cql.hip) --------------------------------------------------------------------------------------------------------
CQL_LOG_UNIF_1 = C.c_float(math.log(0.5)).value  # logf(0.5f): the uniform density's log per action dimension of the box (-1, 1)


def cql_supported(n_actions: int, act_dim: int) -> bool:
    return 0 < n_actions <= nv.CQL_MAX_ACTIONS and 0 < act_dim <= nv.MAX_HEAD_ACT


def cql_log_unif(act_dim: int) -> float:
    """A * logf(0.5f) in float32: the correction of a uniform candidate, evaluated once on the host"""
    return C.c_float(float(act_dim) * CQL_LOG_UNIF_1).value  # two float32 values, their product rounded to float32 once


def cql_candidates(obs, params_cur, params_next, n_actions: int, x, corr=None, u=None, eps=None, rng_ctl=None):
    """x [B * 3N, D + A] row b * 3N + j = [obs_b | a_bj] (j < N uniform, < 2N ~ pi(.|s_b), < 3N ~ pi(.|s'_b)) and corr [B, 3N] =
    A log 0.5 | log pi(a | s) | log pi(a | s') from params_* [B, 2A] = [mean | raw log_std] (cstr_cql_candidates_f32). Noise: u [B, N, A]
    and eps [B, 2N, A] (read), or rng_ctl (drawn on CQL's Philox stream). obs / params_* / x may be row-strided."""
    if (u is None) != (eps is None) or (u is None) == (rng_ctl is None):
        raise ValueError("cql_candidates needs exactly one noise source: (u, eps) tensors or rng_ctl")
    b, d = obs.shape
    a = params_cur.shape[1] // 2
    n = int(n_actions)
    ldo = _rows(obs, "obs", b, d)
    ldp = _rows(params_cur, "params_cur", b, 2 * a)
    if _rows(params_next, "params_next", b, 2 * a) != ldp:
        raise ValueError("params_cur and params_next must share their row stride")
    ldx = _rows(x, "x", b * 3 * n, d + a)
    _opt(corr, "corr", (b, 3 * n), th.float32), _opt(u, "u", (b, n, a), th.float32), _opt(eps, "eps", (b, 2 * n, a), th.float32)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_cql_candidates_f32(ptr(obs), C.c_int64(ldo), ptr(params_cur), ptr(params_next), C.c_int64(ldp), C.c_int64(b),
                                           C.c_int(n), C.c_int(d), C.c_int(a), ptr(u), ptr(eps), ptr(rng_ctl), C.c_float(cql_log_unif(a)),
                                           ptr(x), C.c_int64(ldx), ptr(corr), stream_ptr()), "cstr_cql_candidates_f32")
    return x


def cql_q_loss(q, corr, with_data: bool, q1_t, q2_t, next_logp, rew, done, ent_coef, gamma: float, w: float, temp: float, target_out, gq,
               loss_out=None, loss_sum=None, aux=None):
    """CQL's critic loss as a backward root (cstr_cql_q_loss_f32): q [2, (1 + 3N) B(, 1)] = both critics on [data rows | candidate
    rows], corr [B, 3N] or None (then with_data); gq of q's shape = d loss / d q; aux [4] = {bellman, conservative (x w), mean lse,
    mean Q(s, a)}."""
    b = rew.numel()
    if not (isinstance(q, th.Tensor) and q.is_cuda and q.dtype == th.float32 and q.is_contiguous() and q.shape[0] == 2 and q[0].numel() % b == 0):
        raise ValueError("q: needs a contiguous float32 device tensor [2, (1 + 3N) B(, 1)]")
    rows = q[0].numel()
    n3 = rows // b - 1
    if n3 <= 0 or n3 % 3:
        raise ValueError(f"q: {rows} rows per critic are not (1 + 3N) * {b}")
    _vec(gq, "gq", 2 * rows)
    for t, nm in ((q1_t, "q1_t"), (q2_t, "q2_t"), (rew, "rew"), (done, "done")):
        _vec(t, nm, b)
    for t, nm, k in ((next_logp, "next_logp", b), (ent_coef, "ent_coef", 1), (target_out, "target_out", b), (loss_out, "loss_out", 1),
                     (loss_sum, "loss_sum", 1), (aux, "aux", 4)):
        if t is not None:
            _vec(t, nm, k)
    _opt(corr, "corr", (b, n3), th.float32)
    check(nv.lib().cstr_cql_q_loss_f32(ptr(q), C.c_int64(rows), ptr(corr), C.c_int(int(bool(with_data))), ptr(q1_t), ptr(q2_t), ptr(next_logp),
                                       ptr(rew), ptr(done), ptr(ent_coef), C.c_float(gamma), C.c_float(w), C.c_float(temp), ptr(target_out),
                                       ptr(gq), ptr(loss_out), ptr(loss_sum), ptr(aux), C.c_int64(b), C.c_int(n3 // 3), stream_ptr()),
          "cstr_cql_q_loss_f32")


# ---- IQL (csrc/cstr_iql.hip) --------------------------------------------------------------------------------------------------------
def iql_supported(batch: int, act_dim: int) -> bool:
    return 0 < batch <= nv.IQL_MAX_BATCH and 0 < act_dim <= nv.MAX_HEAD_ACT


def iql_loss(qt1, qt2, v, v_next, q1, q2, params, act, rew, done, gamma: float, expectile: float, beta: float, exp_adv_max: float,
             g_v=None, gq1=None, gq2=None, g_params=None, loss_out=None, loss_sum=None, aux=None, target_out=None, adv_out=None,
             logp_out=None):
    """IQL's three losses as backward roots (cstr_iql_loss_f32): u = min(qt1, qt2) - v; g_v of the expectile value loss; gq1 / gq2 of the
    critic loss against y = rew + (1 - done) gamma v_next (the twin TD loss head's bits); g_params [B, 2A] of the advantage-weighted
    log-prob of the dataset action `act` [B, A] under params [B, 2A] = [mean | raw log_std]. loss_out / loss_sum [3] = {value, critic,
    actor}; aux [6] = {mean u, mean w, clipped share, mean logp, mean v, mean y}; target_out / adv_out / logp_out [B]. params / act may be
    column blocks of wider row-major matrices; v and v_next may be the halves of one [2B] tensor."""
    b = rew.numel()
    for t, nm in ((qt1, "qt1"), (qt2, "qt2"), (v, "v"), (v_next, "v_next"), (q1, "q1"), (q2, "q2"), (rew, "rew"), (done, "done")):
        _vec(t, nm, b)
    if not isinstance(act, th.Tensor) or act.dim() != 2 or act.shape[0] != b:
        raise ValueError(f"act: needs a [{b}, A] matrix, got {tuple(act.shape) if isinstance(act, th.Tensor) else type(act)}")
    a = act.shape[1]
    ldact, ldp = _rows(act, "act", b, a), _rows(params, "params", b, 2 * a)
    if (gq1 is None) != (gq2 is None):
        raise ValueError("gq1 and gq2 are one group: both or neither")
    for t, nm, k in ((g_v, "g_v", b), (gq1, "gq1", b), (gq2, "gq2", b), (g_params, "g_params", b * 2 * a), (loss_out, "loss_out", 3),
                     (loss_sum, "loss_sum", 3), (aux, "aux", 6), (target_out, "target_out", b), (adv_out, "adv_out", b),
                     (logp_out, "logp_out", b)):
        if t is not None:
            _vec(t, nm, k)
    check(nv.lib().cstr_iql_loss_f32(ptr(qt1), ptr(qt2), ptr(v), ptr(v_next), ptr(q1), ptr(q2), ptr(params), C.c_int64(ldp), ptr(act),
                                     C.c_int64(ldact), ptr(rew), ptr(done), C.c_float(gamma), C.c_float(expectile), C.c_float(beta),
                                     C.c_float(exp_adv_max), ptr(g_v), ptr(gq1), ptr(gq2), ptr(g_params), ptr(loss_out), ptr(loss_sum),
                                     ptr(aux), ptr(target_out), ptr(adv_out), ptr(logp_out), C.c_int64(b), C.c_int(a), stream_ptr()),
          "cstr_iql_loss_f32")


# ---- TQC (csrc/cstr_tqc.hip) --------------------------------------------------------------------------------------------------------
def tqc_supported(n_critics: int, n_quantiles: int, drop_per_net: int) -> bool:
    """cstr_tqc_supported: 1 <= G <= MAX_ENS_CRITICS, G * Nq <= TQC_MAX_ATOMS, 0 <= k < Nq."""
    return bool(nv.lib().cstr_tqc_supported(C.c_int(int(n_critics)), C.c_int(int(n_quantiles)), C.c_int(int(drop_per_net))))


def _atoms(t, name):
    if not (isinstance(t, th.Tensor) and t.is_cuda and t.dtype == th.float32 and t.dim() == 3 and t.is_contiguous()):
        raise ValueError(f"{name}: needs a contiguous float32 device tensor [G, B, Nq]")
    return tuple(t.shape)


def tqc_critic_loss(z, z_next, next_logp, rew, done, ent_coef, gamma: float, drop_per_net: int, gz, ws, loss_out=None, loss_sum=None,
                    target_out=None, means_out=None, means_sum=None, alpha=None):
    """TQC's critic loss as a backward root (cstr_tqc_critic_loss_f32): z / z_next [G, B, Nq] = the critics' atoms at (s, a) / the target
    critics' at (s', a'); per row the G * Nq - k * G smallest target atoms give y = rew + (1 - done) gamma (z' - alpha next_logp)
    (target_out [B, n_keep], ascending), gz [G, B, Nq] = d(mean quantile-Huber loss)/dz. means_out / means_sum [2] = {mean y, mean z}.
    ws: float64 [3 B] scratch. `alpha`: SAC's entropy-coefficient part (the dict of `td_twin_q_loss`); without it ent_coef [1]."""
    g, b, nq = _atoms(z, "z")
    if _atoms(z_next, "z_next") != (g, b, nq) or _atoms(gz, "gz") != (g, b, nq):
        raise ValueError(f"z_next / gz: need z's shape {(g, b, nq)}")
    k = int(drop_per_net)
    for t, nm in ((next_logp, "next_logp"), (rew, "rew"), (done, "done")):
        _vec(t, nm, b)
    if not (isinstance(ws, th.Tensor) and ws.is_cuda and ws.dtype == th.float64 and ws.is_contiguous() and ws.numel() == 3 * b):
        raise ValueError(f"ws: needs a contiguous float64 device tensor with {3 * b} elements")
    for t, nm, n in ((loss_out, "loss_out", 1), (loss_sum, "loss_sum", 1), (means_out, "means_out", 2), (means_sum, "means_sum", 2),
                     (target_out, "target_out", b * max(g * nq - k * g, 0))):
        if t is not None:
            _vec(t, nm, n)
    part = None
    if alpha is not None:
        _vec(alpha["logp_pi"], "logp_pi", b)
        for nm in ("log_alpha", "grad_out", "ent_coef_out"):
            _vec(alpha[nm], nm, 1)
        part = nv.AlphaPart(alpha["log_alpha"].data_ptr(), alpha["logp_pi"].data_ptr(), float(alpha["target_entropy"]),
                            alpha["grad_out"].data_ptr(), alpha["ent_coef_out"].data_ptr(),
                            *(None if alpha.get(key) is None else alpha[key].data_ptr() for key in ("loss_out", "loss_sum", "ent_coef_sum")))
    elif ent_coef is None:
        raise ValueError("the entropy term needs ent_coef or the alpha part")
    else:
        _vec(ent_coef, "ent_coef", 1)
    check(nv.lib().cstr_tqc_critic_loss_f32(ptr(z), ptr(z_next), ptr(next_logp), ptr(rew), ptr(done), ptr(None if alpha is not None else ent_coef),
                                            C.c_double(gamma), C.c_int(g), C.c_int(nq), C.c_int(k), ptr(gz), ptr(loss_out), ptr(loss_sum),
                                            ptr(target_out), ptr(means_out), ptr(means_sum), ptr(ws), None if part is None else C.byref(part),
                                            C.c_int64(b), stream_ptr()), "cstr_tqc_critic_loss_f32")


def tqc_actor_loss(z_pi, logp, ent_coef, gz_pi, g_logp, loss_out=None, loss_sum=None, z_pi_mean=None):
    """TQC's actor loss as a backward root (cstr_tqc_actor_loss_f32): loss = mean_b(ent_coef * logp - mean over (g, i) of z_pi [G, B, Nq]);
    gz_pi [G, B, Nq] = -1 / (B G Nq), g_logp [B] = ent_coef / B, z_pi_mean [B] the row means."""
    g, b, nq = _atoms(z_pi, "z_pi")
    if _atoms(gz_pi, "gz_pi") != (g, b, nq):
        raise ValueError(f"gz_pi: needs z_pi's shape {(g, b, nq)}")
    _vec(logp, "logp", b), _vec(g_logp, "g_logp", b), _vec(ent_coef, "ent_coef", 1)
    for t, nm, n in ((loss_out, "loss_out", 1), (loss_sum, "loss_sum", 1), (z_pi_mean, "z_pi_mean", b)):
        if t is not None:
            _vec(t, nm, n)
    check(nv.lib().cstr_tqc_actor_loss_f32(ptr(z_pi), ptr(logp), ptr(ent_coef), C.c_int(g), C.c_int(nq), ptr(gz_pi), ptr(g_logp), ptr(loss_out),
                                           ptr(loss_sum), ptr(z_pi_mean), C.c_int64(b), stream_ptr()), "cstr_tqc_actor_loss_f32")


# ---- row-chain kernels (csrc/cstr_chain.hip, include/cstr_rl_hip.h "row-chain kernels") -------------------------------------------
def chain_supported(h1: int, h2: int, batch: int) -> bool:
    """Widths multiples of 4; forward launches hold a 16 x (H1 + 4) panel and W1 staged as [H1][8 or 16] in 64 KB of LDS."""
    return (16 <= h1 <= nv.CHAIN_MAX_WIDTH and 16 <= h2 <= nv.CHAIN_MAX_WIDTH and h1 % 4 == 0 and h2 % 4 == 0 and 4 * (1664 + 16 * (h1 + 4) + 16 * h1) <= 65536
            and 16 <= batch <= 1024 and batch % 16 == 0)


def chain_tiles_ok(kdim: int, tiles: int, forward: bool = False) -> bool:
    """A wave holds at most 16 (forward chains: 32) 16-wide chunks of the reduction in registers."""
    s = 4 // tiles
    return -(-((kdim + 15) // 16) // s) <= (32 if forward else 16)


def chain_colgroups(width: int, tiles: int) -> int:
    return (width + 16 * tiles - 1) // (16 * tiles)


def _dp(t):
    return None if t is None else t.data_ptr()


def sac_actor_desc(obs_dim: int, act_dim: int, w1, b1, w2, b2, hw, hb) -> "nv.SacActorNet":
    """hw / hb: the merged [mu | log_std] head ([2A, H2]) or a deterministic actor's last Linear ([A, H2])."""
    h1, h2 = w1.shape[0], w2.shape[0]
    hn = hw.shape[0]
    if hn not in (act_dim, 2 * act_dim):
        raise ValueError(f"head: {hn} outputs for {act_dim} actions")
    for t, nm, shape in ((w1, "w1", (h1, obs_dim)), (b1, "b1", (h1,)), (w2, "w2", (h2, h1)), (b2, "b2", (h2,)), (hw, "hw", (hn, h2)),
                         (hb, "hb", (hn,))):
        _chk(t, nm, shape, th.float32)
    return nv.SacActorNet(obs_dim, act_dim, h1, h2, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), hw.data_ptr(), hb.data_ptr())


def sac_actor_chain_fwd(actor: "nv.SacActorNet", batch: int, x_data, x_pi, x_next, out_done, out_rew, a_h1, a_h2, head_part, tiles: int,
                        ring: Optional[DeviceRing] = None, sample_idx=None, advance_ring: bool = False, head_rng_ctl=None, head_rng_offset: int = 0,
                        eps_all=None, rows_mode: int = 0, head_n: Optional[int] = None):
    """cstr_sac_actor_chain_fwd_f32: gather (or packed observation columns) + layer 1 + layer 2 + head partials of an actor pass
    (rows_mode: CHAIN_ROWS_PAIR = SAC's 2B rows, CHAIN_ROWS_NEXT / CHAIN_ROWS_OBS = B rows of a deterministic actor)."""
    w = actor.obs_dim + actor.act_dim
    ncg = chain_colgroups(actor.h2, tiles)
    head_n = 2 * actor.act_dim if head_n is None else head_n
    m = 2 * batch if rows_mode == nv.CHAIN_ROWS_PAIR else batch
    for t, nm in ((x_pi, "x_pi"), (x_next, "x_next")):
        if t is not None and not (t.is_cuda and t.dtype == th.float32 and tuple(t.shape) == (batch, w) and t.stride() == (w, 1)):
            raise ValueError(f"{nm}: needs a float32 device matrix [{batch}, {w}] with row stride {w}")
    _opt(a_h1, "a_h1", (batch, actor.h1), th.float32), _opt(a_h2, "a_h2", (batch, actor.h2), th.float32)
    _chk(head_part, "head_part", (ncg, m, head_n), th.float32)
    _opt(eps_all, "eps_all", (m, actor.act_dim), th.float32), _opt(head_rng_ctl, "head_rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    if not chain_tiles_ok(actor.h1, tiles, forward=True):
        raise ValueError(f"tiles = {tiles}: a wave's share of K = {actor.h1} does not fit")
    if sample_idx is not None:
        _chk(sample_idx, "sample_idx", (2, batch), th.int32)
        _chk(x_data, "x_data", (batch, w), th.float32), _chk(out_done, "out_done", (batch, 1), th.float32), _chk(out_rew, "out_rew", (batch, 1), th.float32)
    check(nv.lib().cstr_sac_actor_chain_fwd_f32(C.byref(actor), None if ring is None else C.byref(ring.c), None if ring is None else ptr(ring.ctl),
                                                C.c_int(1 if advance_ring else 0), ptr(sample_idx),
                                                C.c_int64(batch), ptr(x_data), ptr(x_pi), ptr(x_next), ptr(out_done), ptr(out_rew), ptr(a_h1),
                                                ptr(a_h2), ptr(head_part), ptr(head_rng_ctl), C.c_uint64(int(head_rng_offset)), ptr(eps_all),
                                                C.c_int(rows_mode), C.c_int(head_n), C.c_int(tiles), stream_ptr()),
          "cstr_sac_actor_chain_fwd_f32")


def chain_net(layers, x=None, h1=None, h2=None, q_part=None, role: int = 0) -> "nv.ChainNet":
    """layers = ((w1, b1), (w2, b2), (w3, b3)) of one Q network."""
    (w1, b1), (w2, b2), (w3, b3) = layers
    return nv.ChainNet(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), _dp(x), _dp(h1), _dp(h2),
                       _dp(q_part), role, 0)


def chain_check_nets(nets, w_in: int, h1: int, h2: int) -> None:
    """Every ((w1, b1), (w2, b2), (w3, b3)) of `nets` is what the chain kernels read behind chain_net's raw pointers: float32, contiguous,
    on the current device, shaped by W / H1 / H2. For whoever binds the networks, once (chain_net runs every step)."""
    for i, ((w1, b1), (w2, b2), (w3, b3)) in enumerate(nets):
        for t, nm, shape in ((w1, "w1", (h1, w_in)), (b1, "b1", (h1,)), (w2, "w2", (h2, h1)), (b2, "b2", (h2,)), (w3, "w3", (1, h2)), (b3, "b3", (1,))):
            _chk(t, f"Q network {i}: {nm}", shape, th.float32)


def q_chain_fwd(nets, w_in: int, obs_dim: int, h1: int, h2: int, batch: int, tiles: int, fin: Optional["nv.SacHeadFin"] = None):
    """cstr_q_chain_fwd_f32: n_nets Q networks (layer 1 recomputed, layer 2 one MFMA column group per workgroup, head as partials)."""
    arr = (nv.ChainNet * len(nets))(*nets)
    check(nv.lib().cstr_q_chain_fwd_f32(arr, C.c_int(len(nets)), C.c_int(w_in), C.c_int(obs_dim), C.c_int(h1), C.c_int(h2), C.c_int64(batch),
                                        None if fin is None else C.byref(fin), C.c_int(tiles), stream_ptr()), "cstr_q_chain_fwd_f32")


def linear_bwd_weight_adam_sets(sets, opts, flat=()):
    """cstr_linear_bwd_weight_adam_sets_f32: dW / db of several Linears AND their Adam steps in one launch. `sets`: [(dz [M, N], x [M, K]
    (row-strided ok), weight parameter, bias parameter, optimiser index, shadow tensor or None[, (weight target, bias target, tau)])];
    the parameters' .grad and moment views
    are looked up in `opts` = [FlatAdam, ...] (pre-advanced control words: see chain_root's adam_advance). `flat`: adam_multi segments
    (no shadow) for parameters without a tile and soft target updates."""
    sets, opts = list(sets), list(opts)
    arr = (nv.WgradAdamSet * len(sets))()
    oarr = (nv.AdamOpt * len(opts))()
    for i, o in enumerate(opts):
        g = o.param_groups[0]
        oarr[i] = nv.AdamOpt(o.ctl.data_ptr(), o.lr_dev.data_ptr(), g["betas"][0], g["betas"][1], g["eps"], o.grad_scale, 0)
    for i, st in enumerate(sets):
        dz, x, weight, bias, oi, shadow = st[:6]
        own = st[6] if len(st) > 6 and st[6] is not None else (None, None, 0.0)
        m, n = dz.shape
        k = x.shape[-1]
        _f32c(dz, f"dz[{i}]")
        if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == m):
            raise ValueError(f"x[{i}]: needs a float32 device matrix with unit inner stride and as many rows as dz")
        # a parameter of the optimiser's arena, or an explicit (values, gradient, exp_avg, exp_avg_sq) quadruple of views (merged heads)
        wq = weight if isinstance(weight, tuple) else (weight.detach(), weight.grad, *opts[oi].moments_of(weight))
        bq = bias if isinstance(bias, tuple) else (bias.detach(), bias.grad, *opts[oi].moments_of(bias))
        for t in wq:
            if t is None or _f32c(t, f"weight[{i}]").numel() != n * k:
                raise ValueError(f"set {i}: weight views do not match dz {tuple(dz.shape)} and x {tuple(x.shape)}")
        for t in bq:
            if t is None or _f32c(t, f"bias[{i}]").numel() != n:
                raise ValueError(f"set {i}: bias views do not match dz {tuple(dz.shape)}")
        if shadow is not None and _f32c(shadow, "shadow").numel() != swizzled_numel(n, k):
            raise ValueError("shadow: wrong size")
        arr[i] = nv.WgradAdamSet(nv.WgradSet(dz.data_ptr(), x.data_ptr(), max(x.stride(0), k), wq[1].data_ptr(), bq[1].data_ptr(), m, n, k),
                                 wq[0].data_ptr(), wq[2].data_ptr(), wq[3].data_ptr(), bq[0].data_ptr(), bq[2].data_ptr(), bq[3].data_ptr(),
                                 _dp(shadow), oi, 0, _dp(own[0]), _dp(own[1]), float(own[2]), 0.0)
        if own[0] is not None and (_f32c(own[0], "weight target").numel() != n * k or _f32c(own[1], "bias target").numel() != n):
            raise ValueError(f"set {i}: target views do not match the parameters")
    farr, nf = _adam_segments(flat)
    check(nv.lib().cstr_linear_bwd_weight_adam_sets_f32(arr, C.c_int(len(sets)), oarr, C.c_int(len(opts)), farr, C.c_int(nf), stream_ptr()),
          "cstr_linear_bwd_weight_adam_sets_f32")


def chain_root(mode: str, batch: int, q_parts, b3s, n_parts: int, gamma: float = 0.0, scale: float = 0.0, next_logp=None, rew=None, done=None,
               ent_coef=None, logp=None, target_out=None, q_out=None, gq_out=None, loss_out=None, loss_sum=None, alpha: Optional[dict] = None,
               rng_advance=None, adam_advance=()) -> "nv.ChainRoot":
    part = nv.AlphaPart()
    if alpha is not None:
        part = nv.AlphaPart(alpha["log_alpha"].data_ptr(), alpha["logp_pi"].data_ptr(), float(alpha["target_entropy"]), alpha["grad_out"].data_ptr(),
                            alpha["ent_coef_out"].data_ptr(), *(_dp(alpha.get(k)) for k in ("loss_out", "loss_sum", "ent_coef_sum")))
    qp, bb = (C.c_void_p * 4)(), (C.c_void_p * 4)()
    for i, (q, b) in enumerate(zip(q_parts, b3s)):
        qp[i], bb[i] = q.data_ptr(), b.data_ptr()
    rc_ptr, adv = (None, 0) if rng_advance is None else (rng_advance[0].data_ptr(), int(rng_advance[1]))
    actl, ab1, ab2 = (C.c_void_p * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
    for i, opt in enumerate(adam_advance):  # FlatAdam optimisers whose step counter this launch advances (<= 2)
        actl[i], (ab1[i], ab2[i]) = opt.ctl.data_ptr(), opt.param_groups[0]["betas"]
    return nv.ChainRoot({"td": 1, "sac_actor": 2, "neg_mean": 3}[mode], batch, float(gamma), float(scale), qp, bb, n_parts, 0, _dp(next_logp), _dp(rew),
                        _dp(done), None if alpha is not None else _dp(ent_coef), _dp(logp), _dp(target_out), _dp(q_out), _dp(gq_out), _dp(loss_out),
                        _dp(loss_sum), part, rc_ptr, adv, actl, ab1, ab2)


def q_chain_bwd(nets, root: "nv.ChainRoot", w_in: int, obs_dim: int, h1: int, h2: int, tiles: int, dz2=None, dz1=None, gact_part=None):
    """cstr_q_chain_bwd_f32: loss root + dz2 (recomputed) + one column group of dz1 (+ partial action gradients)."""
    arr = (nv.ChainNet * len(nets))(*nets)
    check(nv.lib().cstr_q_chain_bwd_f32(arr, C.c_int(len(nets)), C.byref(root), C.c_int(w_in), C.c_int(obs_dim), C.c_int(h1), C.c_int(h2), ptr(dz2),
                                        ptr(dz1), ptr(gact_part), C.c_int(tiles), stream_ptr()), "cstr_q_chain_bwd_f32")


def chain_lean(on: int = -1) -> int:
    """cstr_chain_lean: 0 = the generic Q chain and actor forward chain kernels from now on, > 0 = the lean ones where they exist (the
    default), < 0 = query; returns the setting before the call (both kernels write the same bits: tests/test_qchain_lean_bodies.py,
    tests/test_actor_chain_lean_bodies.py)."""
    return int(nv.lib().cstr_chain_lean(C.c_int(on)))


def sac_actor_chain_bwd(actor: "nv.SacActorNet", gact_part, n_nets: int, n_parts: int, ent_coef, x_pi, params, eps, a_h1, a_h2, g_params, dz2, dz1,
                        batch: int, tiles: int, kind: int = 0):
    """cstr_sac_actor_chain_bwd_f32: action gradient from the critic's partials, head backward (kind: CHAIN_HEAD_GAUSSIAN / _DETERMINISTIC),
    dz2 (recomputed), dz1 column group."""
    hn = actor.act_dim if kind == nv.CHAIN_HEAD_DETERMINISTIC else 2 * actor.act_dim
    _chk(gact_part, "gact_part", (n_nets, n_parts, batch, actor.act_dim), th.float32)
    _chk(g_params, "g_params", (batch, hn), th.float32), _chk(dz2, "dz2", (batch, actor.h2), th.float32)
    _chk(dz1, "dz1", (batch, actor.h1), th.float32)
    check(nv.lib().cstr_sac_actor_chain_bwd_f32(C.byref(actor), ptr(gact_part), C.c_int(n_nets), C.c_int(n_parts), ptr(ent_coef), ptr(x_pi), ptr(params),
                                                ptr(eps), ptr(a_h1), ptr(a_h2), ptr(g_params), ptr(dz2), ptr(dz1), C.c_int64(batch), C.c_int(kind),
                                                C.c_int(tiles), stream_ptr()), "cstr_sac_actor_chain_bwd_f32")


def chain_sum_parts(part, out):
    """cstr_chain_sum_parts_f32: out [rows, cols] (row-strided ok) = sum over the leading dimension(s) of part [..., rows, cols]."""
    rows, cols = out.shape
    n_parts = part.numel() // (rows * cols)
    if part.numel() != n_parts * rows * cols or _f32c(part, "part") is None:
        raise ValueError("part: needs [n_parts, rows, cols]")
    if not (out.is_cuda and out.dtype == th.float32 and out.stride(1) == 1):
        raise ValueError("out: needs a float32 device matrix with unit inner stride")
    check(nv.lib().cstr_chain_sum_parts_f32(ptr(part), C.c_int(n_parts), C.c_int64(rows), C.c_int(cols), ptr(out), C.c_int64(out.stride(0)), stream_ptr()),
          "cstr_chain_sum_parts_f32")


# ---- PPO: rollout head, rollout buffer, GAE, minibatch gather, loss, gradient clip (csrc/cstr_ppo.hip) ---------------------------
PPO_SCALARS = ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")


def ppo_supported(obs_dim: int, act_dim: int) -> bool:
    return obs_dim in (4, 8) and act_dim in (2, 4)


def rollout_supported(obs_dim: int, act_dim: int) -> bool:
    """the device rollout buffer's widths: the Gaussian head's, and act_dim 1 (the Categorical head's index as one float)"""
    return obs_dim in (4, 8) and act_dim in (1, 2, 4)


def goal_onpolicy_supported(features_dim: int, act_dim: int) -> bool:
    """PPO / A2C on the goal face: the flat row [achieved_goal | desired_goal | observation] in front of the Gaussian head's valve pair"""
    return features_dim == GOAL_ROW and act_dim == 2


def new_ppo_workspace(device) -> th.Tensor:
    """uint64[CSTR_PPO_WS_WORDS] (as int64) for cstr_ppo_loss_f32 / cstr_grad_clip_f32: zero before the first use, one per stream"""
    return th.zeros(nv.PPO_WS_WORDS, dtype=th.int64, device=device)


class DeviceRollout:
    """cstr_rollout_t + its control words over torch tensors (HBM). Field arrays have the reference's names and shapes
    (core/common/buffers.py:392-399): [T, N, D] / [T, N, A] / [T, N]; ctl = {pos, full, ticket, adds}."""

    FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")

    def __init__(self, rows: int, n_envs: int, obs_dim: int, act_dim: int, device, goal: bool = False):
        """goal: the goal face's buffer, observations [T, N, GOAL_ROW] flat rows (goal_rollout_add / goal_ppo_gather serve it)"""
        if goal and not goal_onpolicy_supported(obs_dim, act_dim):
            raise ValueError(f"DeviceRollout on the goal face needs obs_dim {GOAL_ROW} and act_dim 2, got {obs_dim}/{act_dim}")
        if not goal and not rollout_supported(obs_dim, act_dim):
            raise ValueError(f"DeviceRollout supports obs_dim in (4, 8) and act_dim in (1, 2, 4), got {obs_dim}/{act_dim}")
        self.goal = bool(goal)
        if rows <= 0 or n_envs <= 0:
            raise ValueError(f"DeviceRollout needs rows >= 1 and n_envs >= 1, got {rows}/{n_envs}")
        z = lambda *s: th.zeros(*s, dtype=th.float32, device=device)  # noqa: E731
        self.observations, self.actions = z(rows, n_envs, obs_dim), z(rows, n_envs, act_dim)
        self.rewards, self.episode_starts, self.values, self.log_probs, self.advantages, self.returns = (z(rows, n_envs) for _ in range(6))
        self.ctl = th.zeros(nv.ROLLOUT_CTL_WORDS, dtype=th.int64, device=device)
        self.rows, self.n_envs, self.obs_dim, self.act_dim = rows, n_envs, obs_dim, act_dim
        self.c = nv.Rollout(*(getattr(self, f).data_ptr() for f in self.FIELDS), rows, n_envs, obs_dim, act_dim)


def diag_gaussian_act(mean, log_std, eps, rng_ctl, low, high, deterministic: bool, action, env_action=None, log_prob=None, eps_out=None):
    """action = mean + exp(log_std) * eps (deterministic: mean); env_action = clip(action, low, high); log_prob [n]. eps is read when
    given, drawn from the Philox stream `rng_ctl` otherwise."""
    n, a = mean.shape
    _chk(mean, "mean", (n, a), th.float32), _chk(log_std, "log_std", (a,), th.float32), _chk(action, "action", (n, a), th.float32)
    _opt(eps, "eps", (n, a), th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    _opt(env_action, "env_action", (n, a), th.float32), _opt(log_prob, "log_prob", (n,), th.float32), _opt(eps_out, "eps_out", (n, a), th.float32)
    _opt(low, "low", (a,), th.float32), _opt(high, "high", (a,), th.float32)
    check(nv.lib().cstr_diag_gaussian_act_f32(ptr(mean), ptr(log_std), ptr(eps), ptr(rng_ctl), ptr(low), ptr(high), C.c_int(int(bool(deterministic))),
                                              ptr(action), ptr(env_action), ptr(log_prob), ptr(eps_out), C.c_int64(n), C.c_int(a), stream_ptr()),
          "cstr_diag_gaussian_act_f32")


def rollout_add(rb: DeviceRollout, obs, act, reward, episode_start, value, log_prob, timeout=None, terminal_value=None, gamma: float = 0.99,
                done=None, ep_return=None, ep_len=None, ep_stats=None):
    """RolloutBuffer.add at the device position (+ reward += f32(gamma) * terminal_value where timeout: c_float rounds gamma). With `done`, `episode_start`
    becomes `done` for the next call; with ep_return / ep_len / ep_stats the episode statistics accumulate in the same launch."""
    _rollout_add("cstr_rollout_add_f32", rb, obs, act, reward, episode_start, value, log_prob, timeout, terminal_value, gamma, done, ep_return,
                 ep_len, ep_stats)


def goal_rollout_add(rb: DeviceRollout, rows, act, reward, episode_start, value, log_prob, timeout=None, terminal_value=None,
                     gamma: float = 0.99, done=None, ep_return=None, ep_len=None, ep_stats=None):
    """`rollout_add` on the goal face's buffer: `rows` [n, GOAL_ROW] are the env's flat rows (DictRolloutBuffer.add)"""
    if not rb.goal:
        raise ValueError("goal_rollout_add needs a DeviceRollout of the goal face (goal=True)")
    _rollout_add("cstr_goal_rollout_add_f32", rb, rows, act, reward, episode_start, value, log_prob, timeout, terminal_value, gamma, done,
                 ep_return, ep_len, ep_stats)


def _rollout_add(entry: str, rb, obs, act, reward, episode_start, value, log_prob, timeout, terminal_value, gamma, done, ep_return, ep_len,
                 ep_stats):
    n, d, a = rb.n_envs, rb.obs_dim, rb.act_dim
    _chk(obs, "obs", (n, d), th.float32), _chk(act, "act", (n, a), th.float32)
    for t, nm in ((reward, "reward"), (episode_start, "episode_start"), (value, "value"), (log_prob, "log_prob")):
        _chk(t, nm, (n,), th.float32)
    for t, nm in ((timeout, "timeout"), (terminal_value, "terminal_value"), (done, "done"), (ep_return, "ep_return")):
        _opt(t, nm, (n,), th.float32)
    _opt(ep_len, "ep_len", (n,), th.int32), _opt(ep_stats, "ep_stats", (4,), th.float64)
    check(getattr(nv.lib(), entry)(C.byref(rb.c), ptr(rb.ctl), ptr(obs), ptr(act), ptr(reward), ptr(episode_start), ptr(value), ptr(log_prob),
                                   ptr(timeout), ptr(terminal_value), C.c_float(gamma), ptr(done), ptr(ep_return), ptr(ep_len), ptr(ep_stats),
                                   stream_ptr()), entry)


def gae(rb: DeviceRollout, last_values, dones, gamma: float, gae_lambda: float):
    """compute_returns_and_advantage over the whole buffer (bit-identical to NumPy's evaluation)"""
    t, n = rb.rows, rb.n_envs
    _chk(last_values, "last_values", (n,), th.float32), _chk(dones, "dones", (n,), th.float32)
    check(nv.lib().cstr_gae_f32(ptr(rb.rewards), ptr(rb.values), ptr(rb.episode_starts), ptr(last_values), ptr(dones), C.c_double(gamma),
                                C.c_double(gae_lambda), ptr(rb.advantages), ptr(rb.returns), C.c_int64(t), C.c_int64(n), stream_ptr()),
          "cstr_gae_f32")


def ppo_gather(rb: DeviceRollout, idx, obs, act, old_value, old_log_prob, adv, ret):
    """rows idx (flat swap_and_flatten order: env idx // T, step idx % T) of the six minibatch fields into contiguous tensors"""
    _ppo_gather("cstr_ppo_gather_f32", rb, idx, obs, act, old_value, old_log_prob, adv, ret)


def goal_ppo_gather(rb: DeviceRollout, idx, rows, act, old_value, old_log_prob, adv, ret):
    """`ppo_gather` on the goal face's buffer: `rows` [b, GOAL_ROW] receives the flat observation rows (DictRolloutBuffer.get)"""
    if not rb.goal:
        raise ValueError("goal_ppo_gather needs a DeviceRollout of the goal face (goal=True)")
    _ppo_gather("cstr_goal_ppo_gather_f32", rb, idx, rows, act, old_value, old_log_prob, adv, ret)


def _ppo_gather(entry: str, rb, idx, obs, act, old_value, old_log_prob, adv, ret):
    b = idx.shape[0]
    _chk(idx, "idx", (b,), th.int64), _chk(obs, "obs", (b, rb.obs_dim), th.float32), _chk(act, "act", (b, rb.act_dim), th.float32)
    for t, nm in ((old_value, "old_value"), (old_log_prob, "old_log_prob"), (adv, "adv"), (ret, "ret")):
        _chk(t, nm, (b,), th.float32)
    check(getattr(nv.lib(), entry)(C.byref(rb.c), ptr(idx), C.c_int64(b), ptr(obs), ptr(act), ptr(old_value), ptr(old_log_prob), ptr(adv), ptr(ret),
                                   stream_ptr()), entry)


def ppo_loss(mean, log_std, actions, values, old_values, old_log_prob, adv, returns, clip_range: float, clip_range_vf: Optional[float],
             normalize_advantage: bool, ent_coef: float, vf_coef: float, g_mean, g_value, g_log_std, workspace, scalars_out=None,
             scalars_sum=None, log_prob_out=None):
    """ppo.py:213-264 in one launch: the six scalars (PPO_SCALARS order) and d loss / d (mean, value, log_std)."""
    b, a = actions.shape
    ldm = _rows(mean, "mean", b, a)
    _chk(log_std, "log_std", (a,), th.float32), _chk(actions, "actions", (b, a), th.float32)
    for t, nm in ((values, "values"), (old_log_prob, "old_log_prob"), (adv, "adv"), (returns, "returns"), (g_value, "g_value")):
        _vec(t, nm, b)
    if old_values is not None:
        _vec(old_values, "old_values", b)
    _chk(g_mean, "g_mean", (b, a), th.float32), _vec(g_log_std, "g_log_std", a)
    _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
    for t, nm in ((scalars_out, "scalars_out"), (scalars_sum, "scalars_sum")):
        if t is not None:
            _vec(t, nm, 6)
    if log_prob_out is not None:
        _vec(log_prob_out, "log_prob_out", b)
    p = nv.PpoLoss(mean.data_ptr(), ldm, log_std.data_ptr(), actions.data_ptr(), values.data_ptr(),
                   None if old_values is None else old_values.data_ptr(), old_log_prob.data_ptr(), adv.data_ptr(), returns.data_ptr(), b, a,
                   int(bool(normalize_advantage)), float(clip_range), -1.0 if clip_range_vf is None else float(clip_range_vf), float(ent_coef),
                   float(vf_coef), g_mean.data_ptr(), g_value.data_ptr(), g_log_std.data_ptr(),
                   None if scalars_out is None else scalars_out.data_ptr(), None if scalars_sum is None else scalars_sum.data_ptr(),
                   None if log_prob_out is None else log_prob_out.data_ptr())
    check(nv.lib().cstr_ppo_loss_f32(C.byref(p), ptr(workspace), stream_ptr()), "cstr_ppo_loss_f32")


def grad_clip(grad, max_norm: float, workspace, norm_out=None):
    """torch.nn.utils.clip_grad_norm_ over one flat gradient buffer, in place; the coefficient never visits the host"""
    n = grad.numel()
    _vec(grad, "grad", n), _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
    if norm_out is not None:
        _vec(norm_out, "norm_out", 1)
    check(nv.lib().cstr_grad_clip_f32(ptr(grad), C.c_int64(n), C.c_float(max_norm), ptr(workspace), ptr(norm_out), stream_ptr()),
          "cstr_grad_clip_f32")


# ---- A2C: the loss launch and the flat RMSprop step with the gradient clip folded in (csrc/cstr_a2c.hip) ----------------------------
A2C_SCALARS = ("policy_loss", "value_loss", "entropy_loss", "loss")


def a2c_loss(mean, log_std, actions, values, adv, returns, normalize_advantage: bool, ent_coef: float, vf_coef: float, g_mean, g_value,
             g_log_std, workspace, scalars_out=None, log_prob_out=None):
    """a2c.py:150-171 in one launch: the four scalars (A2C_SCALARS order) and d loss / d (mean, value, log_std). With
    normalize_advantage a single row gives NaN, as torch.std of one element does (the reference has no guard)."""
    b, a = actions.shape
    ldm = _rows(mean, "mean", b, a)
    _chk(log_std, "log_std", (a,), th.float32), _chk(actions, "actions", (b, a), th.float32)
    for t, nm in ((values, "values"), (adv, "adv"), (returns, "returns"), (g_value, "g_value")):
        _vec(t, nm, b)
    _chk(g_mean, "g_mean", (b, a), th.float32), _vec(g_log_std, "g_log_std", a)
    _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
    if scalars_out is not None:
        _vec(scalars_out, "scalars_out", 4)
    if log_prob_out is not None:
        _vec(log_prob_out, "log_prob_out", b)
    p = nv.A2cLoss(mean.data_ptr(), ldm, log_std.data_ptr(), actions.data_ptr(), values.data_ptr(), adv.data_ptr(), returns.data_ptr(), b, a,
                   int(bool(normalize_advantage)), float(ent_coef), float(vf_coef), g_mean.data_ptr(), g_value.data_ptr(), g_log_std.data_ptr(),
                   None if scalars_out is None else scalars_out.data_ptr(), None if log_prob_out is None else log_prob_out.data_ptr())
    check(nv.lib().cstr_a2c_loss_f32(C.byref(p), ptr(workspace), stream_ptr()), "cstr_a2c_loss_f32")


def rmsprop(param, grad, square_avg, lr_dev, alpha: float = 0.99, eps: float = 1e-8, max_norm: Optional[float] = None, workspace=None,
            norm_out=None):
    """torch.optim.RMSprop (momentum 0, not centred, no weight decay) over one flat arena. max_norm > 0: clip_grad_norm_ folded in
    (two launches, the clipped gradient is written back); None or <= 0: one launch, the gradient is only read."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (square_avg, "square_avg")):
        _chk(t, nm, (n,), th.float32)
    _chk(lr_dev, "lr", (1,), th.float64)
    clip = max_norm is not None and max_norm > 0
    if clip:
        _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
        if norm_out is not None:
            _vec(norm_out, "norm_out", 1)
    check(nv.lib().cstr_rmsprop_f32(ptr(param), ptr(grad), ptr(square_avg), ptr(lr_dev), C.c_double(alpha), C.c_double(eps),
                                    C.c_float(max_norm if clip else 0.0), ptr(workspace if clip else None), ptr(norm_out if clip else None),
                                    C.c_int64(n), stream_ptr()), "cstr_rmsprop_f32")


def rmsprop_tf(param, grad, square_avg, lr_dev, alpha: float = 0.99, eps: float = 1e-8, weight_decay: float = 0.0, momentum: float = 0.0,
               momentum_buf=None, grad_avg=None, max_norm: Optional[float] = None, workspace=None, norm_out=None):
    """RMSpropTFLike (square_avg starts at ones, epsilon inside the square root) over one flat arena. momentum_buf iff momentum > 0,
    grad_avg iff the centred form. The clip is hip_ops.rmsprop's: max_norm > 0 folds clip_grad_norm_ in (two launches, the clipped
    gradient is written back); None or <= 0: one launch, the gradient is only read."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (square_avg, "square_avg")):
        _chk(t, nm, (n,), th.float32)
    _opt(momentum_buf, "momentum_buf", (n,), th.float32), _opt(grad_avg, "grad_avg", (n,), th.float32)
    if (momentum_buf is not None) != (momentum > 0):
        raise ValueError("rmsprop_tf: momentum_buf goes with momentum > 0")
    _chk(lr_dev, "lr", (1,), th.float64)
    clip = max_norm is not None and max_norm > 0
    if clip:
        _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
        if norm_out is not None:
            _vec(norm_out, "norm_out", 1)
    check(nv.lib().cstr_rmsprop_tf_f32(ptr(param), ptr(grad), ptr(square_avg), ptr(momentum_buf), ptr(grad_avg), ptr(lr_dev), C.c_double(alpha),
                                       C.c_double(eps), C.c_double(weight_decay), C.c_double(momentum), C.c_float(max_norm if clip else 0.0),
                                       ptr(workspace if clip else None), ptr(norm_out if clip else None), C.c_int64(n), stream_ptr()),
          "cstr_rmsprop_tf_f32")


# ---- DQN on the discrete valve face: exploration draw, action selection, target + gather + Huber loss (csrc/cstr_dqn.hip) -----------
def dqn_supported(n_actions: int, levels: int) -> bool:
    return 2 <= levels <= nv.DQN_MAX_LEVELS and n_actions == levels * levels


def mt19937_rand_flag(mt_state, threshold, flag_out, draw_out=None):
    """flag_out[0] = (one RandomState.random_sample() from the device legacy stream) < threshold[0]; threshold a device double,
    flag_out a device int32, draw_out (optional, device double) keeps the draw. `np.random.rand() < exploration_rate`."""
    _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32), _chk(threshold, "threshold", (1,), th.float64)
    _chk(flag_out, "flag_out", (1,), th.int32), _opt(draw_out, "draw_out", (1,), th.float64)
    check(nv.lib().cstr_mt19937_rand_flag_f64(ptr(mt_state), ptr(threshold), ptr(flag_out), ptr(draw_out), stream_ptr()),
          "cstr_mt19937_rand_flag_f64")


DQN_GREEDY, DQN_ALL_OR_NONE, DQN_PER_ROW = 0, 1, 2


def dqn_act(q, levels: int, mode: int, valve_out, index_out=None, eps=None, flag=None, u=None, rng_ctl=None):
    """Action selection over q [n, levels^2] (rows may be strided): mode DQN_GREEDY = first maximum; DQN_ALL_OR_NONE = every row a
    uniform random index iff flag[0] != 0 (the reference's one draw per vec-step); DQN_PER_ROW = row r explores iff u[r, 0] < eps[0].
    Uniforms are read from `u` [n, 2] when given, drawn from the Philox stream `rng_ctl` otherwise. valve_out [n, 2] receives the
    normalised valve pair of the index, index_out (optional, int64 [n]) the index."""
    n, m = q.shape
    ldq = _rows(q, "q", n, m)
    _chk(valve_out, "valve_out", (n, 2), th.float32), _opt(index_out, "index_out", (n,), th.int64)
    _opt(eps, "eps", (1,), th.float64), _opt(flag, "flag", (1,), th.int32), _opt(u, "u", (n, 2), th.float32)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_dqn_act_f32(ptr(q), C.c_int64(ldq), C.c_int64(n), C.c_int(m), C.c_int(levels), C.c_int(mode), ptr(eps), ptr(flag),
                                    ptr(u), ptr(rng_ctl), ptr(valve_out), ptr(index_out), stream_ptr()), "cstr_dqn_act_f32")


def dqn_loss(q, next_q, valve, reward, done, gamma: float, levels: int, g_q, loss_out, workspace, loss_sum=None, cur_q_out=None,
             target_out=None):
    """dqn.py:195-212 in one launch: target = reward + ((1 - done) * f32(gamma)) * max next_q, cur = q[b, index(valve[b])], loss_out =
    mean Huber loss (beta 1), g_q = d loss / d q (q's shape and row stride). c_float rounds gamma."""
    b, m = q.shape
    ldq = _rows(q, "q", b, m)
    ldn = _rows(next_q, "next_q", b, m)
    if _rows(g_q, "g_q", b, m) != ldq:
        raise ValueError("g_q must have q's row stride")
    _chk(valve, "valve", (b, 2), th.float32)
    for t, nm in ((reward, "reward"), (done, "done")):
        _vec(t, nm, b)
    _vec(loss_out, "loss_out", 1), _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
    if loss_sum is not None:
        _vec(loss_sum, "loss_sum", 1)
    for t, nm in ((cur_q_out, "cur_q_out"), (target_out, "target_out")):
        if t is not None:
            _vec(t, nm, b)
    check(nv.lib().cstr_dqn_loss_f32(ptr(q), C.c_int64(ldq), ptr(next_q), C.c_int64(ldn), ptr(valve), ptr(reward), ptr(done), C.c_float(gamma),
                                     C.c_int64(b), C.c_int(m), C.c_int(levels), ptr(g_q), ptr(loss_out), ptr(loss_sum), ptr(cur_q_out),
                                     ptr(target_out), ptr(workspace), stream_ptr()), "cstr_dqn_loss_f32")


# ---- QR-DQN on the discrete valve face: folded head, greedy target + gathers + quantile-Huber loss (csrc/cstr_qrdqn.hip) ------------
def qrdqn_supported(n_actions: int, levels: int, n_quantiles: int) -> bool:
    """cstr_qrdqn_supported: DQN's face and 1 <= n_quantiles <= QRDQN_MAX_QUANTILES."""
    return bool(nv.lib().cstr_qrdqn_supported(C.c_int(int(n_actions)), C.c_int(int(levels)), C.c_int(int(n_quantiles))))


def qrdqn_fold_head(weight, bias, n_actions: int, w_mean, b_mean):
    """The quantile network's last layer folded over its atoms (cstr_qrdqn_fold_head_f32): weight [Nq * M, H], bias [Nq * M], row
    i * M + a = atom i of action a; w_mean [M, H] = mean_i weight[i * M + a], b_mean [M] = mean_i bias[i * M + a] (float64 sums, i
    ascending). The mean of the atoms is the folded layer applied to the same hidden activations."""
    m = int(n_actions)
    if not (isinstance(weight, th.Tensor) and weight.dim() == 2 and m >= 1 and weight.shape[0] >= m and weight.shape[0] % m == 0):
        raise ValueError(f"weight: needs a [n_quantiles * {m}, H] matrix")
    rows, h = weight.shape
    _chk(weight, "weight", (rows, h), th.float32), _chk(bias, "bias", (rows,), th.float32)
    _chk(w_mean, "w_mean", (m, h), th.float32), _chk(b_mean, "b_mean", (m,), th.float32)
    check(nv.lib().cstr_qrdqn_fold_head_f32(ptr(weight), ptr(bias), C.c_int(m), C.c_int(rows // m), C.c_int64(h), ptr(w_mean), ptr(b_mean),
                                            stream_ptr()), "cstr_qrdqn_fold_head_f32")


def qrdqn_loss(z, z_next, valve, reward, done, gamma: float, levels: int, n_quantiles: int, gz, ws, loss_out=None, loss_sum=None, cur_out=None,
               target_out=None, next_index_out=None):
    """QR-DQN's loss as a backward root (cstr_qrdqn_loss_f32): z / z_next [B, Nq * M] (rows may be strided) = the online network's atoms
    at s / the target network's at s', atom i of action a at i * M + a. Greedy a* over the atom means of z_next, y_j = reward +
    (1 - done) gamma z_next[b, j, a*] (target_out [B, Nq]), the taken action's atoms (cur_out [B, Nq]) from the stored valve pair,
    loss_out = the pairwise quantile-Huber loss summed over the current quantile and averaged over batch and target quantile, gz =
    d loss / d z (z's shape and row stride, zeros off the taken action). next_index_out int64 [B] = a*. ws: float64 [B] scratch."""
    b, nm = z.shape
    nq, k = int(n_quantiles), int(levels)
    if nq < 1 or nm != nq * k * k:
        raise ValueError(f"z: {nm} columns are not n_quantiles * levels^2 = {nq} * {k * k}")
    ldz = _rows(z, "z", b, nm)
    ldn = _rows(z_next, "z_next", b, nm)
    if _rows(gz, "gz", b, nm) != ldz:
        raise ValueError("gz must have z's row stride")
    _chk(valve, "valve", (b, 2), th.float32)
    for t, nm_ in ((reward, "reward"), (done, "done")):
        _vec(t, nm_, b)
    _chk(ws, "ws", (b,), th.float64)
    for t, nm_, n in ((loss_out, "loss_out", 1), (loss_sum, "loss_sum", 1), (cur_out, "cur_out", b * nq), (target_out, "target_out", b * nq)):
        if t is not None:
            _vec(t, nm_, n)
    _opt(next_index_out, "next_index_out", (b,), th.int64)
    check(nv.lib().cstr_qrdqn_loss_f32(ptr(z), C.c_int64(ldz), ptr(z_next), C.c_int64(ldn), ptr(valve), ptr(reward), ptr(done), C.c_double(gamma),
                                       C.c_int64(b), C.c_int(k * k), C.c_int(k), C.c_int(nq), ptr(gz), ptr(loss_out), ptr(loss_sum), ptr(cur_out),
                                       ptr(target_out), ptr(next_index_out), ptr(ws), stream_ptr()), "cstr_qrdqn_loss_f32")


# ---- Categorical head of PPO / A2C on the discrete valve face (csrc/cstr_categorical.hip) -------------------------------------------
def categorical_supported(obs_dim: int, n_actions: int, levels: int) -> bool:
    return obs_dim in (4, 8) and dqn_supported(n_actions, levels)


def categorical_act(logits, levels: int, index_f32, deterministic: bool = False, action_in=None, u=None, rng_ctl=None, index_out=None,
                    valve_out=None, log_prob=None, u_out=None):
    """The Categorical(logits) head over logits [n, levels^2] (rows may be strided) in one launch. The index comes from exactly one
    source: `deterministic` (first maximum of the logits), `action_in` (int64 [n], teacher-forced), `u` ([n] uniforms, inverse CDF) or
    the Philox stream `rng_ctl` (the uniform is drawn). index_f32 [n] (or [n, 1]) receives the index as a float; optional: index_out
    int64 [n], valve_out [n, 2] (the env's valve pair), log_prob [n], u_out [n] (the uniforms used)."""
    n, m = logits.shape
    ldz = _rows(logits, "logits", n, m)
    _vec(index_f32, "index_f32", n)
    _opt(action_in, "action_in", (n,), th.int64), _opt(u, "u", (n,), th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    _opt(index_out, "index_out", (n,), th.int64), _opt(valve_out, "valve_out", (n, 2), th.float32)
    _opt(log_prob, "log_prob", (n,), th.float32), _opt(u_out, "u_out", (n,), th.float32)
    check(nv.lib().cstr_categorical_act_f32(ptr(logits), C.c_int64(ldz), C.c_int64(n), C.c_int(m), C.c_int(levels),
                                            C.c_int(int(bool(deterministic))), ptr(action_in), ptr(u), ptr(rng_ctl), ptr(index_f32),
                                            ptr(index_out), ptr(valve_out), ptr(log_prob), ptr(u_out), stream_ptr()), "cstr_categorical_act_f32")


CAT_PPO, CAT_A2C = 0, 1


def _discrete_loss(struct, symbol: str, face, objective: int, logits, actions, values, adv, returns, normalize_advantage, ent_coef, vf_coef,
                   g_logits, g_value, workspace, old_values, old_log_prob, clip_range, clip_range_vf, scalars_out, scalars_sum, log_prob_out):
    """What categorical_loss and multicategorical_loss share: the two structs differ only in the face's two int32 fields (`face`) and
    in the shape of `actions`, which the caller has checked."""
    b, m = logits.shape
    ldz = _rows(logits, "logits", b, m)
    if _rows(g_logits, "g_logits", b, m) != ldz:
        raise ValueError("g_logits must have the logits' row stride")
    for t, nm in ((values, "values"), (adv, "adv"), (returns, "returns"), (g_value, "g_value")):
        _vec(t, nm, b)
    for t, nm in ((old_values, "old_values"), (old_log_prob, "old_log_prob"), (log_prob_out, "log_prob_out")):
        if t is not None:
            _vec(t, nm, b)
    n_scalars = 6 if objective == CAT_PPO else 4
    for t, nm in ((scalars_out, "scalars_out"), (scalars_sum, "scalars_sum")):
        if t is not None:
            _vec(t, nm, n_scalars)
    _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
    dp = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    p = struct(logits.data_ptr(), ldz, actions.data_ptr(), values.data_ptr(), dp(old_values), dp(old_log_prob), adv.data_ptr(),
               returns.data_ptr(), b, face[0], face[1], int(objective), int(bool(normalize_advantage)), float(clip_range),
               -1.0 if clip_range_vf is None else float(clip_range_vf), float(ent_coef), float(vf_coef), g_logits.data_ptr(),
               g_value.data_ptr(), dp(scalars_out), dp(scalars_sum), dp(log_prob_out))
    check(getattr(nv.lib(), symbol)(C.byref(p), ptr(workspace), stream_ptr()), symbol)


def categorical_loss(objective: int, logits, levels: int, actions, values, adv, returns, normalize_advantage: bool, ent_coef: float,
                     vf_coef: float, g_logits, g_value, workspace, old_values=None, old_log_prob=None, clip_range: float = 0.0,
                     clip_range_vf: Optional[float] = None, scalars_out=None, scalars_sum=None, log_prob_out=None):
    """ppo.py:213-264 (CAT_PPO: the six PPO_SCALARS) or a2c.py:150-171 (CAT_A2C: the four A2C_SCALARS) on a Categorical head in one
    launch: the scalars and d loss / d (logits, value). actions [b] or [b, 1]: the stored index as a float. g_logits has the logits'
    shape and row stride."""
    b, m = logits.shape
    _vec(actions, "actions", b)
    _discrete_loss(nv.CategoricalLoss, "cstr_categorical_loss_f32", (m, int(levels)), objective, logits, actions, values, adv,
                   returns, normalize_advantage, ent_coef, vf_coef, g_logits, g_value, workspace, old_values, old_log_prob, clip_range,
                   clip_range_vf, scalars_out, scalars_sum, log_prob_out)


# ---- MultiCategorical head of PPO / A2C on the MultiDiscrete valve face (csrc/cstr_multicategorical.hip) ---------------------------
def multicategorical_supported(obs_dim: int, nvec) -> bool:
    """two valves, 2 .. MCAT_MAX_LEVELS levels each"""
    return obs_dim in (4, 8) and len(nvec) == 2 and all(2 <= int(k) <= nv.MCAT_MAX_LEVELS for k in nvec)


def _levels_pair(nvec, m: int):
    if len(nvec) != 2 or int(nvec[0]) + int(nvec[1]) != m:
        raise ValueError(f"logits: {m} columns do not fit the level counts {tuple(nvec)} (two valves, K0 + K1 columns)")
    return int(nvec[0]), int(nvec[1])


def multicategorical_act(logits, nvec, action_f32, deterministic: bool = False, action_in=None, u=None, rng_ctl=None, action_out=None,
                         valve_out=None, log_prob=None, u_out=None):
    """The MultiCategorical head over logits [n, K0 + K1] (th.split order; rows may be strided) in one launch. The level pair comes
    from exactly one source: `deterministic` (first maximum of each valve's logits), `action_in` (int64 [n, 2], teacher-forced), `u`
    ([n, 2] uniforms, inverse CDF per valve) or the Philox stream `rng_ctl` (the uniforms are drawn). action_f32 [n, 2] receives the
    pair as floats; optional: action_out int64 [n, 2], valve_out [n, 2] (the env's valve pair), log_prob [n] (summed over the valves),
    u_out [n, 2] (the uniforms used)."""
    n, m = logits.shape
    k0, k1 = _levels_pair(nvec, m)
    ldz = _rows(logits, "logits", n, m)
    _chk(action_f32, "action_f32", (n, 2), th.float32)
    _opt(action_in, "action_in", (n, 2), th.int64), _opt(u, "u", (n, 2), th.float32), _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    _opt(action_out, "action_out", (n, 2), th.int64), _opt(valve_out, "valve_out", (n, 2), th.float32)
    _opt(log_prob, "log_prob", (n,), th.float32), _opt(u_out, "u_out", (n, 2), th.float32)
    check(nv.lib().cstr_multicategorical_act_f32(ptr(logits), C.c_int64(ldz), C.c_int64(n), C.c_int(k0), C.c_int(k1),
                                                 C.c_int(int(bool(deterministic))), ptr(action_in), ptr(u), ptr(rng_ctl), ptr(action_f32),
                                                 ptr(action_out), ptr(valve_out), ptr(log_prob), ptr(u_out), stream_ptr()),
          "cstr_multicategorical_act_f32")


def multicategorical_loss(objective: int, logits, nvec, actions, values, adv, returns, normalize_advantage: bool, ent_coef: float,
                          vf_coef: float, g_logits, g_value, workspace, old_values=None, old_log_prob=None, clip_range: float = 0.0,
                          clip_range_vf: Optional[float] = None, scalars_out=None, scalars_sum=None, log_prob_out=None):
    """categorical_loss on a MultiCategorical head (CAT_PPO: the six PPO_SCALARS, CAT_A2C: the four A2C_SCALARS) in one launch: the
    scalars and d loss / d (logits, value). actions [b, 2]: the stored level pair as floats. g_logits has the logits' shape and row
    stride."""
    b, m = logits.shape
    face = _levels_pair(nvec, m)
    _chk(actions, "actions", (b, 2), th.float32)
    _discrete_loss(nv.MultiCategoricalLoss, "cstr_multicategorical_loss_f32", face, objective, logits, actions, values, adv, returns,
                   normalize_advantage, ent_coef, vf_coef, g_logits, g_value, workspace, old_values, old_log_prob, clip_range, clip_range_vf,
                   scalars_out, scalars_sum, log_prob_out)


# ---- HER: the goal face of the env and the device HerReplayBuffer (csrc/cstr_her.hip) ---------------------------------------------
GOAL_ROW = 6  # flat row [achieved_goal | desired_goal | observation]


class DeviceHer:
    """cstr_her_t over torch tensors (HBM), beside a (4, 2) DeviceRing: desired_goal / ep_start / ep_length [rows, n_envs],
    cur_ep_start [n_envs] (her_replay_buffer.py:97-99) and the two summaries of `ep_length > 0` the sampler reads."""

    def __init__(self, ring: DeviceRing, device):
        if (ring.obs_dim, ring.act_dim) != (4, 2):
            raise ValueError(f"the HER ring is the (4, 2) layout, got {(ring.obs_dim, ring.act_dim)}")
        if ring.rows > nv.HER_MAX_ROWS or ring.n_envs > nv.HER_MAX_ENVS:
            raise ValueError(f"the HER ring holds at most {nv.HER_MAX_ROWS} rows of {nv.HER_MAX_ENVS} envs, got {ring.rows} x {ring.n_envs}")
        rows, n = ring.rows, ring.n_envs
        zi = lambda *s: th.zeros(*s, dtype=th.int32, device=device)  # noqa: E731
        self.desired_goal = th.zeros(rows, n, dtype=th.float32, device=device)
        self.ep_start, self.ep_length, self.cur_ep_start = zi(rows, n), zi(rows, n), zi(n)
        self.row_valid = zi(rows)
        self.words = (n + 63) // 64
        self.valid_bits = th.zeros(rows, self.words, dtype=th.int64, device=device)
        self.status = zi(1)
        self.c = nv.Her(self.desired_goal.data_ptr(), self.ep_start.data_ptr(), self.ep_length.data_ptr(), self.cur_ep_start.data_ptr(),
                        self.row_valid.data_ptr(), self.valid_bits.data_ptr())

    def rebuild_summaries(self) -> None:
        """row_valid / valid_bits from ep_length (after the host wrote ep_length: unpickling, truncate_last_trajectory)."""
        valid = self.ep_length > 0
        self.row_valid.copy_(valid.sum(dim=1).to(th.int32))
        pad = self.words * 64 - valid.shape[1]
        v = th.nn.functional.pad(valid, (0, pad)).reshape(valid.shape[0], self.words, 64).to(th.int64)
        self.valid_bits.copy_((v << th.arange(64, device=v.device, dtype=th.int64)).sum(dim=2))


def goal_vec_step(coef, integrator: str, env_obs, act, step_count, pcg_state, target, next_rows, rows_after, reward, done, timeout,
                  static_init=None, episode=None, goal_seed: int = 0, goal_index_offset: int = 0, goal_lo: float = 0.0, goal_hi: float = 0.0):
    """VecEnv.step on the goal face (cstr_goal_vec_step_f32); `episode` None = targets stay as they are."""
    n = env_obs.shape[0]
    _chk(env_obs, "env_obs", (n, 4), th.float32), _chk(act, "act", (n, 2), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64), _opt(static_init, "static_init", (n, 4), th.float64)
    _chk(target, "target", (n,), th.float32), _opt(episode, "episode", (n,), th.int32)
    _chk(next_rows, "next_rows", (n, GOAL_ROW), th.float32), _chk(rows_after, "rows_after", (n, GOAL_ROW), th.float32)
    for t, nm in ((reward, "reward"), (done, "done"), (timeout, "timeout")):
        _chk(t, nm, (n,), th.float32)
    check(nv.lib().cstr_goal_vec_step_f32(C.byref(coef), C.c_int(INTEGRATORS[integrator]), C.c_int(4), ptr(env_obs), ptr(act), ptr(step_count),
                                          ptr(pcg_state), ptr(static_init), ptr(target), ptr(episode), C.c_uint64(int(goal_seed) & (2**64 - 1)),
                                          C.c_int64(int(goal_index_offset)), C.c_float(goal_lo), C.c_float(goal_hi), ptr(next_rows),
                                          ptr(rows_after), ptr(reward), ptr(done), ptr(timeout), C.c_int64(n), stream_ptr()),
          "cstr_goal_vec_step_f32")


def her_add(ring: DeviceRing, her: DeviceHer, obs_rows, next_rows, act, rew, done, timeout):
    """HerReplayBuffer.add at the device-resident ring position (cstr_her_add_f32)."""
    n = ring.n_envs
    _chk(obs_rows, "obs_rows", (n, GOAL_ROW), th.float32), _chk(next_rows, "next_rows", (n, GOAL_ROW), th.float32)
    _chk(act, "act", (n, 2), th.float32)
    for t, nm in ((rew, "rew"), (done, "done"), (timeout, "timeout")):
        _chk(t, nm, (n,), th.float32)
    check(nv.lib().cstr_her_add_f32(C.byref(ring.c), C.byref(her.c), ptr(ring.ctl), ptr(obs_rows), ptr(next_rows), ptr(act), ptr(rew), ptr(done),
                                    ptr(timeout), stream_ptr()), "cstr_her_add_f32")


def goal_collect_step(coef, integrator: str, ring: DeviceRing, her: DeviceHer, env_obs, rows, step_count, pcg_state, target, policy_out, squashed,
                      act_low, act_high, noise=None, static_init=None, episode=None, goal_seed: int = 0, goal_index_offset: int = 0,
                      goal_lo: float = 0.0, goal_hi: float = 0.0, reward_out=None, done_out=None, timeout_out=None, next_rows_out=None,
                      ep_return=None, ep_stats=None, rng_advance=None):
    """The rollout's vec-step on the goal face in one launch (cstr_goal_collect_step_f32): the action scaling chain on `policy_out`,
    `goal_vec_step` on the env's own arrays (`rows` = the env's flat rows, read as the transition's observation and then overwritten),
    `her_add` at the device-resident ring position and Monitor's episode statistics. `rng_advance` as in `collect_step`."""
    n = ring.n_envs
    _chk(env_obs, "env_obs", (n, 4), th.float32), _chk(rows, "rows", (n, GOAL_ROW), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64), _opt(static_init, "static_init", (n, 4), th.float64)
    _chk(target, "target", (n,), th.float32), _opt(episode, "episode", (n,), th.int32)
    _chk(policy_out, "policy_out", (n, 2), th.float32), _opt(noise, "noise", (n, 2), th.float32)
    for t, nm in ((reward_out, "reward_out"), (done_out, "done_out"), (timeout_out, "timeout_out"), (ep_return, "ep_return")):
        _opt(t, nm, (n,), th.float32)
    _opt(next_rows_out, "next_rows_out", (n, GOAL_ROW), th.float32), _opt(ep_stats, "ep_stats", (4,), th.float64)
    if (ep_return is None) != (ep_stats is None):
        raise ValueError("ep_return and ep_stats go together")
    if len(act_low) != 2 or len(act_high) != 2:
        raise ValueError("act_low/act_high need 2 entries")
    lo = (C.c_float * 2)(*[float(v) for v in act_low])
    hi = (C.c_float * 2)(*[float(v) for v in act_high])
    rng_ctl, rng_count = rng_advance if rng_advance is not None else (None, 0)
    _opt(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_goal_collect_step_f32(C.byref(coef), C.c_int(INTEGRATORS[integrator]), C.c_int(4), C.byref(ring.c), C.byref(her.c),
                                              ptr(ring.ctl), ptr(env_obs), ptr(rows), ptr(step_count), ptr(pcg_state), ptr(static_init),
                                              ptr(target), ptr(episode), C.c_uint64(int(goal_seed) & (2**64 - 1)),
                                              C.c_int64(int(goal_index_offset)), C.c_float(goal_lo), C.c_float(goal_hi), ptr(policy_out),
                                              C.c_int(int(squashed)), lo, hi, ptr(noise), ptr(reward_out), ptr(done_out), ptr(timeout_out),
                                              ptr(next_rows_out), ptr(ep_return), ptr(ep_stats), ptr(rng_ctl), C.c_uint64(int(rng_count)),
                                              stream_ptr()), "cstr_goal_collect_step_f32")


def her_sample(coef, ring: DeviceRing, her: DeviceHer, mt_state, batch: int, nb_virtual: int, strategy: str, out_obs, out_act, out_next_obs,
               out_done, out_rew, out_row_idx=None, out_env_idx=None, out_goal_row=None, forced_row=None, forced_env=None, forced_goal=None):
    """HerReplayBuffer.sample in one launch (cstr_her_sample_f32); her.status[0] tells afterwards whether anything was valid."""
    if strategy not in nv.HER_STRATEGIES:
        raise ValueError(f"strategy must be one of {list(nv.HER_STRATEGIES)}, got {strategy!r}")
    if not 0 < batch <= nv.HER_MAX_BATCH:
        raise ValueError(f"batch_size must be in [1, {nv.HER_MAX_BATCH}], got {batch}")
    if not 0 <= nb_virtual <= batch:
        raise ValueError(f"nb_virtual must be in [0, {batch}], got {nb_virtual}")
    _chk(mt_state, "mt_state", (nv.MT_STATE_WORDS,), th.int32)
    _chk(out_obs, "out_obs", (batch, GOAL_ROW), th.float32), _chk(out_next_obs, "out_next_obs", (batch, GOAL_ROW), th.float32)
    _chk(out_act, "out_act", (batch, 2), th.float32)
    _chk(out_done, "out_done", (batch, 1), th.float32), _chk(out_rew, "out_rew", (batch, 1), th.float32)
    for t, nm in ((out_row_idx, "out_row_idx"), (out_env_idx, "out_env_idx"), (out_goal_row, "out_goal_row"), (forced_row, "forced_row"),
                  (forced_env, "forced_env"), (forced_goal, "forced_goal")):
        _opt(t, nm, (batch,), th.int64)
    if (forced_row is None) != (forced_env is None) or (forced_goal is not None and forced_row is None):
        raise ValueError("forced_row and forced_env go together; forced_goal needs them")
    check(nv.lib().cstr_her_sample_f32(C.byref(coef), C.byref(ring.c), C.byref(her.c), ptr(mt_state), C.c_int64(batch), C.c_int64(nb_virtual),
                                       C.c_int(nv.HER_STRATEGIES[strategy]), ptr(forced_row), ptr(forced_env), ptr(forced_goal), ptr(out_obs),
                                       ptr(out_act), ptr(out_next_obs), ptr(out_done), ptr(out_rew), ptr(out_row_idx), ptr(out_env_idx),
                                       ptr(out_goal_row), ptr(her.status), stream_ptr()), "cstr_her_sample_f32")


def goal_eval_episodes_supported(h1: int, h2: int, n_out: int, head: int) -> bool:
    """cstr_eval_goal_episodes_f32 takes the network shapes of cstr_policy_rows_fwd_f32 on the goal face's flat rows (k0 = 6, two valves)."""
    lds = 4 * (16 * (16 * -(-h1 // 16) + 4 + 16 * -(-h2 // 16) + 4) + 8 * 16 * 8 + 2 * 16 * 8)
    return head in (0, 1) and n_out == (4 if head == 0 else 2) and policy_rows_supported(GOAL_ROW, h1, h2, n_out) and lds <= EVAL_LDS_BYTES


def goal_eval_episodes(w1, b1, w2, b2, w3, b3, act: int, head: int, out_act: int, w2_swz, coef, integrator: str, env_obs, step_count, pcg_state,
                       target, squashed: bool, act_low, act_high, targets, max_vec_steps: int, static_init=None, episode=None, goal_seed: int = 0,
                       goal_index_offset: int = 0, goal_lo: float = 0.0, goal_hi: float = 0.0, tracking: bool = False):
    """Whole evaluation episodes on the goal face in ONE launch (cstr_eval_goal_episodes_f32): `eval_episodes` with the network on the
    flat rows [achieved | desired | observation] (w1 [h1, 6]), the goal reward on the env's own setpoint `target` [N] and, when `episode`
    [N] int32 is given, the setpoint redraw of `goal_vec_step` at every episode end. The launch advances env_obs / step_count / pcg_state /
    target / episode. Returns (ep_return, ep_len, ep_done) like `eval_episodes`; with `tracking` also (ep_goal float32, ep_gap float32,
    ep_abs_gap float64), each [N, max(targets)]: the episode's desired goal, achieved - desired of its terminal row and the f64 sum of
    |achieved - desired| over its steps. Raises RuntimeError if `max_vec_steps` ended the launch before every env had met its target."""
    import numpy as np

    n = env_obs.shape[0]
    h1, h2, n_out = w1.shape[0], w2.shape[0], w3.shape[0]
    if n_out != (4 if head == 0 else 2):
        raise ValueError(f"the goal face has two valves: w3 needs {4 if head == 0 else 2} rows for head {head}, got {n_out}")
    _chk(env_obs, "env_obs", (n, 4), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64), _opt(static_init, "static_init", (n, 4), th.float64)
    _chk(target, "target", (n,), th.float32), _opt(episode, "episode", (n,), th.int32)
    _chk(w1, "w1", (h1, GOAL_ROW), th.float32), _chk(b1, "b1", (h1,), th.float32), _chk(w2, "w2", (h2, h1), th.float32)
    _chk(b2, "b2", (h2,), th.float32), _chk(w3, "w3", (n_out, h2), th.float32), _chk(b3, "b3", (n_out,), th.float32)
    if w2_swz is not None:
        _chk(w2_swz, "w2_swz", (swizzled_numel(h2, h1),), th.float32)
    if len(act_low) != 2 or len(act_high) != 2:
        raise ValueError("act_low/act_high need 2 entries")
    tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int32))
    if tg.shape != (n,):
        raise ValueError(f"targets: shape {tg.shape}, expected {(n,)}")
    if tg.min() < 0:
        raise ValueError("targets must be non-negative")
    stride, dev = int(tg.max()), env_obs.device
    ep_return = th.zeros(n, stride, dtype=th.float64, device=dev)
    ep_len = th.zeros(n, stride, dtype=th.int32, device=dev)
    ep_done = th.zeros(n, dtype=th.int32, device=dev)
    track = (th.zeros(n, stride, dtype=th.float32, device=dev), th.zeros(n, stride, dtype=th.float32, device=dev),
             th.zeros(n, stride, dtype=th.float64, device=dev)) if tracking else (None, None, None)
    goal_eval_episodes_into(w1, b1, w2, b2, w3, b3, act, head, out_act, w2_swz, coef, integrator, env_obs, step_count, pcg_state, target, squashed,
                            act_low, act_high, tg, max_vec_steps, ep_return, ep_len, ep_done, *track, static_init=static_init, episode=episode,
                            goal_seed=goal_seed, goal_index_offset=goal_index_offset, goal_lo=goal_lo, goal_hi=goal_hi)
    short = (ep_done.cpu().numpy() < tg).nonzero()[0]  # the one read-back this wrapper does: a run cut short must not pass for a result
    if short.size:
        raise RuntimeError(f"cstr_eval_goal_episodes_f32: max_vec_steps={int(max_vec_steps)} ended the launch before envs {short.tolist()} had "
                           f"run their episodes (counted {ep_done.cpu().numpy()[short].tolist()}, wanted {tg[short].tolist()})")
    return (ep_return, ep_len, ep_done) + (track if tracking else ())


def goal_eval_episodes_into(w1, b1, w2, b2, w3, b3, act, head, out_act, w2_swz, coef, integrator, env_obs, step_count, pcg_state, target, squashed,
                            act_low, act_high, targets, max_vec_steps, ep_return, ep_len, ep_done, ep_goal=None, ep_gap=None, ep_abs_gap=None,
                            static_init=None, episode=None, goal_seed: int = 0, goal_index_offset: int = 0, goal_lo: float = 0.0,
                            goal_hi: float = 0.0):
    """`goal_eval_episodes` into caller-owned result buffers; nothing is checked beyond what the entry point itself checks. `targets`: a
    contiguous int32 NumPy array that the CALLER keeps alive and unmodified until the stream has passed the launch (see
    `eval_episodes_into`)."""
    n = env_obs.shape[0]
    lo = (C.c_float * 2)(*[float(v) for v in act_low])
    hi = (C.c_float * 2)(*[float(v) for v in act_high])
    net = nv.PolicyMlp(GOAL_ROW, w1.shape[0], w2.shape[0], 2, act, head, out_act, 0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                       w3.data_ptr(), b3.data_ptr(), None if w2_swz is None else w2_swz.data_ptr())
    check(nv.lib().cstr_eval_goal_episodes_f32(C.byref(net), C.byref(coef), C.c_int(INTEGRATORS[integrator]), ptr(env_obs), ptr(step_count),
                                               ptr(pcg_state), ptr(static_init), ptr(target), ptr(episode),
                                               C.c_uint64(int(goal_seed) & (2**64 - 1)), C.c_int64(int(goal_index_offset)), C.c_float(goal_lo),
                                               C.c_float(goal_hi), C.c_int(1 if squashed else 0), lo, hi, targets.ctypes.data_as(C.c_void_p),
                                               C.c_int64(n), C.c_int64(int(max_vec_steps)), ptr(ep_return), ptr(ep_len), ptr(ep_done),
                                               ptr(ep_goal), ptr(ep_gap), ptr(ep_abs_gap), stream_ptr()), "cstr_eval_goal_episodes_f32")


# ---- Augmented Random Search (csrc/cstr_ars.hip) -----------------------------------------------------------------------------------

ARS_STATS_WORDS = 4  # {sum of lengths, sum of returns, NaN returns, the launch's ticket (zero between launches)}


def ars_n_params(obs_dim: int, act_dim: int, hidden, with_bias: bool) -> int:
    """parameters of create_mlp(obs_dim, act_dim, hidden, with_bias=with_bias): the length of `theta`"""
    dims, b = [obs_dim, *hidden, act_dim], 1 if with_bias else 0
    return sum(o * (i + b) for i, o in zip(dims[:-1], dims[1:]))


def ars_supported(obs_dim: int, act_dim: int, hidden, act: int, with_bias: bool, squash: bool, n_delta: int, n_top: int) -> bool:
    """cstr_ars_supported: host only. `hidden`: the hidden widths (0, 1 or 2 of them, each 1..64); act: ACT["relu"] / ACT["tanh"]."""
    hidden = [int(h) for h in hidden]
    if len(hidden) > 2:
        return False
    h1, h2 = (hidden + [0, 0])[:2]
    return bool(nv.lib().cstr_ars_supported(C.c_int(obs_dim), C.c_int(act_dim), C.c_int(len(hidden)), C.c_int(h1), C.c_int(h2), C.c_int(int(act)),
                                            C.c_int(1 if with_bias else 0), C.c_int(1 if squash else 0), C.c_int(int(n_delta)), C.c_int(int(n_top))))


def _ars_policy(obs_dim: int, act_dim: int, hidden, act: int, with_bias: bool, squash: bool) -> "nv.ArsPolicy":
    hidden = [int(h) for h in hidden]
    if len(hidden) > 2:
        raise ValueError(f"ARS kernels take 0, 1 or 2 hidden layers, got {hidden}")
    h1, h2 = (hidden + [0, 0])[:2]
    return nv.ArsPolicy(obs_dim, act_dim, len(hidden), h1, h2, int(act), 1 if with_bias else 0, 1 if squash else 0)


def ars_population(theta, hidden, act: int, with_bias: bool, squash: bool, delta_std: float, seed: int, update_index: int, n_delta: int,
                   n_eval_episodes: int, alive_bonus_offset: float, coef, integrator: str, env_obs, step_count, pcg_state, act_low, act_high,
                   returns, lengths, stats, static_init=None):
    """The population launch (cstr_ars_population_f32): the 2 n_delta candidates theta +- delta_std * delta_k of update `update_index`
    evaluated on the env arrays, candidate c on slot c % n_envs. Writes returns float64 [2 n_delta], lengths int32 [2 n_delta] and the
    statistics block stats float64 [ARS_STATS_WORDS] (word 3 must be zero on entry and is zero on exit); advances the env arrays."""
    n, d = env_obs.shape
    a = len(act_low)
    if (d, a) not in LAYOUTS:
        raise ValueError(f"(obs_dim, act_dim) = {(d, a)} is not a CSTR layout {LAYOUTS}")
    if len(act_high) != a:
        raise ValueError(f"act_low/act_high need {a} entries each")
    pol = _ars_policy(d, a, hidden, act, with_bias, squash)
    _chk(theta, "theta", (ars_n_params(d, a, hidden, with_bias),), th.float32)
    _chk(env_obs, "env_obs", (n, d), th.float32), _chk(step_count, "step_count", (n,), th.int32)
    _chk(pcg_state, "pcg_state", (n, nv.PCG_STATE_WORDS), th.int64)
    _opt(static_init, "static_init", (n, 8 if a == 4 else 4), th.float64)
    _chk(returns, "returns", (2 * n_delta,), th.float64), _chk(lengths, "lengths", (2 * n_delta,), th.int32)
    _chk(stats, "stats", (ARS_STATS_WORDS,), th.float64)
    lo = (C.c_float * a)(*[float(v) for v in act_low])
    hi = (C.c_float * a)(*[float(v) for v in act_high])
    check(nv.lib().cstr_ars_population_f32(C.byref(pol), ptr(theta), C.c_float(delta_std), C.c_uint64(int(seed) & (2**64 - 1)),
                                           C.c_int64(int(update_index)), C.c_int(int(n_delta)), C.c_int(int(n_eval_episodes)),
                                           C.c_double(float(alive_bonus_offset)), C.byref(coef), C.c_int(INTEGRATORS[integrator]), ptr(env_obs),
                                           ptr(step_count), ptr(pcg_state), ptr(static_init), lo, hi, C.c_int64(n), ptr(returns), ptr(lengths),
                                           ptr(stats), stream_ptr()), "cstr_ars_population_f32")


def ars_update(theta, returns, n_delta: int, n_top: int, learning_rate: float, seed: int, update_index: int, out, kept):
    """The update launch (cstr_ars_update_f32): ranking, return_std, step_size and theta += step_size * sum (R+ - R-) delta in place.
    out float64 [2] = {step_size, return_std}; kept int32 [n_top] = the kept directions in rank order."""
    _chk(theta, "theta", (theta.numel(),), th.float32), _chk(returns, "returns", (2 * n_delta,), th.float64)
    _chk(out, "out", (2,), th.float64), _chk(kept, "kept", (n_top,), th.int32)
    check(nv.lib().cstr_ars_update_f32(ptr(theta), C.c_int64(theta.numel()), ptr(returns), C.c_int(int(n_delta)), C.c_int(int(n_top)),
                                       C.c_double(float(learning_rate)), C.c_uint64(int(seed) & (2**64 - 1)), C.c_int64(int(update_index)),
                                       ptr(out), ptr(kept), stream_ptr()), "cstr_ars_update_f32")


# ---- TRPO: tangent layers, the objective / line-search launch, the Fisher head, conjugate gradient (csrc/cstr_trpo.hip) ----------------
def trpo_head(head: int, k0: int, k1: int = 0):
    """(width of the distribution parameters, floats per stored action row) of a TRPO head; raises for a head the kernels decline"""
    if head == nv.TRPO_HEAD_GAUSSIAN and k0 in (2, 4):
        return k0, k0
    if head == nv.TRPO_HEAD_CATEGORICAL and 2 <= k0 <= nv.TRPO_MAX_LOGITS:
        return k0, 1
    if head == nv.TRPO_HEAD_MULTICATEGORICAL and 2 <= k0 <= 32 and 2 <= k1 <= 32:
        return k0 + k1, 2
    raise ValueError(f"TRPO head {head} with widths ({k0}, {k1}) is not built")


def trpo_supported(head: int, k0: int, k1: int = 0) -> bool:
    try:
        trpo_head(head, k0, k1)
        return True
    except ValueError:
        return False


def new_trpo_ctl(device) -> th.Tensor:
    """double[CSTR_TRPO_CTL_WORDS]: the conjugate gradient's and the line search's scalars (nv.TRPO_CTL names the words)"""
    return th.zeros(nv.TRPO_CTL_WORDS, dtype=th.float64, device=device)


def linear_tangent_fwd(x, x_dot, weight, w_dot, b_dot, y, act: int, out=None):
    """z_dot = f'(y) * (x @ w_dot^T + x_dot @ weight^T + b_dot): the tangent of one Linear + activation layer in one launch. x [M, K]
    (rows may be strided), x_dot the same or None (the first layer), weight / w_dot [N, K], b_dot [N], y [M, N] the layer's stored
    output (needed with an activation)."""
    m, k = x.shape
    n = weight.shape[0]
    ldx = max(_rows(x, "x", m, k), k)
    ldxd = 0 if x_dot is None else max(_rows(x_dot, "x_dot", m, k), k)
    _chk(weight, "weight", (n, k), th.float32), _chk(w_dot, "w_dot", (n, k), th.float32), _vec(b_dot, "b_dot", n)
    if act != 0:
        _chk(y, "y", (m, n), th.float32)
    z = th.empty(m, n, dtype=th.float32, device=x.device) if out is None else _chk(out, "out", (m, n), th.float32)
    check(nv.lib().cstr_linear_tangent_fwd_f32(ptr(x), C.c_int64(ldx), ptr(x_dot), C.c_int64(ldxd), ptr(weight), ptr(w_dot), ptr(b_dot),
                                               ptr(y if act != 0 else None), C.c_int(act), ptr(z), C.c_int64(m), C.c_int64(n), C.c_int64(k),
                                               stream_ptr()), "cstr_linear_tangent_fwd_f32")
    return z


def trpo_objective(head: int, k0: int, k1: int, dist, log_std, old_dist, old_log_std, actions, old_log_prob, adv, normalize_advantage: bool,
                   ctl, workspace, g_dist=None, g_log_std=None, scalars_out=None, accepted=None, target_kl: float = 0.0,
                   shrink: float = 0.0):
    """The objective launch. Gradient mode (accepted None): objective, kl and d objective / d (dist, log_std) into g_dist [R, width] and
    g_log_std [k0]; ctl's objective / kl / coeff words are set. Line-search mode (accepted int32 [1]): the decision against ctl's base
    objective and target_kl, the coefficient shrunk by `shrink` on a rejection. dist / old_dist [R, width] (rows may be strided)."""
    width, aw = trpo_head(head, k0, k1)
    b = dist.shape[0]
    ld, old_ld = _rows(dist, "dist", b, width), _rows(old_dist, "old_dist", b, width)
    gauss = head == nv.TRPO_HEAD_GAUSSIAN
    if gauss:
        _vec(log_std, "log_std", width), _vec(old_log_std, "old_log_std", width)
    _vec(actions, "actions", b * aw)
    for t, nm in ((old_log_prob, "old_log_prob"), (adv, "adv")):
        _vec(t, nm, b)
    _chk(ctl, "ctl", (nv.TRPO_CTL_WORDS,), th.float64), _chk(workspace, "workspace", (nv.PPO_WS_WORDS,), th.int64)
    line_search = accepted is not None
    if line_search:
        _chk(accepted, "accepted", (1,), th.int32)
    else:
        _chk(g_dist, "g_dist", (b, width), th.float32)
        if gauss:
            _vec(g_log_std, "g_log_std", width)
    if scalars_out is not None:
        _vec(scalars_out, "scalars_out", 2)
    dp = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    p = nv.TrpoObjective(dist.data_ptr(), ld, dp(log_std) if gauss else None, old_dist.data_ptr(), old_ld, dp(old_log_std) if gauss else None,
                         actions.data_ptr(), old_log_prob.data_ptr(), adv.data_ptr(), b, int(head), int(k0), int(k1),
                         int(bool(normalize_advantage)), int(line_search), 0, float(target_kl), float(shrink), dp(g_dist),
                         dp(g_log_std) if gauss else None, dp(scalars_out), ctl.data_ptr(), dp(accepted))
    check(nv.lib().cstr_trpo_objective_f32(C.byref(p), ptr(workspace), stream_ptr()), "cstr_trpo_objective_f32")


def trpo_fisher_head(head: int, k0: int, k1: int, dist_dot, dist, log_std, v_log_std, upstream, g_log_std):
    """upstream [R, width] = (the head's Fisher metric) @ dist_dot / R; the Gaussian head also writes g_log_std = 2 v_log_std."""
    width, _ = trpo_head(head, k0, k1)
    b = dist_dot.shape[0]
    ldd = _rows(dist_dot, "dist_dot", b, width)
    gauss = head == nv.TRPO_HEAD_GAUSSIAN
    ld = 0
    if gauss:
        _vec(log_std, "log_std", width), _vec(v_log_std, "v_log_std", width), _vec(g_log_std, "g_log_std", width)
    else:
        ld = _rows(dist, "dist", b, width)
    _chk(upstream, "upstream", (b, width), th.float32)
    check(nv.lib().cstr_trpo_fisher_head_f32(C.c_int(head), C.c_int(k0), C.c_int(k1), ptr(dist_dot), C.c_int64(ldd), ptr(None if gauss else dist),
                                             C.c_int64(ld), ptr(log_std if gauss else None), ptr(v_log_std if gauss else None), C.c_int64(b),
                                             ptr(upstream), ptr(g_log_std if gauss else None), stream_ptr()), "cstr_trpo_fisher_head_f32")


def trpo_cg_step(mode: int, x, r, p, ap, g, damping: float, residual_tol: float, ctl, target_kl: float = 0.0, last: bool = False):
    """One conjugate-gradient launch over flat float32 vectors of one length (nv.TRPO_CG_INIT / _STEP / _FINISH); `ap` is the
    Fisher-vector product WITHOUT the damping term."""
    n = x.numel()
    _vec(x, "x", n), _vec(ap, "ap", n)
    for t, nm in ((r, "r"), (p, "p"), (g, "g")):
        if t is not None:
            _vec(t, nm, n)
    _chk(ctl, "ctl", (nv.TRPO_CTL_WORDS,), th.float64)
    check(nv.lib().cstr_trpo_cg_step_f32(C.c_int(mode), ptr(x), ptr(r), ptr(p), ptr(ap), ptr(g), C.c_int64(n), C.c_double(float(damping)),
                                         C.c_double(float(residual_tol)), C.c_double(float(target_kl)), C.c_int(int(bool(last))), ptr(ctl),
                                         stream_ptr()), "cstr_trpo_cg_step_f32")


def trpo_apply_step(theta, theta0, s, mask, ctl):
    """theta = theta0 + ctl[coeff] * ctl[step] * s where mask != 0; every other float of theta keeps its bits"""
    n = theta.numel()
    for t, nm in ((theta, "theta"), (theta0, "theta0"), (s, "s"), (mask, "mask")):
        _vec(t, nm, n)
    _chk(ctl, "ctl", (nv.TRPO_CTL_WORDS,), th.float64)
    check(nv.lib().cstr_trpo_apply_step_f32(ptr(theta), ptr(theta0), ptr(s), ptr(mask), C.c_int64(n), ptr(ctl), stream_ptr()),
          "cstr_trpo_apply_step_f32")


def trpo_value_loss(values, returns, g_value, loss_out=None, loss_sum=None):
    """mse(returns, values) and its gradient 2 (values - returns) / B in one launch; loss_sum[0] += loss"""
    b = values.numel()
    _vec(values, "values", b), _vec(returns, "returns", b), _vec(g_value, "g_value", b)
    for t, nm in ((loss_out, "loss_out"), (loss_sum, "loss_sum")):
        if t is not None:
            _vec(t, nm, 1)
    check(nv.lib().cstr_trpo_value_loss_f32(ptr(values), ptr(returns), C.c_int64(b), ptr(g_value), ptr(loss_out), ptr(loss_sum), stream_ptr()),
          "cstr_trpo_value_loss_f32")


def trpo_x0(x, mask, scale: float, rng_ctl):
    """x = scale * N(0, 1) where mask != 0 and 0 elsewhere, drawn on TRPO's own Philox stream (nv.TRPO_TAG)"""
    n = x.numel()
    _vec(x, "x", n), _vec(mask, "mask", n), _chk(rng_ctl, "rng_ctl", (nv.RNG_CTL_WORDS,), th.int64)
    check(nv.lib().cstr_trpo_x0_f32(ptr(x), ptr(mask), C.c_int64(n), C.c_float(float(scale)), ptr(rng_ctl), stream_ptr()), "cstr_trpo_x0_f32")
