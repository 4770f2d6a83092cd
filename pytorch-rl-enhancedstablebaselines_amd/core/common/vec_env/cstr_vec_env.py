"""VecEnv protocol (reference: core/common/vec_env/base_vec_env.py:50-335) and the device-resident
`CSTRVecEnv` that replaces `DummyVecEnv([lambda: TwoSeriesCSTREnv()] * N)`: N reactor trains live in HBM
and one HIP launch advances all of them (reference loop: core/common/vec_env/dummy_vec_env.py:56-73).

Two faces:
  * compatibility path  -- `reset()/step(actions)` take and return NumPy exactly like the reference
    (copies, bool dones, infos with "TimeLimit.truncated"/"terminal_observation");
  * fast path           -- `step_device(actions)` and the fused `collect_step` used by the off-policy
    loop keep everything in HBM and never synchronise with the host.
"""
from typing import Optional, Sequence

import numpy as np
import torch as th

from core import _native as nv
from core.common import hip_ops
from core.common.spaces import Box, Dict, Discrete, MultiDiscrete
from core.common.vec_env.base_vec_env import VecEnv

MIN_VALVE_LEVELS, MAX_VALVE_LEVELS = 2, 16
MAX_MULTI_VALVE_LEVELS = 32  # the MultiDiscrete face: one categorical per valve (csrc/cstr_multicategorical.hip)


def valve_levels(levels: int) -> np.ndarray:
    """v(q) for q = 0 .. levels - 1: f32(-1) + f32(2 q) / f32(levels - 1), evaluated in float32 in that order (what
    cstr_dqn_act_f32 writes)."""
    q = np.arange(levels, dtype=np.int64)
    return np.float32(-1) + (2 * q).astype(np.float32) / np.float32(levels - 1)


def decode_valve_index(index, levels: int) -> np.ndarray:
    """indices a [...] -> normalised valve pairs [..., 2] = (v(a // levels), v(a % levels))"""
    a = np.asarray(index, dtype=np.int64)
    v = valve_levels(levels)
    return np.stack([v[a // levels], v[a % levels]], axis=-1)


def encode_valve_pair(valve, levels: int) -> np.ndarray:
    """valve pairs [..., 2] (as stored in the replay ring) -> indices [...]: q = rint((v + 1) * (levels - 1) / 2) in float32"""
    v = np.asarray(valve, dtype=np.float32)
    q = np.rint(((v + np.float32(1)) * np.float32(levels - 1)) / np.float32(2))
    q = np.clip(q, 0, levels - 1).astype(np.int64)
    return q[..., 0] * levels + q[..., 1]


def decode_valve_levels(pairs, nvec) -> np.ndarray:
    """level pairs [..., 2] of the MultiDiscrete face -> normalised valve pairs [..., 2] = (v_0(a_0), v_1(a_1))"""
    a = np.asarray(pairs, dtype=np.int64)
    return np.stack([valve_levels(int(nvec[0]))[a[..., 0]], valve_levels(int(nvec[1]))[a[..., 1]]], axis=-1)


GOAL_KEYS = ("achieved_goal", "desired_goal", "observation")  # sorted: the column order of the flat row


def goal_rows_to_dict(rows: np.ndarray) -> dict:
    """flat rows [..., 6] -> {achieved_goal [..., 1], desired_goal [..., 1], observation [..., 4]} (copies)"""
    rows = np.asarray(rows)
    return {"achieved_goal": rows[..., 0:1].copy(), "desired_goal": rows[..., 1:2].copy(), "observation": rows[..., 2:6].copy()}


def goal_dict_to_rows(obs: dict) -> np.ndarray:
    """the inverse: the sub-arrays concatenated in key order, float32"""
    return np.concatenate([np.asarray(obs[k], np.float32).reshape(np.shape(obs["observation"])[:-1] + (-1,)) for k in GOAL_KEYS], axis=-1)


def goal_reward_np(coef, achieved_goal, desired_goal) -> np.ndarray:
    """The goal face's reward, float32, in this order (goals [B] or [B, 1] -> rewards [B]):
    C2 = s_lo2 + (ag + 1) * s_span2 / 2;  T = s_lo2 + (dg + 1) * s_span2 / 2;  ne = |C2 - T| / conc_span;  r = -5 (ne ne) - 2 ne"""
    lo2, span2, cs = np.float32(coef.s_lo[2]), np.float32(coef.s_span[2]), np.float32(coef.conc_span)
    ag = np.asarray(achieved_goal, np.float32)
    dg = np.asarray(desired_goal, np.float32)
    ag = ag.reshape(-1) if ag.ndim > 1 else ag
    dg = dg.reshape(-1) if dg.ndim > 1 else dg
    c2 = lo2 + (ag + np.float32(1)) * span2 / np.float32(2)
    t = lo2 + (dg + np.float32(1)) * span2 / np.float32(2)
    ne = np.abs(c2 - t) / cs
    return (np.float32(-5) * (ne * ne) - np.float32(2) * ne).astype(np.float32)


def _philox4x32_10(c: np.ndarray, key: int) -> np.ndarray:
    """Philox4x32-10 on counters c uint32 [n, 4] with a 64-bit key -> uint32 [n, 4] (the device function of csrc/cstr_rng_device.h)"""
    c = [c[:, i].astype(np.uint64) for i in range(4)]
    m32 = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


def draw_goal_targets(goal_seed: int, env_index, episode, lo: float, hi: float) -> np.ndarray:
    """The target an env draws for its episode of ordinal `episode`: f32 lo + (hi - lo) * u, u = (x >> 8) * 2^-24, x = word 0 of
    Philox4x32-10 with key goal_seed and counter (env index [64 bit], episode, tag). What cstr_goal_vec_step_f32 draws at an auto-reset."""
    idx = np.asarray(env_index, np.int64).astype(np.uint64)
    c = np.zeros((idx.shape[0], 4), np.uint32)
    c[:, 0], c[:, 1] = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    c[:, 2], c[:, 3] = np.asarray(episode, np.int64).astype(np.uint32), nv.HER_GOAL_TAG
    u = (_philox4x32_10(c, int(goal_seed) & (2**64 - 1))[:, 0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.float32(lo) + (np.float32(hi) - np.float32(lo)) * u


class CSTRVecEnv(VecEnv):
    """N independent two-series CSTR environments (reference: twoseriescstr.py:15-503) stepped by one HIP kernel.

    :param num_envs: number of reactor trains held by this process / GPU
    :param obs_dim: 4 = the reference's observation [C1,T1,C2,T2] normalised to [-1,1];
                    8 = [normalised | raw] (both halves are emitted by the reference's `info`)
    :param twin: with obs_dim=8: TWO reactor trains side by side per env -- observation [train A | train B] (both
                    normalised), 4 actions [F1A,F2A,F1B,F2B], reward rA + rB, one step counter / reset stream per env.
                    The 8-obs/4-act environment a 4-agent MADDPG needs (constructed, not in the reference)
    :param integrator: "euler" (reference, parity-pinned) or "rk4" (north_star's ask; not in the reference)
    :param default_target, min_concentration, max_concentration, init_mode: TwoSeriesCSTREnv ctor args
    :param seed_offset: added to env seeds, used by data-parallel shards (rank * num_envs)
    :param discrete_actions: K in 2..16 (twin=False only): a DISCRETE face over the same two valves, for DQN. `action_space` is
                    Discrete(K * K); index a stands for the valve levels (i, j) = (a // K, a % K) and the normalised valve action
                    v(q) = f32(-1) + f32(2 q) / f32(K - 1). `valve_space` = Box(-1, 1, (2,)) is what the env kernels and the replay
                    ring see: `step()` / `step_async()` take index arrays [N] (or [N, 1]) and decode them, `step_device` keeps
                    taking [N, 2] valve tensors. A constructed face, like twin=True: the reference's env has the Box face only
    :param multi_discrete_actions: K or (K0, K1), each in 2..32 (twin=False, no discrete_actions, no goal face): a FACTORED discrete
                    face, one categorical per valve, for PPO / A2C. `action_space` is MultiDiscrete([K0, K1]); level q of valve g is
                    the normalised valve action v_g(q) = f32(-1) + f32(2 q) / f32(K_g - 1) (`valve_levels(K_g)`). `step()` /
                    `step_async()` take integer arrays [N, 2]; `step_device`, `valve_space` and the env kernels keep seeing the
                    valve pair. `discrete_actions` stays None on this face: it names the joint-index face alone
    :param goal_conditioned: the GOAL face (obs_dim=4, twin=False, continuous valves only), for HER. `observation_space` is
                    Dict(achieved_goal: Box(-1, 1, (1,)), desired_goal: Box(-1, 1, (1,)), observation: Box(-1, 1, (4,))):
                    achieved_goal = observation[2] (normalised C2), desired_goal = the env's OWN target through the same affine
                    map. Targets are per env (`targets` [N] f32 in HBM, `set_targets`). The reward is the reference's concentration
                    term only (twoseriescstr.py:288-291) -- a GoalEnv reward is a function of (achieved, desired), so the
                    temperature penalty is not part of this face; `compute_reward` is the same statement in NumPy.
                    `step_device` and the learner see one flat row per env in key order, [achieved | desired | observation];
                    `reset()` / `step()` return dicts of NumPy arrays. A constructed face, like twin=True and discrete_actions
    :param goal_range: (lo, hi) or None. With a range an env's target is redrawn uniformly in [lo, hi] at every reset, auto-resets
                    included, from Philox keyed by (goal_seed, seed_offset + env index, episode ordinal of that env): counter-based,
                    the only state is an int32 episode counter per env, and the env's PCG64 reset stream is not touched
    :param goal_seed: key of that draw
    """

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 4}
    max_steps = 400

    def __init__(self, num_envs: int, obs_dim: int = 4, integrator: str = "euler", device="cuda",
                 default_target: float = 0.20, min_concentration: float = 0.05, max_concentration: float = 0.45,
                 init_mode: str = "random", seed_offset: int = 0, twin: bool = False, discrete_actions: Optional[int] = None,
                 goal_conditioned: bool = False, goal_range=None, goal_seed: int = 0, multi_discrete_actions=None):
        if multi_discrete_actions is not None:
            if twin:
                raise ValueError("multi_discrete_actions needs twin=False (one valve pair per env)")
            if discrete_actions is not None:
                raise ValueError("multi_discrete_actions and discrete_actions are two faces over the same valves: choose one")
            if goal_conditioned:
                raise ValueError("multi_discrete_actions needs goal_conditioned=False (the goal face has continuous valves only)")
            pair = (multi_discrete_actions,) * 2 if isinstance(multi_discrete_actions, (int, np.integer)) else tuple(multi_discrete_actions)
            if len(pair) != 2 or not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool)
                                         and MIN_VALVE_LEVELS <= k <= MAX_MULTI_VALVE_LEVELS for k in pair):
                raise ValueError(f"multi_discrete_actions must be an integer or a pair of integers in [{MIN_VALVE_LEVELS}, "
                                 f"{MAX_MULTI_VALVE_LEVELS}], got {multi_discrete_actions!r}")
            multi_discrete_actions = (int(pair[0]), int(pair[1]))
        if goal_conditioned and (twin or obs_dim != 4 or discrete_actions is not None):
            raise ValueError("goal_conditioned=True needs obs_dim=4, twin=False and continuous valves (discrete_actions=None)")
        if goal_range is not None:
            if not goal_conditioned:
                raise ValueError("goal_range needs goal_conditioned=True")
            lo_g, hi_g = (float(v) for v in goal_range)
            if not min_concentration <= lo_g <= hi_g <= max_concentration:
                raise ValueError(f"goal_range must lie in [{min_concentration}, {max_concentration}] with lo <= hi, got {goal_range!r}")
        if discrete_actions is not None:
            if twin:
                raise ValueError("discrete_actions needs twin=False (one valve pair per env)")
            if not (isinstance(discrete_actions, (int, np.integer)) and MIN_VALVE_LEVELS <= discrete_actions <= MAX_VALVE_LEVELS):
                raise ValueError(f"discrete_actions must be an integer in [{MIN_VALVE_LEVELS}, {MAX_VALVE_LEVELS}], got {discrete_actions!r}")
        if obs_dim not in (4, 8):
            raise ValueError(f"obs_dim must be 4 or 8, got {obs_dim}")
        if twin and obs_dim != 8:
            raise ValueError("twin=True needs obs_dim=8 (two 4-dim reactor trains per env)")
        if integrator not in nv.INTEGRATORS:
            raise ValueError(f"integrator must be one of {list(nv.INTEGRATORS)}, got {integrator!r}")
        if init_mode not in ("random", "static"):
            raise ValueError(f"init_mode={init_mode} is not supported, please choose 'random' or 'static'")  # twoseriescstr.py:257
        from core.common.utils import get_device

        self.device = get_device(device)
        nv.lib()  # fail loudly if the HIP extension is missing
        one = np.ones(obs_dim, np.float32)
        self.twin, self.act_dim = twin, (4 if twin else 2)
        if obs_dim == 8 and not twin:
            lo = np.concatenate([-one[:4], np.array([0.0, 273.15, 0.0, 273.15], np.float32)])
            hi = np.concatenate([one[:4], np.array([0.7, 400.0, 0.7, 400.0], np.float32)])
        else:
            lo, hi = -one, one
        a1 = np.ones(self.act_dim, np.float32)
        self.valve_space = Box(-a1, a1, dtype=np.float32)
        self.discrete_actions = None if discrete_actions is None else int(discrete_actions)
        self.multi_discrete_actions = multi_discrete_actions
        if multi_discrete_actions is not None:
            action_space = MultiDiscrete(list(multi_discrete_actions))
        else:
            action_space = self.valve_space if discrete_actions is None else Discrete(self.discrete_actions ** 2)
        self.goal_conditioned = bool(goal_conditioned)
        self.goal_range = None if goal_range is None else (float(goal_range[0]), float(goal_range[1]))
        self.goal_seed = int(goal_seed)
        if goal_conditioned:
            g1 = np.ones(1, np.float32)
            observation_space = Dict({"achieved_goal": Box(-g1, g1, dtype=np.float32), "desired_goal": Box(-g1, g1, dtype=np.float32),
                                      "observation": Box(lo, hi, dtype=np.float32)})
        else:
            observation_space = Box(lo, hi, dtype=np.float32)
        super().__init__(num_envs, observation_space, action_space)
        self.obs_dim, self.integrator, self.seed_offset = obs_dim, integrator, seed_offset
        self.target_C2, self.min_concentration, self.max_concentration = default_target, min_concentration, max_concentration
        self.init_mode = init_mode
        self.coef = nv.default_coef(default_target, min_concentration, max_concentration, self.max_steps)
        n, dev = num_envs, self.device
        with th.cuda.device(dev):
            self.obs = th.zeros(n, obs_dim, dtype=th.float32, device=dev)          # TwoSeriesCSTREnv.state (+ raw half)
            self.step_count = th.zeros(n, dtype=th.int32, device=dev)              # TwoSeriesCSTREnv.current_step
            self.pcg_state = th.zeros(n, nv.PCG_STATE_WORDS, dtype=th.int64, device=dev)  # per-env np_random (PCG64)
            self._next_obs = th.zeros(n, obs_dim, dtype=th.float32, device=dev)
            self._reset_buf = th.zeros(n, obs_dim, dtype=th.float32, device=dev)
            self._rew, self._done, self._timeout = (th.zeros(n, dtype=th.float32, device=dev) for _ in range(3))
            # init_mode="static": every env's f64 `init_state`, which each reset perturbs in place (twoseriescstr.py:94-96,
            # :246-255); None = init_mode="random"
            self.static_init = None
            if init_mode == "static":
                base = th.tensor([0.45, 310.0, 0.25, 290.0], dtype=th.float64, device=dev)
                self.static_init = base.repeat(n, 2 if twin else 1).contiguous()
            if goal_conditioned:
                self.flat = th.zeros(n, hip_ops.GOAL_ROW, dtype=th.float32, device=dev)  # [achieved | desired | observation] per env
                self._next_rows = th.zeros(n, hip_ops.GOAL_ROW, dtype=th.float32, device=dev)
                self.targets = th.full((n,), float(np.float32(default_target)), dtype=th.float32, device=dev)
                self.episode = th.zeros(n, dtype=th.int32, device=dev) if goal_range is not None else None  # ordinal of the next episode
        self._rng_seeded = False
        self._pending_actions: Optional[th.Tensor] = None
        self.numpy_reseed: Optional[int] = None  # last `np.random.seed` a seeded reset performed (twoseriescstr.py:164)
        self._has_reset = False

    # ---- seeding / reset -----------------------------------------------------------------------------
    def set_target(self, target: float) -> bool:
        """reference: twoseriescstr.py:114-127"""
        if self.min_concentration <= target <= self.max_concentration:
            self.target_C2 = target
            self.coef = nv.default_coef(target, self.min_concentration, self.max_concentration, self.max_steps)
            if self.goal_conditioned:
                self.set_targets(target)
            return True
        return False

    # ---- the goal face -------------------------------------------------------------------------------
    def _need_goal_face(self) -> None:
        if not self.goal_conditioned:
            raise ValueError("this method belongs to the goal face: construct the env with goal_conditioned=True")

    def set_targets(self, targets) -> bool:
        """Per-env setpoints (a scalar sets all envs), validated against [min_concentration, max_concentration] like set_target."""
        self._need_goal_face()
        t = np.broadcast_to(np.asarray(targets, np.float32), (self.num_envs,)) if np.ndim(targets) == 0 else np.asarray(targets, np.float32)
        if t.shape != (self.num_envs,):
            raise ValueError(f"targets shape {t.shape} != {(self.num_envs,)}")
        if not (np.all(t >= np.float32(self.min_concentration)) and np.all(t <= np.float32(self.max_concentration))):
            return False
        self.targets.copy_(th.from_numpy(np.ascontiguousarray(t)))
        self.flat[:, 1].copy_(th.from_numpy(self.goal_of_target(t)))
        return True

    def goal_of_target(self, target) -> np.ndarray:
        """desired_goal of a raw target: g = 2 (target - s_lo[2]) / s_span[2] - 1 in float32 (the observation's own map of C2)"""
        k = self.coef
        return np.float32(2) * (np.asarray(target, np.float32) - np.float32(k.s_lo[2])) / np.float32(k.s_span[2]) - np.float32(1)

    def compute_reward(self, achieved_goal, desired_goal, infos=None) -> np.ndarray:
        """GoalEnv.compute_reward, vectorised, float32: the reference's concentration term (twoseriescstr.py:288-291) on
        (achieved, desired), the statement the env step and the HER sampler evaluate on the device."""
        self._need_goal_face()
        return goal_reward_np(self.coef, achieved_goal, desired_goal)

    def _refresh_flat(self, redraw: bool) -> None:
        """flat rows from `obs` and `targets` on the host (reset / set_state; not on the stepping path)."""
        if redraw and self.goal_range is not None:
            ordinal = self.episode.cpu().numpy()
            idx = self.seed_offset + np.arange(self.num_envs, dtype=np.int64)
            self.targets.copy_(th.from_numpy(draw_goal_targets(self.goal_seed, idx, ordinal, *self.goal_range)))
            self.episode += 1
        obs = self.obs.cpu().numpy()
        rows = np.concatenate([obs[:, 2:3], self.goal_of_target(self.targets.cpu().numpy())[:, None], obs], axis=1)
        self.flat.copy_(th.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)))

    def _seed_rng(self, seeds: Sequence[Optional[int]]) -> None:
        """Per-env `seeding.np_random(seed)` = Generator(PCG64(SeedSequence(seed))) (twoseriescstr.py:162). The
        SeedSequence hashing runs in NumPy on the host (once); only the 4 state words go to the GPU."""
        m = (1 << 64) - 1
        words = np.empty((self.num_envs, 4), np.uint64)
        for i, s in enumerate(seeds):
            st = np.random.PCG64(np.random.SeedSequence(None if s is None else int(s))).state["state"]
            words[i] = (st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)
        self.pcg_state.copy_(th.from_numpy(words.view(np.int64)))
        self._rng_seeded = True

    def reset_device(self) -> th.Tensor:
        """reference: dummy_vec_env.py:75-83 + TwoSeriesCSTREnv.reset (twoseriescstr.py:226-269)."""
        seeds = list(self._seeds)
        if any(s is not None for s in seeds):
            # a seeded reset re-creates every seeded env's generator and reseeds the GLOBAL numpy stream with the
            # env's seed (twoseriescstr.py:163-164): the last env wins -> seed + N - 1 (SURVEY a-6)
            if not all(s is not None for s in seeds):
                raise ValueError("CSTRVecEnv.reset: either all or none of the envs must be seeded")
            self._seed_rng([s + self.seed_offset for s in seeds])
            self.numpy_reseed = int(seeds[-1] + self.seed_offset) & 0xFFFFFFFF
        elif not self._rng_seeded:
            self._seed_rng([None] * self.num_envs)  # unseeded envs draw OS entropy, like gymnasium does
        with th.cuda.device(self.device):
            hip_ops.reset_draw(self.pcg_state, None, self.obs, self.act_dim, static_init=self.static_init)
            self.step_count.zero_()
        self._reset_seeds()
        self._reset_options()
        self._has_reset = True
        if self.goal_conditioned:
            self._refresh_flat(redraw=True)
            return self.flat
        return self.obs

    def reset(self):
        out = self.reset_device().cpu().numpy()
        return goal_rows_to_dict(out) if self.goal_conditioned else out

    def set_state(self, obs, step_count=None) -> None:
        """Inject observations / step counters (tests, fixtures). obs: [N, 4] normalised or [N, obs_dim]."""
        obs = th.as_tensor(np.asarray(obs, np.float32))
        if obs.shape == (self.num_envs, 4) and self.obs_dim == 8 and not self.twin:
            lo = th.tensor([0.0, 273.15, 0.0, 273.15])
            hi = th.tensor([0.7, 400.0, 0.7, 400.0])
            raw = th.minimum(th.maximum(lo + (obs + 1.0) * (hi - lo) / 2.0, lo), hi)
            obs = th.cat([obs, raw], dim=1)
        if tuple(obs.shape) != (self.num_envs, self.obs_dim):
            raise ValueError(f"obs shape {tuple(obs.shape)} != {(self.num_envs, self.obs_dim)}")
        self.obs.copy_(obs)
        if step_count is not None:
            self.step_count.copy_(th.as_tensor(np.asarray(step_count, np.int32)))
        if not self._rng_seeded:
            self._seed_rng([None] * self.num_envs)
        self._has_reset = True
        if self.goal_conditioned:
            self._refresh_flat(redraw=False)

    # ---- stepping ------------------------------------------------------------------------------------
    def step_device(self, actions: th.Tensor):
        """One launch for all envs, no host sync. Returns device views
        (obs_after, reward, done, timeout, next_obs): `next_obs` is the terminal observation where done."""
        if not self._has_reset:
            raise ValueError("Please call env.reset() to reset the env first!")  # twoseriescstr.py:401-402
        if self.goal_conditioned:  # one launch: step, goal reward, auto-reset draw, target redraw, flat rows
            with th.cuda.device(self.device):
                lo_g, hi_g = self.goal_range if self.goal_range is not None else (0.0, 0.0)
                hip_ops.goal_vec_step(self.coef, self.integrator, self.obs, actions, self.step_count, self.pcg_state, self.targets,
                                      self._next_rows, self.flat, self._rew, self._done, self._timeout, static_init=self.static_init,
                                      episode=self.episode, goal_seed=self.goal_seed, goal_index_offset=self.seed_offset, goal_lo=lo_g,
                                      goal_hi=hi_g)
            return self.flat, self._rew, self._done, self._timeout, self._next_rows
        with th.cuda.device(self.device):
            # reset source for envs that finish now: draw lazily for ALL envs would advance every stream, so the
            # draw kernel runs masked AFTER the step on a scratch copy of the observations
            hip_ops.vec_step(self.coef, self.integrator, self.obs, actions, self.step_count, self.obs, self._next_obs,
                             self._reset_buf, self._rew, self._done, self._timeout)
            # _reset_buf now holds obs_after with the OLD obs where done; overwrite those rows with fresh draws
            hip_ops.reset_draw(self.pcg_state, self._done.to(th.uint8), self._reset_buf, self.act_dim, static_init=self.static_init)
            self.obs.copy_(self._reset_buf)
        return self.obs, self._rew, self._done, self._timeout, self._next_obs

    def collect_step_device(self, ring, her, policy_out: th.Tensor, squashed: int, act_low, act_high, noise=None, ep_return=None, ep_stats=None,
                            rng_advance=None):
        """The rollout's vec-step on the goal face in ONE launch (hip_ops.goal_collect_step), no host sync: the action scaling chain on
        `policy_out`, `step_device` on the env's own arrays and the HerReplayBuffer add of (`flat` before the step, the terminal-aware next
        rows, the buffer action) into `ring` / `her`. `flat` is read as the transition's observation and then holds what VecEnv.step
        returns. Returns the same device views as `step_device`."""
        self._need_goal_face()
        if not self._has_reset:
            raise ValueError("Please call env.reset() to reset the env first!")  # twoseriescstr.py:401-402
        with th.cuda.device(self.device):
            lo_g, hi_g = self.goal_range if self.goal_range is not None else (0.0, 0.0)
            hip_ops.goal_collect_step(self.coef, self.integrator, ring, her, self.obs, self.flat, self.step_count, self.pcg_state, self.targets,
                                      policy_out, squashed, act_low, act_high, noise=noise, static_init=self.static_init, episode=self.episode,
                                      goal_seed=self.goal_seed, goal_index_offset=self.seed_offset, goal_lo=lo_g, goal_hi=hi_g,
                                      reward_out=self._rew, done_out=self._done, timeout_out=self._timeout, next_rows_out=self._next_rows,
                                      ep_return=ep_return, ep_stats=ep_stats, rng_advance=rng_advance)
        return self.flat, self._rew, self._done, self._timeout, self._next_rows

    def step_async(self, actions) -> None:
        if self.discrete_actions is not None:
            idx = actions.cpu().numpy() if isinstance(actions, th.Tensor) else np.asarray(actions)
            if not np.issubdtype(idx.dtype, np.integer) or idx.shape not in ((self.num_envs,), (self.num_envs, 1)):
                raise ValueError(f"discrete actions: expected integer indices of shape {(self.num_envs,)}, got {idx.dtype} {idx.shape}")
            idx = idx.reshape(self.num_envs)
            if idx.min() < 0 or idx.max() >= self.action_space.n:
                raise ValueError(f"discrete actions: indices must lie in [0, {self.action_space.n})")
            actions = decode_valve_index(idx, self.discrete_actions)
        elif self.multi_discrete_actions is not None:
            pairs = actions.cpu().numpy() if isinstance(actions, th.Tensor) else np.asarray(actions)
            if not np.issubdtype(pairs.dtype, np.integer) or pairs.shape != (self.num_envs, 2):
                raise ValueError(f"multi-discrete actions: expected integer level pairs of shape {(self.num_envs, 2)}, got {pairs.dtype} {pairs.shape}")
            nvec = self.action_space.nvec
            if pairs.min() < 0 or (pairs >= nvec).any():
                raise ValueError(f"multi-discrete actions: levels must lie in [0, {nvec[0]}) x [0, {nvec[1]})")
            actions = decode_valve_levels(pairs, nvec)
        a = th.as_tensor(np.asarray(actions, dtype=np.float32)) if not isinstance(actions, th.Tensor) else actions
        if tuple(a.shape) != (self.num_envs, self.act_dim):
            raise ValueError(f"actions shape {tuple(a.shape)} != {(self.num_envs, self.act_dim)}")
        self._pending_actions = a.to(self.device, th.float32).contiguous()

    def step_wait(self):
        obs, rew, done, timeout, next_obs = self.step_device(self._pending_actions)
        obs_h, rew_h = obs.cpu().numpy(), rew.cpu().numpy()
        done_h, tout_h = done.cpu().numpy().astype(bool), timeout.cpu().numpy().astype(bool)
        infos: list = [{"TimeLimit.truncated": bool(t)} for t in tout_h]
        if done_h.any():
            term = next_obs.cpu().numpy()
            for i in np.nonzero(done_h)[0]:
                infos[i]["terminal_observation"] = goal_rows_to_dict(term[i]) if self.goal_conditioned else term[i].copy()
        return (goal_rows_to_dict(obs_h) if self.goal_conditioned else obs_h), rew_h, done_h, infos
