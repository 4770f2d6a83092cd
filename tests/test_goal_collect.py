"""GPU tests of the goal face's fused collect step (cstr_goal_collect_step_f32) and of hipGraph replay of HER iterations.

  1. The kernel against the launches it replaces, through the C ABI, on a twin state: the float32 statements of the action chain in NumPy
     (the reference's grouping `lo + (0.5 * (s + 1) * (hi - lo))`), cstr_goal_vec_step_f32, cstr_her_add_f32. Bit-identical after every
     step: env state, flat rows, step counters, PCG64 words, static init states, targets, episode ordinals, the four outputs, every ring
     and HER array, the control words, the per-env returns. The two unfused launches are held to the NumPy restatement of
     tests/_her_reference.py on the same inputs, so the refactor into shared device functions is covered as well.
  2. SAC / TD3 on the goal face with CSTR_HER_FUSED_COLLECT 1 against 0: the same training state, bit for bit.
  3. Eager against hipGraph replay (one and four iterations per graph): the same training state, bit for bit; callbacks, checkpoints.
  4. A HER SAC run under replay still learns (the criterion and sizes of tests/test_her.py).

Tolerances: none but one. `ep_stats[1]`, the f64 sum of the finished episodes' f32 returns, is accumulated by one f64 atomicAdd per
finished episode in no fixed order: it is compared with NumPy's f64 sum within n_envs * 2^-53 relative, the first-order bound
(n - 1) u sum|x| of any summation order of n same-sign f64 terms (u = 2^-53); every launch of test 1 sums into a zeroed slot, so a slot
holds at most n_envs terms. The episode count and the length sum are integers in f64 and exact.
NaN: a NaN action reaches the env only without action noise (with noise the kernel's fminf / fmaxf clip a NaN to -1, as
cstr_collect_step_f32 does on the Box face, where NumPy's clip propagates it), so the NaN cases run without noise. The buffer action of a
NaN lane is a NaN computed by the device in one twin and by NumPy in the other: IEEE 754 leaves the payload of such a NaN open, so the
ring's action array is compared as "NaN in the same places, equal bits elsewhere" in the NaN case and bit for bit in all others."""
import os

import numpy as np
import pytest
import torch as th

from _her_reference import HerNp, goal_of_target, goal_reward

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]
DEV = "cuda:0"
SENTINEL, PAD = -777, 64
BIG_SEED, INDEX_OFFSET = (1 << 40) + 7, 1000
F = np.float32


@pytest.fixture(scope="module")
def ops():
    from core import _native as nv
    from core.common import hip_ops

    nv.lib()
    assert th.cuda.is_available()
    return hip_ops


def dev(x, dtype=None):
    t = th.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(t: th.Tensor) -> th.Tensor:
    """the tensor's bit pattern (NaN-proof equality)"""
    return t.view({4: th.int32, 8: th.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a: th.Tensor, b: th.Tensor) -> bool:
    return th.equal(bits(a), bits(b))


# ---- 1. the kernel against the launches it replaces ------------------------------------------------------------------------------------
class Twin:
    """One copy of everything the collect step touches, every array between sentinel pads."""

    STATE = ("obs", "flat", "step", "pcg", "init", "target", "episode")
    OUT = ("rew", "done", "tout", "next_rows", "ep_ret", "stats")
    RING = ("r_obs", "r_next", "r_act", "r_rew", "r_done", "r_tout")
    HER = ("goal", "start", "length", "cur", "valid", "bits")

    def __init__(self, env, rows, steps):
        from core import _native as nv

        n = env.num_envs
        words = (n + 63) // 64
        f, i32, i64, f64 = th.float32, th.int32, th.int64, th.float64
        spec = dict(obs=((n, 4), f), flat=((n, 6), f), step=((n,), i32), pcg=((n, 4), i64), init=((n, 4), f64), target=((n,), f), episode=((n,), i32),
                    rew=((n,), f), done=((n,), f), tout=((n,), f), next_rows=((n, 6), f), ep_ret=((n,), f), stats=((steps, 4), f64),
                    r_obs=((rows, n, 4), f), r_next=((rows, n, 4), f), r_act=((rows, n, 2), f), r_rew=((rows, n), f), r_done=((rows, n), f),
                    r_tout=((rows, n), f), goal=((rows, n), f), start=((rows, n), i32), length=((rows, n), i32), cur=((n,), i32),
                    valid=((rows,), i32), bits=((rows, words), i64), ctl=((4,), i64), rng=((16,), i64))
        self.full, self.v = {}, {}
        for k, (shape, dt) in spec.items():
            numel = int(np.prod(shape))
            self.full[k] = th.full((numel + 2 * PAD,), SENTINEL, dtype=dt, device=DEV)
            self.v[k] = self.full[k][PAD:PAD + numel].view(shape)
            self.v[k].zero_()
        v = self.v
        v["obs"].copy_(env.obs), v["flat"].copy_(env.flat), v["step"].copy_(env.step_count), v["pcg"].copy_(env.pcg_state)
        v["target"].copy_(env.targets)
        self.init = None
        if env.static_init is not None:
            v["init"].copy_(env.static_init)
            self.init = v["init"]
        self.episode = None
        if env.episode is not None:
            v["episode"].copy_(env.episode)
            self.episode = v["episode"]
        v["rng"].copy_(th.arange(16, dtype=i64) * 1000003)
        self.ring = type("R", (), {})()
        self.ring.c = nv.Ring(*(v[k].data_ptr() for k in self.RING), rows, n, 4, 2)
        self.ring.ctl, self.ring.n_envs, self.ring.rows = v["ctl"], n, rows
        self.her = type("H", (), {})()
        self.her.c = nv.Her(*(v[k].data_ptr() for k in self.HER))

    def pads_untouched(self):
        for k, t in self.full.items():
            body = self.v[k].numel()
            assert bool((t[:PAD] == SENTINEL).all()) and bool((t[PAD + body:] == SENTINEL).all()), k


def goal_env(n, max_steps, init_mode, goal_range, integrator, rng, seed_offset=0):
    from core import _native as nv
    from core.common.vec_env import CSTRVecEnv

    env = CSTRVecEnv(n, device=DEV, goal_conditioned=True, goal_range=goal_range, goal_seed=BIG_SEED, init_mode=init_mode, integrator=integrator,
                     seed_offset=seed_offset)
    env.coef = nv.default_coef(0.20, 0.05, 0.45, max_steps)
    env.seed(9)
    env.reset()
    if goal_range is None:
        assert env.set_targets(rng.uniform(0.10, 0.40, n).astype(F))
    # episode ends staggered over the envs: env i starts at step i % max_steps
    env.set_state(rng.uniform(-0.5, 0.5, (n, 4)).astype(F), (np.arange(n) % max_steps).astype(np.int32))
    return env


def chain_np(pol, squashed, lo, hi, z):
    """off_policy_algorithm.py:364-411 in NumPy float32 -> (buffer action, env action)"""
    one, half, two = F(1), F(0.5), F(2)
    v = lo + (half * (pol + one) * (hi - lo)) if squashed else pol  # predict(): unscale_action
    sc = two * ((v - lo) / (hi - lo)) - one                        # scale_action
    if z is not None:
        sc = np.clip(sc + z, F(-1), F(1))                          # :401-402
    ea = lo + (half * (sc + one) * (hi - lo))                      # unscale_action (:406)
    assert sc.dtype == F and ea.dtype == F
    return np.ascontiguousarray(sc), np.ascontiguousarray(ea)


def step_inputs(rng, n, squashed, lo, hi, noise):
    pol = rng.uniform(-1, 1, (n, 2)).astype(F) if squashed else rng.uniform(lo, hi, (n, 2)).astype(F)
    z = None if noise == "none" else rng.normal(0, 0.1 if noise == "small" else 1.5, (n, 2)).astype(F)
    return pol, z


def fused_step(ops, env, tw, t, pol, z, squashed, lo, hi, omit=(), rng_advance=None):
    v = tw.v
    out = dict(reward_out=v["rew"], done_out=v["done"], timeout_out=v["tout"], next_rows_out=v["next_rows"], ep_return=v["ep_ret"],
               ep_stats=v["stats"][t])
    for k in omit:
        out[k] = None
    lo_g, hi_g = env.goal_range if env.goal_range is not None else (0.0, 0.0)
    ops.goal_collect_step(env.coef, env.integrator, tw.ring, tw.her, v["obs"], v["flat"], v["step"], v["pcg"], v["target"], dev(pol), squashed,
                          lo, hi, noise=None if z is None else dev(z), static_init=tw.init, episode=tw.episode, goal_seed=env.goal_seed,
                          goal_index_offset=env.seed_offset, goal_lo=lo_g, goal_hi=hi_g, rng_advance=rng_advance, **out)


def unfused_step(ops, env, tw, sc, ea):
    """the launches the fused one replaces, on the twin's arrays -> the add's inputs as NumPy arrays"""
    v = tw.v
    prev = v["flat"].clone()  # _last_obs: the step overwrites the env's rows
    lo_g, hi_g = env.goal_range if env.goal_range is not None else (0.0, 0.0)
    ops.goal_vec_step(env.coef, env.integrator, v["obs"], dev(ea), v["step"], v["pcg"], v["target"], v["next_rows"], v["flat"], v["rew"], v["done"],
                      v["tout"], static_init=tw.init, episode=tw.episode, goal_seed=env.goal_seed, goal_index_offset=env.seed_offset,
                      goal_lo=lo_g, goal_hi=hi_g)
    ops.her_add(tw.ring, tw.her, prev, v["next_rows"], dev(sc), v["rew"], v["done"], v["tout"])
    return tuple(x.cpu().numpy() for x in (prev, v["next_rows"], v["rew"], v["done"], v["tout"]))


def u32(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def check_unfused_against_restatement(tw, h, prev, nxt, sc, rew, done, tout, clean, where):
    """cstr_goal_vec_step_f32's reward / goals and cstr_her_add_f32's state against tests/_her_reference.py on the same inputs"""
    assert np.array_equal(u32(rew[clean]), u32(goal_reward(nxt[clean, 0], prev[clean, 1]))), where
    assert np.array_equal(u32(nxt[:, 1]), u32(prev[:, 1])) and np.array_equal(u32(nxt[:, 0]), u32(nxt[:, 4])), where
    assert np.array_equal(u32(tw.v["flat"][:, 1].cpu().numpy()), u32(goal_of_target(tw.v["target"].cpu().numpy()))), where
    h.add(prev, nxt, sc, rew, done, tout)
    v = tw.v
    assert np.array_equal(v["start"].cpu().numpy(), h.ep_start) and np.array_equal(v["length"].cpu().numpy(), h.ep_length), where
    assert np.array_equal(v["cur"].cpu().numpy(), h.cur) and v["ctl"].tolist() == [h.pos, int(h.full), 0, h.adds], where
    for k, want in (("r_obs", h.observation), ("r_next", h.next_observation), ("goal", h.desired_goal), ("r_act", h.actions),
                    ("r_rew", h.rewards), ("r_done", h.dones), ("r_tout", h.timeouts)):
        assert np.array_equal(u32(v[k].cpu().numpy()), u32(want)), (where, k)
    valid = h.ep_length > 0
    assert np.array_equal(v["valid"].cpu().numpy(), valid.sum(axis=1)), where
    b = v["bits"].cpu().numpy().view(np.uint64)
    got = ((b[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(h.rows, -1)[:, :h.n_envs].astype(bool)
    assert np.array_equal(got, valid), where


def compare_twins(a, b, where, skip=(), nan_act=False):
    for k in Twin.STATE + Twin.RING + Twin.HER + ("ctl", "rew", "done", "tout", "next_rows"):
        if k in skip:
            continue
        if k == "r_act" and nan_act:
            x, y = a.full[k], b.full[k]
            nan = th.isnan(x)
            assert th.equal(nan, th.isnan(y)) and th.equal(bits(x)[~nan], bits(y)[~nan]), (where, k)
            continue
        assert same_bits(a.full[k], b.full[k]), (where, k)


def run_case(ops, n, rows, max_steps, squashed, noise, bounds, integrator, init_mode, goal_range, rng_adv=None, nan_at=None, omit=(), steps=None,
             seed_offset=0):
    """Drive a fused twin and an unfused twin through `steps` vec-steps (default: three wraps of the ring) and compare after every step."""
    rng = np.random.default_rng(1000 * n + 10 * rows + max_steps)
    env = goal_env(n, max_steps, init_mode, goal_range, integrator, rng, seed_offset)
    steps = 3 * rows + 2 if steps is None else steps
    a, b = Twin(env, rows, steps), Twin(env, rows, steps)
    h = HerNp(rows, n)
    lo, hi = (np.asarray(x, F) for x in bounds)
    ep_ret = np.zeros(n, F)
    seen = dict(done_on_invalidating_row=False, clip_binds=False, uneven=False, nan=False)
    n_done, len_sum = 0, 0
    for t in range(steps):
        where = (n, rows, max_steps, t)
        pol, z = step_inputs(rng, n, squashed, lo, hi, noise)
        nan_env = None
        if nan_at is not None and t in nan_at:
            kind, nan_env = nan_at[t]
            if kind == "action":
                pol[nan_env, 1] = np.nan
            else:  # a NaN state: the env's observation and its copies in the flat row, in both twins
                for tw in (a, b):
                    tw.v["obs"][nan_env, 1] = float("nan")
                    tw.v["flat"][nan_env, 3] = float("nan")
        sc, ea = chain_np(pol, squashed, lo, hi, z)
        if z is not None:
            seen["clip_binds"] |= bool((np.abs(chain_np(pol, squashed, lo, hi, None)[0] + z) > 1).any())
        step_before = b.v["step"].cpu().numpy().copy()
        pos_before = int(b.v["ctl"][0])
        invalidating = b.v["length"][pos_before].cpu().numpy() > 0
        rng_before = a.v["rng"].clone()
        fused_step(ops, env, a, t, pol, z, squashed, lo, hi, omit=omit, rng_advance=None if rng_adv is None else (a.v["rng"], rng_adv))
        prev, nxt, rew, done, tout = unfused_step(ops, env, b, sc, ea)
        th.cuda.synchronize()
        clean = np.ones(n, bool)
        if nan_env is not None:
            clean[nan_env] = False
            seen["nan"] = True
            assert rew[nan_env] == F(-10) and done[nan_env] == 1 and tout[nan_env] == 1, where
        check_unfused_against_restatement(b, h, prev, nxt, sc, rew, done, tout, clean, where)
        skip = {"reward_out": "rew", "done_out": "done", "timeout_out": "tout", "next_rows_out": "next_rows"}
        compare_twins(a, b, where, skip=tuple(skip[k] for k in omit if k in skip), nan_act=nan_at is not None)
        # Monitor's statistics: per-env returns bit for bit, the finished episodes of this launch in its own zeroed slot
        ret = ep_ret + rew
        fin = done > 0
        ep_ret = np.where(fin, F(0), ret).astype(F)
        seen["done_on_invalidating_row"] |= bool((invalidating & fin).any())
        seen["uneven"] |= bool(fin.any() and not fin.all())
        n_done += int(fin.sum())
        len_sum += int((step_before[fin] + 1).sum())
        if "ep_return" not in omit:
            assert np.array_equal(u32(a.v["ep_ret"].cpu().numpy()), u32(ep_ret)), where
            got = a.v["stats"][t].cpu().numpy()
            want = float(np.sum(ret[fin].astype(np.float64)))
            assert (ret[fin] <= 0).all(), where  # one sign: the bound below is for same-sign terms
            print(f"{where}: episodes {got[0]:.0f} (want {fin.sum()}), length sum {got[2]:.0f} (want {(step_before[fin] + 1).sum()}), "
                  f"return sum {got[1]!r} (want {want!r})")
            assert got[0] == fin.sum() and got[2] == (step_before[fin] + 1).sum() and got[3] == 0, where
            assert abs(got[1] - want) <= n * 2.0 ** -53 * abs(want), where
        # the Philox offset word: advanced by exactly the advance, once per launch; no other word of the block moves
        want_rng = rng_before.clone()
        if rng_adv is not None:
            want_rng[1] += rng_adv
        assert th.equal(a.v["rng"], want_rng), where
    a.pads_untouched()
    for k in omit:  # an output that was left out was not written anywhere
        name = dict(reward_out="rew", done_out="done", timeout_out="tout", next_rows_out="next_rows", ep_return="ep_ret", ep_stats="stats")[k]
        assert bool((a.v[name] == 0).all()), k
    assert n_done > 0 and int(a.v["ctl"][3]) == steps
    return seen, a


# n_envs at the word boundaries of valid_bits x rings of 4 and 7 rows; episode limits of 1, 2, the ring length and longer than the ring;
# both action modes; no / small / clipping noise; bounds other than (-1, 1); both integrators; both reset modes; targets that stay
# (episode NULL) and redrawn targets with a seed above 2^32 (BIG_SEED) and an index offset; with and without the Philox advance
UNIT, WIDE = ((-1.0, -1.0), (1.0, 1.0)), ((-2.0, 0.5), (1.5, 3.0))
CASES = [
    # n, rows, max_steps, squashed, noise, bounds, integrator, init_mode, goal_range, rng_adv, seed_offset
    (1, 4, 1, 1, "none", UNIT, "euler", "random", (0.10, 0.40), None, 0),
    (1, 7, 10, 0, "large", WIDE, "rk4", "static", None, 1, INDEX_OFFSET),
    (63, 4, 2, 0, "small", WIDE, "euler", "static", (0.10, 0.40), 63, INDEX_OFFSET),
    (63, 7, 7, 1, "large", UNIT, "rk4", "random", None, None, 0),
    (64, 4, 4, 1, "large", WIDE, "rk4", "random", (0.10, 0.40), 12345, INDEX_OFFSET),
    (64, 7, 2, 0, "none", UNIT, "euler", "static", (0.15, 0.15), None, 0),
    (65, 4, 7, 1, "small", UNIT, "euler", "static", (0.10, 0.40), 65, 0),
    (65, 7, 1, 0, "large", WIDE, "rk4", "random", None, None, INDEX_OFFSET),
    (130, 4, 4, 0, "none", WIDE, "rk4", "static", None, 130, 0),
    (130, 7, 10, 1, "large", UNIT, "euler", "random", (0.10, 0.40), 1 << 33, INDEX_OFFSET),
    (130, 7, 7, 1, "none", WIDE, "euler", "random", (0.10, 0.40), None, 0),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-r{c[1]}-T{c[2]}-sq{c[3]}-{c[4]}-{c[6]}-{c[7]}")
def test_fused_collect_equals_chain_step_add(ops, case):
    n, rows, max_steps, squashed, noise, bounds, integrator, init_mode, goal_range, rng_adv, seed_offset = case
    seen, _ = run_case(ops, n, rows, max_steps, squashed, noise, bounds, integrator, init_mode, goal_range, rng_adv=rng_adv, seed_offset=seed_offset)
    if max_steps in (1, rows):
        assert seen["done_on_invalidating_row"], seen
    if noise == "large":
        assert seen["clip_binds"], seen
    if n > 1 and max_steps > 1:
        assert seen["uneven"], seen


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_fused_collect_nan_action_and_nan_state(ops, integrator):
    """A NaN action (step 2, env 3) and a NaN state (step 5, env 64): old state, -10, truncated; the episode ends, the env resets."""
    seen, _ = run_case(ops, 65, 4, 6, 1, "none", WIDE, integrator, "random", (0.10, 0.40), nan_at={2: ("action", 3), 5: ("state", 64)})
    assert seen["nan"]


@pytest.mark.parametrize("omit", [("reward_out",), ("done_out",), ("timeout_out",), ("next_rows_out",), ("ep_return", "ep_stats"),
                                  ("reward_out", "done_out", "timeout_out", "next_rows_out", "ep_return", "ep_stats")], ids=lambda o: "+".join(o))
def test_fused_collect_optional_outputs_left_out(ops, omit):
    run_case(ops, 65, 4, 3, 1, "small", UNIT, "euler", "random", (0.10, 0.40), omit=omit, steps=9)


def test_fused_collect_relaunches_identically_and_accumulates_statistics(ops):
    """The same inputs on two copies of the state give the same bits (the f64 return sum within its bound); ep_stats accumulates over
    launches that share a slot."""
    n, rows, steps = 130, 7, 16
    runs = []
    for _ in range(2):
        rng = np.random.default_rng(3)
        env = goal_env(n, 5, "random", (0.10, 0.40), "euler", rng)
        tw = Twin(env, rows, 1)
        lo, hi = (np.asarray(x, F) for x in WIDE)
        for t in range(steps):
            pol, z = step_inputs(rng, n, 1, lo, hi, "large")
            fused_step(ops, env, tw, 0, pol, z, 1, lo, hi, rng_advance=(tw.v["rng"], n))
        th.cuda.synchronize()
        tw.pads_untouched()
        runs.append(tw)
    a, b = runs
    for k in a.full:
        if k != "stats":
            assert same_bits(a.full[k], b.full[k]), k
    sa, sb = a.v["stats"][0].cpu().numpy(), b.v["stats"][0].cpu().numpy()
    print(f"accumulated statistics of two equal runs: {sa.tolist()} / {sb.tolist()}")
    assert sa[0] == sb[0] == n * steps // 5 and sa[2] == sb[2] and sa[3] == sb[3] == 0
    assert sa[1] < 0 and abs(sa[1] - sb[1]) <= 2 * sa[0] * 2.0 ** -53 * abs(sa[1])  # each within (terms) u of the exact sum
    assert int(a.v["rng"][1]) == 1000003 + n * steps


# ---- 2. / 3. the learners ---------------------------------------------------------------------------------------------------------------
N_ENVS, WARMUP_STEPS = 5, 8


def make_model(algo):
    import core
    from core import _native as nv
    from core.common.noise import NormalActionNoise
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    env = CSTRVecEnv(N_ENVS, device=DEV, goal_conditioned=True, goal_range=(0.10, 0.40))
    env.coef = nv.default_coef(0.20, 0.05, 0.45, 7)
    kw = dict(seed=0, replay_buffer_class=HerReplayBuffer, device=DEV, buffer_size=16 * N_ENVS, learning_starts=WARMUP_STEPS * N_ENVS,
              batch_size=16, policy_kwargs=dict(net_arch=[16, 16]))
    if algo == "SAC":
        kw.update(replay_buffer_kwargs=dict(goal_selection_strategy="future"))
    else:
        kw.update(replay_buffer_kwargs=dict(goal_selection_strategy="episode"), policy_delay=2,
                  action_noise=NormalActionNoise(np.zeros(2), 0.1 * np.ones(2)))
    return getattr(core, algo)("MultiInputPolicy", env, **kw)


def snapshot(model) -> dict:
    """weights, optimiser state, every ring / HER array, the sampler stream image, env state and targets, the counters"""
    th.cuda.synchronize()
    env, rb = model.get_env().unwrapped, model.replay_buffer
    s = {f"weights/{k}": v for k, v in model.policy.state_dict().items()}
    opts = dict(actor=model.actor.optimizer, critic=model.critic.optimizer)
    if getattr(model, "ent_coef_optimizer", None) is not None:
        opts["ent_coef"] = model.ent_coef_optimizer
        s["weights/log_ent_coef"] = model.log_ent_coef.detach()
    for name, opt in opts.items():
        s[f"opt/{name}/exp_avg"], s[f"opt/{name}/exp_avg_sq"], s[f"opt/{name}/ctl"] = opt.exp_avg, opt.exp_avg_sq, opt.ctl
    r, h = rb.ring, rb.her
    s.update(ring_obs=r.observations, ring_next=r.next_observations, ring_act=r.actions, ring_rew=r.rewards, ring_done=r.dones,
             ring_tout=r.timeouts, ring_ctl=r.ctl, goal=h.desired_goal, ep_start=h.ep_start, ep_length=h.ep_length, cur=h.cur_ep_start,
             row_valid=h.row_valid, valid_bits=h.valid_bits, sampler=rb.sampler_stream, env_obs=env.obs, env_flat=env.flat,
             env_steps=env.step_count, env_pcg=env.pcg_state, targets=env.targets, episode=env.episode)
    out = {k: v.detach().cpu().numpy().copy() for k, v in s.items()}
    out["counters"] = np.array([model._episode_num, model.num_timesteps, model._n_updates, rb._adds], np.int64)
    return out


def assert_same_state(base: dict, other: dict, what: str) -> None:
    assert base.keys() == other.keys()
    for k in base:  # print each figure before asserting
        a, b = np.asarray(base[k], np.float64), np.asarray(other[k], np.float64)
        print(f"{what} {k}: max |diff| = {np.nanmax(np.abs(a - b)) if a.size else 0.0:.3e}, equal bits = {base[k].tobytes() == other[k].tobytes()}")
    for k in base:
        assert base[k].tobytes() == other[k].tobytes(), (what, k)


def learn(algo, iters, fused=True, graph=None, monkeypatch=None, callback=None):
    from core.common import off_policy_algorithm as opa

    if not fused:
        monkeypatch.setattr(opa, "HER_FUSED_COLLECT", False)
    model = make_model(algo)
    if graph is not None:
        model.enable_graph_capture(True, unroll=graph)
    model.learn(N_ENVS * (WARMUP_STEPS + iters), callback=callback)
    return model


_EAGER = {}


def eager_reference(algo, iters):
    """the eager run with the fused launch, computed once per (algorithm, length) and left unchanged"""
    if (algo, iters) not in _EAGER:
        model = learn(algo, iters)
        assert model.graph_status()["replays"] == 0 and model._n_updates == iters
        _EAGER[algo, iters] = snapshot(model)
    return _EAGER[algo, iters]


@pytest.mark.parametrize("algo", ["SAC", "TD3"])
def test_fused_collect_equals_elementwise_in_learn(ops, algo, monkeypatch):
    """Warm-up (host-drawn uniform actions, squashed = 0) and ten training iterations with CSTR_HER_FUSED_COLLECT at 1 and at 0."""
    base = eager_reference(algo, 10)
    model = learn(algo, 10, fused=False, monkeypatch=monkeypatch)
    assert model._n_updates == 10 and hasattr(model, "_ep_len") and (algo == "SAC" or type(model.action_noise).__name__ == "LegacyStreamNormalActionNoise")
    assert_same_state(base, snapshot(model), f"{algo} element-wise")
    assert base["counters"][0] > 0 and (base["ep_length"] > 0).any()


GRAPH_ITERS = 56


@pytest.mark.parametrize("algo", ["SAC", "TD3"])
@pytest.mark.parametrize("unroll", [1, 4])
def test_graph_replay_equals_eager(ops, algo, unroll):
    base = eager_reference(algo, GRAPH_ITERS)
    model = learn(algo, GRAPH_ITERS, graph=unroll)
    st = model.graph_status()
    print(f"{algo} unroll {unroll}: replays {st['replays']}, eager iterations {st['eager_iterations']}, graphs {st['graphs']}, "
          f"launches per iteration {st['abi_launches_per_iteration']}")
    assert st["active"] and st["error"] is None and st["replays"] > 0 and st["replays"] + st["eager_iterations"] == WARMUP_STEPS + GRAPH_ITERS
    assert model._her_checked and st["abi_launches_per_iteration"]
    assert_same_state(base, snapshot(model), f"{algo} unroll {unroll}")


def test_elementwise_collect_is_never_replayed(ops, monkeypatch):
    from core.common import off_policy_algorithm as opa

    monkeypatch.setattr(opa, "HER_FUSED_COLLECT", False)
    model = make_model("SAC")
    model.enable_graph_capture(True)
    model.learn(N_ENVS * (WARMUP_STEPS + 12))
    st = model.graph_status()
    assert st["replays"] == 0 and st["graphs"] == 0 and st["error"] is None and st["eager_iterations"] == WARMUP_STEPS + 12 and model._n_updates == 12


def test_replay_waits_for_the_one_time_episode_check(ops):
    """No episode has ended when training starts: the eager iteration that checks raises the reference's error, replay or not."""
    import core
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    env = CSTRVecEnv(2, device=DEV, goal_conditioned=True)  # 400-step episodes
    model = core.SAC("MultiInputPolicy", env, seed=0, replay_buffer_class=HerReplayBuffer, device=DEV, buffer_size=64, learning_starts=4, batch_size=8,
                     policy_kwargs=dict(net_arch=[16, 16]))
    model.enable_graph_capture(True)
    with pytest.raises(RuntimeError, match="Unable to sample before the end of the first episode"):
        model.learn(2 * 8)
    assert model.graph_status()["replays"] == 0


def test_eval_callback_and_checkpoint_under_replay(ops, tmp_path):
    """SAC under replay with EvalCallback(eval_freq=11, fused=None) and CheckpointCallback(save_freq=20, with the replay buffer): the
    training state and evaluations.npz of the eager run, one eager iteration per event; a checkpoint saved mid-run loads and continues."""
    import core
    from core import _native as nv
    from core.common.callbacks import CheckpointCallback, EvalCallback
    from core.common.graph_replay import GRAPH_WARMUP_ITERATIONS
    from core.common.vec_env import CSTRVecEnv

    def run(mode):
        ev_env = CSTRVecEnv(4, device=DEV, goal_conditioned=True, goal_range=(0.10, 0.40))
        ev_env.coef = nv.default_coef(0.20, 0.05, 0.45, 7)
        ev_env.seed(21)
        d = tmp_path / mode
        ev = EvalCallback(ev_env, n_eval_episodes=3, eval_freq=11, log_path=str(d / "log"), verbose=0, warn=False)
        ck = CheckpointCallback(save_freq=20, save_path=str(d / "ck"), name_prefix="m", save_replay_buffer=True)
        model = learn("SAC", GRAPH_ITERS, graph=None if mode == "eager" else 1, callback=[ev, ck])
        return model, snapshot(model), dict(np.load(d / "log" / "evaluations.npz")), ev, ck, sorted(os.listdir(d / "ck"))

    m0, base, e0, ev0, ck0, files0 = run("eager")
    m1, state, e1, ev1, ck1, files1 = run("graph")
    assert_same_state(base, state, "SAC with callbacks under replay")
    calls = WARMUP_STEPS + GRAPH_ITERS
    assert sorted(e0) == sorted(e1) == ["ep_lengths", "results", "timesteps"] and all(e0[k].tobytes() == e1[k].tobytes() and e0[k].shape == e1[k].shape for k in e0)
    assert e0["timesteps"].tolist() == [11 * N_ENVS * k for k in range(1, calls // 11 + 1)] and e0["results"].shape[0] == calls // 11
    assert (ev1.n_calls, ck1.n_calls, files1) == (ev0.n_calls, ck0.n_calls, files0) and ev0.n_calls == calls
    st = m1.graph_status()
    events = len(set(range(11, calls + 1, 11)) | set(range(20, calls + 1, 20)))
    warm = sum(m1._graph_warm.values())
    print(f"replays {st['replays']}, eager iterations {st['eager_iterations']}, graphs {st['graphs']}, events {events}, warm-up {warm}, "
          f"launches per iteration {st['abi_launches_per_iteration']}")
    assert st["active"] and st["error"] is None and st["replays"] > 0 and st["replays"] + st["eager_iterations"] == calls
    assert warm <= GRAPH_WARMUP_ITERATIONS * (st["graphs"] + 1)
    # eager: the warm-up vec-steps, the iteration that makes the one-time episode check, the graphs' warm-up, one per event
    assert st["eager_iterations"] == WARMUP_STEPS + 1 + warm + events
    # a checkpoint written while iterations were being replayed
    t = 40 * N_ENVS
    assert f"m_{t}_steps.zip" in files1 and f"m_replay_buffer_{t}_steps.pkl" in files1
    env2 = CSTRVecEnv(N_ENVS, device=DEV, goal_conditioned=True, goal_range=(0.10, 0.40))
    env2.coef = nv.default_coef(0.20, 0.05, 0.45, 7)
    loaded = core.SAC.load(str(tmp_path / "graph" / "ck" / f"m_{t}_steps.zip"), env=env2, device=DEV)
    loaded.load_replay_buffer(str(tmp_path / "graph" / "ck" / f"m_replay_buffer_{t}_steps.pkl"), truncate_last_traj=False)
    assert loaded.num_timesteps == t and loaded.replay_buffer._adds == 40
    loaded.enable_graph_capture(True)
    loaded.learn(N_ENVS * 12, reset_num_timesteps=False)
    st2 = loaded.graph_status()
    assert loaded.num_timesteps == t + 12 * N_ENVS and loaded.replay_buffer._adds == 52 and st2["replays"] > 0 and st2["error"] is None
    assert all(bool(th.isfinite(p).all()) for p in loaded.policy.parameters())


# ---- 4. it still learns --------------------------------------------------------------------------------------------------------------------
def test_sac_her_learns_setpoint_tracking_under_replay(ops):
    """tests/test_her.py::test_sac_her_learns_setpoint_tracking with the iterations replayed from hipGraphs: the same sizes, the same
    criterion (the mean evaluation reward over 16 fixed targets ends above the untrained policy's)."""
    import core
    from core.common.evaluation import evaluate_policy
    from core.common.vec_env import CSTRVecEnv
    from core.her import HerReplayBuffer

    n = 64
    env = CSTRVecEnv(n, device=DEV, goal_conditioned=True, goal_range=(0.10, 0.40))
    model = core.SAC("MultiInputPolicy", env, seed=0, replay_buffer_class=HerReplayBuffer, device=DEV, buffer_size=n * 1024, learning_starts=n * 410)
    model.enable_graph_capture(True)
    ev = CSTRVecEnv(16, device=DEV, goal_conditioned=True)
    ev.coef = env.coef
    targets = np.linspace(0.10, 0.40, 16).astype(np.float32)

    def evaluate():  # evaluate_policy resets the env: targets are set after its reset through a reset hook of the test
        orig = ev.reset_device

        def reset_then_targets():
            out = orig()
            ev.set_targets(targets)
            return out

        ev.reset_device = reset_then_targets
        try:
            ev.seed(123)
            return evaluate_policy(model, ev, n_eval_episodes=16, warn=False)[0]
        finally:
            ev.reset_device = orig

    before = evaluate()
    model.learn(n * 4000)
    after = evaluate()
    st = model.graph_status()
    print(f"SAC + HER under replay, mean evaluation reward over 16 fixed targets: untrained {before:.2f}, trained {after:.2f}; "
          f"replays {st['replays']}, eager iterations {st['eager_iterations']}")
    assert st["replays"] > 3000 and st["error"] is None
    assert model._n_updates == 4000 - 410 and after > before, (before, after)
