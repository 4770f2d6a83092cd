"""The three ARS entry points (csrc/cstr_ars.hip). CPU: cstr_ars_supported over the shape table and every BADARG / UNSUPPORTED
condition of the two launches through ctypes (argument checks run before anything is dereferenced or enqueued). GPU: the population
launch against the restatement of tests/_ars_reference.py (job model on the oracle env) and the update launch against its fp64 update.

Population launch: lengths, step_count, the reset-draw state (pcg_state, static_init) and the observations the last reset draw left
are compared exactly; every buffer sits between guard bands (tests/_sentinel_bufs.py) and idle slots must keep their bits.
Tolerance of `returns`: per case d = max over the candidates of |f32 restatement - fp64 restatement| (two references, never the
kernel); the kernel must be within max(4 d, 2e-6 |R64|) of the fp64 value R64 (4: a different but legal f32 summation order in up to
64-term dot products; 2e-6: the project's relative bar, for cases where the two restatements agree to the last bit). Each case prints
d, the kernel's worst distance and the bar before it asserts.
Update launch: theta within 1e-6 |want| + 1e-7 of the fp64 restatement, kept indices exact, step_size / return_std to 1e-12.

MEASURED on an MI355X (profiles/ars_probe.txt holds the same run). The two restatements agree to the last bit in 15 of the 16 cases
(the likely reason, not verified: their actions differ by units in the last place and the env's float32 valve map, 30 .. 250 L/min
from [-1, 1], rounds that away); where they differ (d = 1.2e-07) the kernel sits on the float32 one. The kernel equals the fp64 value bit for bit in 14 cases and is within
1.2e-07 in the other two, i.e. at most 0.006 of the bar. Case: d between the restatements | the kernel's worst |got - R64| | that
distance over the bar | the range of |R64|:
  ('lin', 'relu', 1, (4, 2), 'euler', 'random', 1, 1, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [0.2488, 10.98]
  ('lin', 'relu', 0, (8, 4), 'rk4', 'static', 2, 2, -1.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [34.52, 50.13]
  ('lin', 'relu', 1, (4, 2), 'euler', 'random', 7, 1, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [1.733, 11.39]
  ('linb', 'relu', 1, (8, 4), 'euler', 'random', 5, 1, -1.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [8.911, 16.37]
  ('linb', 'relu', 0, (4, 2), 'rk4', 'static', 7, 2, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [4.583, 11.81]
  ('linb', 'relu', 1, (8, 4), 'rk4', 'static', 1, 1, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [7.793, 15.1]
  ('h5', 'relu', 1, (4, 2), 'euler', 'static', 2, 2, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [4.43, 25.8]
  ('h5', 'tanh', 0, (8, 4), 'rk4', 'random', 1, 1, -1.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [12.47, 23.67]
  ('h5', 'tanh', 1, (4, 2), 'rk4', 'random', 7, 1, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [1.718, 4.102]
  ('h64_12', 'relu', 0, (4, 2), 'euler', 'random', 5, 2, -1.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [16.77, 27.08]
  ('h64_12', 'tanh', 1, (8, 4), 'rk4', 'static', 7, 1, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [4.111, 11.86]
  ('h64_12', 'relu', 1, (8, 4), 'euler', 'static', 1, 2, 0.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [6.561, 19.51]
  ('h64_64', 'relu', 1, (4, 2), 'rk4', 'random', 1, 2, -1.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [16.1, 26.72]
  ('h64_64', 'tanh', 0, (8, 4), 'euler', 'static', 5, 1, 0.0): d = 1.192e-07 | kernel 1.192e-07 | err / bar 0.006 | |R64| in [6.529, 11.04]
  ('h64_64', 'relu', 0, (8, 4), 'rk4', 'random', 7, 2, -1.0): d = 0.000e+00 | kernel 2.980e-08 | err / bar 0.001 | |R64| in [22.15, 35.65]
  ('h64_64', 'tanh', 1, (4, 2), 'euler', 'static', 2, 1, -1.0): d = 0.000e+00 | kernel 0.000e+00 | err / bar 0.000 | |R64| in [12.39, 15.75]
Update launch: worst error 0.055 of its bar over all cases; learn() (tests/test_ars.py): 0.043."""
import ctypes as C

import numpy as np
import pytest
import torch as th

import _ars_reference as ref
from core import _native as nv
from oracle import cstr_oracle as orc

DEV = "cuda:0"
ACT = {"relu": 1, "tanh": 2}
POLICIES = {"lin": ([], False), "linb": ([], True), "h5": ([5], True), "h64_12": ([64, 12], True), "h64_64": ([64, 64], True)}
N_DELTA, MAX_STEPS, SEED = 3, 7, 0x5EED0A25
# (policy, activation, squash, (obs_dim, act_dim), integrator, init_mode, n_envs, n_eval_episodes, alive_bonus_offset): every value of
# every factor with both mappings (a lane per slot: lin / linb; a wave per slot: the rest); n_envs = 7 > 6 jobs leaves slot 6 idle
CASES = [
    ("lin", "relu", 1, (4, 2), "euler", "random", 1, 1, 0.0),
    ("lin", "relu", 0, (8, 4), "rk4", "static", 2, 2, -1.0),
    ("lin", "relu", 1, (4, 2), "euler", "random", 7, 1, 0.0),
    ("linb", "relu", 1, (8, 4), "euler", "random", 5, 1, -1.0),
    ("linb", "relu", 0, (4, 2), "rk4", "static", 7, 2, 0.0),
    ("linb", "relu", 1, (8, 4), "rk4", "static", 1, 1, 0.0),
    ("h5", "relu", 1, (4, 2), "euler", "static", 2, 2, 0.0),
    ("h5", "tanh", 0, (8, 4), "rk4", "random", 1, 1, -1.0),
    ("h5", "tanh", 1, (4, 2), "rk4", "random", 7, 1, 0.0),
    ("h64_12", "relu", 0, (4, 2), "euler", "random", 5, 2, -1.0),
    ("h64_12", "tanh", 1, (8, 4), "rk4", "static", 7, 1, 0.0),
    ("h64_12", "relu", 1, (8, 4), "euler", "static", 1, 2, 0.0),
    ("h64_64", "relu", 1, (4, 2), "rk4", "random", 1, 2, -1.0),
    ("h64_64", "tanh", 0, (8, 4), "euler", "static", 5, 1, 0.0),
    ("h64_64", "relu", 0, (8, 4), "rk4", "random", 7, 2, -1.0),
    ("h64_64", "tanh", 1, (4, 2), "euler", "static", 2, 1, -1.0),
]


def _spec(pol, act, squash, lay):
    hidden, bias = POLICIES[pol]
    return dict(obs_dim=lay[0], act_dim=lay[1], hidden=hidden, act=act, with_bias=bias, squash=bool(squash))


# ---- CPU: the shape predicate and the refusals ------------------------------------------------------------------------------------

def test_supported_shape_table():
    f = nv.lib().cstr_ars_supported
    ok = lambda *a: f(*[C.c_int(int(v)) for v in a])  # noqa: E731  (obs, act, n_hidden, h1, h2, act, bias, squash, n_delta, n_top)
    for d, a in ((4, 2), (8, 2), (8, 4)):
        assert ok(d, a, 0, 0, 0, 1, 0, 1, 8, 8) == 1 and ok(d, a, 0, 0, 0, 0, 1, 0, 1, 1) == 1   # linear: the activation is ignored
        for h1, h2 in ((1, 1), (5, 64), (64, 12), (64, 64)):
            for act in (1, 2):
                assert ok(d, a, 1, h1, 0, act, 1, 1, 8, 4) == 1 and ok(d, a, 2, h1, h2, act, 0, 0, nv.ARS_MAX_DELTA, nv.ARS_MAX_DELTA) == 1
    for d, a in ((4, 4), (5, 2), (8, 3), (6, 2)):
        assert ok(d, a, 0, 0, 0, 1, 0, 1, 8, 8) == 0                                              # not a CSTR layout
    assert ok(4, 2, 3, 8, 8, 1, 1, 1, 8, 8) == 0 and ok(4, 2, -1, 8, 8, 1, 1, 1, 8, 8) == 0       # depth
    assert ok(4, 2, 1, 65, 0, 1, 1, 1, 8, 8) == 0 and ok(4, 2, 1, 0, 0, 1, 1, 1, 8, 8) == 0       # width
    assert ok(4, 2, 2, 64, 65, 1, 1, 1, 8, 8) == 0 and ok(4, 2, 2, 64, 0, 1, 1, 1, 8, 8) == 0
    assert ok(4, 2, 1, 8, 0, 0, 1, 1, 8, 8) == 0 and ok(4, 2, 1, 8, 0, 3, 1, 1, 8, 8) == 0         # hidden layers need ReLU or Tanh
    assert ok(4, 2, 1, 8, 0, 1, 2, 1, 8, 8) == 0 and ok(4, 2, 1, 8, 0, 1, 1, 2, 8, 8) == 0         # flags are 0 / 1
    assert ok(4, 2, 0, 0, 0, 1, 0, 1, 0, 0) == 0 and ok(4, 2, 0, 0, 0, 1, 0, 1, nv.ARS_MAX_DELTA + 1, 1) == 0
    assert ok(4, 2, 0, 0, 0, 1, 0, 1, 8, 9) == 0 and ok(4, 2, 0, 0, 0, 1, 0, 1, 8, 0) == 0         # n_top in 1 .. n_delta


def test_launches_refuse_bad_arguments_on_the_host():
    """every BADARG / UNSUPPORTED condition returns its code before anything is dereferenced or enqueued (the pointers are fakes)"""
    lib = nv.lib()
    null, coef = C.c_void_p(None), nv.default_coef()
    P = lambda a: C.c_void_p(a)  # noqa: E731
    lo, hi = (C.c_float * 4)(-1, -1, -1, -1), (C.c_float * 4)(1, 1, 1, 1)
    base = dict(pol=nv.ArsPolicy(4, 2, 2, 64, 64, 1, 1, 1), theta=P(0x10000), std=0.05, seed=1, upd=0, nd=3, ep=1, alive=0.0, coef=C.byref(coef),
                integ=0, obs=P(0x20000), step=P(0x30000), pcg=P(0x40000), static=null, lo=lo, hi=hi, n=4, ret=P(0x50000), lens=P(0x60000),
                stats=P(0x70000))

    def pop(**kw):
        a = dict(base, **kw)
        pol = a["pol"]
        return lib.cstr_ars_population_f32(null if pol is None else C.byref(pol), a["theta"], C.c_float(a["std"]), C.c_uint64(a["seed"]),
                                           C.c_int64(a["upd"]), C.c_int(a["nd"]), C.c_int(a["ep"]), C.c_double(a["alive"]), a["coef"],
                                           C.c_int(a["integ"]), a["obs"], a["step"], a["pcg"], a["static"], a["lo"], a["hi"], C.c_int64(a["n"]),
                                           a["ret"], a["lens"], a["stats"], null)

    for name in ("pol", "theta", "coef", "obs", "step", "pcg", "lo", "hi", "ret", "lens", "stats"):
        assert pop(**{name: None if name == "pol" else null}) == -1, name
    assert pop(n=0) == -1 and pop(nd=0) == -1 and pop(ep=0) == -1 and pop(std=0.0) == -1 and pop(std=-1.0) == -1 and pop(std=float("nan")) == -1
    assert pop(alive=float("nan")) == -1 and pop(upd=-1) == -1 and pop(upd=1 << 32) == -1
    assert pop(hi=(C.c_float * 4)(1, -1, 1, 1)) == -1                                              # act_high <= act_low
    for name, addr in (("obs", 0x20008), ("pcg", 0x40008), ("theta", 0x10002), ("step", 0x30002), ("lens", 0x60002), ("ret", 0x50004),
                       ("stats", 0x70004), ("static", 0x80004)):
        assert pop(**{name: P(addr)}) == -1, name                                                  # alignment
    assert pop(ret=P(0x10000)) == -1 and pop(lens=P(0x50010)) == -1 and pop(stats=P(0x20000)) == -1 and pop(static=P(0x40000)) == -1  # overlap
    for bad in (nv.ArsPolicy(5, 2, 0, 0, 0, 1, 0, 1), nv.ArsPolicy(4, 2, 3, 8, 8, 1, 1, 1), nv.ArsPolicy(4, 2, 1, 65, 0, 1, 1, 1),
                nv.ArsPolicy(4, 2, 2, 8, 0, 1, 1, 1), nv.ArsPolicy(4, 2, 1, 8, 0, 0, 1, 1), nv.ArsPolicy(4, 2, 1, 8, 0, 1, 1, 2)):
        assert pop(pol=bad) == -2
    assert pop(nd=nv.ARS_MAX_DELTA + 1, ret=P(0x100000), lens=P(0x200000)) == -2 and pop(integ=7) == -2

    def upd(theta=P(0x10000), n=36, ret=P(0x50000), nd=5, nt=2, lr=0.02, u=0, out=P(0x70000), kept=P(0x80000)):
        return lib.cstr_ars_update_f32(theta, C.c_int64(n), ret, C.c_int(nd), C.c_int(nt), C.c_double(lr), C.c_uint64(1), C.c_int64(u), out, kept, null)

    assert upd(theta=null) == -1 and upd(ret=null) == -1 and upd(out=null) == -1 and upd(kept=null) == -1
    assert upd(n=0) == -1 and upd(nd=0) == -1 and upd(nt=0) == -1 and upd(nt=6) == -1 and upd(u=-1) == -1 and upd(u=1 << 32) == -1
    assert upd(lr=float("nan")) == -1
    assert upd(theta=P(0x10002)) == -1 and upd(ret=P(0x50004)) == -1 and upd(out=P(0x70004)) == -1 and upd(kept=P(0x80002)) == -1
    assert upd(theta=P(0x50000)) == -1 and upd(out=P(0x50008)) == -1 and upd(kept=P(0x70008)) == -1  # overlap
    assert upd(nd=nv.ARS_MAX_DELTA + 1, nt=1) == -2 and upd(n=4997) == -2


# ---- GPU: the population launch ---------------------------------------------------------------------------------------------------

def _initial_state(rng, lay, n, init_mode):
    d, a = lay
    obs = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    step = rng.integers(0, MAX_STEPS, n).astype(np.int32)  # a job's reset draw zeroes it
    pcg = orc.pcg64_states_from_seeds(rng.integers(1, 2**31, n)).view(np.uint64).reshape(n, 4)
    static = None
    if init_mode == "static":
        static = np.tile(np.array(orc.STATIC_INIT_STATE), (n, a // 2)) + rng.uniform(-0.01, 0.01, (n, 2 * a)) * np.tile([1.0, 100.0, 1.0, 100.0], a // 2)
    return obs, step, pcg, static


def _launch(spec, theta, delta_std, n_eval, alive, integ, state, bufs=None):
    """one population launch on guarded copies of `state` -> (bufs, tensors)"""
    from _sentinel_bufs import GuardedBufs
    from core.common import hip_ops

    obs, step, pcg, static = state
    g = GuardedBufs(DEV)
    put_theta = g.put if np.isnan(theta).any() else g.put_ro  # (the read-only check compares values: NaN != NaN)
    t = dict(theta=put_theta("theta", theta), obs=g.put("obs", obs), step=g.put("step", step, dtype=th.int32),
             pcg=g.put("pcg", pcg.view(np.int64), dtype="uint64"), static=None if static is None else g.put("static", static, dtype=th.float64),
             returns=g.new("returns", 2 * N_DELTA, dtype=th.float64), lengths=g.new("lengths", 2 * N_DELTA, dtype=th.int32),
             stats=g.put("stats", np.zeros(4), dtype=th.float64))
    coef = nv.default_coef(0.20, 0.05, 0.45, MAX_STEPS)
    a = spec["act_dim"]
    hip_ops.ars_population(t["theta"], spec["hidden"], ACT[spec["act"]], spec["with_bias"], spec["squash"], delta_std, SEED, 2, N_DELTA, n_eval, alive,
                           coef, integ, t["obs"], t["step"], t["pcg"], [-1.0] * a, [1.0] * a, t["returns"], t["lengths"], t["stats"], static_init=t["static"])
    g.check(written=("returns", "lengths"))
    return g, t


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_population_launch_matches_the_restatement(case):
    pol, act, squash, lay, integ, init_mode, n, n_eval, alive = case
    spec = _spec(pol, act, squash, lay)
    rng = np.random.default_rng(CASES.index(case))
    theta = (rng.normal(size=ref.n_params(spec)) * 0.3).astype(np.float32)
    state = _initial_state(rng, lay, n, init_mode)
    coef = orc.default_coef(0.20, 0.05, 0.45, MAX_STEPS)
    args = (theta, spec, 0.05, SEED, 2, N_DELTA, n_eval, alive, coef, integ, state[0], state[1], state[2], state[3], [-1.0] * lay[1], [1.0] * lay[1])
    r64, r32 = ref.run_population(*args, np.float64), ref.run_population(*args, np.float32)
    g, t = _launch(spec, theta, 0.05, n_eval, alive, integ, state)
    got = t["returns"].cpu().numpy()
    d = float(np.abs(r32["returns"] - r64["returns"]).max())
    bar = np.maximum(4.0 * d, 2e-6 * np.abs(r64["returns"]))
    err = np.abs(got - r64["returns"])
    print(f"ARS population {case}: restatement distance d = {d:.3e}, kernel worst |got - R64| = {err.max():.3e}, worst err / bar = "
          f"{float((err / bar).max()):.3f}, |R64| in [{np.abs(r64['returns']).min():.4g}, {np.abs(r64['returns']).max():.4g}]")
    assert np.array_equal(r32["lengths"], r64["lengths"]) and np.array_equal(r32["pcg"], r64["pcg"])
    assert np.array_equal(t["lengths"].cpu().numpy(), r64["lengths"])
    assert np.array_equal(t["step"].cpu().numpy(), r64["step_count"])
    assert np.array_equal(t["pcg"].cpu().numpy().view(np.uint64), r64["pcg"])
    assert np.array_equal(t["obs"].cpu().numpy(), r64["obs"])  # what the last reset draw left (idle slots: what they held)
    if state[3] is not None:
        assert np.array_equal(t["static"].cpu().numpy(), r64["static_init"])
    for i in range(2 * N_DELTA, n):  # idle slots keep their bits
        assert np.array_equal(t["obs"].cpu().numpy()[i], state[0][i]) and t["step"].cpu().numpy()[i] == state[1][i]
        assert np.array_equal(t["pcg"].cpu().numpy().view(np.uint64)[i], state[2][i])
    stats = t["stats"].cpu().numpy()
    assert stats[0] == r64["lengths"].sum() and stats[2] == 0 and stats[3] == 0
    assert abs(stats[1] - got.sum()) <= 1e-12 * np.abs(got).sum()
    assert (err <= bar).all(), (err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("pol", ["linb", "h64_12"])
def test_population_relaunch_gives_the_same_bits(pol):
    spec = _spec(pol, "tanh", 1, (4, 2))
    rng = np.random.default_rng(5)
    theta = (rng.normal(size=ref.n_params(spec)) * 0.3).astype(np.float32)
    state = _initial_state(rng, (4, 2), 2, "static")
    g1, t1 = _launch(spec, theta, 0.05, 2, -1.0, "rk4", state)
    g2, t2 = _launch(spec, theta, 0.05, 2, -1.0, "rk4", state)
    for name in ("returns", "lengths", "stats", "obs", "step", "pcg", "static"):
        assert th.equal(t1[name], t2[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("pol", ["lin", "h5"])
def test_population_nan_policy_takes_the_env_nan_path(pol):
    """a NaN parameter: every action is NaN, every episode ends on its first step with -10 (the env's NaN path), and the job still
    draws its resets: the trip counts differ from a healthy job's and nothing waits for them"""
    spec = _spec(pol, "relu", 1, (4, 2))
    rng = np.random.default_rng(6)
    theta = np.full(ref.n_params(spec), np.nan, np.float32)
    state = _initial_state(rng, (4, 2), 2, "random")
    coef = orc.default_coef(0.20, 0.05, 0.45, MAX_STEPS)
    want = ref.run_population(theta, spec, 0.05, SEED, 2, N_DELTA, 2, -1.0, coef, "euler", *state, [-1.0, -1.0], [1.0, 1.0], np.float64)
    g, t = _launch(spec, theta, 0.05, 2, -1.0, "euler", state)
    assert np.array_equal(want["lengths"], np.full(2 * N_DELTA, 2)) and np.array_equal(want["returns"], np.full(2 * N_DELTA, -22.0))
    assert np.array_equal(t["lengths"].cpu().numpy(), want["lengths"]) and np.array_equal(t["returns"].cpu().numpy(), want["returns"])
    assert np.array_equal(t["pcg"].cpu().numpy().view(np.uint64), want["pcg"]) and np.array_equal(t["obs"].cpu().numpy(), want["obs"])


# ---- GPU: the update launch ---------------------------------------------------------------------------------------------------------

NAN = float("nan")
UPDATE_RETURNS = {
    "distinct": [-50.0, -42.5, -61.0, -40.0, -55.5, -49.0, -43.0, -60.0, -47.0, -58.0],
    "tie_across_k": [-40.0, -45.0, -40.0, -52.0, -40.0, -41.0, -40.0, -47.0, -40.0, -60.0],   # top = -40 for k = 0, 1, 2, 4: ties
    "minus_wins": [-60.0, -42.5, -61.0, -70.0, -55.5, -30.0, -43.0, -35.0, -47.0, -58.0],     # R- is the greater of the pair for k = 0, 2, 3
    "one_nan": [-50.0, -42.5, -61.0, -40.0, -55.5, -49.0, -43.0, NAN, -47.0, -58.0],           # direction 2 is kept first
    "all_equal": [-3.0] * 10,                                                                  # return_std = 0: step_size = lr / 1e-6
}


@pytest.mark.gpu
@pytest.mark.parametrize("n_params", [37, 1100])  # not a multiple of 4; more than one workgroup (256 threads x 4 parameters)
@pytest.mark.parametrize("n_top", [1, 2, 5])
@pytest.mark.parametrize("name", list(UPDATE_RETURNS))
def test_update_launch_matches_the_restatement(name, n_top, n_params):
    from _sentinel_bufs import GuardedBufs
    from core.common import hip_ops

    n_delta, lr, upd = 5, 0.02, 7
    rng = np.random.default_rng(n_params + n_top)
    theta0 = rng.normal(size=n_params).astype(np.float32)
    returns = np.array(UPDATE_RETURNS[name], np.float64)
    want, step, std, kept = ref.update(theta0, returns, n_delta, n_top, lr, ref.deltas(SEED, upd, n_delta, n_params))
    g = GuardedBufs(DEV)
    # (the read-only check compares values, NaN != NaN: the NaN case compares the bits itself below)
    theta = g.put("theta", theta0)
    ret = (g.put if name == "one_nan" else g.put_ro)("returns", returns, dtype=th.float64)
    out, kp = g.new("out", 2, dtype=th.float64), g.new("kept", n_top, dtype=th.int32)
    hip_ops.ars_update(theta, ret, n_delta, n_top, lr, SEED, upd, out, kp)
    g.check(written=("out", "kept"))
    got, o = theta.cpu().numpy().astype(np.float64), out.cpu().numpy()
    assert np.array_equal(ret.cpu().numpy().view(np.int64), returns.view(np.int64))  # the launch does not write its input
    assert np.array_equal(kp.cpu().numpy(), kept), (kp.cpu().numpy(), kept)
    if name == "one_nan" and 2 in kept:
        assert np.isnan(step) and np.isnan(o[0]) and np.isnan(o[1]) and np.isnan(got).all() and np.isnan(want).all()
        return
    if name == "all_equal":
        assert o[1] == 0.0 and o[0] == lr / 1e-6 and np.array_equal(got, theta0.astype(np.float64))
    assert abs(o[0] - step) <= 1e-12 * abs(step) and abs(o[1] - std) <= 1e-12 * abs(std) + 1e-300
    err, bar = np.abs(got - want), 1e-6 * np.abs(want) + 1e-7
    print(f"ARS update {name} n_top={n_top} P={n_params}: worst err / bar = {float((err / bar).max()):.3f}, step_size = {o[0]:.6g}")
    assert (err <= bar).all(), float((err / bar).max())
