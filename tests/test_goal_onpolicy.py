"""GPU checks of PPO and A2C on the goal face of the env ("MultiInputPolicy", DictRolloutBuffer).

Kernels (csrc/cstr_ppo.hip, the add and gather bodies instantiated on the 6-float row): cstr_goal_rollout_add_f32 and
cstr_goal_ppo_gather_f32 against the Box-face entry points run on a width-4 twin buffer with the same operands (every field but the
observations bit-identical), against the NumPy restatement of tests/test_goal_onpolicy_abi.py, with sentinel padding in front of and
behind every array. Then the classes against fixtures written by the unmodified reference (tests/golden/*_goal_*.npz,
tools/refharness/gen_golden.py --only ppo_goal,a2c_goal) with the assertions and bars of tests/test_ppo.py and tests/test_a2c.py,
the one-launch evaluation against the evaluate_policy loop, save / load, the switch between the device rollout and the host loop,
the refusals, and a short learning run."""
import warnings

import numpy as np
import pytest
import torch as th

from _parity_helpers import q_err
from test_a2c import check_step, rollout_arrays
from test_goal_onpolicy_abi import KEYS, add_numpy, gather_numpy
from test_ppo import ROLLOUT_FIELDS, check_train, scale_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = float(np.float32(12345.678))
PAD = 64
FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def dev(a, dtype=th.float32):
    return th.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


@pytest.fixture(scope="module")
def ops():
    from core.common import hip_ops

    return hip_ops


# ---- kernels ------------------------------------------------------------------------------------------------------------------
class Padded:
    """device arrays with PAD sentinel words in front of and behind each (256 bytes: the arrays keep their 16-byte alignment)"""

    def __init__(self):
        self.whole = {}

    def new(self, name, shape, dtype=th.float32, fill=None):
        n = int(np.prod(shape))
        sent = SENT if dtype in (th.float32, th.float64) else 123456789
        w = th.full((n + 2 * PAD,), sent, dtype=dtype, device=DEV)
        self.whole[name] = (w, n, sent)
        t = w[PAD:PAD + n].view(*shape)
        if fill is not None:
            t.copy_(th.as_tensor(np.ascontiguousarray(fill)).to(DEV, dtype).reshape(t.shape))
        return t

    def check(self):
        th.cuda.synchronize()
        for name, (w, n, sent) in self.whole.items():
            assert bool((w[:PAD] == sent).all()) and bool((w[PAD + n:] == sent).all()), f"{name}: the padding around the array was written"

    def snapshot(self):
        return {k: w.clone() for k, (w, _, _) in self.whole.items()}

    def same_as(self, snap):
        for k, (w, _, _) in self.whole.items():
            assert th.equal(w, snap[k]), f"{k}: differs from the snapshot"


class PaddedRollout:
    """what hip_ops' wrappers read of a DeviceRollout, over sentinel-padded arrays filled with 7.0"""

    def __init__(self, pad: Padded, tag: str, T: int, N: int, D: int, A: int, goal: bool):
        from core import _native as nv

        self.rows, self.n_envs, self.obs_dim, self.act_dim, self.goal = T, N, D, A, goal
        shapes = dict(observations=(T, N, D), actions=(T, N, A))
        for f in FIELDS:
            setattr(self, f, pad.new(f"{tag}/{f}", shapes.get(f, (T, N)), fill=np.full(shapes.get(f, (T, N)), 7.0, np.float32)))
        self.ctl = pad.new(f"{tag}/ctl", (4,), th.int64, fill=np.zeros(4, np.int64))
        self.c = nv.Rollout(*(getattr(self, f).data_ptr() for f in FIELDS), T, N, D, A)

    def host(self):
        return {f: getattr(self, f).cpu().numpy() for f in FIELDS}


@pytest.mark.parametrize("bootstrap", [True, False], ids=["bootstrap", "plain"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_goal_add_against_the_box_twin_and_numpy(ops, N, T, bootstrap):
    """T + 1 launches with IDENTICAL host arguments (the position is a device control word) on the goal buffer and on a width-4 twin
    that receives the rows' observation columns. Bit-identical: every non-observation field, ctl, ep_return / ep_len, the episode count
    and the sum of lengths. The f64 sum of returns is accumulated with atomics in an order the launch does not fix (header of
    csrc/cstr_ppo.hip): n f64 additions of values below 2^3 in magnitude differ between two orders by at most n * 2^-53 * sum|r|."""
    rng = np.random.default_rng(1000 * N + 10 * T + bootstrap)
    pad, gamma = Padded(), 0.99
    goal = PaddedRollout(pad, "goal", T, N, 6, 2, True)
    twin = PaddedRollout(pad, "twin", T, N, 4, 2, False)
    rows_h = rng.normal(size=(N, 6)).astype(np.float32)
    host = dict(act=rng.normal(size=(N, 2)), reward=rng.uniform(-8, 0, N), value=rng.normal(size=N), log_prob=rng.normal(size=N),
                tv=rng.normal(size=N), done=(rng.uniform(size=N) < 0.5))
    host = {k: np.asarray(v, np.float32) for k, v in host.items()}
    host["done"][0] = 1.0  # at least one episode ends, at N = 1 too
    host["timeout"] = ((rng.uniform(size=N) < 0.6) & (host["done"] > 0)).astype(np.float32)
    host["timeout"][0] = 1.0
    rows = pad.new("rows", (N, 6), fill=rows_h)
    obs4 = pad.new("obs4", (N, 4), fill=rows_h[:, 2:6])
    d = {k: pad.new(k, v.shape, fill=v) for k, v in host.items()}
    state = {}
    for tag in ("goal", "twin"):
        state[tag] = dict(start=pad.new(f"{tag}/start", (N,), fill=np.ones(N, np.float32)), ep_ret=pad.new(f"{tag}/ep_ret", (N,), fill=np.zeros(N, np.float32)),
                          ep_len=pad.new(f"{tag}/ep_len", (N,), th.int32, fill=np.zeros(N, np.int32)),
                          stats=pad.new(f"{tag}/stats", (4,), th.float64, fill=np.zeros(4)))
    tail = (d["timeout"], d["tv"]) if bootstrap else (None, None)

    def launch(tag):
        s = state[tag]
        if tag == "goal":
            ops.goal_rollout_add(goal, rows, d["act"], d["reward"], s["start"], d["value"], d["log_prob"], *tail, gamma, d["done"], s["ep_ret"],
                                 s["ep_len"], s["stats"])
        else:
            ops.rollout_add(twin, obs4, d["act"], d["reward"], s["start"], d["value"], d["log_prob"], *tail, gamma, d["done"], s["ep_ret"],
                            s["ep_len"], s["stats"])

    # the NumPy restatement alongside
    ref = {f: np.full(tuple(getattr(goal, f).shape), 7.0, np.float32) for f in FIELDS}
    r_ctl, r_start = [0, 0, 0, 0], np.ones(N, np.float32)
    r_ret, r_len, r_stats = np.zeros(N, np.float32), np.zeros(N, np.int32), np.zeros(4)
    for t in range(T):
        launch("goal"), launch("twin")
        add_numpy(ref, r_ctl, rows_h, host["act"], host["reward"], r_start, host["value"], host["log_prob"], host["timeout"] if bootstrap else None,
                  host["tv"] if bootstrap else None, gamma, host["done"], r_ret, r_len, r_stats)
    pad.check()
    assert goal.ctl.tolist() == twin.ctl.tolist() == r_ctl == [T, 1, 0, T]
    g_h, t_h = goal.host(), twin.host()
    for f in FIELDS[1:]:
        assert g_h[f].tobytes() == t_h[f].tobytes(), f            # bit-identical to the Box-face launch
        np.testing.assert_array_equal(g_h[f], ref[f], err_msg=f)   # and to the NumPy statement
    for t in range(T):
        assert g_h["observations"][t].tobytes() == rows_h.tobytes()  # stored rows are the input rows, bit for bit
        assert t_h["observations"][t].tobytes() == rows_h[:, 2:6].tobytes()
    want_rew = np.where(host["timeout"] != 0, host["reward"] + np.float32(gamma) * host["tv"], host["reward"]).astype(np.float32) if bootstrap else host["reward"]
    np.testing.assert_array_equal(g_h["rewards"][0], want_rew)
    assert bootstrap == (not np.array_equal(want_rew, host["reward"]))
    np.testing.assert_array_equal(g_h["episode_starts"][0], np.ones(N, np.float32))
    if T > 1:  # episode_start was overwritten with done after it was stored: the next row's episode starts
        np.testing.assert_array_equal(g_h["episode_starts"][1], host["done"])
    sg, st = state["goal"], state["twin"]
    assert th.equal(sg["start"], st["start"]) and th.equal(sg["start"], d["done"]) and np.array_equal(r_start, host["done"])
    assert th.equal(sg["ep_ret"], st["ep_ret"]) and th.equal(sg["ep_len"], st["ep_len"])
    np.testing.assert_array_equal(sg["ep_ret"].cpu().numpy(), r_ret), np.testing.assert_array_equal(sg["ep_len"].cpu().numpy(), r_len)
    a, b = sg["stats"].cpu().numpy(), st["stats"].cpu().numpy()
    n_done = int((host["done"] > 0).sum())
    assert a[0] == b[0] == r_stats[0] == T * n_done and a[2] == b[2] == r_stats[2] and a[3] == b[3] == 0.0
    slack = T * n_done * 2.0 ** -53 * float(np.abs(host["reward"]).sum()) * T
    assert abs(a[1] - b[1]) <= slack and abs(a[1] - r_stats[1]) <= slack and a[1] < 0
    # a full buffer takes no further row: nothing at all changes
    snap = pad.snapshot()
    launch("goal"), launch("twin")
    pad.check()
    pad.same_as(snap)


@pytest.mark.parametrize("B", [1, 12, 255, 256, 1030])
def test_goal_gather_against_the_box_twin_and_numpy(ops, B):
    T, N = 3, 65
    rng = np.random.default_rng(B)
    pad = Padded()
    goal = PaddedRollout(pad, "goal", T, N, 6, 2, True)
    twin = PaddedRollout(pad, "twin", T, N, 4, 2, False)
    host = {f: rng.normal(size=tuple(getattr(goal, f).shape)).astype(np.float32) for f in FIELDS}
    for f in FIELDS:
        getattr(goal, f).copy_(dev(host[f]))
        getattr(twin, f).copy_(dev(host[f][..., 2:6] if f == "observations" else host[f]))
    idx = rng.integers(0, T * N, B)
    if B >= 12:
        idx[:3] = idx[3]                       # repeated indices
        idx[5], idx[6], idx[7] = -5, T * N + 9, T * N  # out of range: clamped into the buffer
    else:
        idx[0] = T * N - 1                     # the last cell
    idx_d = pad.new("idx", (B,), th.int64, fill=idx.astype(np.int64))
    out = {tag: [pad.new(f"{tag}/out{k}", s) for k, s in enumerate(((B, 6 if tag == "goal" else 4), (B, 2), (B,), (B,), (B,), (B,)))]
           for tag in ("goal", "twin")}
    ops.goal_ppo_gather(goal, idx_d, *out["goal"])
    ops.ppo_gather(twin, idx_d, *out["twin"])
    pad.check()
    want = gather_numpy(host, idx)
    flat = host["observations"].swapaxes(0, 1).reshape(T * N, 6)
    assert out["goal"][0].cpu().numpy().tobytes() == flat[np.clip(idx, 0, T * N - 1)].tobytes() == np.ascontiguousarray(want[0]).tobytes()
    assert out["twin"][0].cpu().numpy().tobytes() == np.ascontiguousarray(want[0][:, 2:6]).tobytes()
    for k in range(1, 6):
        got = out["goal"][k].cpu().numpy()
        assert got.tobytes() == out["twin"][k].cpu().numpy().tobytes(), k
        np.testing.assert_array_equal(got.reshape(B, -1), np.asarray(want[k]).reshape(B, -1))
    snap = pad.snapshot()
    ops.goal_ppo_gather(goal, idx_d, *out["goal"])
    pad.check()
    pad.same_as(snap)  # a relaunch is bit-identical, the buffer itself untouched


# ---- the classes ----------------------------------------------------------------------------------------------------------------
def goal_env(n, **kw):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n, device=DEV, goal_conditioned=True, **kw)


def make_ppo(g, prefix="before", env=None, **kw):
    from core.ppo import PPO

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the truncated-minibatch warning
        model = PPO("MultiInputPolicy", goal_env(int(g["n_envs"])) if env is None else env, seed=int(g["seed"]), n_steps=int(g["n_steps"]),
                    batch_size=int(g["batch_size"]), n_epochs=int(g["n_epochs"]), learning_rate=float(g["learning_rate"]),
                    ent_coef=float(g["ent_coef"]), policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]]), device=DEV, **kw)
    with th.no_grad():
        for k, v in model.policy.state_dict().items():
            v.copy_(th.as_tensor(g[f"{prefix}/policy/{k}"]))
    return model


def make_a2c(g, prefix="before", **kw):
    from core.a2c import A2C

    model = A2C("MultiInputPolicy", goal_env(int(g["n_envs"])), seed=int(g["seed"]), n_steps=int(g["n_steps"]),
                learning_rate=float(g["learning_rate"]), ent_coef=float(g["ent_coef"]),
                policy_kwargs=dict(net_arch=[int(w) for w in g["net_arch"]]), device=DEV, **kw)
    with th.no_grad():
        for k, v in model.policy.state_dict().items():
            v.copy_(th.as_tensor(g[f"{prefix}/policy/{k}"]))
    return model


def inject(model, g):
    """the fixture's targets, initial observations and step counters, after _setup_learn's reset"""
    env = model.env
    assert env.set_targets(g["targets"])
    env.set_state(g["init_obs"][:, 2:6], g["init_steps"])
    np.testing.assert_array_equal(env.flat.cpu().numpy(), g["init_obs"])  # the flat rows, the desired goal's affine map included


def test_rollout_teacher_forced(golden):
    """tests/test_ppo.py::test_rollout_teacher_forced on the goal face: the `before/` weights, targets, initial rows and step
    counters injected, the recorded Normal draws forced. Truncations happen inside the 8 steps."""
    from core.common.buffers import DictRolloutBuffer
    from core.common.policies import MultiInputActorCriticPolicy

    g = golden("ppo_goal_train_kat_small.npz")
    model = make_ppo(g)
    assert isinstance(model.policy, MultiInputActorCriticPolicy) and type(model.rollout_buffer) is DictRolloutBuffer
    assert model.fused_learner and model._device_rollout()
    _, cb = model._setup_learn(int(g["n_envs"] * g["n_steps"]), None)
    inject(model, g)
    model._fast.eps_queue = [th.as_tensor(e) for e in g["eps"]]
    assert model.collect_rollouts(model.env, cb, model.rollout_buffer, int(g["n_steps"]))
    rb = model.rollout_buffer
    assert rb.full and rb.rb.ctl.tolist() == [int(g["n_steps"]), 1, 0, int(g["n_steps"])] and not model._fast.eps_queue
    np.testing.assert_array_equal(rb.episode_starts.cpu().numpy(), g["rollout/episode_starts"])
    assert g["rollout/episode_starts"][1:].sum() >= 2 and g["timeouts"].sum() >= 2  # the truncations are in the fixture
    assert scale_err(rb.rows, g["rollout/observations"]) < 1e-5
    for k, (a, b) in zip(KEYS, ((0, 1), (1, 2), (2, 6))):  # the reference's dict, as views of the rows
        assert rb.observations[k].data_ptr() == rb.rows.data_ptr() + 4 * a and tuple(rb.observations[k].shape) == (8, 4, b - a)
        assert scale_err(rb.observations[k], g["rollout/observations"][..., a:b]) < 1e-5, k
    np.testing.assert_array_equal(rb.rows[..., 1].cpu().numpy(), g["rollout/observations"][..., 1])  # fixed targets: the goals bit for bit
    for f in ("actions", "values", "log_probs", "rewards"):
        assert scale_err(getattr(rb, f), g[f"rollout/{f}"]) < 1e-5, f
    np.testing.assert_array_equal(model._denv._done.cpu().numpy(), g["dones"])
    for f in ("advantages", "returns"):  # the device GAE on the device rollout
        assert scale_err(getattr(rb, f), g[f"rollout/{f}"]) < 1e-5, f
    assert scale_err(model._last_obs, g["last_obs"]) < 1e-5 and tuple(model._last_obs.shape) == (4, 6)
    n_ep, ret_sum, len_sum, _ = model._ep_stats.cpu().tolist()
    assert n_ep == g["rollout/episode_starts"][1:].sum() + g["dones"].sum() and len_sum > 0 and ret_sum < 0


def dict_buffer(model, arrays, as_dict):
    from core.common.buffers import DictRolloutBuffer

    arrays = dict(arrays)
    if as_dict:
        rows = arrays["observations"]
        arrays["observations"] = {"achieved_goal": rows[..., 0:1], "desired_goal": rows[..., 1:2], "observation": rows[..., 2:6]}
    return DictRolloutBuffer.from_arrays(model.goal_space, model.action_space, DEV, gamma=model.gamma, gae_lambda=model.gae_lambda, **arrays)


def test_dict_rollout_buffer_views_from_arrays_and_samples(golden):
    g = golden("ppo_goal_train_kat_small.npz")
    model = make_ppo(g)
    arrays = {f: g[f"rollout/{f}"] for f in ROLLOUT_FIELDS}
    a, b = dict_buffer(model, arrays, True), dict_buffer(model, arrays, False)
    for buf in (a, b):
        assert buf.full and buf.pos == 8 and list(buf.observations) == list(KEYS) and buf.obs_shape == {"achieved_goal": (1,), "desired_goal": (1,), "observation": (4,)}
        np.testing.assert_array_equal(buf.rows.cpu().numpy(), g["rollout/observations"])
        for f in ROLLOUT_FIELDS[1:]:
            np.testing.assert_array_equal(getattr(buf, f).cpu().numpy().reshape(g[f"rollout/{f}"].shape), g[f"rollout/{f}"])
    a.rows[2, 1, 3] = 42.0  # the views alias the storage
    assert float(a.observations["observation"][2, 1, 1]) == 42.0
    perm = np.random.RandomState(0).permutation(32)
    b.forced_permutations = [perm]
    flat = g["rollout/observations"].swapaxes(0, 1).reshape(32, 6)
    seen = 0
    for mb in b.get(12):
        n = mb.actions.shape[0]
        part = perm[seen:seen + n]
        assert mb.rows.shape == (n, 6) and mb.observations["observation"].data_ptr() == mb.rows.data_ptr() + 8
        np.testing.assert_array_equal(mb.rows.cpu().numpy(), flat[part])
        np.testing.assert_array_equal(mb.observations["desired_goal"].cpu().numpy(), flat[part][:, 1:2])
        np.testing.assert_array_equal(mb.old_values.cpu().numpy(), g["rollout/values"].swapaxes(0, 1).reshape(32)[part])
        seen += n
    assert seen == 32
    # add() with dict observations (NumPy, as the host loop hands them over) and a full buffer's IndexError
    c = type(a)(2, model.goal_space, model.action_space, device=DEV, n_envs=4)
    obs = {k: g["rollout/observations"][0][:, s] for k, s in zip(KEYS, (slice(0, 1), slice(1, 2), slice(2, 6)))}
    z = np.zeros(4, np.float32)
    c.add(obs, g["rollout/actions"][0], z, np.ones(4, np.float32), z, z)
    c.add(g["rollout/observations"][1], g["rollout/actions"][1], z, z, z, z)  # flat rows are taken too
    np.testing.assert_array_equal(c.rows.cpu().numpy(), g["rollout/observations"][:2])
    with pytest.raises(IndexError, match="out of bounds"):
        c.add(obs, g["rollout/actions"][0], z, z, z, z)
    c.reset()
    assert c.pos == 0 and float(c.rows.abs().sum()) == 0.0 and c.rb.ctl.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
@pytest.mark.parametrize("name", ["small", "default"])
def test_ppo_train_teacher_forced(golden, name, path, monkeypatch):
    """tests/test_ppo.py::check_train with its bars unchanged, on the first layers at K = 6"""
    from core.common import fused

    g = golden(f"ppo_goal_train_kat_{name}.npz")
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    model = make_ppo(g)
    if path == "torch":
        model.fused_learner = False
    assert model.fused_learner == (path != "torch")
    model.rollout_buffer = dict_buffer(model, {f: g[f"rollout/{f}"] for f in ROLLOUT_FIELDS}, as_dict=name == "small")
    model.rollout_buffer.forced_permutations = [p for p in g["permutations"]]
    model.debug_capture = True
    model.train()
    check_train(model, g, path)
    if name == "small":
        assert [c["values"].shape[0] for c in model.last_train_minibatches] == [12, 12, 8] * 3
        assert any(float(g[f"mb{k}/scalars"][5]) > 0 for k in range(int(g["n_minibatches"])))


@pytest.mark.parametrize("path", ["fused", "rocblas", "torch"])
def test_a2c_train_teacher_forced_two_iterations(golden, path, monkeypatch):
    """tests/test_a2c.py::check_step with its bars unchanged; the kernel path evaluates the buffer's T * N flat rows in place"""
    from core.common import fused, hip_ops
    from core.common.arena import FlatRMSprop

    g = golden("a2c_goal_train_kat_small.npz")
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    model = make_a2c(g)
    if path == "torch":
        model.fused_learner = False
    assert model.fused_learner == (path != "torch") and isinstance(model.policy.optimizer, FlatRMSprop)
    gathers = []
    gather = hip_ops.goal_ppo_gather
    monkeypatch.setattr(hip_ops, "goal_ppo_gather", lambda *a: (gathers.append(1), gather(*a))[1])
    model.debug_capture = True
    total = int(g["iterations"]) * int(g["n_envs"]) * int(g["n_steps"])
    for it in range(int(g["iterations"])):
        model.rollout_buffer = dict_buffer(model, rollout_arrays(g, "", it), as_dict=it == 0)
        model.rollout_buffer.forced_permutations = [g[f"it{it}/permutation"]]
        model._update_current_progress_remaining((it + 1) * int(g["n_envs"]) * int(g["n_steps"]), total)
        model.train()
        assert not model.rollout_buffer.forced_permutations
        check_step(model, g, "", it, path, logger=True)
    assert len(gathers) == (2 if path == "torch" else 0)  # in place on the kernel path: no gather launch


def test_predict_matches_the_reference(golden):
    g, small = golden("ppo_goal_predict_kat.npz"), golden("ppo_goal_train_kat_small.npz")
    model = make_ppo({**{k: small[k] for k in small.files}, **{f"before/policy/{k[7:]}": g[k] for k in g.files if k.startswith("policy/")}})
    rows = g["rows"]
    obs = {"achieved_goal": rows[:, 0:1], "desired_goal": rows[:, 1:2], "observation": rows[:, 2:6]}
    for given in (obs, rows):
        act, state = model.predict(given, deterministic=True)
        assert state is None and act.shape == (16, 2) and act.dtype == np.float32 and scale_err(act, g["deterministic"]) < 1e-5
        model._fast.eps_queue.append(th.as_tensor(g["eps"]))
        act, _ = model.predict(given, deterministic=False)
        assert scale_err(act, g["sampled"]) < 1e-5 and np.abs(act).max() <= 1.0
    one, _ = model.predict({k: v[3] for k, v in obs.items()}, deterministic=True)
    assert one.shape == (2,) and scale_err(one, g["deterministic"][3]) < 1e-5
    with th.no_grad():
        values = model.policy.predict_values(dev(rows))
    assert values.shape == (16, 1) and q_err(values.cpu().numpy(), g["values"], "ppo_fused") < 1e-5
    a1, _ = model.predict(obs, deterministic=False)  # unforced: the Philox stream
    a2, _ = model.predict(obs, deterministic=False)
    assert not np.array_equal(a1, a2)


# ---- evaluation -------------------------------------------------------------------------------------------------------------------
GOAL_RANGE = (0.10, 0.40)


def short_goal_env(n, seed, **kw):
    from core.common.vec_env import CSTRVecEnv

    class ShortGoalEnv(CSTRVecEnv):
        max_steps = 7

    e = ShortGoalEnv(n, device=DEV, goal_conditioned=True, goal_range=GOAL_RANGE, goal_seed=5, **kw)
    e.seed(seed)
    return e


def onpolicy_model(algo, n=4, env=None, **kw):
    import core

    kw.setdefault("policy_kwargs", dict(net_arch=[32, 32]))
    if algo == "PPO":
        kw.setdefault("n_steps", 8), kw.setdefault("batch_size", 16), kw.setdefault("n_epochs", 2)
    return getattr(core, algo)("MultiInputPolicy", short_goal_env(n, 0) if env is None else env, seed=3, device=DEV, **kw)


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_one_launch_evaluation_against_the_loop(algo):
    """tests/test_goal_eval.py's comparison for the on-policy classes (head 1, no output activation, clipped): order and lengths equal,
    returns at its rtol = 1e-4, the env left as the loop leaves it; evaluate_goal_tracking reports the same episodes, from one launch."""
    from core.common.evaluation import evaluate_goal_tracking, evaluate_policy, evaluate_policy_fused, supported

    model = onpolicy_model(algo)
    with th.no_grad():  # away from the 0.01-gain initial head: some action means beyond the bounds (clipped), some inside
        rows = dev(np.random.default_rng(1).uniform(-1, 1, (64, 6)))
        model.policy.action_net.weight.mul_(1.0 / float(model._fast.mean(rows).abs().median()))  # the head is linear: median |mean| = 1
        probe = model._fast.mean(rows).abs()
    assert bool((probe > 1).any()) and bool((probe < 1).any())
    env, loop_env = short_goal_env(4, 9), short_goal_env(4, 9)
    assert supported(model, env) and not supported(model, env, deterministic=False)
    with pytest.warns(UserWarning, match="Monitor"):
        rets, lens = evaluate_policy_fused(model, env, n_eval_episodes=8, return_episode_rewards=True)
    rets_l, lens_l = evaluate_policy(model, loop_env, n_eval_episodes=8, return_episode_rewards=True, warn=False)
    a, b = np.asarray(rets, np.float64), np.asarray(rets_l, np.float64)
    print(f"{algo} goal face, launch against loop: largest relative difference of an episode return = {np.abs(a / b - 1.0).max():.3e}")
    assert len(rets) == 8 and lens == [int(v) for v in lens_l] == [7] * 8 and len(set(rets)) == 8
    np.testing.assert_allclose(a, b, rtol=1e-4)
    # the env state left behind is the loop's (8 episodes over 4 envs: every env runs two, so neither keeps stepping a finished env)
    assert env.episode.tolist() == loop_env.episode.tolist() == [3, 3, 3, 3] and env.step_count.tolist() == loop_env.step_count.tolist() == [0] * 4
    assert _bits(env.pcg_state.cpu().numpy()) == _bits(loop_env.pcg_state.cpu().numpy()) and th.equal(env.targets, loop_env.targets)
    assert th.equal(env.obs, loop_env.obs)  # fresh reset draws: no policy arithmetic in them
    assert th.equal(env.flat[:, 2:], loop_env.flat[:, 2:]) and th.equal(env.flat[:, 0], loop_env.flat[:, 0])
    out = evaluate_goal_tracking(model, short_goal_env(4, 9), n_eval_episodes=8, warn=False)
    assert set(out) == {"episode_rewards", "episode_lengths", "target", "final_error", "mean_abs_error"}
    assert out["episode_rewards"].tolist() == rets and out["episode_lengths"].tolist() == lens
    assert ((out["target"] >= 0.10 - 1e-6) & (out["target"] <= 0.40 + 1e-6)).all() and (out["mean_abs_error"] > 0).all()
    from core.common.vec_env import CSTRVecEnv

    for e in (CSTRVecEnv(4, device=DEV),):  # a goal-face model on an env without the face
        assert not supported(model, e)
        with pytest.raises(ValueError, match="evaluate_goal_tracking does not cover"):
            evaluate_goal_tracking(model, e, n_eval_episodes=2, warn=False)


@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_eval_callback_modes_leave_identical_training_state(algo, tmp_path):
    from core.common import evaluation
    from core.common.callbacks import EvalCallback

    got, state = {}, {}
    for fused in (None, False, True):
        model = onpolicy_model(algo, policy_kwargs=dict(net_arch=[16, 16]))
        ev = EvalCallback(short_goal_env(4, 21), n_eval_episodes=8, eval_freq=10, log_path=str(tmp_path / str(fused)), verbose=0, warn=False, fused=fused)
        assert evaluation.supported(model, ev.eval_env)
        model.learn(4 * 32, callback=ev)
        th.cuda.synchronize()
        env, rb = model.get_env().unwrapped, model.rollout_buffer
        got[fused] = np.load(tmp_path / str(fused) / "evaluations.npz")
        state[fused] = dict(weights=np.concatenate([p.detach().cpu().numpy().ravel() for p in model.policy.parameters()]),
                            rows=rb.rows.cpu().numpy(), actions=rb.actions.cpu().numpy(), rewards=rb.rewards.cpu().numpy(), ctl=rb.rb.ctl.cpu().numpy(),
                            env_obs=env.obs.cpu().numpy(), env_pcg=env.pcg_state.cpu().numpy(), env_targets=env.targets.cpu().numpy(),
                            env_episode=env.episode.cpu().numpy(), rng=model._rng_ctl.cpu().numpy())
        assert model._n_updates > 0 and ev.n_calls == model.num_timesteps // 4 >= 32
    for k in state[None]:
        assert _bits(state[None][k]) == _bits(state[False][k]) == _bits(state[True][k]), k
    for fused in (None, False, True):
        assert got[fused]["timesteps"].tolist() == [40, 80, 120] and got[fused]["ep_lengths"].tolist() == [[7] * 8] * 3
    np.testing.assert_allclose(got[None]["results"], got[False]["results"], rtol=1e-4)
    assert _bits(got[None]["results"]) == _bits(got[True]["results"]) and evaluation.FUSED_BY_DEFAULT  # fused=None took the launch


# ---- model plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_save_load_round_trip(algo, tmp_path):
    import core
    from core.common.vec_env import CSTRVecEnv

    cls = getattr(core, algo)
    model = onpolicy_model(algo, env=goal_env(4, goal_range=GOAL_RANGE))
    model.learn(4 * 16)
    path = str(tmp_path / "model.zip")
    model.save(path)
    loaded = cls.load(path, env=goal_env(4, goal_range=GOAL_RANGE), device=DEV)
    assert type(loaded.policy) is type(model.policy) and type(loaded.rollout_buffer).__name__ == "DictRolloutBuffer" and loaded.goal_space == model.goal_space
    for (k, a), (_, b) in zip(model.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(a, b), k
    assert loaded.policy.optimizer.step_count == model.policy.optimizer.step_count > 0 and loaded.num_timesteps == model.num_timesteps
    rows = np.random.default_rng(0).uniform(-1, 1, (5, 6)).astype(np.float32)
    np.testing.assert_array_equal(model.predict(rows, deterministic=True)[0], loaded.predict(rows, deterministic=True)[0])
    loaded.learn(4 * 8)
    with pytest.raises(ValueError, match="archive holds a model of the goal face"):
        cls.load(path, env=CSTRVecEnv(4, device=DEV), device=DEV)
    box = cls("MlpPolicy", CSTRVecEnv(4, device=DEV), seed=0, device=DEV, **(dict(n_steps=8, batch_size=16) if algo == "PPO" else {}))
    box_path = str(tmp_path / "box.zip")
    box.save(box_path)
    with pytest.raises(ValueError, match="the env has the goal face"):
        cls.load(box_path, env=goal_env(4), device=DEV)
    with pytest.raises(ValueError, match="Observation spaces do not match"):
        loaded.set_env(CSTRVecEnv(4, device=DEV))


@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_kernel_path_host_loop_switch_logger_keys_and_abi_calls(algo):
    """learn() on the kernel path (device rollout), then the host loop (dict observations through policy.obs_to_tensor, a dict
    terminal_observation), then the device rollout again; the logger keys; and train() makes as many ABI calls as on the Box face at
    the same shapes (add and gather are replaced one for one)."""
    import core
    from core import _native as nv
    from core.common.vec_env import CSTRVecEnv

    cls = getattr(core, algo)
    kw = dict(n_steps=8, batch_size=16, n_epochs=2) if algo == "PPO" else dict(n_steps=5)
    per_iter = 4 * kw["n_steps"]
    env = goal_env(4, goal_range=GOAL_RANGE)
    model = cls("MultiInputPolicy", env, seed=1, device=DEV, **kw)
    assert model.fused_learner and model._device_rollout()
    model.learn(per_iter * 2)
    env.step_count.fill_(397)  # truncations inside the host loop's rollout: the dict terminal_observation is bootstrapped
    model.fused_learner = False
    assert not model._device_rollout()
    model.learn(per_iter * 2, reset_num_timesteps=False)
    assert isinstance(model._last_obs, dict) and len(model.ep_info_buffer) > 0
    model.fused_learner = True
    assert model._device_rollout()
    model.learn(per_iter * 2, reset_num_timesteps=False, log_interval=1)
    th.cuda.synchronize()
    assert model.num_timesteps == per_iter * 6 and model._n_updates == (12 if algo == "PPO" else 6)
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
    keys = set(model.logger.last_dump) | set(model.logger.resolved())
    want = {"train/entropy_loss", "train/value_loss", "train/explained_variance", "train/std", "train/n_updates", "train/learning_rate",
            "time/iterations", "time/fps", "time/total_timesteps"}
    want |= {"train/policy_gradient_loss", "train/approx_kl", "train/clip_fraction", "train/loss", "train/clip_range"} if algo == "PPO" else {"train/policy_loss"}
    assert want <= keys, want - keys

    def train_calls(m):
        _, cb = m._setup_learn(per_iter, None)
        m.collect_rollouts(m.env, cb, m.rollout_buffer, m.n_steps)
        before = nv.ABI_CALLS[0]
        m.train()
        return nv.ABI_CALLS[0] - before

    box = cls("MlpPolicy", CSTRVecEnv(4, device=DEV), seed=1, device=DEV, **kw)
    n_goal, n_box = train_calls(cls("MultiInputPolicy", goal_env(4), seed=1, device=DEV, **kw)), train_calls(box)
    print(f"{algo} train(): {n_goal} ABI calls on the goal face, {n_box} on the Box face")
    assert n_goal == n_box > 0


def test_refusals(monkeypatch):
    import core
    from core.common import distributed as dist_util
    from core.common.buffers import RolloutBuffer
    from core.common.vec_env import CSTRVecEnv, VecNormalize

    goal, box = goal_env(4), CSTRVecEnv(4, device=DEV)
    for name in ("PPO", "A2C"):
        cls = getattr(core, name)
        with pytest.raises(ValueError, match="does not support a Dict observation space.*MultiInputPolicy"):
            cls("MlpPolicy", goal, device=DEV)
        with pytest.raises(ValueError, match="MultiInputPolicy needs a Dict observation space"):
            cls("MultiInputPolicy", box, device=DEV)
        with pytest.raises(ValueError, match="does not support gSDE"):
            cls("MultiInputPolicy", goal, use_sde=True, device=DEV)
        model = cls("MultiInputPolicy", goal, device=DEV, **(dict(n_steps=8, batch_size=16) if name == "PPO" else {}))
        with pytest.raises(NotImplementedError, match="hipGraph"):
            model.enable_graph_capture(True)
        with pytest.raises(ValueError, match="Observation spaces do not match"):
            model.set_env(box)
        with monkeypatch.context() as m:
            m.setattr(dist_util, "rank_world", lambda: (0, 2))
            with pytest.raises(ValueError, match="does not run data-parallel"):
                cls("MultiInputPolicy", goal, device=DEV)
        # a Box-face buffer class on the face: its constructor refuses the Dict space
        with pytest.raises(ValueError, match="Unsupported space"):
            cls("MultiInputPolicy", goal, rollout_buffer_class=RolloutBuffer, device=DEV)
    with pytest.raises(ValueError, match="not built for the goal face"):
        VecNormalize(goal)
    with pytest.raises(ValueError, match="does not support a Dict observation space"):
        core.DQN("MlpPolicy", goal, device=DEV)
    with pytest.raises(ValueError, match="MultiInputPolicy unknown"):
        core.DQN("MultiInputPolicy", goal, device=DEV)
    for kw in (dict(discrete_actions=3), dict(multi_discrete_actions=(3, 5))):  # the discrete faces do not combine with the goal face
        with pytest.raises(ValueError, match="goal"):
            CSTRVecEnv(4, device=DEV, goal_conditioned=True, **kw)


# ---- learning ---------------------------------------------------------------------------------------------------------------------
def test_it_learns_to_track():
    """the pattern of tests/test_her.py's learning test: a short PPO run on redrawn setpoints ends with a lower mean |C2 - setpoint|
    on a fixed target set than the untrained policy"""
    from core.common.evaluation import evaluate_goal_tracking
    from core.ppo import PPO

    fixed = np.linspace(0.12, 0.38, 8).astype(np.float32)

    def score(model):
        env = goal_env(8)
        env.seed(1000)
        assert env.set_targets(fixed)
        out = evaluate_goal_tracking(model, env, n_eval_episodes=8, warn=False)
        np.testing.assert_allclose(np.sort(out["target"]), fixed, atol=1e-6)
        return float(out["mean_abs_error"].mean())

    model = PPO("MultiInputPolicy", goal_env(32, goal_range=GOAL_RANGE), n_steps=64, batch_size=512, n_epochs=10, learning_rate=1e-3, seed=0, device=DEV)
    assert model.fused_learner and model._device_rollout()
    before = score(model)
    model.learn(32 * 64 * 40)
    after = score(model)
    print(f"PPO goal face: mean |C2 - setpoint| before {before:.4f} mol/L, after {after:.4f} mol/L")
    assert np.isfinite(after) and after < before
