"""TQC on the HIP learner (core/tqc, csrc/cstr_tqc.hip) against the fp64 statement of tests/_tqc_reference.py (RefTQC).

Teacher-forced learning: atoms and targets through `q_err` (tests/_parity_helpers.py), the row means of Z(s, a_pi) and the scalars at
1e-5 of their scale, the log-probs at tests/test_cql.py's log-prob bar, weights within 2e-5 of the tensor's scale + 1e-4 relative: the
bars tests/test_cql.py and tests/test_iql.py use for the same comparison. The runs start from output biases at the mean reward, as
theirs do and for the reason measured there: `q_err` asks 5e-8 of an untrained output of 0 +- 0.1, which the float32 torch statement
itself does not give. The float32 torch statement on the CPU (RefTQC in float32 against float64, three seeds, both configurations) is
at most 0.13 of the log-prob bar, 0.15 of the per-element target bar and 0.55 of the weight bar: no bar is widened. Each run prints
its worst error-to-bar ratios before it asserts. The two loss launches alone: tests/test_tqc_abi.py.

Measured on MI355X: atoms within 9e-8 of their scale on every path, targets within 1.1e-6, log-probs at most 0.14 of their bar, losses
and logged means within 1.4e-7; weights after the two steps at most 0.17 of their bar on the kernel paths (0.61 on the torch
statements, class defaults). A gradient step at the class defaults makes 26 ABI calls. 256 envs x 6000 replayed iterations move the
evaluation return from -319.8 to -167.2. Launches and times: profiles/tqc_probe.txt (tools/tqc_probe.py)."""
import hashlib

import numpy as np
import pytest
import torch as th

import _tqc_reference as ref
from _parity_helpers import q_err, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Training and eval env are not of the same type")]

DEV = "cuda"
MODS = ["actor", "critic", "critic_target"]


def _env(n=1, **kw):
    from core.common.vec_env import CSTRVecEnv

    return CSTRVecEnv(n, **kw)


def _short_env(n, seed):
    from core.common.vec_env import CSTRVecEnv

    class Short(CSTRVecEnv):
        max_steps = 20

    e = Short(n)
    e.seed(seed)
    return e


def _raw_dataset(rows=2048, seed=3):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-1, 1, (rows, 4)).astype(np.float32)
    nobs = np.clip(obs + rng.normal(0, 0.05, obs.shape), -1, 1).astype(np.float32)
    act = rng.uniform(-1, 1, (rows, 2)).astype(np.float32)
    rew = rng.uniform(-8, 0, rows).astype(np.float32)
    done = (rng.uniform(size=rows) < 0.1).astype(np.float32)
    return dict(observations=obs, next_observations=nobs, actions=act, rewards=rew, dones=done)


def _fill(rb, raw, sampler_seed=5):
    rows = raw["rewards"].shape[0]
    f = lambda a, *sh: th.as_tensor(np.asarray(a, np.float32)).reshape(*sh)  # noqa: E731
    rb.observations.copy_(f(raw["observations"], rows, 1, 4)), rb.next_observations.copy_(f(raw["next_observations"], rows, 1, 4))
    rb.actions.copy_(f(raw["actions"], rows, 1, 2)), rb.rewards.copy_(f(raw["rewards"], rows, 1)), rb.dones.copy_(f(raw["dones"], rows, 1))
    rb._adds = rows
    rb.ring.ctl[0], rb.ring.ctl[1] = 0, 1
    rb.seed_sampler(sampler_seed)


def _model(raw=None, arch=(32, 32), B=64, seed=0, **kw):
    """a TQC model on one env whose replay ring holds `raw`"""
    from core.tqc import TQC

    raw = _raw_dataset() if raw is None else raw
    pk = dict(kw.pop("policy_kwargs", {}))
    if arch is not None:
        pk.setdefault("net_arch", list(arch))
    model = TQC("MlpPolicy", _env(), seed=seed, batch_size=B, buffer_size=raw["rewards"].shape[0], policy_kwargs=pk, **kw)
    _fill(model.replay_buffer, raw)
    return model


def _select_path(monkeypatch, model, path):
    from core.common import fused

    assert model.fused_learner
    if path == "rocblas":
        monkeypatch.setattr(fused, "USE_FUSED_LINEAR", False)
    if path == "aten":
        model.fused_learner = False


def _ref_policy(model, arch):
    from core.common.spaces import Box
    from core.tqc.policies import TQCPolicy

    pk = {} if arch is None else dict(net_arch=list(arch))
    p = TQCPolicy(Box(-1, 1, (4,)), Box(-1, 1, (2,)), lambda _: 3e-4, **pk)
    p.load_state_dict({k: v.detach().cpu() for k, v in model.policy.state_dict().items()})
    return p.double()


# ------------------------------------------------------------------------------------ teacher-forced steps
@pytest.mark.parametrize("path", ["fused", "rocblas", "aten"])
@pytest.mark.parametrize("tag", ["small", "default"])
def test_tqc_teacher_forced(tag, path, monkeypatch):
    """Two consecutive steps on a seeded model ((32, 32) nets at batch 64, and the class defaults) on a fixed ring, the actor's noise
    forced (eps_queue), on the kernel path, on it with CSTR_FUSED_LINEAR=0 (rocBLAS GEMMs) and on the torch statements, against RefTQC
    in float64. ONE change is made to the model and the reference alike: the output biases of the critics and their targets start at
    the ring's mean reward (see the module docstring). Every path draws the same batches, bit for bit."""
    arch, B = ((32, 32), 64) if tag == "small" else (None, 256)
    raw = _raw_dataset()
    model = _model(raw, arch=arch, B=B)
    with th.no_grad():
        for critic in (model.critic, model.critic_target):
            for qnet in critic.q_networks:
                qnet[-1].bias.fill_(float(raw["rewards"].mean()))
    _select_path(monkeypatch, model, path)
    assert (model.top_quantiles_to_drop_per_net, model.n_critics, model.n_quantiles, model.n_target_quantiles) == (2, 2, 25, 46)
    assert (model.tau, model.gamma, model.lr_schedule(1), model.target_entropy) == (0.005, 0.99, 3e-4, -2.0) and float(model.log_ent_coef.detach()) == 0.0
    refm = ref.RefTQC(_ref_policy(model, arch), 3e-4, model.gamma, model.tau, 2, target_entropy=-2.0)
    index = {a.tobytes(): i for i, a in enumerate(raw["actions"])}
    model.debug_capture = True
    gen = th.Generator().manual_seed(11)
    lab = f"tqc_{tag}_{path}"
    rs = np.random.RandomState(5)  # the sampler's stream (seed_sampler(5)): every path draws NumPy's indices, so the same batches
    for k in range(2):
        eps_pi, eps_next = th.randn(B, 2, generator=gen), th.randn(B, 2, generator=gen)
        model.actor.action_dist.eps_queue = [eps_pi.clone(), eps_next.clone()]
        model.train(gradient_steps=1, batch_size=B)
        assert not model.actor.action_dist.eps_queue
        b = model._static_batch
        idx = np.array([index[r.tobytes()] for r in b.actions.cpu().numpy()])
        want_idx = rs.randint(0, raw["rewards"].shape[0], size=B)
        rs.randint(0, 1, size=B)
        np.testing.assert_array_equal(idx, want_idx)
        for name in ("observations", "actions", "next_observations", "rewards", "dones"):
            np.testing.assert_array_equal(getattr(b, name).cpu().numpy().reshape(B, -1), raw[name][idx].reshape(B, -1), err_msg=f"{lab} step {k} {name}")
        want = refm.step(raw["observations"][idx], raw["actions"][idx], raw["next_observations"][idx], raw["rewards"][idx], raw["dones"][idx],
                         eps_pi.numpy(), eps_next.numpy())
        t = {n: v.cpu().numpy().astype(np.float64) for n, v in model.last_train_tensors.items()}
        assert t["z"].shape == (B, 2, 25) and t["y"].shape == (B, 46)
        e_z, e_y = q_err(t["z"].reshape(-1), want["z"].reshape(-1), lab), q_err(t["y"].reshape(-1), want["y"].reshape(-1), lab)
        e_zm = rel_err(t["z_pi_mean"], want["z_pi_mean"], float(np.abs(want["z_pi_mean"]).mean()))
        # log-probs: tests/test_cql.py's bar: 1e-5 of max(|v|, mean|v|) plus what float32 can do to the tanh correction log(1 - a^2 + 1e-6)
        # of a nearly saturated action (a and a^2 carry 2^-23 between them, divided by 1 - a^2 + 1e-6; 4 x that). e_lp is error / bar * 1e-5.
        lp_bar = 1e-5 * np.maximum(np.abs(want["log_prob"]), np.abs(want["log_prob"]).mean()) + 4 * 2.0 ** -23 * (1.0 / (1 - want["a_pi"] ** 2 + 1e-6)).sum(axis=1)
        e_lp = 1e-5 * float((np.abs(t["log_prob"].reshape(-1) - want["log_prob"]) / lp_bar).max())
        one = lambda a: float(np.asarray(a).reshape(-1)[0])  # noqa: E731
        e_l = [rel_err(one(t["critic_loss"]), want["critic_loss"], 1e-3), rel_err(one(t["actor_loss"]), want["actor_loss"], 1e-3),
               rel_err(one(t["ent_coef"]), want["ent_coef"], 1e-3)]
        e_m = [rel_err(t["means"][0], want["target_mean"], 1e-3), rel_err(t["means"][1], want["atom_mean"], 1e-3)]
        lv = model.logger.name_to_value
        logged = [float(lv[f"train/{n}"]) for n in ("critic_loss", "actor_loss", "ent_coef", "target_mean", "atom_mean")]
        have = [one(t["critic_loss"]), one(t["actor_loss"]), one(t["ent_coef"]), t["means"][0], t["means"][1]]
        assert all(abs(a - g) <= 2 * np.spacing(np.float32(abs(g))) for a, g in zip(logged, have)), (logged, have)
        assert rel_err(float(lv["train/ent_coef_loss"]), want["ent_coef_loss"], 1e-3) < 1e-5
        line = (f"{lab} step {k}: error / 1e-5 of scale: z {e_z / 1e-5:.3f} y {e_y / 1e-5:.3f} z_pi_mean {e_zm / 1e-5:.3f} logp {e_lp / 1e-5:.3f} "
                f"critic_loss {e_l[0] / 1e-5:.3f} actor_loss {e_l[1] / 1e-5:.3f} ent_coef {e_l[2] / 1e-5:.3f} target_mean {e_m[0] / 1e-5:.3f} "
                f"atom_mean {e_m[1] / 1e-5:.3f}")
        print(line)
        assert e_z < 1e-5 and e_y < 1e-5 and e_zm < 1e-5 and e_lp < 1e-5 and max(e_l) < 1e-5 and max(e_m) < 1e-5, line
    assert model._n_updates == 2 and all(o.step_count == 2 for o in (model.actor.optimizer, model.critic.optimizer, model.ent_coef_optimizer))
    worst = 0.0
    for nm in MODS:
        wsd = getattr(refm.p, nm).state_dict()
        for k, v in getattr(model.policy, nm).state_dict().items():
            got, w = v.detach().cpu().numpy().astype(np.float64), wsd[k].numpy()
            scale = max(float(np.abs(w).max()), 1e-3)
            worst = max(worst, float((np.abs(got - w) / (2e-5 * scale + 1e-4 * np.abs(w))).max()))
    la, la_ref = float(model.log_ent_coef.detach()), float(refm.log_ent_coef.detach())
    e_ent = abs(la - la_ref) / (2e-5 * 1e-3 + 1e-4 * abs(la_ref))
    print(f"{lab}: weights of the three networks after 2 steps, worst err / (2e-5 scale + 1e-4 |w|) = {worst:.3f}; log_ent_coef {e_ent:.3f}")
    assert worst < 1.0 and e_ent < 1.0, (worst, e_ent)


# ------------------------------------------------------------------------------------ graph replay, allocations, launches, paths
def _digest(model, env):
    rb = model.replay_buffer
    h = hashlib.sha256()
    for t in [p.detach() for p in model.policy.parameters()] + [model.log_ent_coef.detach(), rb.observations, rb.next_observations, rb.actions, rb.rewards,
                                                                rb.dones, rb.sampler_stream, rb.ring.ctl, env.obs, env.step_count]:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("unroll", [1, 4])
def test_graph_replay_equals_eager(unroll):
    from core.tqc import TQC

    n, iters = 64, 41
    out = []
    for graph in (False, True):
        env = _env(n, device=DEV)
        model = TQC("MlpPolicy", env, seed=5, device=DEV, batch_size=64, learning_starts=n, buffer_size=n * 16, policy_kwargs=dict(net_arch=[32, 32]))
        model.enable_graph_capture(graph, unroll=unroll)
        model.learn(n * iters)
        th.cuda.synchronize()
        st = model.graph_status()
        assert model._n_updates == iters - 1 and model.fused_learner
        if graph:
            assert st["active"] and st["replays"] >= (16 if unroll == 1 else 4) and st["error"] is None, st
        else:
            assert st["replays"] == 0
        out.append(_digest(model, env))
    assert out[0] == out[1]


def test_nothing_is_allocated_after_the_second_step():
    model = _model(B=64)
    model.train(1, 64)
    model.train(1, 64)
    th.cuda.synchronize()
    ptrs = lambda: [t.data_ptr() for t in (model._gz, model._gz_pi, model._g_logp, model._target_y, model._z_pi_mean, model._tqc_ws,  # noqa: E731
                                           model._packed.x_data, model._packed.x_pn)]
    before, mem = ptrs(), th.cuda.memory_allocated()
    model.train(1, 64)
    th.cuda.synchronize()
    assert ptrs() == before and th.cuda.memory_allocated() == mem


# sample 1; actor pair pass 3; target critics 3, critics 3; critic loss 1; critic backward 3 + dW/db 1; critic Adam with the entropy step 1;
# critics on x_pi 3; actor loss 1; backward through the critics 3, through the actor 2 + dW/db 1; actor Adam with the soft update 1
STEP_ABI_CALLS = 26


def test_abi_calls_of_a_step_are_pinned(monkeypatch):
    """Every launching entry point reports through hip_ops' `check`: a recording wrapper sees a gradient step's calls in order. Exactly
    one of them is cstr_tqc_critic_loss_f32 (its two launches are one call) and one cstr_tqc_actor_loss_f32; the critic loss follows a
    forward launch and is followed by a backward launch; so is the actor loss. The count is pinned."""
    from core.common import hip_ops

    names = []
    orig = hip_ops.check

    def recording(rc, what):
        names.append(what)
        return orig(rc, what)

    model = _model(B=256, arch=None)
    model.train(1, 256)
    model.train(1, 256)
    monkeypatch.setattr(hip_ops, "check", recording)
    model.train(1, 256)
    first = list(names)
    names.clear()
    model.train(1, 256)
    print(f"ABI calls of one TQC gradient step at the class defaults: {len(names)}: " + " ".join(n.replace("cstr_", "").replace("_f32", "") for n in names))
    assert names == first and names.count("cstr_tqc_critic_loss_f32") == 1 and names.count("cstr_tqc_actor_loss_f32") == 1
    for loss in ("cstr_tqc_critic_loss_f32", "cstr_tqc_actor_loss_f32"):
        i = names.index(loss)
        assert "_fwd" in names[i - 1] and "_bwd" in names[i + 1], names
    assert len(names) == STEP_ABI_CALLS, len(names)


def test_path_selection(monkeypatch):
    from core.common import hip_ops

    calls = {}

    def counting(name):
        orig = getattr(hip_ops, name)

        def wrapped(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(hip_ops, name, wrapped)

    counting("tqc_critic_loss"), counting("tqc_actor_loss")
    model = _model()
    assert model.fused_learner and model._kernel_path() and model._chain_for(64) is None and type(model).chain_type is None
    model.train(gradient_steps=2, batch_size=64)
    assert calls == dict(tqc_critic_loss=2, tqc_actor_loss=2), calls
    calls.clear()
    model.fused_learner = False
    model.train(gradient_steps=2, batch_size=64)
    assert not calls and model._n_updates == 4
    # a non-default optimiser and more atoms than the launches take: the torch statements
    for extra in (dict(policy_kwargs=dict(optimizer_class=th.optim.AdamW)), dict(policy_kwargs=dict(n_quantiles=129)),
                  dict(policy_kwargs=dict(n_critics=17, n_quantiles=3), top_quantiles_to_drop_per_net=1)):
        calls.clear()
        m = _model(**extra)
        assert not m.fused_learner and not m._kernel_path(), extra
        m.debug_capture = True
        m.train(gradient_steps=2, batch_size=64)
        t = m.last_train_tensors
        assert not calls and m._n_updates == 2 and t["z"].shape == (64, m.n_critics, m.n_quantiles) and t["y"].shape == (64, m.n_target_quantiles)
        assert all(bool(th.isfinite(t[n]).all()) for n in t)
    # what the launches do take: one critic, five, the cap, a constant entropy coefficient, several steps per call, a slower soft update
    for kw in (dict(policy_kwargs=dict(n_critics=1, n_quantiles=7)), dict(policy_kwargs=dict(n_critics=5)), dict(policy_kwargs=dict(n_critics=16, n_quantiles=16),
               top_quantiles_to_drop_per_net=3), dict(ent_coef=0.2), dict(gradient_steps=3), dict(target_update_interval=2, top_quantiles_to_drop_per_net=0)):
        m = _model(**kw)
        calls.clear()
        m.train(gradient_steps=m.gradient_steps, batch_size=64)
        assert m.fused_learner and calls == dict(tqc_critic_loss=m.gradient_steps, tqc_actor_loss=m.gradient_steps), (kw, calls)
        assert np.isfinite(m._loss_sum_buf.cpu().numpy()).all() and all(bool(th.isfinite(p).all()) for p in m.policy.parameters())


# ------------------------------------------------------------------------------------ learn(), predict, checkpoints
class _Dumps:
    def __init__(self):
        self.rows = []

    def write(self, vals, excluded, step):
        self.rows.append((step, dict(vals)))


def test_online_learn_counters_and_logger_keys():
    """learn() on 64 device envs through SAC's one-launch rollout, replayed from a hipGraph"""
    from core.common.logger import Logger
    from core.tqc import TQC

    n = 64
    model = TQC("MlpPolicy", _short_env(n, 3), seed=0, batch_size=64, learning_starts=n, buffer_size=n * 64, policy_kwargs=dict(net_arch=[64, 64]))
    assert model._use_packed_batch()
    model.stats_sync_interval = 10
    dumps = _Dumps()
    model.set_logger(Logger(output_formats=[dumps]))
    model.enable_graph_capture(True)
    assert model.learn(n * 60, log_interval=4) is model
    th.cuda.synchronize()
    st = model.graph_status()
    assert model.num_timesteps == n * 60 and model._n_updates == 59 and model.replay_buffer._adds == 60
    assert st["active"] and st["replays"] > 0 and st["error"] is None, st
    assert all(o.step_count == 59 for o in (model.actor.optimizer, model.critic.optimizer, model.ent_coef_optimizer))
    want = {"train/n_updates", "train/ent_coef", "train/actor_loss", "train/critic_loss", "train/ent_coef_loss", "train/target_mean", "train/atom_mean",
            "rollout/ep_rew_mean", "rollout/ep_len_mean", "time/fps", "time/total_timesteps"}
    assert dumps.rows
    for step, row in dumps.rows:
        assert want <= set(row), (step, sorted(want - set(row)))
        assert all(np.isfinite(float(row[k])) for k in want) and row["rollout/ep_len_mean"] == 20.0
        assert float(row["train/critic_loss"]) > 0 and float(row["train/ent_coef"]) > 0
    # above 1024 envs the rollout is SAC's ONE launch (policy network + collect step + replay index draw): it takes a TQC model
    wide = TQC("MlpPolicy", _env(2048), seed=0, batch_size=64, learning_starts=2048, buffer_size=2048 * 8, policy_kwargs=dict(net_arch=[64, 64]))
    wide.enable_graph_capture(True)
    wide.learn(2048 * 12)
    th.cuda.synchronize()
    st = wide.graph_status()
    assert wide._rollout_net() is not None and st["active"] and st["replays"] > 0 and st["error"] is None and wide._n_updates == 11
    assert all(bool(th.isfinite(p).all()) for p in wide.policy.parameters())


def test_predict_is_sacs():
    model = _model()
    model.train(4, 64)
    obs = np.random.default_rng(0).uniform(-1, 1, (7, 4)).astype(np.float32)
    act, state = model.predict(obs, deterministic=True)
    assert state is None and act.shape == (7, 2)
    with th.no_grad():
        want = model.policy.unscale_action(model.actor(th.as_tensor(obs, device=DEV), deterministic=True).cpu().numpy())
    np.testing.assert_array_equal(act, np.clip(want, model.action_space.low, model.action_space.high))
    a1, a2 = model.predict(obs)[0], model.predict(obs)[0]
    assert a1.shape == (7, 2) and not np.array_equal(a1, a2)  # stochastic by default, as SAC


def test_state_dict_keys_and_arenas():
    model = _model(policy_kwargs=dict(n_critics=3, n_quantiles=13))
    sd = model.policy.state_dict()
    want = [f"{c}.qf{i}.{l}.{p}" for c in ("critic", "critic_target") for i in range(3) for l in (0, 2, 4) for p in ("weight", "bias")]
    assert set(want) <= set(sd) and tuple(sd["critic.qf2.4.weight"].shape) == (13, 32) and not any("qf3" in k for k in sd)
    assert {"actor.mu.weight", "actor.log_std.bias", "actor.latent_pi.0.weight"} <= set(sd)
    pol = model.policy
    assert pol.critic.quantiles_nets is pol.critic.q_networks and len(pol.critic_stack) == 3
    w, wg, b, bg = pol.critic_stack[-1]
    assert tuple(w.shape) == (3, 13, 32) and tuple(b.shape) == (3, 13) and wg is not None and bg is not None
    assert w.data_ptr() == pol.critic.qf0[4].weight.data_ptr()  # the stacked views alias the modules' parameters


def test_checkpoint_round_trip_continues_identically(tmp_path):
    import json
    import zipfile

    from core.tqc import TQC

    raw = _raw_dataset()
    model = _model(raw, top_quantiles_to_drop_per_net=3, policy_kwargs=dict(n_quantiles=13, n_critics=3))
    model.train(5, 64)
    path = str(tmp_path / "tqc_ckpt")
    model.save(path)
    with zipfile.ZipFile(path + ".zip") as z:
        assert {"data", "policy.pth", "actor.optimizer.pth", "critic.optimizer.pth", "ent_coef_optimizer.pth"} <= set(z.namelist())
        data = json.loads(z.read("data"))
    assert data["top_quantiles_to_drop_per_net"] == 3
    clone = TQC.load(path, env=_env())
    assert clone._n_updates == 5 and clone.fused_learner and clone.top_quantiles_to_drop_per_net == 3
    assert (clone.n_critics, clone.n_quantiles, clone.n_target_quantiles) == (3, 13, 30)
    _fill(clone.replay_buffer, raw)
    assert list(model.policy.state_dict()) == list(clone.policy.state_dict())
    for a, b in zip(model.policy.state_dict().values(), clone.policy.state_dict().values()):
        assert th.equal(a, b)
    assert th.equal(model.log_ent_coef, clone.log_ent_coef)
    for o, c in ((model.actor.optimizer, clone.actor.optimizer), (model.critic.optimizer, clone.critic.optimizer),
                 (model.ent_coef_optimizer, clone.ent_coef_optimizer)):
        assert o.step_count == c.step_count and th.equal(o.exp_avg, c.exp_avg) and th.equal(o.exp_avg_sq, c.exp_avg_sq)
    obs = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(model.predict(obs, deterministic=True)[0], clone.predict(obs, deterministic=True)[0])
    outs = []
    for m in (model, clone):
        m.set_random_seed(7)
        m.replay_buffer.seed_sampler(99)
        m.train(gradient_steps=3, batch_size=64)
        outs.append([p.detach().clone() for p in m.policy.parameters()] + [m.log_ent_coef.detach().clone()])
    for a, b in zip(*outs):
        assert th.equal(a, b)


def test_every_refusal():
    from core.common import distributed as dist_util
    from core.common.vec_env import VecNormalize
    from core.her import HerReplayBuffer
    from core.tqc import TQC

    with pytest.raises(ValueError, match="VecNormalize"):
        TQC("MlpPolicy", VecNormalize(_env()))
    with pytest.raises(ValueError, match="does not support a Dict observation space"):
        TQC("MlpPolicy", _env(goal_conditioned=True, goal_range=(0.10, 0.40)))
    with pytest.raises(ValueError, match="HerReplayBuffer"):
        TQC("MlpPolicy", _env(), replay_buffer_class=HerReplayBuffer)
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        TQC("MlpPolicy", _env(discrete_actions=3))
    with pytest.raises(AssertionError, match="The algorithm only supports"):
        TQC("MlpPolicy", _env(multi_discrete_actions=(3, 5)))
    with pytest.raises(ValueError, match="does not support gSDE"):
        TQC("MlpPolicy", _env(), use_sde=True)
    with pytest.raises(ValueError, match="does not support gSDE"):
        TQC("MlpPolicy", _env(), policy_kwargs=dict(use_sde=True))
    with pytest.raises(ValueError, match="MultiInputPolicy"):
        TQC("MultiInputPolicy", _env())
    orig = dist_util.rank_world
    try:
        dist_util.rank_world = lambda: (0, 2)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            TQC("MlpPolicy", _env())
    finally:
        dist_util.rank_world = orig
    for kw, msg in ((dict(policy_kwargs=dict(n_quantiles=0)), "n_quantiles"), (dict(top_quantiles_to_drop_per_net=-1), "negative"),
                    (dict(top_quantiles_to_drop_per_net=25), "drops every atom"),
                    (dict(top_quantiles_to_drop_per_net=7, policy_kwargs=dict(n_quantiles=7)), "drops every atom")):
        with pytest.raises(ValueError, match=msg):
            TQC("MlpPolicy", _env(), **kw)
    m = TQC("MlpPolicy", _env(), top_quantiles_to_drop_per_net=24, policy_kwargs=dict(net_arch=[32, 32]))  # one atom per critic is left
    assert m.n_target_quantiles == 2 and m.fused_learner


# ------------------------------------------------------------------------------------ evaluation, collection
def test_fused_evaluation_and_collection_take_a_tqc_model():
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused, evaluate_trajectories, supported
    from core.common.offline_dataset import collect_offline_dataset
    from core.sac import SAC

    def both_ways(m):
        loop = evaluate_policy(m, _short_env(4, 21), n_eval_episodes=8, return_episode_rewards=True, warn=False)
        fused = evaluate_policy_fused(m, _short_env(4, 21), n_eval_episodes=8, return_episode_rewards=True, warn=False)
        assert len(loop[0]) == len(fused[0]) == 8 and loop[1] == fused[1] and all(n == 20 for n in fused[1])
        return np.asarray(loop[0], np.float64), np.asarray(fused[0], np.float64)

    # the bar: 4 x what a plain SAC model of the same shape and seed shows between the two evaluations, floor one ulp of a step reward per step
    loop, fused = both_ways(SAC("MlpPolicy", _env(1), seed=0, policy_kwargs=dict(net_arch=[32, 32])))
    d0 = max(float(np.abs(loop - fused).max()), 20 * float(np.spacing(np.float32(np.abs(loop).max() / 20))))
    model = _model()
    model.train(4, 64)
    assert supported(model, _short_env(4, 21))
    loop, fused = both_ways(model)
    print(f"TQC (32, 32): worst |fused - loop| return {float(np.abs(loop - fused).max()):.3e}, bar {4 * d0:.3e}")
    assert float(np.abs(loop - fused).max()) <= 4 * d0
    tr = evaluate_trajectories(model, _short_env(4, 3), n_eval_episodes=4)
    rets, lens = evaluate_policy_fused(model, _short_env(4, 3), n_eval_episodes=4, return_episode_rewards=True, warn=False)
    assert tr["states"].shape == (4, 20, 4) and list(tr["episode_lengths"]) == lens
    np.testing.assert_allclose(tr["episode_rewards"], rets, rtol=1e-6)
    rb, stats = collect_offline_dataset(model, _short_env(8, 5), num_episodes=16, random_action_prob=0.2, seed=1)
    assert rb.size() == 40 and rb.n_envs == 8 and stats["num_episodes"] >= 16
    from twoseriescstr import evaluate_model

    ep_rewards, ep_states = evaluate_model(model, _short_env(4, 3), num_episodes=4, plot=False)
    assert len(ep_rewards) == 4 and np.asarray(ep_states).shape == (4, 20, 4) and np.isfinite(ep_rewards).all()
    from core.tqc import TQC

    online = TQC("MlpPolicy", _short_env(8, 2), seed=0, batch_size=32, learning_starts=8, buffer_size=8 * 64, policy_kwargs=dict(net_arch=[32, 32]))
    ev = EvalCallback(_short_env(4, 7), n_eval_episodes=4, eval_freq=5, verbose=0, warn=False)
    online.learn(8 * 10, callback=ev)
    assert ev.n_calls == 10 and np.isfinite(ev.last_mean_reward)


# ------------------------------------------------------------------------------------ a learning run
def test_tqc_learns():
    """the size of tests/test_sde.py's run: 256 envs, 6000 replayed iterations at the class defaults; the evaluation return improves"""
    from core.common.evaluation import evaluate_policy
    from core.tqc import TQC

    n = 256
    env, eval_env = _env(n), _env(64)
    model = TQC("MlpPolicy", env, seed=0, learning_starts=n * 10)
    model.enable_graph_capture()
    eval_env.seed(1234)
    before, _ = evaluate_policy(model, eval_env, n_eval_episodes=64)
    model.learn(n * 6000)
    assert model.graph_status()["active"] and model.fused_learner
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters())
    eval_env.seed(1234)
    after, _ = evaluate_policy(model, eval_env, n_eval_episodes=64)
    print(f"TQC, 256 envs x 6000 iterations: evaluation return {before:.1f} -> {after:.1f}")
    assert np.isfinite(after) and after > before, (before, after)
