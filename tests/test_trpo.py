"""GPU checks of core.TRPO: one train() of the kernel path and of the torch path against the fp64 statements of
tests/_trpo_reference.py on the same filled buffer, the same forced permutations and the same `cg_init_queue`; the invariants of the
actor and critic phases; a training run and the public interface.

Sizes: CSTRVecEnv(4), n_steps 8, batch_size 8; CSTRVecEnv(5), n_steps 13 (ragged tails); episodes of 6 steps, so truncations occur
inside a rollout.

Bars. `g` and a single Fisher-vector product are judged like tests/test_trpo_abi.py's whole product: per element in units of
2**-24 * M at BARS["fvp"], against the fp64 statement on the float32 activations the kernel path itself stored (g: the objective launch
is float64 inside and rounds d objective / d dist once, then the same backward as the product's runs). `s`, `step` and the weights
come out of 15 CG iterations, which amplify rounding by the conditioning of F: there the kernel path's error against fp64 may be at most
4 times the torch float32 path's error against fp64 on the same inputs -- the margin the project uses between ATen and a kernel with
another summation order --, both measured here and printed. All three paths must take the same accept / reject decisions, and
the fp64 reference's own decisions must be 100 bars clear of both thresholds (asserted, never skipped).
Measured on MI355X (2026-10-21; kernel path / torch path against fp64, max-norm; all in profiles/trpo_gpu_tests.txt): the worst ratios,
multi k = 1: actor weights 3.8e-08 / 2.7e-08, and discrete k = 1: value weights 2.1e-07 / 1.1e-07; the largest errors, the shrink case:
step 3.7e-06 / 3.0e-05, actor weights 9.2e-06 / 2.3e-05. A single product 1.17 .. 1.19 units and g 1.4 .. 2.5 units of the 4.88-unit bar."""
import numpy as np
import pytest
import torch as th

import _trpo_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = th.float64
FACES = {"box": dict(), "discrete": dict(discrete_actions=3), "multi": dict(multi_discrete_actions=(3, 5))}
HEAD = {"box": ("gauss", 2), "discrete": ("cat", 9), "multi": ("mcat", (3, 5))}


def _env(n, seed=0, **face):
    from core.common.vec_env import CSTRVecEnv

    class Short(CSTRVecEnv):
        max_steps = 6

    e = Short(n, device=DEV, **face)
    e.seed(seed)
    return e


def _model(face="box", n_envs=4, n_steps=8, seed=1, **kw):
    from core import TRPO

    kw.setdefault("batch_size", 8)
    kw.setdefault("n_critic_updates", 2)
    return TRPO("MlpPolicy", _env(n_envs, **FACES[face]), n_steps=n_steps, seed=seed, device=DEV, **kw)


def _fill(model):
    _, cb = model._setup_learn(model.n_envs * model.n_steps, None)
    assert model.collect_rollouts(model.env, cb, model.rollout_buffer, model.n_steps)
    assert model.rollout_buffer.full
    th.cuda.synchronize()


def _state(model):
    opt = model.policy.optimizer
    return dict(flat=model.policy.arena.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), ctl=opt.ctl.clone())


def _restore(model, st):
    opt = model.policy.optimizer
    model.policy.arena.flat.copy_(st["flat"]), opt.exp_avg.copy_(st["m"]), opt.exp_avg_sq.copy_(st["v"]), opt.ctl.copy_(st["ctl"])


def _actor_of(model, face):
    names = [n for n, _ in model._actor_params]
    want = (["log_std"] if face == "box" else []) + [f"mlp_extractor.policy_net.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")] + ["action_net.weight", "action_net.bias"]
    assert names == want, names
    ps = {n: p.detach().cpu().numpy().copy() for n, p in model._actor_params}
    ws = [(ps[f"mlp_extractor.policy_net.{i}.weight"], ps[f"mlp_extractor.policy_net.{i}.bias"]) for i in (0, 2)] + [(ps["action_net.weight"], ps["action_net.bias"])]
    return dict(ws=ws, log_std=ps.get("log_std"), act="tanh", head=HEAD[face])


def _value_of(model):
    sd = {n: p.detach().cpu().numpy().copy() for n, p in model.policy.named_parameters() if "value" in n}
    return [(sd[f"mlp_extractor.value_net.{i}.weight"], sd[f"mlp_extractor.value_net.{i}.bias"]) for i in (0, 2)] + [(sd["value_net.weight"], sd["value_net.bias"])]


def _batches(model, perms, k):
    """what train() will read from the buffer under the forced permutations: the actor batch (every k-th row) and the critic minibatches"""
    rb = model.rollout_buffer
    rb.forced_permutations = [perms[0]]
    rd = next(iter(rb.get(None)))
    batch = dict(obs=rd.observations[::k].cpu().numpy().copy(), actions=rd.actions[::k].cpu().numpy().copy(),
                 old_log_prob=rd.old_log_prob[::k].cpu().numpy().copy(), adv=rd.advantages[::k].cpu().numpy().copy())
    mbs = []
    for perm in perms[1:]:
        rb.forced_permutations = [perm]
        for mb in rb.get(model.batch_size):
            mbs.append((mb.observations.cpu().numpy().copy(), mb.returns.cpu().numpy().copy()))
    return batch, mbs


def _train(model, perms, x0, fused):
    model.fused_learner = fused
    model.rollout_buffer.forced_permutations = [p.copy() for p in perms]
    model.cg_init_queue = [th.as_tensor(x0)]
    model.debug_capture = True
    model.train()
    th.cuda.synchronize()
    assert not model.rollout_buffer.forced_permutations and not model.cg_init_queue
    cap = model.last_train_tensors
    out = {k: cap[k].detach().cpu().numpy().astype(np.float64) for k in ("g", "x0", "s", "step", "sFs")}
    out["ls"] = list(cap["line_search"])
    out["actor"] = np.concatenate([p.detach().cpu().numpy().reshape(-1) for _, p in model._actor_params]).astype(np.float64)
    out["value"] = np.concatenate([p.detach().cpu().numpy().reshape(-1) for n, p in model.policy.named_parameters() if "value" in n]).astype(np.float64)
    return out


def _reference(model, face, batch, mbs, x0):
    actor = _actor_of(model, face)
    theta0 = th.as_tensor(R.flat_of(actor)).to(F64)
    obj0, kl0, g = R.objective_grad(actor, theta0, batch)
    acts = [a.numpy() for a in R.forward(actor, theta0, batch["obs"])]
    fvp = lambda v: R.fvp_fisher(actor, theta0.numpy(), acts, v.numpy(), model.cg_damping)  # noqa: E731
    s, hist, iters = R.cg_solve(fvp, g, th.as_tensor(x0).to(F64), model.cg_max_steps)
    sfs = float(s @ fvp(s))
    step = float(np.sqrt(2 * model.target_kl / sfs))
    old = R.old_of(actor, theta0, batch["obs"])
    ev = lambda t: tuple(float(v) for v in R.objective_kl(actor, t, batch, *old))  # noqa: E731
    theta, coeff, recs = R.line_search(ev, theta0, s, step, float(obj0), model.target_kl, model.line_search_shrinking_factor, model.line_search_max_iter)
    vws, losses = R.critic_pass(_value_of(model), "tanh", mbs, model.learning_rate)
    value = np.concatenate([t.numpy().reshape(-1) for i in (0, 1) for t in vws[i]] + [t.numpy().reshape(-1) for t in vws[2]])
    return dict(g=g.numpy(), s=s.numpy(), step=step, sFs=sfs, ls=recs, coeff=coeff, actor=theta.numpy(), obj0=float(obj0), value=value, actor_dict=actor,
                theta0=theta0)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("face", list(FACES))
def test_one_train_against_fp64(face, k):
    n_envs, n_steps = (4, 8) if k == 1 else (5, 13)
    model = _model(face, n_envs, n_steps, sub_sampling_factor=k)
    assert model.fused_learner
    _fill(model)
    total = n_envs * n_steps
    rng = np.random.default_rng(7 + k)
    perms = [rng.permutation(total) for _ in range(1 + model.n_critic_updates)]
    x0 = (1e-4 * rng.standard_normal(model._n_actor)).astype(np.float32)
    st = _state(model)
    batch, mbs = _batches(model, perms, k)
    assert batch["obs"].shape[0] == -(-total // k)
    ref = _reference(model, face, batch, mbs, x0)
    # the reference's own line-search decisions are 100 bars clear of both thresholds
    margins = R.ls_margins(ref["ls"], ref["obj0"], model.target_kl)
    print(f"TRPO train {face} k {k}: fp64 line search {ref['ls']}, margins {[round(m) for m in margins]}")
    assert min(margins) >= 100.0, margins
    fused = _train(model, perms, x0, True)
    # a single product and g on the activations the kernel path stored: the ABI bar of the whole product
    with th.cuda.device(0):
        _restore(model, st)
        model.fused_learner = True
        obs = th.as_tensor(batch["obs"]).to(DEV)
        acts = model._actor_forward(obs)
        acts_h = [a.cpu().numpy() for a in acts]
        v = rng.standard_normal(model._n_actor).astype(np.float32)
        model.policy.arena.grad.zero_()
        model._fvp_fused(model._scatter(th.as_tensor(v), model._vec["p"]), acts, model._head_of(model._fast), model._rows(obs.shape[0]))
        got = model._flat(model.policy.arena.grad).cpu().numpy().astype(np.float64) + model.cg_damping * v
        assert not bool(model.policy.arena.grad[model._mask == 0].any())  # the value segments (and the padding) stay exactly zero
        model.policy.arena.grad.zero_()
    actor = ref["actor_dict"]
    c = dict(actor=actor, theta0=R.flat_of(actor), acts=acts_h, v=v, damping=model.cg_damping)
    fig = R.worst(got, R.fvp_eval(c), R.fvp_eval(c, mag=True))
    print(f"TRPO train {face} k {k}: single FVP {fig:.3f} units of a bar of {R.BARS['fvp']}")
    assert fig <= R.BARS["fvp"]
    # g: fp64 d objective / d dist on the stored float32 dist, the fp64 backward on the stored activations, its magnitude pass
    t64 = lambda a: th.as_tensor(a).to(F64)  # noqa: E731
    d = t64(acts_h[-1]).requires_grad_(True)
    ls = None if actor["log_std"] is None else t64(actor["log_std"]).requires_grad_(True)
    logp, _ = R.logp_kl(actor["head"], d, ls, d.detach(), None if ls is None else ls.detach(), batch["actions"])
    obj = (R.normalize(batch["adv"]) * th.exp(logp - t64(batch["old_log_prob"]))).mean()
    gd = th.autograd.grad(obj, [d] + ([] if ls is None else [ls]))
    _, ws = R.split(actor, t64(R.flat_of(actor)))
    want = ([gd[1]] if ls is not None else []) + [t.reshape(-1) for wb in R.backward_layers(actor, ws, acts_h, gd[0]) for t in wb]
    mag = ([gd[1].abs() + 1e-300] if ls is not None else []) + [t.reshape(-1) for wb in R.backward_layers(actor, ws, acts_h, gd[0], mag=True) for t in wb]
    if ls is not None:  # d objective / d log_std is a float64 batch sum stored as float32: the fp64 bar, not units of a magnitude
        assert R.close64(fused["g"][:ls.numel()], gd[1].numpy())[1]
        lo = ls.numel()
    else:
        lo = 0
    fig = R.worst(fused["g"][lo:], th.cat(want).numpy()[lo:], th.cat(mag).numpy()[lo:])
    print(f"TRPO train {face} k {k}: g {fig:.3f} units of a bar of {R.BARS['fvp']}")
    assert fig <= R.BARS["fvp"]
    _restore(model, st)
    _compare_paths(model, f"{face} k {k}", perms, x0, st, ref, fused)
    assert _err(fused["g"], ref["g"]) <= 1e-4 * np.abs(ref["g"]).max()  # the whole chain from float32 forward to g, coarse


def _compare_paths(model, tag, perms, x0, st, ref, fused):
    """the torch path on the same inputs; the same decisions in all three paths; the issue's rule for s, step and the weights"""
    torch = _train(model, perms, x0, False)
    _restore(model, st)
    model.fused_learner = True
    assert np.array_equal(fused["x0"], x0.astype(np.float64)) and np.array_equal(torch["x0"], fused["x0"])
    dec = lambda recs: [(round(c_, 12), ok) for c_, _, _, ok in recs]  # noqa: E731
    assert dec(fused["ls"]) == dec(torch["ls"]) == dec(ref["ls"]), (fused["ls"], torch["ls"], ref["ls"])
    for key in ("s", "step", "actor", "value"):
        ek, et = _err(fused[key], ref[key]), _err(torch[key], ref[key])
        print(f"TRPO train {tag}: {key} kernel path {ek:.3e}, torch path {et:.3e} against fp64")
        assert ek <= 4.0 * et, (key, ek, et)


def test_train_shrinks_before_accepting():
    """a line search that rejects its first step(s) and then accepts, through train() on all three paths: apply_step with coeff < 1, the
    re-forward, a second read. The trust region is widened (and the damping lowered) until the fp64 reference's own search, on the buffer this test filled,
    shrinks at least once and then accepts with every decision 100 bars clear of both thresholds (chosen from the reference alone)."""
    model = _model("box", 4, 8)
    _fill(model)
    rng = np.random.default_rng(11)
    perms = [rng.permutation(32) for _ in range(1 + model.n_critic_updates)]
    x0 = (1e-4 * rng.standard_normal(model._n_actor)).astype(np.float32)
    st = _state(model)
    batch, mbs = _batches(model, perms, 1)
    ref = None
    for damping, target_kl in [(d, t) for d in (0.1, 0.001) for t in (8.0, 32.0, 128.0, 256.0, 512.0, 1024.0, 4096.0)]:
        model.cg_damping, model.target_kl = damping, target_kl
        cand = _reference(model, "box", batch, mbs, x0)
        margins = R.ls_margins(cand["ls"], cand["obj0"], target_kl)
        print(f"TRPO shrink cg_damping {damping} target_kl {target_kl}: fp64 line search {[(c, round(o, 4), round(kl, 4), ok) for c, o, kl, ok in cand['ls']]}, "
              f"margins {[round(m) for m in margins]}")
        if cand["coeff"] is not None and len(cand["ls"]) >= 2 and min(margins) >= 100.0:
            ref = cand
            break
    assert ref is not None, "no trust region in the list makes the fp64 line search shrink and then accept"
    fused = _train(model, perms, x0, True)
    assert fused["ls"][-1][3] and fused["ls"][-1][0] < 1.0 and len(fused["ls"]) == len(ref["ls"])
    assert model.logger.name_to_value["train/is_line_search_success"] == 1.0
    _restore(model, st)
    _compare_paths(model, f"shrink cg_damping {model.cg_damping} target_kl {model.target_kl}", perms, x0, st, ref, fused)


def test_invariants_of_the_two_phases():
    model = _model("box", 4, 8)
    _fill(model)
    arena, opt, mask = model.policy.arena, model.policy.optimizer, model._mask.bool()
    before = _state(model)
    # a failed line search: constant advantages normalise to zero, the objective cannot increase, theta0 comes back bit for bit
    adv = model.rollout_buffer.advantages.clone()
    model.rollout_buffer.advantages.fill_(1.0)
    model.n_critic_updates = 0
    model.train()
    th.cuda.synchronize()
    assert th.equal(arena.flat, before["flat"]) and model.logger.name_to_value["train/is_line_search_success"] == 0.0
    assert float(model.logger.name_to_value["train/kl_divergence_loss"]) == 0.0 and model._n_updates == 1
    assert not bool(arena.grad.any())
    model.rollout_buffer.advantages.copy_(adv)
    # the critic phase leaves the actor's weights and Adam moments bit-identical: the same train() from the same state, the same
    # permutations and the same x0, once without the critic phase and once with it
    perms = [np.random.default_rng(5).permutation(32) for _ in range(3)]
    x0 = th.as_tensor((1e-4 * np.random.default_rng(6).standard_normal(model._n_actor)).astype(np.float32))
    model.rollout_buffer.forced_permutations, model.cg_init_queue = [perms[0].copy()], [x0]
    model.train()
    th.cuda.synchronize()
    actor_only = arena.flat.clone()
    assert th.equal(actor_only[~mask], before["flat"][~mask])  # the actor phase leaves the value segments alone
    _restore(model, before)
    model.n_critic_updates = 2
    model.debug_capture = True
    model.rollout_buffer.forced_permutations, model.cg_init_queue = [q.copy() for q in perms], [x0]
    model.train()
    th.cuda.synchronize()
    cap = model.last_train_tensors
    assert th.equal(arena.flat[mask], actor_only[mask])
    assert th.equal(opt.exp_avg[mask], before["m"][mask]) and th.equal(opt.exp_avg_sq[mask], before["v"][mask])
    assert not bool(opt.exp_avg[mask].any()) and bool(opt.exp_avg[~mask].any())
    assert not th.equal(arena.flat[~mask], before["flat"][~mask])  # the critic moved
    ok = cap["line_search"][-1][3]
    log = model.logger.name_to_value
    assert log["train/is_line_search_success"] == float(ok)
    if ok:
        assert float(log["train/kl_divergence_loss"]) < model.target_kl and float(log["train/policy_objective"]) > float(model._scalars0[0])
        coeff = cap["line_search"][-1][0]  # theta0 + coeff * step * s on the actor's tensors, nothing else
        s_full = model._scatter(cap["s"], th.zeros_like(before["flat"]))
        want = (before["flat"].double() + coeff * float(cap["step"]) * s_full.double()).float()
        assert th.equal(arena.flat[mask], want[mask])
    # with the critic switched off, train() touches the actor only
    model.n_critic_updates = 0
    mid = arena.flat.clone()
    model.train()
    th.cuda.synchronize()
    assert th.equal(arena.flat[~mask], mid[~mask])


def test_learn_logs_reproducibility_and_checkpoints(tmp_path):
    from core import TRPO

    def run():
        m = _model("box", 4, 8, seed=3)
        m.learn(3 * 4 * 8)
        th.cuda.synchronize()
        return m

    a, b = run(), run()
    assert a._n_updates == 3 and a.fused_learner and a.num_timesteps == 96
    keys = {"train/policy_objective", "train/value_loss", "train/kl_divergence_loss", "train/explained_variance", "train/is_line_search_success",
            "train/std", "train/n_updates"}
    assert keys <= set(a.logger.name_to_value), set(a.logger.name_to_value)
    assert all(np.isfinite(float(a.logger.name_to_value[k])) for k in keys - {"train/explained_variance"})
    for (n, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
        assert th.equal(p, q), n  # a seeded run repeated gives identical weights (the x0 stream is keyed by the seed)
    assert all(bool(th.isfinite(p).all()) for p in a.policy.parameters())
    path = str(tmp_path / "trpo_model.zip")
    a.save(path)
    loaded = TRPO.load(path, env=_env(4), device=DEV)
    for (k_, x), (_, y) in zip(a.policy.state_dict().items(), loaded.policy.state_dict().items()):
        assert th.equal(x, y), k_
    for key in TRPO._ctor_keys():
        if key != "policy_kwargs":
            assert getattr(loaded, key) == getattr(a, key), key
    assert loaded._n_updates == 3 and loaded.fused_learner
    obs = np.zeros((4, 4), np.float32)
    assert np.array_equal(a.predict(obs, deterministic=True)[0], loaded.predict(obs, deterministic=True)[0])
    loaded.learn(4 * 8, reset_num_timesteps=False)
    assert loaded._n_updates == 4
    # the discrete faces train too, and their logs have no std
    for face in ("discrete", "multi"):
        m = _model(face, 5, 13, seed=4, sub_sampling_factor=2)
        m.learn(2 * 5 * 13)
        th.cuda.synchronize()
        assert m._n_updates == 2 and m.fused_learner and "train/std" not in m.logger.name_to_value
        assert all(bool(th.isfinite(p).all()) for p in m.policy.parameters())


def test_interface_calls_and_refusals():
    import core
    from core import TRPO
    from core.common.callbacks import EvalCallback
    from core.common.evaluation import evaluate_policy, evaluate_policy_fused
    from core.common.offline_dataset import collect_offline_dataset
    from core.common.vec_env import CSTRVecEnv, VecNormalize

    assert TRPO is core.TRPO and "TRPO" in core.__all__
    model = _model("box", 4, 8, seed=5)
    act, state = model.predict(np.zeros((4, 4), np.float32), deterministic=True)
    assert act.shape == (4, 2) and state is None
    loop = evaluate_policy(model, _env(4, 21), n_eval_episodes=4, return_episode_rewards=True, warn=False)
    fused = evaluate_policy_fused(model, _env(4, 21), n_eval_episodes=4, return_episode_rewards=True, warn=False)
    assert loop[1] == fused[1] == [6] * 4 and np.allclose(loop[0], fused[0], rtol=1e-4, atol=1e-4)
    ev = EvalCallback(_env(4, 7), n_eval_episodes=4, eval_freq=8, verbose=0, warn=False)
    model.learn(2 * 4 * 8, callback=ev)
    assert ev.n_calls == 16 and np.isfinite(ev.last_mean_reward)
    rb, stats = collect_offline_dataset(model, _env(8, 5), num_episodes=16, random_action_prob=0.2, seed=1)
    assert rb.size() > 0 and stats["num_episodes"] >= 16
    # the refusals of the PPO family, and TRPO's own
    with pytest.raises(ValueError, match="gSDE"):
        TRPO("MlpPolicy", CSTRVecEnv(4, device=DEV), use_sde=True, device=DEV)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        TRPO("MlpPolicy", VecNormalize(CSTRVecEnv(4, device=DEV)), device=DEV)
    with pytest.raises(NotImplementedError, match="hipGraph"):
        model.enable_graph_capture(True)
    with pytest.raises(ValueError, match="Dict observation space"):
        TRPO("MlpPolicy", CSTRVecEnv(4, goal_conditioned=True, device=DEV), device=DEV)
    with pytest.raises(ValueError, match="Dict observation space"):
        TRPO("MultiInputPolicy", CSTRVecEnv(4, goal_conditioned=True, device=DEV), device=DEV)
    for kw, word in ((dict(cg_max_steps=0), "cg_max_steps"), (dict(line_search_max_iter=0), "line_search_max_iter"),
                     (dict(line_search_shrinking_factor=1.5), "line_search_shrinking_factor"), (dict(target_kl=0.0), "target_kl"),
                     (dict(sub_sampling_factor=0), "sub_sampling_factor"), (dict(n_critic_updates=-1), "n_critic_updates")):
        with pytest.raises(ValueError, match=word):
            TRPO("MlpPolicy", CSTRVecEnv(4, device=DEV), device=DEV, **kw)
    with pytest.raises(AssertionError, match="batch_size"):
        TRPO("MlpPolicy", CSTRVecEnv(4, device=DEV), batch_size=1, device=DEV)
    with pytest.warns(UserWarning, match="truncated mini-batch"):
        TRPO("MlpPolicy", CSTRVecEnv(4, device=DEV), n_steps=8, batch_size=7, device=DEV)
    # another optimiser class runs the published torch statements; the kernel path cannot be switched on for it
    sgd = TRPO("MlpPolicy", _env(4), n_steps=8, batch_size=8, n_critic_updates=1, seed=0, device=DEV,
               policy_kwargs=dict(optimizer_class=th.optim.SGD, optimizer_kwargs=dict()))
    assert not sgd.fused_learner
    with pytest.raises(ValueError, match="no kernel path"):
        sgd.fused_learner = True
    sgd.learn(4 * 8)
    assert sgd._n_updates == 1 and all(bool(th.isfinite(p).all()) for p in sgd.policy.parameters())
    # a Categorical head of more than 64 logits (9 levels per valve: 81): the TRPO launches decline it, and with them the device rollout
    wide = TRPO("MlpPolicy", _env(4, discrete_actions=9), n_steps=8, batch_size=8, n_critic_updates=1, seed=0, device=DEV)
    assert not wide.fused_learner and wide.policy.fast is None and not wide._device_rollout() and wide.policy.action_net.out_features == 81
    with pytest.raises(ValueError, match="no kernel path"):
        wide.fused_learner = True
    wide.learn(2 * 4 * 8)
    index, _ = wide.predict(np.zeros((2, 4), np.float32), deterministic=True)
    assert wide._n_updates == 2 and index.shape == (2,) and all(bool(th.isfinite(p).all()) for p in wide.policy.parameters())
