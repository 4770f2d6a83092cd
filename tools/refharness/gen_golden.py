#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the UNMODIFIED reference in the dev container.

Usage (dev container only; /root/reference must exist):
    python tools/refharness/gen_golden.py [--only env,sampler,replay,sac,sac_sde,td3,bcq,ppo,a2c,dqn,ppo_discrete,a2c_discrete,ppo_multidiscrete,a2c_multidiscrete,ppo_goal,a2c_goal,init,vecenv,callbacks,rmsprop_tf]

Every array written is data (inputs + the reference's outputs); no reference source is copied.
Injected quantities (never produced by the stand-in gymnasium): initial states, actions, batches.
Recorded-by-hook quantities: the Normal eps draws and the (current_q, target_q) arguments of
mse_loss; the hooks wrap torch-level functions, the reference code itself is untouched.

Reference entry points exercised (file:line in /root/reference):
  twoseriescstr.py:394-503              TwoSeriesCSTREnv.step / _dynamics / compute_reward
  core/common/vec_env/dummy_vec_env.py:56-73   auto-reset, terminal_observation, TimeLimit.truncated
  core/common/buffers.py:106-115,247-325 ReplayBuffer.add / sample / _get_samples
  core/sac/sac.py:199-296                SAC.train
  core/td3/td3.py:154-211                TD3.train
  core/bcq/bcq.py:129-213                BCQ.train; core/bcq/policies.py:426-435 BCQPolicy._predict
  core/ppo/ppo.py:184-300                PPO.train; core/common/on_policy_algorithm.py:162-268 collect_rollouts
  core/a2c/a2c.py:132-190                A2C.train
  core/common/sb2_compat/rmsprop_tf_like.py:78-137  RMSpropTFLike.step (--only rmsprop_tf)
  core/dqn/dqn.py:168-256                DQN._on_step / train / predict
  core/her/her_replay_buffer.py:135-408  HerReplayBuffer.add / sample / truncate_last_trajectory (--only her)
  core/common/utils.py:457-481           polyak_update
  core/common/callbacks.py:146-680       EventCallback ... StopTrainingOnNoModelImprovement (structure only)
"""
import argparse
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refload  # noqa: E402

refload.load()
OUT = os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests", "golden")
os.makedirs(OUT, exist_ok=True)
th.set_num_threads(1)


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


def slim_weights(out, keep=4096, head=64, with_shape=True):
    """Digest form for class-default nets: tensors above `keep` elements are stored as sum / abs-sum / first `head` values
    (the initial weights are reproducible from the seed -- checked bit-exactly by the init KAT and by #head/#sum here)."""
    slim = {}
    for k, v in out.items():
        if (k.startswith("before/") or k.startswith("after/")) and v.size > keep:
            slim[k + "#sum"] = np.float64(v.astype(np.float64).sum())
            slim[k + "#abs"] = np.float64(np.abs(v.astype(np.float64)).sum())
            slim[k + "#head"] = v.reshape(-1)[:head].copy()
            if with_shape:
                slim[k + "#shape"] = np.array(v.shape, np.int64)
        else:
            slim[k] = v
    return slim


# --------------------------------------------------------------------------------------- env
def gen_env():
    from twoseriescstr import TwoSeriesCSTREnv

    rng = np.random.default_rng(20250418)
    env = TwoSeriesCSTREnv()
    env.reset(seed=0)

    # ---- single-step known-answer tests -------------------------------------------------
    edge_obs = [
        [0, 0, 0, 0], [1, 1, 1, 1], [-1, -1, -1, -1], [1, -1, 1, -1], [-1, 1, -1, 1],
        [0.5, 0.9, 0.5, 0.9], [-0.42857143, -0.2, -0.42857143, -0.5], [1.5, 1.5, -1.5, -1.5],
        [0.3, 0.99, 0.2, 0.97], [-0.9, -0.95, -0.99, -0.9],
    ]
    edge_act = [
        [0, 0], [-1, -1], [1, 1], [2, -3], [-1, 1], [0.25, -0.75], [1, -1], [-5, 5], [0.999, -0.999], [0.1, 0.1],
    ]
    K = 4096
    obs = rng.uniform(-1.0, 1.0, size=(K, 4)).astype(np.float32)
    # a slice slightly outside the box exercises the raw-state safety clip (twoseriescstr.py:406-410)
    obs[:256] = rng.uniform(-1.2, 1.2, size=(256, 4)).astype(np.float32)
    # hot reactors (runaway region: big exp term, upper clip)
    obs[256:768, 1] = rng.uniform(0.5, 1.0, size=512).astype(np.float32)
    obs[512:768, 3] = rng.uniform(0.5, 1.0, size=256).astype(np.float32)
    act = rng.uniform(-1.0, 1.0, size=(K, 2)).astype(np.float32)
    act[:256] = rng.uniform(-1.5, 1.5, size=(256, 2)).astype(np.float32)
    obs = np.concatenate([np.array(edge_obs, np.float32), obs])
    act = np.concatenate([np.array(edge_act, np.float32), act])
    step_in = rng.integers(0, 399, size=len(obs)).astype(np.int32)
    step_in[:16] = [398, 399, 0, 397, 398, 399, 1, 2, 398, 399, 398, 399, 100, 200, 398, 399]

    n = len(obs)
    o2 = np.zeros((n, 4), np.float32)
    rew = np.zeros(n, np.float32)
    trunc = np.zeros(n, np.uint8)
    term = np.zeros(n, np.uint8)
    raw_next = np.zeros((n, 4), np.float32)
    raw_act = np.zeros((n, 2), np.float32)
    conc_r = np.zeros(n, np.float32)
    temp_p = np.zeros(n, np.float32)
    for i in range(n):
        env.reset()  # clears the stateful reward memory
        env.state = obs[i].copy()
        env.current_step = int(step_in[i])
        s, r, te, tr, info = env.step(act[i].copy())
        assert s.dtype == np.float32 and isinstance(r, np.floating) and r.dtype == np.float32
        o2[i], rew[i], term[i], trunc[i] = s, r, te, tr
        raw_next[i], raw_act[i] = info["original_state"], info["raw_action"]
        conc_r[i], temp_p[i] = info["concentration_reward"], info["temp_penalty"]
    save("env_step_kat.npz", obs=obs, act=act, step_in=step_in, obs_next=o2, reward=rew, terminated=term,
         truncated=trunc, raw_next=raw_next, raw_action=raw_act, concentration_reward=conc_r, temp_penalty=temp_p)

    # ---- NaN action: dynamics raises -> (old state, -10, False, True) twoseriescstr.py:413-421
    env.reset()
    env.state = np.array([0.1, 0.2, -0.3, 0.4], np.float32)
    env.current_step = 7
    import contextlib
    import io

    with contextlib.redirect_stdout(io.StringIO()):
        s, r, te, tr, info = env.step(np.array([np.nan, 0.0], np.float32))
    save("env_nan_kat.npz", obs=np.array([0.1, 0.2, -0.3, 0.4], np.float32), act=np.array([np.nan, 0.0], np.float32),
         obs_next=np.asarray(s, np.float32), reward=np.float32(r), terminated=np.uint8(te), truncated=np.uint8(tr),
         step_after=np.int32(env.current_step))

    # ---- 400-step trajectories under fixed action tapes -----------------------------------
    M, T = 6, 400
    obs0 = np.array([
        [0.28571430, -0.41931412, -0.28571430, -0.73472524],  # raw ~[0.45,310,0.25,290]
        [0.0, 0.0, 0.0, 0.0],
        [-0.5, 0.2, -0.6, 0.1],
        [0.9, 0.6, 0.8, 0.5],
        [-0.8, -0.8, -0.9, -0.9],
        [0.2, 0.75, 0.1, 0.7],
    ], np.float32)
    t = np.arange(T, dtype=np.float32)
    actions = np.zeros((T, M, 2), np.float32)
    actions[:, 0] = [0.0, 0.0]
    actions[:, 1] = np.stack([np.sin(0.05 * t), np.cos(0.03 * t)], 1)
    actions[:, 2] = rng.uniform(-1, 1, size=(T, 2))
    actions[:, 3] = [1.0, 1.0]
    actions[:, 4] = [-1.0, -1.0]
    actions[:, 5] = rng.uniform(-1, 1, size=(T, 2)) * 0.3
    actions = actions.astype(np.float32)
    obs_t = np.zeros((T, M, 4), np.float32)
    rew_t = np.zeros((T, M), np.float32)
    trunc_t = np.zeros((T, M), np.uint8)
    for m in range(M):
        env.reset()
        env.state = obs0[m].copy()
        env.current_step = 0
        for k in range(T):
            s, r, te, tr, info = env.step(actions[k, m].copy())
            obs_t[k, m], rew_t[k, m], trunc_t[k, m] = s, r, tr
    save("env_traj_kat.npz", obs0=obs0, actions=actions, obs=obs_t, reward=rew_t, truncated=trunc_t)


# ----------------------------------------------------------------------------------- vec env
def gen_vecenv():
    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from twoseriescstr import TwoSeriesCSTREnv

    rng = np.random.default_rng(7)
    N, T = 5, 6
    venv = DummyVecEnv([lambda: TwoSeriesCSTREnv() for _ in range(N)])
    venv.seed(11)
    venv.reset()
    obs0 = rng.uniform(-0.8, 0.8, size=(N, 4)).astype(np.float32)
    step0 = np.array([397, 398, 399, 10, 396], np.int32)
    for i, e in enumerate(venv.envs):
        e.state = obs0[i].copy()
        e.current_step = int(step0[i])
    actions = rng.uniform(-1, 1, size=(T, N, 2)).astype(np.float32)
    obs = np.zeros((T, N, 4), np.float32)       # what VecEnv.step returns (post-reset obs for done envs)
    term_obs = np.zeros((T, N, 4), np.float32)  # next_obs as stored in the buffer (terminal obs on done)
    rew = np.zeros((T, N), np.float32)
    done = np.zeros((T, N), np.uint8)
    timeout = np.zeros((T, N), np.uint8)
    for k in range(T):
        o, r, d, infos = venv.step(actions[k])
        obs[k], rew[k], done[k] = o, r, d
        for i in range(N):
            timeout[k, i] = infos[i].get("TimeLimit.truncated", False)
            term_obs[k, i] = infos[i]["terminal_observation"] if d[i] else o[i]
    # reset_obs[k, i] is the INJECTED reset source: the post-reset observation the reference drew
    # (gymnasium np_random -> stand-in -> unpinned), so it is an input of this fixture, not an output.
    save("vecenv_autoreset_kat.npz", obs0=obs0, step0=step0, actions=actions, obs=obs, next_obs_for_buffer=term_obs,
         reward=rew, done=done, timeout=timeout, reset_obs=obs.copy())


# ----------------------------------------------------------------------------------- sampler
def gen_sampler():
    """np.random.randint exactly as called at core/common/buffers.py:113-114 and :309."""
    cases = [
        # (seed, [(upper, B), (n_envs, B)] * calls)
        (0, [(244, 256), (4096, 256)]),
        (3, [(1, 256), (4, 256), (2, 256), (4, 256), (3, 256), (4, 256)]),
        (4095, [(1, 256), (4096, 256), (2, 256), (4096, 256), (244, 256), (4096, 256)]),
        (42, [(100000, 256), (1, 256), (99999, 100), (1, 100)]),
        (123, [(244, 256), (4096, 256)] * 8),
        (7, [(976, 256), (1024, 256)] * 4),
        (2**32 - 1, [(5, 1), (7, 1), (1000, 3), (6, 2048), (65536, 700), (65537, 700)]),
        (99, [(2**31 - 1, 64), (2**32, 64), (3, 1500)]),
    ]
    out = {}
    for ci, (seed, calls) in enumerate(cases):
        np.random.seed(seed)
        res = []
        for (upper, b) in calls:
            r = np.random.randint(0, upper, size=b)
            assert r.dtype == np.int64
            res.append(r)
        st = np.random.get_state()
        out[f"c{ci}_seed"] = np.uint64(seed)
        out[f"c{ci}_calls"] = np.array(calls, np.int64)
        out[f"c{ci}_out"] = np.concatenate(res)
        out[f"c{ci}_key"] = st[1].astype(np.uint32)
        out[f"c{ci}_pos"] = np.int32(st[2])
    out["n_cases"] = np.int32(len(cases))
    save("mt19937_randint_kat.npz", **out)


# ------------------------------------------------------------------------------------ replay
def gen_replay():
    from core.common.buffers import ReplayBuffer
    from gymnasium import spaces

    rng = np.random.default_rng(5)
    out = {}
    for tag, (R, N, D, A, n_add, B) in {"small": (5, 3, 4, 2, 8, 16), "wide": (7, 8, 8, 2, 5, 64)}.items():
        ospace = spaces.Box(-1, 1, (D,), np.float32)
        aspace = spaces.Box(-1, 1, (A,), np.float32)
        buf = ReplayBuffer(R * N, ospace, aspace, device="cpu", n_envs=N)
        assert buf.buffer_size == R
        obs = rng.uniform(-1, 1, (n_add, N, D)).astype(np.float32)
        nobs = rng.uniform(-1, 1, (n_add, N, D)).astype(np.float32)
        act = rng.uniform(-1, 1, (n_add, N, A)).astype(np.float32)
        rew = rng.uniform(-8, 0, (n_add, N)).astype(np.float32)
        done = (rng.uniform(size=(n_add, N)) < 0.4)
        tout = done & (rng.uniform(size=(n_add, N)) < 0.6)
        samples = []
        np.random.seed(1234)
        for k in range(n_add):
            infos = [{"TimeLimit.truncated": bool(tout[k, i])} for i in range(N)]
            buf.add(obs[k], nobs[k], act[k], rew[k], done[k], infos)
            s = buf.sample(B)
            samples.append([x.numpy() for x in s])
        out.update({
            f"{tag}_dims": np.array([R, N, D, A, n_add, B], np.int64), f"{tag}_obs": obs, f"{tag}_next_obs": nobs,
            f"{tag}_act": act, f"{tag}_rew": rew, f"{tag}_done": done.astype(np.uint8), f"{tag}_timeout": tout.astype(np.uint8),
            f"{tag}_ring_obs": buf.observations.copy(), f"{tag}_ring_next_obs": buf.next_observations.copy(),
            f"{tag}_ring_act": buf.actions.copy(), f"{tag}_ring_rew": buf.rewards.copy(),
            f"{tag}_ring_done": buf.dones.copy(), f"{tag}_ring_timeout": buf.timeouts.copy(),
            f"{tag}_pos": np.int64(buf.pos), f"{tag}_full": np.uint8(buf.full),
        })
        for fi, fname in enumerate(["observations", "actions", "next_observations", "dones", "rewards"]):
            out[f"{tag}_s_{fname}"] = np.stack([s[fi] for s in samples])
    out["seed"] = np.int64(1234)
    save("replay_kat.npz", **out)


# ------------------------------------------------------------------------------ learner KATs
class _Recorder:
    def __init__(self):
        self.eps, self.mse = [], []


def _flat_sd(prefix, sd):
    return {f"{prefix}/{k}": v.detach().cpu().numpy().copy() for k, v in sd.items()}


def _fill_buffer(model, rng, n_rows, N, D, A):
    for _ in range(n_rows):
        obs = rng.uniform(-1, 1, (N, D)).astype(np.float32)
        nobs = np.clip(obs + rng.normal(0, 0.05, (N, D)), -1, 1).astype(np.float32)
        act = rng.uniform(-1, 1, (N, A)).astype(np.float32)
        rew = rng.uniform(-8, 0, (N,)).astype(np.float32)
        done = rng.uniform(size=N) < 0.2
        tout = done & (rng.uniform(size=N) < 0.5)
        model.replay_buffer.add(obs, nobs, act, rew, done, [{"TimeLimit.truncated": bool(t)} for t in tout])


def _make_venv(N):
    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from twoseriescstr import TwoSeriesCSTREnv

    return DummyVecEnv([lambda: TwoSeriesCSTREnv() for _ in range(N)])


def gen_sac():
    for tag, net_arch, B, n_steps in (("small", [64, 64], 64, 3), ("default", None, 256, 2)):
        _gen_sac(tag, net_arch, B, n_steps)


def gen_sac_ncrit():
    """SAC with policy_kwargs n_critics != 2 (reference core/common/policies.py:934-965; core/sac/sac.py:249-250, :261, :273-275):
    every critic's mse_loss call is recorded, N per gradient step."""
    _gen_sac("ncrit3", [64, 64], 64, 3, n_critics=3)
    _gen_sac("ncrit3_default", None, 256, 2, n_critics=3)
    _gen_sac("ncrit1", [64, 64], 64, 3, n_critics=1)


def gen_sac_sde():
    """SAC with gSDE (use_sde=True; reference core/sac/policies.py:89-175, core/common/distributions.py:421-617, core/sac/sac.py:218-219):
    the construction draws (exploration_mat [L, A], then exploration_matrices [1, L, A]) and the two draws of every gradient step's
    reset_noise() are recorded from torch's _standard_normal, in call order."""
    _gen_sac("sde_small", [64, 64], 64, 3, sde={})
    _gen_sac("sde_default", None, 256, 2, sde={})
    _gen_sac("sde_variants", [64, 64], 64, 3, sde=dict(use_expln=True, full_std=False, clip_mean=0.0))
    _gen_sac_sde_predict()


def _gen_sac_sde_predict():
    """predict() of a gSDE SAC on 4 envs: per-env matrices (reset_noise(4)), one env (exploration_mat), deterministic, and after one
    gradient step (its batch-1 draw: every row uses exploration_mat)."""
    import torch.distributions.normal as tdn

    from core.common.logger import Logger
    from core.sac.sac import SAC

    draws = []
    orig_sn = tdn._standard_normal

    def rec_sn(shape, dtype, device):
        e = orig_sn(shape, dtype, device)
        draws.append(e.clone())
        return e

    N, D, A, B = 4, 4, 2, 64
    tdn._standard_normal = rec_sn
    try:
        model = SAC("MlpPolicy", _make_venv(N), seed=0, device="cpu", batch_size=B, buffer_size=64 * N, use_sde=True,
                    policy_kwargs=dict(net_arch=[64, 64]))
        model.set_logger(Logger(folder=None, output_formats=[]))
        out = {}
        out.update(_flat_sd("before/actor", model.actor.state_dict()))
        out.update(_flat_sd("before/critic", model.critic.state_dict()))
        out.update(_flat_sd("before/critic_target", model.critic_target.state_dict()))
        assert len(draws) == 2
        out["init/z_mat"], out["init/z_mats"] = draws[0].numpy(), draws[1].numpy()
        rng = np.random.default_rng(5)
        obs = rng.uniform(-1, 1, (N, D)).astype(np.float32)
        out["obs"] = obs

        def actor_out(x, deterministic=False):
            with th.no_grad():
                return model.actor(th.as_tensor(x), deterministic=deterministic).numpy().copy()

        model.actor.reset_noise(N)
        out["per_env/z_mat"], out["per_env/z_mats"] = draws[2].numpy(), draws[3].numpy()
        out["per_env/actions"] = actor_out(obs)
        out["per_env/predict"] = model.predict(obs)[0]
        out["single/actions"] = actor_out(obs[:1])
        out["single/predict"] = model.predict(obs[:1])[0]
        out["deterministic/actions"] = actor_out(obs, True)
        out["deterministic/predict"] = model.predict(obs, deterministic=True)[0]
        _fill_buffer(model, np.random.default_rng(99), 40, N, D, A)
        rb = model.replay_buffer
        out.update(ring_obs=rb.observations.copy(), ring_next_obs=rb.next_observations.copy(), ring_act=rb.actions.copy(),
                   ring_rew=rb.rewards.copy(), ring_done=rb.dones.copy(), ring_timeout=rb.timeouts.copy(),
                   ring_pos=np.int64(rb.pos), ring_full=np.uint8(rb.full))
        np.random.seed(2024)
        model.train(gradient_steps=1, batch_size=B)
        assert len(draws) == 6
        out["train/z_mat"], out["train/z_mats"] = draws[4].numpy(), draws[5].numpy()
        out.update(_flat_sd("after/actor", model.actor.state_dict()))
        out["after_train/actions"] = actor_out(obs)
        out["after_train/predict"] = model.predict(obs)[0]
    finally:
        tdn._standard_normal = orig_sn
    out["np_seed"] = np.int64(2024)
    save("sac_sde_predict_kat.npz", **out)


_HER_STEPS, _HER_TARGETS = (7, 9, 12, 15), (0.12, 0.20, 0.33, 0.40)  # per-env episode lengths / setpoints of the HER learner fixtures


def _her_kwargs():
    from core.her.her_replay_buffer import HerReplayBuffer

    return dict(replay_buffer_class=HerReplayBuffer)


def _fill_her(model, venv, rng, steps):
    """Scripted steps of the goal-face envs into the model's HerReplayBuffer; returns the add inputs as flat rows (`adds_*`), from
    which a test rebuilds the ring and its episode bookkeeping."""
    N = venv.num_envs
    flat = lambda d: np.concatenate([d["achieved_goal"], d["desired_goal"], d["observation"]], axis=1).astype(np.float32)  # noqa: E731
    rec = {k: [] for k in ("obs", "next", "act", "rew", "done", "timeout")}
    venv.seed(11)
    obs = venv.reset()
    for _ in range(steps):
        a = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
        nobs, r, d, infos = venv.step(a)
        nxt = {k: v.copy() for k, v in nobs.items()}
        for i in range(N):
            if d[i]:
                for k in nxt:
                    nxt[k][i] = infos[i]["terminal_observation"][k]
        model.replay_buffer.add(obs, nxt, a, r, d, infos)
        for k, v in (("obs", flat(obs)), ("next", flat(nxt)), ("act", a), ("rew", np.asarray(r, np.float32)), ("done", d.astype(np.float32)),
                     ("timeout", np.array([i.get("TimeLimit.truncated", False) for i in infos], np.float32))):
            rec[k].append(v)
        obs = nobs
    return {f"adds_{k}": np.stack(v) for k, v in rec.items()}


def _flat_batch(s):
    """a DictReplayBufferSamples as the five arrays of a flat batch: observations in key order"""
    cat = lambda d: np.concatenate([d[k].numpy() for k in ("achieved_goal", "desired_goal", "observation")], axis=1)  # noqa: E731
    return [cat(s.observations), s.actions.numpy().copy(), cat(s.next_observations), s.dones.numpy().copy(), s.rewards.numpy().copy()]


def gen_her_learners():
    """sac_her_train_kat_small.npz / td3_her_train_kat_small.npz: the reference's MultiInputPolicy + HerReplayBuffer (future, 4 goals),
    seeded initial weights, then teacher-forced train() steps on recorded batches, as the *_train_kat_small fixtures."""
    _gen_sac("small", [64, 64], 64, 3, her=True)
    _gen_td3("small", her=True)


def _gen_sac(tag, net_arch, B, n_steps, n_critics=2, sde=None, her=False):
    import torch.distributions.normal as tdn
    import torch.nn.functional as F_real

    import core.sac.sac as sacmod
    from core.common.logger import Logger
    from core.sac.sac import SAC

    rec = _Recorder()
    orig_sn = tdn._standard_normal

    def rec_sn(shape, dtype, device):
        e = orig_sn(shape, dtype, device)
        rec.eps.append(e.clone())
        return e

    class FProxy:
        def __getattr__(self, name):
            return getattr(F_real, name)

        @staticmethod
        def mse_loss(a, b, *args, **kw):
            rec.mse.append((a.detach().clone(), b.detach().clone()))
            return F_real.mse_loss(a, b, *args, **kw)

    N, D, A = 4, 4, 2
    venv = _make_goal_venv(_HER_STEPS, _HER_TARGETS) if her else _make_venv(N)
    pk = {} if net_arch is None else {"policy_kwargs": dict(net_arch=net_arch)}
    if her:
        pk.update(_her_kwargs())
    if n_critics != 2:
        pk.setdefault("policy_kwargs", {})["n_critics"] = n_critics
    if sde is not None:  # gSDE: the construction draws are recorded too
        sde = dict(sde)
        policy = "MlpPolicy"
        if "full_std" in sde:  # the reference's SACPolicy has no full_std argument: its Actor's, set through the actor kwargs
            from core.sac.policies import SACPolicy

            full_std = sde.pop("full_std")

            class FullStdPolicy(SACPolicy):
                def make_actor(self, features_extractor=None):
                    self.actor_kwargs["full_std"] = full_std
                    return super().make_actor(features_extractor)

            policy = FullStdPolicy
        if sde:
            pk.setdefault("policy_kwargs", {}).update(sde)
        tdn._standard_normal = rec_sn
        try:
            model = SAC(policy, venv, seed=0, device="cpu", batch_size=B, buffer_size=64 * N, use_sde=True, **pk)
        finally:
            tdn._standard_normal = orig_sn
        assert len(rec.eps) == 2
        init_draws, rec.eps = rec.eps, []
    else:
        model = SAC("MultiInputPolicy" if her else "MlpPolicy", venv, seed=0, device="cpu", batch_size=B, buffer_size=64 * N, **pk)
    assert len(model.critic.q_networks) == n_critics
    model.set_logger(Logger(folder=None, output_formats=[]))
    rng = np.random.default_rng(99)
    out = {}
    if her:
        out.update(_fill_her(model, venv, rng, 40))
    else:
        _fill_buffer(model, rng, 40, N, D, A)
    out.update(_flat_sd("before/actor", model.actor.state_dict()))
    out.update(_flat_sd("before/critic", model.critic.state_dict()))
    out.update(_flat_sd("before/critic_target", model.critic_target.state_dict()))
    out["before/log_ent_coef"] = model.log_ent_coef.detach().numpy().copy()
    rb = model.replay_buffer
    if not her:
        out.update(ring_obs=rb.observations.copy(), ring_next_obs=rb.next_observations.copy(), ring_act=rb.actions.copy(),
                   ring_rew=rb.rewards.copy(), ring_done=rb.dones.copy(), ring_timeout=rb.timeouts.copy(),
                   ring_pos=np.int64(rb.pos), ring_full=np.uint8(rb.full))
    np.random.seed(2024)
    th.manual_seed(77)
    orig_sample = rb.sample
    batches = []

    def rec_sample(batch_size, env=None):
        s = orig_sample(batch_size, env=env)
        batches.append(_flat_batch(s) if her else [x.numpy().copy() for x in s])
        return s

    rb.sample = rec_sample
    tdn._standard_normal = rec_sn
    sacmod.F = FProxy()
    try:
        for k in range(n_steps):
            model.train(gradient_steps=1, batch_size=B)
            lv = model.logger.name_to_value
            out[f"step{k}/critic_loss"] = np.float32(lv["train/critic_loss"])
            out[f"step{k}/actor_loss"] = np.float32(lv["train/actor_loss"])
            out[f"step{k}/ent_coef_loss"] = np.float32(lv["train/ent_coef_loss"])
            out[f"step{k}/ent_coef"] = np.float32(lv["train/ent_coef"])
    finally:
        tdn._standard_normal = orig_sn
        sacmod.F = F_real
        rb.sample = orig_sample
    assert len(rec.eps) == 2 * n_steps and len(rec.mse) == n_critics * n_steps
    if sde is not None:  # per gradient step: reset_noise()'s exploration_mat, then exploration_matrices
        out["init/z_mat"], out["init/z_mats"] = init_draws[0].numpy(), init_draws[1].numpy()
    for k in range(n_steps):
        for fi, fname in enumerate(["observations", "actions", "next_observations", "dones", "rewards"]):
            out[f"step{k}/batch_{fname}"] = batches[k][fi]
        if sde is not None:
            out[f"step{k}/z_mat"] = rec.eps[2 * k].numpy()
            out[f"step{k}/z_mats"] = rec.eps[2 * k + 1].numpy()
        else:
            out[f"step{k}/eps_pi"] = rec.eps[2 * k].numpy()
            out[f"step{k}/eps_next"] = rec.eps[2 * k + 1].numpy()
        for i in range(n_critics):
            out[f"step{k}/current_q{i + 1}"] = rec.mse[n_critics * k + i][0].numpy()
        out[f"step{k}/target_q"] = rec.mse[n_critics * k][1].numpy()
    out.update(_flat_sd("after/actor", model.actor.state_dict()))
    out.update(_flat_sd("after/critic", model.critic.state_dict()))
    out.update(_flat_sd("after/critic_target", model.critic_target.state_dict()))
    out["after/log_ent_coef"] = model.log_ent_coef.detach().numpy().copy()
    out["hyper"] = np.array([model.gamma, model.tau, model.target_entropy, model.lr_schedule(1), B, n_steps], np.float64)
    out["np_seed"], out["th_seed"] = np.int64(2024), np.int64(77)
    if net_arch is None:
        # keep the committed fixture small: weights are reproducible from seed 0 (checked by the
        # init KAT), so store only digests of the big tensors for the default-size nets
        out = slim_weights(out, with_shape=False)
    if her:
        return save(f"sac_her_train_kat_{tag}.npz", **out)
    save(f"sac_sde_train_kat_{tag[len('sde_'):]}.npz" if sde is not None else f"sac_train_kat_{tag}.npz", **out)


def gen_td3():
    _gen_td3("small")
    _gen_td3("default")


def gen_ddpg():
    _gen_td3("small", algo="ddpg")
    _gen_td3("default", algo="ddpg")


def gen_td3_ncrit():
    """TD3 with policy_kwargs n_critics=3 (core/td3/td3.py:174-175, :182): small nets, four steps (two policy updates)."""
    _gen_td3("small", n_critics=3)


def _gen_td3(tag, algo="td3", n_critics=None, her=False):
    """tag "small": net_arch [48, 32], batch 64; "default": the class default [400, 300] (td3/policies.py:141-145), batch 256.
    algo "ddpg": core/ddpg/ddpg.py:14-130 -- TD3.train with policy_delay 1, ONE critic (one mse_loss per step) and a
    target-smoothing draw clamped to [-0, 0] (target_policy_noise 0.1, target_noise_clip 0.0).
    n_critics: policy_kwargs n_critics (None: the class default), written as {algo}_train_kat_ncrit{n}.npz."""
    import torch.nn.functional as F_real

    import core.td3.td3 as td3mod
    from core.common.logger import Logger
    from core.td3.td3 import TD3

    if algo == "ddpg":
        from core.ddpg.ddpg import DDPG as TD3
    n_q = n_critics or (1 if algo == "ddpg" else 2)

    rec = _Recorder()

    class FProxy:
        def __getattr__(self, name):
            return getattr(F_real, name)

        @staticmethod
        def mse_loss(a, b, *args, **kw):
            rec.mse.append((a.detach().clone(), b.detach().clone()))
            return F_real.mse_loss(a, b, *args, **kw)

    N, D, A, n_steps = 4, 4, 2, 4
    B = 64 if tag == "small" else 256
    venv = _make_goal_venv(_HER_STEPS, _HER_TARGETS) if her else _make_venv(N)
    pk = dict(policy_kwargs=dict(net_arch=[48, 32])) if tag == "small" else {}
    if her:
        pk.update(_her_kwargs())
    if n_critics is not None:
        pk.setdefault("policy_kwargs", {})["n_critics"] = n_critics
    model = TD3("MultiInputPolicy" if her else "MlpPolicy", venv, seed=0, device="cpu", batch_size=B, buffer_size=64 * N, **pk)
    model.set_logger(Logger(folder=None, output_formats=[]))
    rng = np.random.default_rng(314)
    out = {}
    if her:
        out.update(_fill_her(model, venv, rng, 40))
    else:
        _fill_buffer(model, rng, 40, N, D, A)
    for nm in ("actor", "actor_target", "critic", "critic_target"):
        out.update(_flat_sd(f"before/{nm}", getattr(model, nm).state_dict()))
    rb = model.replay_buffer
    if not her:
        out.update(ring_obs=rb.observations.copy(), ring_next_obs=rb.next_observations.copy(), ring_act=rb.actions.copy(),
                   ring_rew=rb.rewards.copy(), ring_done=rb.dones.copy(), ring_timeout=rb.timeouts.copy(),
                   ring_pos=np.int64(rb.pos), ring_full=np.uint8(rb.full))
    np.random.seed(555)
    orig_sample = rb.sample
    batches = []

    def rec_sample(batch_size, env=None):
        s = orig_sample(batch_size, env=env)
        batches.append(_flat_batch(s) if her else [x.numpy().copy() for x in s])
        return s

    rb.sample = rec_sample
    td3mod.F = FProxy()
    try:
        for k in range(n_steps):
            th.manual_seed(1000 + k)
            # the target-smoothing noise td3.py:169 is the first torch-RNG consumer of the step
            g = th.Generator().manual_seed(1000 + k)
            out[f"step{k}/noise_raw"] = th.empty(B, A).normal_(0, model.target_policy_noise, generator=g).numpy()
            model.train(gradient_steps=1, batch_size=B)
            lv = model.logger.name_to_value
            out[f"step{k}/critic_loss"] = np.float32(lv["train/critic_loss"])
            if model._n_updates % model.policy_delay == 0:
                out[f"step{k}/actor_loss"] = np.float32(lv["train/actor_loss"])
    finally:
        td3mod.F = F_real
        rb.sample = orig_sample
    assert len(rec.mse) == n_q * n_steps and len(model.critic.q_networks) == n_q
    for k in range(n_steps):
        for fi, fname in enumerate(["observations", "actions", "next_observations", "dones", "rewards"]):
            out[f"step{k}/batch_{fname}"] = batches[k][fi]
        for i in range(n_q):
            out[f"step{k}/current_q{i + 1}"] = rec.mse[n_q * k + i][0].numpy()
        out[f"step{k}/target_q"] = rec.mse[n_q * k][1].numpy()
    for nm in ("actor", "actor_target", "critic", "critic_target"):
        out.update(_flat_sd(f"after/{nm}", getattr(model, nm).state_dict()))
    out["hyper"] = np.array([model.gamma, model.tau, model.target_policy_noise, model.target_noise_clip,
                             model.policy_delay, model.lr_schedule(1), B, n_steps], np.float64)
    out["np_seed"] = np.int64(555)
    if her:
        save(f"{algo}_her_train_kat_{tag}.npz", **out)
    elif n_critics is not None:
        save(f"{algo}_train_kat_ncrit{n_critics}.npz", **out)
    elif tag == "default":
        assert model.actor.mu[0].out_features == 400 and model.actor.mu[2].out_features == 300
        save(f"{algo}_train_kat_default.npz", **slim_weights(out))
    else:
        save(f"{algo}_train_kat.npz", **out)


def gen_iddpg():
    gen_maddpg(algo="iddpg")


def gen_maddpg_default():
    gen_maddpg(tag="default")


class _BoxOnlyEnv:
    """Harness-side env for learner fixtures whose shape no reference env has (BASELINE config 5: 4 agents, 8 obs / 4 act):
    MADDPG.train() (maddpg.py:117-191) uses the env's SPACES only -- the batch comes from the injected ring rows."""

    def __new__(cls, D, A):
        import gymnasium
        from gymnasium import spaces

        class BoxOnly(gymnasium.Env):
            observation_space = spaces.Box(-1, 1, (D,), np.float32)
            action_space = spaces.Box(-1, 1, (A,), np.float32)

            def reset(self, *, seed=None, options=None):
                return np.zeros(D, np.float32), {}

            def step(self, action):
                return np.zeros(D, np.float32), 0.0, False, False, {}

        return BoxOnly()


def gen_maddpg4_default():
    gen_maddpg(tag="default", n_agents=4)


def gen_maddpg4():
    gen_maddpg(tag="small", n_agents=4)


def gen_maddpg(algo="maddpg", tag="small", n_agents=2):
    """MADDPG / IDDPG on the natural 2-agent split of the CSTR env: agent 0 = reactor 1 ([C1,T1] -> F1), agent 1 = reactor 2.
    tag "default": the class-default per-agent nets [400, 300] (maddpg/policies.py:344-353), batch 256.
    n_agents=4: BASELINE config 5's learner shape -- 8 obs / 4 act, one agent per (C, T) pair and coolant flow
    (obs splits [[0,1],[2,3],[4,5],[6,7]], act splits [[0],[1],[2],[3]]); the env only supplies the spaces."""
    import torch.nn.functional as F_real

    from core.common.logger import Logger
    if algo == "maddpg":
        import core.maddpg.maddpg as mmod
        from core.maddpg.maddpg import MADDPG
    else:
        import core.iddpg.iddpg as mmod
        from core.iddpg.iddpg import IDDPG as MADDPG

    rec = _Recorder()

    class FProxy:
        def __getattr__(self, name):
            return getattr(F_real, name)

        @staticmethod
        def mse_loss(a, b, *args, **kw):
            rec.mse.append((a.detach().clone(), b.detach().clone()))
            return F_real.mse_loss(a, b, *args, **kw)

    N, D, A, n_steps = 4, 2 * n_agents, n_agents, 4
    B = 64 if tag == "small" else 256
    if n_agents == 2:
        venv = _make_venv(N)
    else:
        from core.common.vec_env.dummy_vec_env import DummyVecEnv

        venv = DummyVecEnv([lambda: _BoxOnlyEnv(D, A) for _ in range(N)])
    pk = dict(policy_kwargs=dict(net_arch=[[32, 24]] * n_agents)) if tag == "small" else {}
    model = MADDPG(n_agents, "MlpPolicy", venv, [[2 * a, 2 * a + 1] for a in range(n_agents)], [[a] for a in range(n_agents)],
                   learning_rate_list=[1e-3] * n_agents, seed=0, device="cpu", batch_size=B, buffer_size=64 * N, **pk)
    model.set_logger(Logger(folder=None, output_formats=[]))
    rng = np.random.default_rng(2718)
    _fill_buffer(model, rng, 40, N, D, A)
    out = {}
    for nm in ("actor", "actor_target", "critic", "critic_target"):
        out.update(_flat_sd(f"before/{nm}", getattr(model, nm).state_dict()))
    rb = model.replay_buffer
    out.update(ring_obs=rb.observations.copy(), ring_next_obs=rb.next_observations.copy(), ring_act=rb.actions.copy(),
               ring_rew=rb.rewards.copy(), ring_done=rb.dones.copy(), ring_timeout=rb.timeouts.copy(),
               ring_pos=np.int64(rb.pos), ring_full=np.uint8(rb.full))
    np.random.seed(777)
    orig_sample = rb.sample
    batches = []

    def rec_sample(batch_size, env=None):
        s = orig_sample(batch_size, env=env)
        batches.append([x.numpy().copy() for x in s])
        return s

    rb.sample = rec_sample
    mmod.F = FProxy()
    try:
        for k in range(n_steps):
            th.manual_seed(2000 + k)
            g = th.Generator().manual_seed(2000 + k)
            for a in range(n_agents):  # maddpg.py:137: one normal_ draw per agent, in agent order
                out[f"step{k}/noise_raw_agent{a}"] = th.empty(B, 1).normal_(0, model.target_policy_noise, generator=g).numpy()
            model.train(gradient_steps=1, batch_size=B)
            lv = model.logger.name_to_value
            for a in range(n_agents):
                out[f"step{k}/agent{a}_critic_loss"] = np.float32(lv[f"train/agent_{a}_critic_loss"])
                if model._n_updates % model.policy_delay == 0:
                    out[f"step{k}/agent{a}_actor_loss"] = np.float32(lv[f"train/agent_{a}_actor_loss"])
    finally:
        mmod.F = F_real
        rb.sample = orig_sample
    assert len(rec.mse) == 2 * n_agents * n_steps, len(rec.mse)
    for k in range(n_steps):
        for fi, fname in enumerate(["observations", "actions", "next_observations", "dones", "rewards"]):
            out[f"step{k}/batch_{fname}"] = batches[k][fi]
        for a in range(n_agents):
            base = 2 * n_agents * k + 2 * a
            out[f"step{k}/agent{a}_current_q1"] = rec.mse[base][0].numpy()
            out[f"step{k}/agent{a}_current_q2"] = rec.mse[base + 1][0].numpy()
            out[f"step{k}/agent{a}_target_q"] = rec.mse[base][1].numpy()
    for nm in ("actor", "actor_target", "critic", "critic_target"):
        out.update(_flat_sd(f"after/{nm}", getattr(model, nm).state_dict()))
    out["hyper"] = np.array([model.gamma, model.tau, model.target_policy_noise, model.target_noise_clip, model.policy_delay,
                             1e-3, B, n_steps, n_agents], np.float64)
    out["np_seed"] = np.int64(777)
    # the reference's _sample_action for multi-agent algos: no scaling, no noise (multiagent_policy_algorithm.py:369, 391-392)
    obs = rng.uniform(-1, 1, (N, D)).astype(np.float32)
    model._last_obs = obs
    model.num_timesteps = 10**6
    from core.common.noise import NormalActionNoise

    act, buf_act = model._sample_action(0, NormalActionNoise(np.zeros(1), np.ones(1)), N)
    pred, _ = model.predict(obs, deterministic=False)
    out.update(sa_obs=obs, sa_action=act, sa_buffer_action=buf_act, sa_predict=pred)
    name = algo if n_agents == 2 else f"{algo}{n_agents}"
    if tag == "default":
        shapes = sorted({tuple(v.shape) for k, v in out.items() if k.startswith("before/actor/") and v.ndim == 2})
        assert (400, 2) in shapes and (300, 400) in shapes, shapes
        save(f"{name}_train_kat_default.npz", **slim_weights(out))
    else:
        save(f"{name}_train_kat.npz", **out)


def gen_config1():
    """BASELINE config 1 (plumbing): the unmodified reference SAC("MlpPolicy") at the class defaults on ONE CSTR env, learn(10_000)
    on the CPU. Recorded: the counters and the global legacy numpy stream afterwards. With n_envs = 1 the env-index draw
    `randint(0, high=1)` consumes nothing (buffers.py:309), so the stream position is a function of the row-index draws only."""
    import time

    from core.common.logger import Logger
    from core.sac.sac import SAC

    seed, total = 0, 10_000
    model = SAC("MlpPolicy", _make_venv(1), seed=seed, device="cpu")
    model.set_logger(Logger(folder=None, output_formats=[]))
    t0 = time.time()
    model.learn(total)
    dt = time.time() - t0
    st = np.random.get_state()
    rb = model.replay_buffer
    save("config1_sac_single_env_kat.npz", seed=np.int64(seed), total_timesteps=np.int64(total), num_timesteps=np.int64(model.num_timesteps),
         n_updates=np.int64(model._n_updates), episode_num=np.int64(model._episode_num), ring_pos=np.int64(rb.pos), ring_full=np.uint8(rb.full),
         ring_rows=np.int64(rb.buffer_size), batch_size=np.int64(model.batch_size), learning_starts=np.int64(model.learning_starts),
         mt_key=st[1].astype(np.uint32), mt_pos=np.int32(st[2]), mt_has_gauss=np.int32(st[3]),
         reference_env_steps_per_s=np.float64(total / dt), actor_adam_step=np.float64(float(model.actor.optimizer.state_dict()["state"][0]["step"])),
         dones_sum=np.float64(rb.dones[:rb.pos].sum()), timeouts_sum=np.float64(rb.timeouts[:rb.pos].sum()))
    print(f"reference SAC, 1 env, {total} steps: {total / dt:.1f} env-steps/s on this container (1 torch thread)")


def gen_checkpoint():
    """A checkpoint WRITTEN BY THE REFERENCE (SAC.save, base_class.py:842-888) after two gradient steps, plus the
    deterministic predictions of the saved model: the product's SAC.load must read it (weights_only tensors + JSON)."""
    from core.common.logger import Logger
    from core.sac.sac import SAC

    N, D, A, B = 4, 4, 2, 64
    model = SAC("MlpPolicy", _make_venv(N), seed=0, device="cpu", batch_size=B, buffer_size=64 * N, learning_starts=77, gamma=0.98,
                policy_kwargs=dict(net_arch=[64, 64]))
    model.set_logger(Logger(folder=None, output_formats=[]))
    rng = np.random.default_rng(4242)
    _fill_buffer(model, rng, 40, N, D, A)
    np.random.seed(1)
    th.manual_seed(1)
    model.train(gradient_steps=2, batch_size=B)
    model.num_timesteps = 1234
    path = os.path.join(OUT, "sac_reference_checkpoint.zip")
    model.save(path)
    obs = rng.uniform(-1, 1, (16, D)).astype(np.float32)
    pred, _ = model.predict(obs, deterministic=True)
    with th.no_grad():
        q1, q2 = model.critic(th.as_tensor(obs), th.as_tensor(pred))
    opt = model.critic.optimizer.state_dict()
    save("sac_reference_checkpoint_kat.npz", obs=obs, pred=pred, q1=q1.numpy(), q2=q2.numpy(), log_ent_coef=model.log_ent_coef.detach().numpy(),
         critic_adam_step=np.float32(float(opt["state"][0]["step"])), critic_exp_avg0=opt["state"][0]["exp_avg"].numpy(),
         n_updates=np.int64(model._n_updates))
    print("wrote", path, os.path.getsize(path))


def gen_eval():
    """The reference's evaluate_policy (core/common/evaluation.py:11-140) over DummyVecEnv([TwoSeriesCSTREnv] * N):
    (a) a replaying predictor (any object with predict(), evaluation.py:88-93) over a fixed action tape with out-of-range
        actions and two NaN actions (-> the env's exception path ends that episode early, twoseriescstr.py:413-421),
        n_eval_episodes = 7 over 3 envs (targets [2, 2, 3], evaluation.py:79-82): per-episode returns (f64 sums of f32 rewards),
        lengths, their order, and the (mean, std) form;
    (b) the seeded, untrained SAC / TD3 policies at the class defaults, deterministic=True, 6 episodes over 4 envs."""
    import contextlib
    import io

    from core.common.evaluation import evaluate_policy
    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from core.sac.sac import SAC
    from core.td3.td3 import TD3
    from twoseriescstr import TwoSeriesCSTREnv

    N, n_eval, T = 3, 7, 1300
    rng = np.random.default_rng(808)
    tape = rng.uniform(-1.2, 1.2, size=(T, N, 2)).astype(np.float32)
    tape[137, 0, 1] = np.nan    # env 0's first episode ends at length 138
    tape[655, 2, 0] = np.nan    # env 2's second episode ends at length 256

    class Tape:
        def __init__(self):
            self.t = 0

        def predict(self, observations, state=None, episode_start=None, deterministic=False):
            a = tape[self.t].copy()
            self.t += 1
            return a, state

    def run(model, n_envs, seed, n_episodes, **kw):
        venv = DummyVecEnv([lambda: TwoSeriesCSTREnv() for _ in range(n_envs)])
        venv.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            return evaluate_policy(model, venv, n_eval_episodes=n_episodes, warn=False, **kw)

    out = dict(tape=tape, tape_dims=np.array([N, n_eval, 11], np.int64))
    tm = Tape()
    rets, lens = run(tm, N, 11, n_eval, return_episode_rewards=True)
    out.update(tape_returns=np.asarray(rets, np.float64), tape_lengths=np.asarray(lens, np.int64), tape_steps_used=np.int64(tm.t))
    mean, std = run(Tape(), N, 11, n_eval)
    out.update(tape_mean=np.float64(mean), tape_std=np.float64(std))
    for name, cls in (("sac", SAC), ("td3", TD3)):
        model = cls("MlpPolicy", DummyVecEnv([lambda: TwoSeriesCSTREnv() for _ in range(2)]), seed=0, device="cpu")
        rets, lens = run(model, 4, 5, 6, deterministic=True, return_episode_rewards=True)
        out[f"{name}_returns"], out[f"{name}_lengths"] = np.asarray(rets, np.float64), np.asarray(lens, np.int64)
    out["model_dims"] = np.array([4, 6, 5, 0], np.int64)  # n_envs, n_eval_episodes, env seed, model seed
    save("evaluate_policy_kat.npz", **out)


def gen_evalmodel():
    """The reference's evaluate_model (twoseriescstr.py:522-588), unmodified, under the Agg backend: a seeded, untrained TD3 with
    net_arch [16, 16] on DummyVecEnv([TwoSeriesCSTREnv(init_mode=m)]) for m in static, random; 3 episodes each. Stored per mode: the
    returned episode_rewards and episode_states [3, 400, 4], and the actions `model.predict` returned, taken by a recording proxy around
    the model (the reference only calls `.predict` on it); once: the actor's weights and the env seed."""
    import contextlib
    import io

    os.environ["MPLBACKEND"] = "Agg"
    import matplotlib

    matplotlib.use("Agg", force=True)
    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from core.td3.td3 import TD3
    from twoseriescstr import TwoSeriesCSTREnv, evaluate_model

    env_seed, model_seed, n_episodes = 21, 4, 3

    class Recorder:
        def __init__(self, model):
            self.model, self.actions = model, []

        def predict(self, *a, **kw):
            out = self.model.predict(*a, **kw)
            self.actions.append(np.array(out[0], np.float32).reshape(-1))
            return out

    model = TD3("MlpPolicy", DummyVecEnv([lambda: TwoSeriesCSTREnv()]), seed=model_seed, device="cpu", policy_kwargs=dict(net_arch=[16, 16]))
    sd = {k: v.detach().cpu().numpy().copy() for k, v in model.actor.mu.state_dict().items()}
    out = dict(dims=np.array([env_seed, model_seed, n_episodes, 16, 16], np.int64), w1=sd["0.weight"], b1=sd["0.bias"], w2=sd["2.weight"],
               b2=sd["2.bias"], w3=sd["4.weight"], b3=sd["4.bias"])
    for mode in ("static", "random"):
        venv = DummyVecEnv([lambda: TwoSeriesCSTREnv(init_mode=mode)])
        venv.seed(env_seed)
        rec = Recorder(model)
        with contextlib.redirect_stdout(io.StringIO()):
            rewards, states = evaluate_model(rec, venv, num_episodes=n_episodes)
        assert states.shape == (n_episodes, 400, 4) and len(rec.actions) == n_episodes * 400
        out[f"{mode}/episode_rewards"] = np.asarray(rewards, np.float64)
        out[f"{mode}/episode_rewards_dtype"] = np.array(str(np.asarray(rewards).dtype))
        out[f"{mode}/episode_states"] = np.asarray(states)
        out[f"{mode}/actions"] = np.stack(rec.actions).reshape(n_episodes, 400, 2)
    save("evaluate_model_kat.npz", **out)


def gen_info():
    """The 16-key `info` dict of TwoSeriesCSTREnv.step (twoseriescstr.py:441-452) with the nine compute_reward diagnostics (:379-389),
    five of which carry weight 0.0 and per-env memory: a seeded 80-step trajectory that approaches the target (stability counter runs),
    leaves it, and is reset in between (memory cleared)."""
    from twoseriescstr import TwoSeriesCSTREnv

    env = TwoSeriesCSTREnv()
    rng = np.random.default_rng(77)
    keys = ["concentration_reward", "concentration_proximity_reward", "concentration_trend_reward", "stability_reward", "temp_penalty",
            "action_smoothness_penalty", "extreme_penalty", "concentration_error", "stable_steps"]
    T = 80
    acts = rng.uniform(-1, 1, (T, 2)).astype(np.float32)
    acts[0:36] = np.array([0.34522182, 0.3167114], np.float32) + rng.normal(0, 0.01, (36, 2)).astype(np.float32)  # a calm stretch near the target
    acts[60] = np.array([1.7, -2.0], np.float32)
    starts = {0: np.array([-0.59437853, 0.23396769, -0.42535093, 0.3727205], np.float32), 45: np.array([0.9, 0.9, 0.95, 0.8], np.float32)}
    out = {k: np.zeros(T, np.float64) for k in keys}
    obs_next, rew, raw_next, raw_act, step_no = np.zeros((T, 4), np.float32), np.zeros(T, np.float32), np.zeros((T, 4), np.float32), np.zeros((T, 2), np.float32), np.zeros(T, np.int64)
    for t in range(T):
        if t in starts:
            env.reset(seed=1)
            env.state = starts[t].copy()
        s, r, te, tr, info = env.step(acts[t].copy())
        assert set(info) == set(keys) | {"reward", "raw_action", "truncated", "state", "original_state", "target_C2", "step"}
        for k in keys:
            out[k][t] = info[k]
        obs_next[t], rew[t], raw_next[t], raw_act[t], step_no[t] = s, r, info["original_state"], info["raw_action"], info["step"]
    save("env_info_kat.npz", actions=acts, reset_at=np.array(sorted(starts), np.int64), reset_state=np.stack([starts[k] for k in sorted(starts)]),
         obs_next=obs_next, reward=rew, original_state=raw_next, raw_action=raw_act, step=step_no, **out)


def gen_init():
    """Initial weights of the reference policies for seed 0 (construction order = RNG order)."""
    from core.sac.sac import SAC
    from core.td3.td3 import TD3

    out = {}
    for name, cls in (("sac", SAC), ("td3", TD3)):
        for seed in (0, 5):
            model = cls("MlpPolicy", _make_venv(2), seed=seed, device="cpu")
            mods = ["actor", "critic", "critic_target"] + (["actor_target"] if name == "td3" else [])
            for nm in mods:
                for k, v in getattr(model, nm).state_dict().items():
                    a = v.numpy()
                    out[f"{name}{seed}/{nm}/{k}#shape"] = np.array(a.shape, np.int64)
                    out[f"{name}{seed}/{nm}/{k}#sum"] = np.float64(a.astype(np.float64).sum())
                    out[f"{name}{seed}/{nm}/{k}#head"] = a.reshape(-1)[:16].copy()
            # global legacy numpy stream after construction (seed clobbering is in reset, see SURVEY a-6)
            st = np.random.get_state()
            out[f"{name}{seed}/np_key_head"] = st[1][:8].astype(np.uint32)
            out[f"{name}{seed}/np_pos"] = np.int32(st[2])
            model._setup_learn(100, None)
            st = np.random.get_state()
            out[f"{name}{seed}/np_key_head_after_setup_learn"] = st[1][:8].astype(np.uint32)
            out[f"{name}{seed}/np_pos_after_setup_learn"] = np.int32(st[2])
    save("policy_init_kat.npz", **out)


def gen_resets():
    """TwoSeriesCSTREnv.reset (twoseriescstr.py:226-269) in both init modes: seeded first reset, then unseeded resets that
    continue the env's generator; "static" also records the drifting f64 init_state. The generator behind
    `self.np_random` is the harness stand-in's Generator(PCG64(SeedSequence(seed))) = gymnasium's documented construction."""
    from twoseriescstr import TwoSeriesCSTREnv

    seeds, n_resets = [0, 1, 7, 42, 4095, 123456], 6
    out = {"seeds": np.array(seeds, np.int64)}
    for mode in ("random", "static"):
        obs = np.zeros((len(seeds), n_resets, 4), np.float32)
        init = np.zeros((len(seeds), n_resets, 4), np.float64)
        for i, sd in enumerate(seeds):
            env = TwoSeriesCSTREnv(init_mode=mode)
            for k in range(n_resets):
                o, info = env.reset(seed=sd) if k == 0 else env.reset()
                assert o.dtype == np.float32
                obs[i, k] = o
                if mode == "static":
                    init[i, k] = env.init_state
            # a few steps between resets must not touch the reset stream
        out[f"{mode}_obs"] = obs
        if mode == "static":
            out["static_init_state"] = init
    # static mode through the vectorised env: auto-reset draws continue each env's own stream
    from core.common.vec_env.dummy_vec_env import DummyVecEnv

    N, T = 3, 5
    venv = DummyVecEnv([lambda: TwoSeriesCSTREnv(init_mode="static") for _ in range(N)])
    venv.seed(21)
    o0 = venv.reset()
    step0 = np.array([398, 399, 397], np.int32)
    for i, e in enumerate(venv.envs):
        e.current_step = int(step0[i])
    rng = np.random.default_rng(3)
    actions = rng.uniform(-1, 1, size=(T, N, 2)).astype(np.float32)
    obs = np.zeros((T, N, 4), np.float32)
    done = np.zeros((T, N), np.uint8)
    for k in range(T):
        o, r, d, infos = venv.step(actions[k])
        obs[k], done[k] = o, d
    out.update(vec_seed=np.int64(21), vec_obs0=o0, vec_step0=step0, vec_actions=actions, vec_obs=obs, vec_done=done,
               vec_init_state=np.stack([e.init_state for e in venv.envs]))
    save("env_reset_kat.npz", **out)


def gen_vecnorm():
    """The reference's VecNormalize / RunningMeanStd (core/common/vec_env/vec_normalize.py:174-290,
    core/common/running_mean_std.py) driven by a replaying inner VecEnv: inputs are the raw obs / reward / done sequences,
    outputs the normalised obs / rewards and the running statistics after every step, plus normalize_obs /
    normalize_reward of a held-out batch as ReplayBuffer._get_samples applies them (buffers.py:143-155, :312-323)."""
    from core.common.vec_env.base_vec_env import VecEnv
    from core.common.vec_env.vec_normalize import VecNormalize
    from gymnasium import spaces

    N, D, T = 48, 4, 25
    rng = np.random.default_rng(5)
    scale, shift = np.array([0.3, 2.0, 0.05, 7.0]), np.array([0.1, -1.0, 0.0, 3.0])
    raw_obs = (rng.normal(size=(T + 1, N, D)) * scale + shift).astype(np.float32)
    raw_rew = (rng.normal(size=(T, N)) * 5.0 - 20.0).astype(np.float32)
    done = (rng.uniform(size=(T, N)) < 0.08)

    class Replay(VecEnv):
        def __init__(self):
            super().__init__(N, spaces.Box(-np.inf, np.inf, (D,), np.float32), spaces.Box(-1, 1, (2,), np.float32))
            self.k = 0

        def reset(self):
            self.k = 0
            return raw_obs[0].copy()

        def step_async(self, actions):
            pass

        def step_wait(self):
            k = self.k
            self.k += 1
            return raw_obs[k + 1].copy(), raw_rew[k].copy(), done[k].copy(), [{} for _ in range(N)]

        def close(self):
            pass

        def get_attr(self, attr_name, indices=None):
            return [None] * N

        def set_attr(self, attr_name, value, indices=None):
            pass

        def env_method(self, method_name, *a, indices=None, **kw):
            return [None] * N

        def env_is_wrapped(self, wrapper_class, indices=None):
            return [False] * N

    out = dict(raw_obs=raw_obs, raw_rew=raw_rew, done=done.astype(np.uint8))
    held_obs = (rng.normal(size=(64, D)) * scale * 3 + shift).astype(np.float32)
    held_rew = (rng.normal(size=(64, 1)) * 30.0 - 20.0).astype(np.float32)
    out.update(held_obs=held_obs, held_rew=held_rew)
    for tag, kw in (("default", {}), ("tight", dict(clip_obs=1.5, clip_reward=0.8, gamma=0.9, epsilon=1e-4)),
                    ("obs_only", dict(norm_reward=False)), ("rew_only", dict(norm_obs=False))):
        vn = VecNormalize(Replay(), **kw)
        o = vn.reset()
        n_obs, n_rew = [o], []
        stats = []
        for k in range(T):
            if tag == "default" and k == 18:
                vn.training = False  # frozen statistics for the tail
            o, r, d, _ = vn.step(np.zeros((N, 2), np.float32))
            n_obs.append(o)
            n_rew.append(r)
            om = vn.obs_rms if vn.norm_obs else None
            stats.append(np.concatenate([om.mean if om else np.zeros(D), om.var if om else np.ones(D), [om.count if om else 0.0],
                                         [vn.ret_rms.mean, vn.ret_rms.var, vn.ret_rms.count]]))
            assert np.array_equal(vn.get_original_obs(), raw_obs[k + 1]) and np.array_equal(vn.get_original_reward(), raw_rew[k])
        out[f"{tag}_norm_obs"] = np.stack(n_obs).astype(np.float32)
        out[f"{tag}_norm_rew"] = np.stack(n_rew).astype(np.float32)
        out[f"{tag}_stats"] = np.stack(stats)
        out[f"{tag}_returns"] = vn.returns.copy()
        out[f"{tag}_held_obs"] = vn.normalize_obs(held_obs)
        out[f"{tag}_held_rew"] = vn.normalize_reward(held_rew).astype(np.float32)
        out[f"{tag}_unnorm_obs"] = np.asarray(vn.unnormalize_obs(out[f"{tag}_held_obs"]), np.float64)
        out[f"{tag}_unnorm_rew"] = np.asarray(vn.unnormalize_reward(out[f"{tag}_held_rew"]), np.float64)
    save("vecnormalize_kat.npz", **out)


# --------------------------------------------------------------------------------------- BCQ
def _bcq_dataset(tmpdir, n_rows, D=4, A=2, seed=2718):
    """A pickle of the reference's own ReplayBuffer (one env, `_fill_buffer`-style seeded rows): what BCQ(dataset=<path>) loads
    (core/common/offline_policy_algorithm.py:196-242)."""
    import types

    from core.common.buffers import ReplayBuffer
    from core.common.save_util import save_to_pkl
    from gymnasium import spaces

    buf = ReplayBuffer(n_rows + 56, spaces.Box(-1, 1, (D,), np.float32), spaces.Box(-1, 1, (A,), np.float32), device="cpu", n_envs=1)
    _fill_buffer(types.SimpleNamespace(replay_buffer=buf), np.random.default_rng(seed), n_rows, 1, D, A)
    path = os.path.join(tmpdir, "bcq_dataset.pkl")
    save_to_pkl(path, buf, 0)
    return path


class _BcqHooks:
    """th.randn / th.randn_like of core/bcq/policies.py and F.mse_loss of core/bcq/bcq.py, recorded in call order."""

    def __init__(self):
        import torch.nn.functional as F_real

        import core.bcq.bcq as bcqmod
        import core.bcq.policies as polmod

        self.draws, self.mse, self.F_real, self.bcqmod, self.polmod = [], [], F_real, bcqmod, polmod
        hooks = self

        class ThProxy:
            def __getattr__(self, name):
                return getattr(th, name)

            @staticmethod
            def randn(*a, **k):
                e = th.randn(*a, **k)
                hooks.draws.append(e.clone())
                return e

            @staticmethod
            def randn_like(*a, **k):
                e = th.randn_like(*a, **k)
                hooks.draws.append(e.clone())
                return e

        class FProxy:
            def __getattr__(self, name):
                return getattr(F_real, name)

            @staticmethod
            def mse_loss(a, b, *args, **kw):
                hooks.mse.append((a.detach().clone(), b.detach().clone()))
                return F_real.mse_loss(a, b, *args, **kw)

        self._th, self._F = ThProxy(), FProxy()

    def __enter__(self):
        self.polmod.th, self.bcqmod.F = self._th, self._F
        return self

    def __exit__(self, *exc):
        self.polmod.th, self.bcqmod.F = th, self.F_real


def _bcq_train(tag, tmpdir):
    """The teacher-forced BCQ run (core/bcq/bcq.py:129-213): returns (model, out). Per step: th.manual_seed(1000 + k), so the three
    draws -- randn_like [B, L] (policies.py:82), randn [10B, L] (:123), on actor steps randn [B, L] (:123) -- are the first
    consumers of a generator seeded with `step{k}/th_seed`; the [10B, L] draw is stored as that seed + digests."""
    from core.bcq.bcq import BCQ
    from core.common.logger import Logger

    D, A = 4, 2
    B, n_steps = (64, 4) if tag == "small" else (256, 2)
    pk = dict(policy_kwargs=dict(critic_net_arch=[64, 64])) if tag == "small" else {}
    model = BCQ("MlpPolicy", _make_venv(1), dataset=_bcq_dataset(tmpdir, 200), seed=0, device="cpu", batch_size=B, **pk)
    model.set_logger(Logger(folder=None, output_formats=[]))
    L = model.actor.vae.latent_dim
    out = {}
    mods = ("actor", "actor_target", "critic", "critic_target")
    for nm in mods:
        out.update(_flat_sd(f"before/{nm}", getattr(model, nm).state_dict()))
    out["state_dict_keys"] = np.array(list(model.policy.state_dict().keys()))
    rb = model.replay_buffer
    assert rb.n_envs == 1 and rb.size() == 200
    out.update(ring_obs=rb.observations.copy(), ring_next_obs=rb.next_observations.copy(), ring_act=rb.actions.copy(),
               ring_rew=rb.rewards.copy(), ring_done=rb.dones.copy(), ring_timeout=rb.timeouts.copy(),
               ring_pos=np.int64(rb.pos), ring_full=np.uint8(rb.full))
    np.random.seed(777)
    orig_sample = rb.sample
    batches = []

    def rec_sample(batch_size, env=None):
        s = orig_sample(batch_size, env=env)
        batches.append([x.numpy().copy() for x in s])
        return s

    rb.sample = rec_sample
    with _BcqHooks() as hk:
        try:
            for k in range(n_steps):
                th.manual_seed(1000 + k)
                d0, m0 = len(hk.draws), len(hk.mse)
                model.train(gradient_steps=1, batch_size=B)
                actor_step = model._n_updates % model.actor_delay == 0
                draws, mse = hk.draws[d0:], hk.mse[m0:]
                assert len(draws) == (3 if actor_step else 2) and len(mse) == 3
                assert tuple(draws[0].shape) == (B, L) and tuple(draws[1].shape) == (10 * B, L)
                gen = th.Generator().manual_seed(1000 + k)  # the stored seed reproduces the draws
                assert th.equal(th.randn(B, L, generator=gen), draws[0]) and th.equal(th.randn(10 * B, L, generator=gen), draws[1])
                out[f"step{k}/th_seed"] = np.int64(1000 + k)
                out[f"step{k}/draw_vae"] = draws[0].numpy()
                out[f"step{k}/draw_target#sum"] = np.float64(draws[1].double().sum())
                out[f"step{k}/draw_target#head"] = draws[1].reshape(-1)[:64].numpy().copy()
                if actor_step:
                    assert th.equal(th.randn(B, L, generator=gen), draws[2])
                    out[f"step{k}/draw_actor"] = draws[2].numpy()
                out[f"step{k}/recon"] = mse[0][0].numpy()
                out[f"step{k}/current_q1"], out[f"step{k}/current_q2"] = mse[1][0].numpy(), mse[2][0].numpy()
                out[f"step{k}/target_q"] = mse[1][1].numpy()
                lv = model.logger.name_to_value
                out[f"step{k}/vae_loss"] = np.float32(lv["train/vae_loss"])
                out[f"step{k}/critic_loss"] = np.float32(lv["train/critic_loss"])
                if actor_step:
                    out[f"step{k}/actor_loss"] = np.float32(lv["train/actor_loss"])
                for fi, fname in enumerate(["observations", "actions", "next_observations", "dones", "rewards"]):
                    out[f"step{k}/batch_{fname}"] = batches[k][fi]
        finally:
            rb.sample = orig_sample
    for nm in mods:
        out.update(_flat_sd(f"after/{nm}", getattr(model, nm).state_dict()))
    out["hyper"] = np.array([model.gamma, model.tau, model.actor_delay, model.lr_schedule(1), B, n_steps, L,
                             model.actor.perturbation.max_perturbation], np.float64)
    out["np_seed"] = np.int64(777)
    out["n_params"] = np.array([sum(p.numel() for g in o.param_groups for p in g["params"])
                                for o in (model.actor.vae_optimizer, model.actor.perturbation_optimizer, model.critic.optimizer)], np.int64)
    return model, out


def gen_bcq():
    """BCQ.train (core/bcq/bcq.py:129-213): bcq_train_kat_small.npz (critics [64, 64], B = 64, 4 steps = two actor steps) and
    bcq_train_kat_default.npz (class defaults, B = 256, 2 steps, digests for the large tensors)."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        _, out = _bcq_train("small", tmp)
        save("bcq_train_kat_small.npz", **out)
        model, out = _bcq_train("default", tmp)
        assert [l.out_features for l in model.critic.q_networks[0] if hasattr(l, "out_features")] == [400, 300, 1]
        save("bcq_train_kat_default.npz", **slim_weights(out, with_shape=False))


def gen_bcq_predict():
    """BCQ.predict (core/bcq/policies.py:426-435) after the four steps of the small case on 64 seeded single observations. Every call
    is made with the generator seeded alike, so ONE raw [100, L] draw serves all of them. The 100 q1 values are the reference's own
    modules evaluated on the recorded draw (asserted to select the action predict() returned)."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        model, _ = _bcq_train("small", tmp)
    n_obs, S = 64, 100
    obs = np.random.default_rng(4242).uniform(-1, 1, (n_obs, 4)).astype(np.float32)
    out = dict(obs=obs, q1=np.zeros((n_obs, S), np.float32), action=np.zeros((n_obs, 2), np.float32),
               scaled_action=np.zeros((n_obs, 2), np.float32), index=np.zeros(n_obs, np.int64))
    pol = model.policy
    draw0 = None
    with _BcqHooks() as hk:
        for i in range(n_obs):
            th.manual_seed(4000)
            d0 = len(hk.draws)
            action, _ = model.predict(obs[i:i + 1], deterministic=True)
            (draw,) = hk.draws[d0:]
            draw0 = draw if draw0 is None else draw0
            assert th.equal(draw, draw0) and action.shape == (1, 2)
            with th.no_grad():
                rep = th.as_tensor(obs[i:i + 1]).repeat(S, 1)
                cand = pol.actor.perturbation(rep, pol.actor.vae.decode(rep, draw.clamp(-0.5, 0.5)))
                q1 = pol.critic.q1_forward(rep, cand)[:, 0]
            idx = int(q1.argmax())
            np.testing.assert_array_equal(pol.unscale_action(cand[idx:idx + 1].numpy()), action)
            out["q1"][i], out["action"][i], out["scaled_action"][i], out["index"][i] = q1.numpy(), action[0], cand[idx].numpy(), idx
    out["draw"] = draw0.numpy()
    top = np.sort(out["q1"], axis=1)
    gap = (top[:, -1] - top[:, -2]) / np.abs(top[:, -1])
    out["rel_gap"] = gap.astype(np.float64)
    close = float((gap <= 4 * 1e-4).mean())
    print(f"bcq predict: {100 * close:.1f} % of {n_obs} observations have a top-two relative q1 gap <= 4e-4; smallest {gap.min():.2e}")
    assert close <= 0.15
    out["low"], out["high"] = np.asarray(model.action_space.low, np.float32), np.asarray(model.action_space.high, np.float32)
    save("bcq_predict_kat.npz", **out)



# --------------------------------------------------------------------------------------- PPO
def _inner_env(e):
    """the TwoSeriesCSTREnv behind a DummyVecEnv member: itself, or what the goal face's wrapper (_make_goal_venv) holds as `inner`"""
    return getattr(e.unwrapped, "inner", e.unwrapped)


def _obs_rows(o):
    """observations as one float32 array; a dict of the goal face becomes its flat rows [achieved_goal | desired_goal | observation]"""
    if isinstance(o, dict):
        return np.concatenate([np.asarray(o[k], np.float32) for k in ("achieved_goal", "desired_goal", "observation")], axis=-1)
    return np.array(o, np.float32).copy()


class _PpoHooks:
    """Records, around the UNMODIFIED reference: every standard-normal draw of Normal.rsample, every np.random.permutation, the infos of
    every vec-step, and -- read from train()'s frame when it calls clip_grad_norm_ (core/ppo/ppo.py:277) -- each minibatch's values,
    log-probs, the six scalars and the gradient norm."""

    def __enter__(self):
        import sys as _sys

        import torch.distributions.normal as tdn
        from core.common.vec_env.dummy_vec_env import DummyVecEnv

        self.draws, self.perms, self.infos, self.minibatches = [], [], [], []
        self._tdn, self._std_normal = tdn, tdn._standard_normal
        self._perm, self._clip, self._step_wait, self._dummy = np.random.permutation, th.nn.utils.clip_grad_norm_, DummyVecEnv.step_wait, DummyVecEnv

        def std_normal(shape, dtype, device):
            e = self._std_normal(shape, dtype, device)
            self.draws.append(e.clone())
            return e

        def permutation(n):
            pm = self._perm(n)
            self.perms.append(np.asarray(pm).copy())
            return pm

        def clip(parameters, max_norm, *a, **kw):
            norm = self._clip(parameters, max_norm, *a, **kw)
            self.minibatches.append(self.capture(_sys._getframe(1).f_locals, norm))
            return norm

        def step_wait(env_self):
            out = self._step_wait(env_self)
            self.infos.append([dict(i) for i in out[3]])
            return out

        tdn._standard_normal, np.random.permutation, th.nn.utils.clip_grad_norm_, DummyVecEnv.step_wait = std_normal, permutation, clip, step_wait
        return self

    @staticmethod
    def capture(f, norm):
        return dict(values=f["values"].detach().numpy().copy(), log_prob=f["log_prob"].detach().numpy().copy(),
                    scalars=np.array([float(f["policy_loss"]), float(f["value_loss"]), float(f["entropy_loss"]),
                                      float(f["loss"]), float(f["approx_kl_div"]), float(f["clip_fraction"])], np.float32),
                    grad_norm=np.float32(float(norm)), ratio=f["ratio"].detach().numpy().copy(), epoch=int(f["epoch"]),
                    old_values=f["rollout_data"].old_values.numpy().copy())

    def __exit__(self, *exc):
        self._tdn._standard_normal, np.random.permutation, th.nn.utils.clip_grad_norm_ = self._std_normal, self._perm, self._clip
        self._dummy.step_wait = self._step_wait


def _ppo_run(seed, n_envs, n_steps, batch_size, n_epochs, net_arch=None, late=(), lr=3e-3, ent_coef=0.01, target_kl=None, venv=None,
             policy="MlpPolicy", gaussian=None, **kw):
    """One teacher-forceable PPO iteration of the reference on the CPU: _setup_learn (which resets the envs), THEN the step counters of
    the envs in `late` are set near the time limit (set before learn() they would be undone by the reset), collect_rollouts, train()."""
    from core.common.logger import Logger
    from core.common.utils import obs_as_tensor
    from core.ppo.ppo import PPO

    import warnings as _w

    pk = {} if net_arch is None else dict(policy_kwargs=dict(net_arch=net_arch))
    with _w.catch_warnings():
        _w.simplefilter("ignore")
        model = PPO(policy, _make_venv(n_envs) if venv is None else venv, seed=seed, device="cpu", n_steps=n_steps, batch_size=batch_size, n_epochs=n_epochs,
                    learning_rate=lr, ent_coef=ent_coef, target_kl=target_kl, **pk, **kw)
    model.set_logger(Logger(folder=None, output_formats=[]))
    out = _flat_sd("before/policy", model.policy.state_dict())
    out["state_dict_keys"] = np.array(list(model.policy.state_dict().keys()))
    _, cb = model._setup_learn(n_envs * n_steps, None, True, "PPO", False)
    for i, st in late:
        _inner_env(model.env.envs[i]).current_step = st
    out["init_obs"] = _obs_rows(model._last_obs)
    out["init_steps"] = np.array([_inner_env(e).current_step for e in model.env.envs], np.int32)
    with _PpoHooks() as hk:
        assert model.collect_rollouts(model.env, cb, model.rollout_buffer, n_steps)
        rb = model.rollout_buffer
        for f in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            out[f"rollout/{f}"] = _obs_rows(getattr(rb, f))
        assert len(hk.infos) == n_steps
        if (venv is None if gaussian is None else gaussian):  # a Discrete face samples through multinomial: no Normal draws; the indices are rollout/actions
            assert len(hk.draws) == n_steps
            out["eps"] = np.stack([d.numpy() for d in hk.draws])
        else:
            assert not hk.draws
        out["timeouts"] = np.array([[bool(i.get("TimeLimit.truncated", False)) and "terminal_observation" in i for i in step] for step in hk.infos],
                                   np.float32)
        with th.no_grad():
            out["last_values"] = model.policy.predict_values(obs_as_tensor(model._last_obs, model.device)).numpy().reshape(-1).copy()
        out["dones"] = np.array(model._last_episode_starts, np.float32)
        out["last_obs"] = _obs_rows(model._last_obs)
        model.train()
    out["permutations"] = np.stack(hk.perms) if hk.perms else np.zeros((0, n_envs * n_steps), np.int64)
    for k, mb in enumerate(hk.minibatches):
        for name in ("values", "log_prob", "scalars", "grad_norm"):
            out[f"mb{k}/{name}"] = mb[name]
    out["n_minibatches"], out["mb_epochs"] = np.int64(len(hk.minibatches)), np.array([mb["epoch"] for mb in hk.minibatches], np.int64)
    lv = model.logger.name_to_value
    out["logged_keys"] = np.array(sorted(lv.keys()))
    out["logged_values"] = np.array([float(lv[k]) for k in sorted(lv.keys())], np.float64)
    out.update(_flat_sd("after/policy", model.policy.state_dict()))
    out["optimizer_steps"] = np.int64(next(iter(model.policy.optimizer.state.values()))["step"]) if model.policy.optimizer.state else np.int64(0)
    out["n_updates"], out["n_truncations"] = np.int64(model._n_updates), np.int64(out["timeouts"].sum())
    arch = net_arch if net_arch is not None else [64, 64]
    out.update(seed=np.int64(seed), n_envs=np.int64(n_envs), n_steps=np.int64(n_steps), batch_size=np.int64(batch_size), n_epochs=np.int64(n_epochs),
               net_arch=np.array(arch, np.int64), gamma=np.float64(model.gamma), gae_lambda=np.float64(model.gae_lambda),
               learning_rate=np.float64(lr), ent_coef=np.float64(ent_coef), vf_coef=np.float64(model.vf_coef),
               max_grad_norm=np.float64(model.max_grad_norm), clip_range=np.float64(model.clip_range(1)))
    return model, out, hk


def _ppo_margins_ok(hk, clip_range, clip_range_vf):
    """no row within 1e-4 of a clip bound, so clip_fraction (and which side of a clamp a row is on) compares exactly"""
    for mb in hk.minibatches:
        if np.min(np.abs(np.abs(mb["ratio"] - 1) - clip_range)) <= 1e-4:
            return False
        if clip_range_vf is not None and np.min(np.abs(np.abs(mb["values"] - mb["old_values"]) - clip_range_vf)) <= 1e-4:
            return False
    return True


def gen_ppo():
    """PPO.collect_rollouts + train (core/common/on_policy_algorithm.py:162-268, core/ppo/ppo.py:184-300):
    ppo_train_kat_small.npz (4 envs, n_steps 8, batch 12 -> a last minibatch of 8 rows, 3 epochs, nets [32, 32]; + a target_kl run),
    ppo_train_kat_vfclip.npz (the same with clip_range_vf = 0.2, advantage normalisation on and off), ppo_train_kat_default.npz (class
    default nets, 8 envs, n_steps 16, batch 64, 2 epochs) and ppo_predict_kat.npz."""
    late = ((1, 396), (2, 399), (3, 395))
    small = dict(n_envs=4, n_steps=8, batch_size=12, n_epochs=3, net_arch=[32, 32], late=late)
    for seed in range(7, 60):
        model, out, hk = _ppo_run(seed, **small)
        clipped = max(float(mb["scalars"][5]) for mb in hk.minibatches)
        if not (clipped > 0 and int(out["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, None)):
            continue
        # the target_kl run: the same iteration stops at the first minibatch whose approx_kl clearly exceeds every earlier one
        kl = np.array([float(mb["scalars"][4]) for mb in hk.minibatches])
        per_epoch = -(-32 // 12)
        cand = [(kl[k] / kl[:k].max(), k) for k in range(per_epoch, len(kl)) if kl[:k].max() > 0 and kl[k] > 1.3 * kl[:k].max()]
        if not cand:
            continue
        _, k = max(cand)
        thr = float(np.sqrt(kl[k] * kl[:k].max()))
        m2, out2, hk2 = _ppo_run(seed, target_kl=thr / 1.5, **small)
        assert len(hk2.minibatches) == k and int(out2["n_updates"]) == k // per_epoch + 1
        out.update({"tkl/target_kl": np.float64(thr / 1.5), "tkl/stop_minibatch": np.int64(k), "tkl/n_updates": out2["n_updates"],
                    "tkl/optimizer_steps": out2["optimizer_steps"], "tkl/approx_kl": np.float64(kl[k])})
        out.update({f"tkl/{key}": v for key, v in out2.items() if key.startswith("after/")})
        print(f"ppo small: seed {seed}, max clip_fraction {clipped:.3f}, truncations {int(out['n_truncations'])}, target_kl stop at minibatch {k}")
        save("ppo_train_kat_small.npz", **out)
        break
    else:
        raise RuntimeError("no seed met the conditions of the small PPO fixture")
    for seed in range(int(out["seed"]), 60):
        runs = {}
        for tag, norm in (("norm", True), ("raw", False)):
            model, o, hk = _ppo_run(seed, clip_range_vf=0.2, normalize_advantage=norm, **small)
            engaged = any((np.abs(mb["values"] - mb["old_values"]) > 0.2).any() for mb in hk.minibatches)
            ok = engaged and int(o["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, 0.2) and max(float(mb["scalars"][5]) for mb in hk.minibatches) > 0
            runs[tag] = (o, ok)
        if all(ok for _, ok in runs.values()):
            o = dict(runs["norm"][0])
            o.update({f"raw/{k}": v for k, v in runs["raw"][0].items() if k.startswith(("mb", "after/", "logged_", "n_minibatches", "n_updates",
                                                                                        "optimizer_steps", "permutations"))})
            o["clip_range_vf"] = np.float64(0.2)
            print(f"ppo vfclip: seed {seed}")
            save("ppo_train_kat_vfclip.npz", **o)
            break
    else:
        raise RuntimeError("no seed met the conditions of the vfclip PPO fixture")
    model, o, hk = _ppo_run(11, n_envs=8, n_steps=16, batch_size=64, n_epochs=2, late=((0, 390), (5, 397), (6, 399)))
    assert int(o["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, None)
    save("ppo_train_kat_default.npz", **o)
    # predict: the trained small model on seeded observations, deterministic and sampled (the draw is recorded), and predict_values
    model, _, _ = _ppo_run(int(out["seed"]), **small)
    obs = np.random.default_rng(99).uniform(-1, 1, (16, 4)).astype(np.float32)
    p = _flat_sd("policy", model.policy.state_dict())
    p["obs"], p["net_arch"], p["seed"] = obs, np.array([32, 32], np.int64), out["seed"]
    p["deterministic"], _ = model.predict(obs, deterministic=True)
    with _PpoHooks() as hk:
        p["sampled"], _ = model.predict(obs, deterministic=False)
        p["eps"] = hk.draws[0].numpy()
    with th.no_grad():
        p["values"] = model.policy.predict_values(th.as_tensor(obs)).numpy()
    save("ppo_predict_kat.npz", **p)


# --------------------------------------------------------------------------------------- A2C
class _A2cHooks(_PpoHooks):
    """The same recorders around the UNMODIFIED reference's A2C.train (core/a2c/a2c.py:178 calls clip_grad_norm_): per-row values and
    log-probs in the order of get(None), the four scalars and the gradient norm."""

    @staticmethod
    def capture(f, norm):
        return dict(values=f["values"].detach().numpy().copy(), log_prob=f["log_prob"].detach().numpy().copy(),
                    scalars=np.array([float(f["policy_loss"]), float(f["value_loss"]), float(f["entropy_loss"]), float(f["loss"])], np.float32),
                    grad_norm=np.float32(float(norm)))


def _a2c_run(seed, n_envs, n_steps=5, net_arch=None, late=(), lr=3e-3, ent_coef=0.01, iterations=2, opt_state=True, venv=None,
             policy_kwargs=None, policy="MlpPolicy", gaussian=None, **kw):
    """`iterations` consecutive teacher-forceable A2C iterations of the reference on the CPU (rollout, train, rollout, train: the
    second step meets a non-zero square_avg): _setup_learn, THEN the step counters of the envs in `late` are set near the time limit."""
    from core.a2c.a2c import A2C
    from core.common.logger import Logger
    from core.common.utils import obs_as_tensor

    pk = {} if net_arch is None else dict(policy_kwargs=dict(net_arch=net_arch))
    if policy_kwargs:  # e.g. the optimiser class and its kwargs (gen_rmsprop_tf)
        pk = dict(policy_kwargs=dict(pk.get("policy_kwargs", {}), **policy_kwargs))
    model = A2C(policy, _make_venv(n_envs) if venv is None else venv, seed=seed, device="cpu", n_steps=n_steps, learning_rate=lr,
                ent_coef=ent_coef, **pk, **kw)
    model.set_logger(Logger(folder=None, output_formats=[]))
    out = _flat_sd("before/policy", model.policy.state_dict())
    out["state_dict_keys"] = np.array(list(model.policy.state_dict().keys()))
    _, cb = model._setup_learn(iterations * n_envs * n_steps, None, True, "A2C", False)
    for i, st in late:
        _inner_env(model.env.envs[i]).current_step = st
    out["init_obs"] = _obs_rows(model._last_obs)
    out["init_steps"] = np.array([_inner_env(e).current_step for e in model.env.envs], np.int32)
    names = [n for n, _ in model.policy.named_parameters()]
    n_trunc = 0
    for it in range(iterations):
        pre = f"it{it}/"
        with _A2cHooks() as hk:
            assert model.collect_rollouts(model.env, cb, model.rollout_buffer, n_steps)
            rb = model.rollout_buffer
            for f in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
                out[f"{pre}rollout/{f}"] = _obs_rows(getattr(rb, f))
            assert len(hk.infos) == n_steps
            if (venv is None if gaussian is None else gaussian):  # a Discrete face samples through multinomial: no Normal draws; the indices are rollout/actions
                assert len(hk.draws) == n_steps
                out[pre + "eps"] = np.stack([d.numpy() for d in hk.draws])
            else:
                assert not hk.draws
            out[pre + "timeouts"] = np.array([[bool(i.get("TimeLimit.truncated", False)) and "terminal_observation" in i for i in step]
                                              for step in hk.infos], np.float32)
            n_trunc += int(out[pre + "timeouts"].sum())
            with th.no_grad():
                out[pre + "last_values"] = model.policy.predict_values(obs_as_tensor(model._last_obs, model.device)).numpy().reshape(-1).copy()
            out[pre + "dones"] = np.array(model._last_episode_starts, np.float32)
            out[pre + "last_obs"] = _obs_rows(model._last_obs)
            model._update_current_progress_remaining(model.num_timesteps, iterations * n_envs * n_steps)
            model.train()
        assert len(hk.perms) == 1 and len(hk.minibatches) == 1
        out[pre + "permutation"] = np.asarray(hk.perms[0], np.int64)
        for name in ("values", "log_prob", "scalars", "grad_norm"):
            out[pre + name] = hk.minibatches[0][name]
        lv = model.logger.name_to_value
        out[pre + "logged_keys"] = np.array(sorted(lv.keys()))
        out[pre + "logged_values"] = np.array([float(lv[k]) for k in sorted(lv.keys())], np.float64)
        out.update(_flat_sd(pre + "after/policy", model.policy.state_dict()))
        st = model.policy.optimizer.state
        out[pre + "optimizer_steps"] = np.int64(next(iter(st.values()))["step"]) if st else np.int64(0)
        out[pre + "n_updates"] = np.int64(model._n_updates)
        if opt_state and isinstance(model.policy.optimizer, th.optim.RMSprop):
            for name, p_ in zip(names, model.policy.optimizer.param_groups[0]["params"]):
                out[f"{pre}opt/square_avg/{name}"] = st[p_]["square_avg"].numpy().copy()
        elif opt_state and type(model.policy.optimizer).__name__ == "RMSpropTFLike":
            for name, p_ in zip(names, model.policy.optimizer.param_groups[0]["params"]):
                for key in ("square_avg", "momentum_buffer", "grad_avg"):
                    if key in st[p_]:
                        out[f"{pre}opt/{key}/{name}"] = st[p_][key].numpy().copy()
    arch = net_arch if net_arch is not None else [64, 64]
    out.update(seed=np.int64(seed), n_envs=np.int64(n_envs), n_steps=np.int64(n_steps), iterations=np.int64(iterations),
               net_arch=np.array(arch, np.int64), gamma=np.float64(model.gamma), gae_lambda=np.float64(model.gae_lambda),
               learning_rate=np.float64(lr), ent_coef=np.float64(ent_coef), vf_coef=np.float64(model.vf_coef),
               max_grad_norm=np.float64(model.max_grad_norm), n_truncations=np.int64(n_trunc),
               optimizer=np.array(type(model.policy.optimizer).__name__), rms_prop_eps=np.float64(1e-5))
    return model, out


def gen_a2c():
    """A2C.collect_rollouts + train (core/a2c/a2c.py:132-190), two consecutive iterations each: a2c_train_kat_small.npz (4 envs,
    n_steps 5, nets [32, 32], ent_coef 0.01, lr 3e-3; the clip engaged in both steps), a2c_train_kat_variants.npz (normalize_advantage,
    a max_grad_norm that never engages, use_rms_prop=False, as prefixes norm/ noclip/ adam/ over the same initial weights) and
    a2c_train_kat_default.npz (class defaults, 8 envs, the big tensors after each step as digests)."""
    late = ((1, 396), (2, 399), (3, 392))
    small = dict(n_envs=4, net_arch=[32, 32], late=late)
    for seed in range(7, 60):
        model, out = _a2c_run(seed, **small)
        norms = [float(out[f"it{k}/grad_norm"]) for k in range(2)]
        trunc = [int(out[f"it{k}/timeouts"].sum()) for k in range(2)]
        if min(norms) > 1.05 * 0.5 and min(trunc) >= 1:
            break
    else:
        raise RuntimeError("no seed met the conditions of the small A2C fixture")
    assert all(n > 0.5 for n in norms) and int(out["n_truncations"]) >= 2  # the clip is engaged in both steps
    assert float(np.abs(out["it0/opt/square_avg/log_std"]).max()) > 0 and str(out["optimizer"]) == "RMSprop"
    print(f"a2c small: seed {seed}, gradient norms {norms}, truncations {trunc}")
    save("a2c_train_kat_small.npz", **out)
    # the variants: smaller nets, their own initial weights; what does not depend on the variant (initial weights, env states, the
    # first rollout) is stored once, the recorded draws / last observations / logger values only in the small fixture
    variants, tiny = {}, dict(n_envs=4, net_arch=[16, 16], late=late)
    shared = ("before/", "it0/rollout/", "state_dict_keys", "init_obs", "init_steps", "seed", "n_envs", "n_steps", "iterations", "net_arch",
              "gamma", "gae_lambda", "learning_rate", "ent_coef", "vf_coef", "rms_prop_eps")
    dropped = ("eps", "timeouts", "last_values", "dones", "last_obs", "logged_keys", "logged_values")
    for tag, kw in (("norm", dict(normalize_advantage=True)), ("noclip", dict(max_grad_norm=1e6)), ("adam", dict(use_rms_prop=False))):
        _, o = _a2c_run(seed, opt_state=False, **tiny, **kw)
        assert int(o["n_truncations"]) >= 2
        for key in list(o):
            if key.split("/")[-1] in dropped:
                del o[key]
            elif key.startswith(shared):
                if key in variants:
                    np.testing.assert_array_equal(o[key], variants[key])
                variants[key] = o.pop(key)
        variants.update({f"{tag}/{k}": v for k, v in o.items()})
    assert max(float(variants[f"noclip/it{k}/grad_norm"]) for k in range(2)) < 1e6 and str(variants["adam/optimizer"]) == "Adam"
    assert min(float(variants[f"noclip/it{k}/grad_norm"]) for k in range(2)) > 0.5  # max_grad_norm = 0.5 would have engaged
    assert int(variants["adam/it1/optimizer_steps"]) == 2 and float(variants["norm/max_grad_norm"]) == 0.5
    save("a2c_train_kat_variants.npz", **variants)
    _, o = _a2c_run(11, n_envs=8, lr=7e-4, ent_coef=0.0, late=((0, 397), (5, 393), (6, 399)), opt_state=False)
    assert int(o["n_truncations"]) >= 2
    slim = {}
    for k, v in o.items():  # slim_weights on the per-iteration keys: big tensors as digests under the key check_weights looks up
        if "after/" in k and v.size > 4000:
            slim.update({k + "#sum": np.float64(v.astype(np.float64).sum()), k + "#abs": np.float64(np.abs(v.astype(np.float64)).sum()),
                         k + "#head": v.reshape(-1)[:64].copy(), k + "#shape": np.array(v.shape, np.int64)})
        elif k.split("/")[-1] not in ("eps", "last_obs", "logged_keys", "logged_values"):
            slim[k] = v
    save("a2c_train_kat_default.npz", **slim)


# ------------------------------------------------------------------------------ RMSpropTFLike
RMSPROP_TF_FORMS = (("plain", {}), ("a2c", dict(eps=1e-5)), ("momentum", dict(momentum=0.9)), ("centered", dict(centered=True)),
                    ("centered_momentum", dict(centered=True, momentum=0.9)), ("weight_decay", dict(weight_decay=1e-2)))


def gen_rmsprop_tf():
    """rmsprop_tf_kat.npz: three steps of the reference's RMSpropTFLike (core/common/sb2_compat/rmsprop_tf_like.py:78-137) in six forms
    on two tensors of 257 and 1024 elements (shared initial values and gradients, magnitudes 1e-6 .. 1), every state tensor after
    each step. a2c_tflike_train_kat_small.npz / a2c_tflike_train_kat_variants.npz: two consecutive teacher-forceable A2C iterations
    (as gen_a2c's small fixture) with optimizer_class=RMSpropTFLike, optimizer_kwargs eps=1e-5, and with momentum=0.9, centered=True
    on [16, 16] nets."""
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

    rng = np.random.default_rng(20260417)
    sizes = (257, 1024)
    out = {"sizes": np.array(sizes, np.int64), "forms": np.array([f for f, _ in RMSPROP_TF_FORMS]), "steps": np.int64(3)}
    for i, n in enumerate(sizes):
        out[f"param0/w{i}"] = rng.uniform(-1.5, 1.5, n).astype(np.float32)
        for k in range(3):
            out[f"grad{k}/w{i}"] = (10.0 ** rng.uniform(-6, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    for form, kw in RMSPROP_TF_FORMS:
        ps = [th.nn.Parameter(th.tensor(out[f"param0/w{i}"])) for i in range(len(sizes))]
        opt = RMSpropTFLike(ps, **kw)
        g0 = opt.param_groups[0]
        for key in ("lr", "alpha", "eps", "weight_decay", "momentum"):
            out[f"{form}/{key}"] = np.float64(g0[key])
        out[f"{form}/centered"] = np.bool_(g0["centered"])
        for k in range(3):
            for i, p in enumerate(ps):
                p.grad = th.tensor(out[f"grad{k}/w{i}"])
            opt.step()
            for i, p in enumerate(ps):
                st = opt.state[p]
                assert isinstance(st["step"], int) and st["step"] == k + 1
                assert set(st) == {"step", "square_avg"} | ({"momentum_buffer"} if g0["momentum"] > 0 else set()) | \
                    ({"grad_avg"} if g0["centered"] else set())
                out[f"{form}/step{k}/param/w{i}"] = p.detach().numpy().copy()
                for key in st:
                    if key != "step":
                        out[f"{form}/step{k}/{key}/w{i}"] = st[key].numpy().copy()
        assert all(np.isfinite(out[f"{form}/step2/param/w{i}"]).all() for i in range(len(sizes)))
    save("rmsprop_tf_kat.npz", **out)
    late = ((1, 396), (2, 399), (3, 392))
    for name, net_arch, okw in (("small", [32, 32], dict(eps=1e-5)), ("variants", [16, 16], dict(eps=1e-5, momentum=0.9, centered=True))):
        pk = dict(optimizer_class=RMSpropTFLike, optimizer_kwargs=okw)
        for seed in range(7, 60):
            model, o = _a2c_run(seed, n_envs=4, net_arch=net_arch, late=late, policy_kwargs=pk)
            norms = [float(o[f"it{k}/grad_norm"]) for k in range(2)]
            trunc = [int(o[f"it{k}/timeouts"].sum()) for k in range(2)]
            if min(norms) > 1.05 * 0.5 and min(trunc) >= 1:
                break
        else:
            raise RuntimeError(f"no seed met the conditions of the {name} RMSpropTFLike A2C fixture")
        assert str(o["optimizer"]) == "RMSpropTFLike" and int(o["it1/optimizer_steps"]) == 2
        assert float(np.abs(o["it0/opt/square_avg/log_std"] - 1).max()) > 0  # the second step meets a square_avg that has moved off ones
        assert ("it1/opt/momentum_buffer/log_std" in o) == ("momentum" in okw) and ("it1/opt/grad_avg/log_std" in o) == ("centered" in okw)
        for key, v in okw.items():
            o[f"optimizer_kwargs/{key}"] = np.float64(v)
        print(f"a2c tflike {name}: seed {seed}, gradient norms {norms}, truncations {trunc}")
        save(f"a2c_tflike_train_kat_{name}.npz", **o)


# ------------------------------------------------------------------------------ DQN on the discretised valve face
def _valve(q, K):
    """v(q) of the discrete valve face, float32, in exactly this order (core/common/vec_env/cstr_vec_env.py states the same)"""
    return np.float32(-1) + np.float32(2 * q) / np.float32(K - 1)


def _make_discrete_venv(N, K):
    """Harness code of ours: the reference's TwoSeriesCSTREnv behind a Discrete(K * K) action space; index a = i * K + j opens the
    two valves to v(i), v(j)."""
    from gymnasium import spaces

    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from twoseriescstr import TwoSeriesCSTREnv

    class DiscreteValveCSTR(TwoSeriesCSTREnv):
        def __init__(self):
            super().__init__()
            self._valve_box, self.action_space = self.action_space, spaces.Discrete(K * K)

        def step(self, action):
            a = int(action)
            face, self.action_space = self.action_space, self._valve_box  # the env's own step clips into its Box
            try:
                return super().step(np.array([_valve(a // K, K), _valve(a % K, K)], np.float32))
            finally:
                self.action_space = face

    return DummyVecEnv([lambda: DiscreteValveCSTR() for _ in range(N)])


class _DqnHooks:
    """Around the UNMODIFIED reference (core/dqn/dqn.py): the (current_q, target_q) arguments of smooth_l1_loss and the gradient norm
    clip_grad_norm_ returns; np.random.rand / randint calls with their results."""

    def __enter__(self):
        import torch.nn.functional as F_real

        import core.dqn.dqn as dqnmod

        self.huber, self.norms, self.rands, self.randints = [], [], [], []
        self._mod, self._F, self._clip, self._rand, self._randint = dqnmod, F_real, th.nn.utils.clip_grad_norm_, np.random.rand, np.random.randint
        hooks = self

        class FProxy:
            def __getattr__(self, name):
                return getattr(F_real, name)

            @staticmethod
            def smooth_l1_loss(a, b, *args, **kw):
                hooks.huber.append((a.detach().clone(), b.detach().clone()))
                return F_real.smooth_l1_loss(a, b, *args, **kw)

        def clip(parameters, max_norm, *a, **kw):
            norm = self._clip(parameters, max_norm, *a, **kw)
            self.norms.append(float(norm))
            return norm

        def rand(*a):
            r = self._rand(*a)
            self.rands.append(float(r))
            return r

        def randint(*a, **kw):
            r = self._randint(*a, **kw)
            self.randints.append((a, dict(kw), np.asarray(r).copy()))
            return r

        dqnmod.F, th.nn.utils.clip_grad_norm_, np.random.rand, np.random.randint = FProxy(), clip, rand, randint
        return self

    def __exit__(self, *exc):
        self._mod.F, th.nn.utils.clip_grad_norm_, np.random.rand, np.random.randint = self._F, self._clip, self._rand, self._randint


def _gen_dqn_train(tag, K, B, n_steps, update_after, **kw):
    """Teacher-forced DQN.train (core/dqn/dqn.py:184-226): injected batches, one gradient step per call; `update_after`: the
    reference's own _on_step performs a target update behind that step."""
    from core.common.logger import Logger
    from core.common.type_aliases import ReplayBufferSamples
    from core.dqn.dqn import DQN

    N, D = 4, 4
    model = DQN("MlpPolicy", _make_discrete_venv(N, K), seed=0, device="cpu", batch_size=B, buffer_size=64 * N, **kw)
    model.set_logger(Logger(folder=None, output_formats=[]))
    out = {}
    for nm in ("q_net", "q_net_target"):
        out.update(_flat_sd(f"before/{nm}", getattr(model, nm).state_dict()))
    assert sorted(model.policy.state_dict()) == sorted(f"{n}.q_net.{i}.{p}" for n in ("q_net", "q_net_target") for i in (0, 2, 4) for p in ("weight", "bias"))
    rng = np.random.default_rng(2024 + K)
    batches = []
    for k in range(n_steps):
        obs = rng.uniform(-1, 1, (B, D)).astype(np.float32)
        nobs = np.clip(obs + rng.normal(0, 0.05, (B, D)), -1, 1).astype(np.float32)
        index = rng.integers(0, K * K, (B, 1)).astype(np.int64)
        # rewards on both sides of the Huber threshold (the untrained Q values are small)
        rew = np.where(rng.uniform(size=(B, 1)) < 0.5, rng.uniform(-0.8, 0.8, (B, 1)), rng.uniform(-8, 0, (B, 1))).astype(np.float32)
        done = (rng.uniform(size=(B, 1)) < 0.25).astype(np.float32)
        batches.append((obs, index, nobs, done, rew))
    feed = list(batches)
    model.replay_buffer.sample = lambda batch_size, env=None: ReplayBufferSamples(*(th.as_tensor(x) for x in feed.pop(0)))
    logged = []
    with _DqnHooks() as hk:
        for k in range(n_steps):
            model.train(gradient_steps=1, batch_size=B)
            lv = model.logger.name_to_value
            logged.append(sorted(lv))
            out[f"step{k}/loss"] = np.float32(lv["train/loss"])
            out[f"step{k}/n_updates"] = np.int64(lv["train/n_updates"])
            out[f"step{k}/learning_rate"] = np.float64(lv["train/learning_rate"])
            if k == update_after:  # the reference's own _on_step: _n_calls hits the update period
                model._n_calls = max(model.target_update_interval // model.n_envs, 1) - 1
                before = [p.detach().clone() for p in model.q_net_target.parameters()]
                model._on_step()
                assert any(not th.equal(a, b) for a, b in zip(before, model.q_net_target.parameters()))
            for nm in ("q_net", "q_net_target"):
                out.update(_flat_sd(f"after/step{k}/{nm}", getattr(model, nm).state_dict()))
            st = model.policy.optimizer.state_dict()["state"]
            out[f"step{k}/optimizer_step"] = np.int64(int(next(iter(st.values()))["step"]))
    assert len(hk.huber) == n_steps and len(hk.norms) == n_steps
    for k in range(n_steps):
        for fi, fname in enumerate(["observations", "index", "next_observations", "dones", "rewards"]):
            out[f"step{k}/batch_{fname}"] = batches[k][fi]
        out[f"step{k}/current_q"], out[f"step{k}/target_q"] = hk.huber[k][0].numpy(), hk.huber[k][1].numpy()
        out[f"step{k}/grad_norm"] = np.float32(hk.norms[k])
        d = np.abs(out[f"step{k}/current_q"] - out[f"step{k}/target_q"])
        assert (d < 1).any() and (d > 1).any(), "both Huber branches"
    out["logged_keys"] = np.array(logged[-1])
    out["hyper"] = np.array([model.gamma, model.tau, model.max_grad_norm, model.lr_schedule(1), B, n_steps, K, update_after], np.float64)
    out["clip_engaged"] = np.uint8(any(n > model.max_grad_norm for n in hk.norms))
    print(f"dqn {tag}: grad norms {hk.norms}, max_grad_norm {model.max_grad_norm}")
    return out


def _gen_dqn_predict():
    from core.dqn.dqn import DQN

    K = 3
    model = DQN("MlpPolicy", _make_discrete_venv(1, K), seed=3, device="cpu", policy_kwargs=dict(net_arch=[64, 64]))
    rng = np.random.default_rng(77)
    obs = rng.uniform(-1, 1, (96, 4)).astype(np.float32)
    with th.no_grad():
        q = model.q_net(th.as_tensor(obs)).numpy()
    top = np.sort(q, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-3 * np.abs(q).mean()  # the generator filters; the test leaves out no row
    obs, q = obs[keep], q[keep]
    act, _ = model.predict(obs, deterministic=True)
    one, _ = model.predict(obs[0], deterministic=True)
    assert act.shape == (len(obs),) and act.dtype == np.int64 and one.shape == () and int(one) == int(act[0])
    out = dict(obs=obs, actions=act, q=q, levels=np.int64(K), kept=np.int64(keep.sum()), drawn=np.int64(len(keep)))
    out.update(_flat_sd("before/q_net", model.q_net.state_dict()))
    save("dqn_predict_kat.npz", **out)


def _gen_dqn_explore():
    """A short seeded learn(): per post-warm-up vec-step the exploration rate in force and the rand() drawn against it; per gradient
    step the sampled batch_inds / env_indices. They depend on the streams and the ring position only."""
    from core.common.logger import Logger
    from core.dqn.dqn import DQN

    N, K, B, seed, total = 4, 3, 16, 11, 64
    model = DQN("MlpPolicy", _make_discrete_venv(N, K), seed=seed, device="cpu", batch_size=B, buffer_size=64 * N, learning_starts=8, train_freq=4,
                target_update_interval=24, exploration_fraction=0.8, policy_kwargs=dict(net_arch=[64, 64]))
    model.set_logger(Logger(folder=None, output_formats=[]))
    state0 = {}
    rates_in_force = []
    orig_collect, orig_predict = model.collect_rollouts, model.predict

    def collect(*a, **kw):
        if not state0:
            st = np.random.get_state()
            state0.update(key=st[1].copy(), pos=np.int64(st[2]))
        return orig_collect(*a, **kw)

    def predict(*a, **kw):
        rates_in_force.append(float(model.exploration_rate))
        return orig_predict(*a, **kw)

    model.collect_rollouts, model.predict = collect, predict
    with _DqnHooks() as hk:
        model.learn(total)
    st = np.random.get_state()
    sized = [(a, kw, r) for a, kw, r in hk.randints if np.size(r) == B]
    assert len(hk.rands) == len(rates_in_force) and len(sized) == 2 * model._n_updates
    out = dict(n_envs=np.int64(N), levels=np.int64(K), batch_size=np.int64(B), seed=np.int64(seed), total_timesteps=np.int64(total),
               learning_starts=np.int64(8), train_freq=np.int64(4), target_update_interval=np.int64(24), exploration_fraction=np.float64(0.8),
               exploration_initial_eps=np.float64(model.exploration_initial_eps), exploration_final_eps=np.float64(model.exploration_final_eps),
               mt_key0=state0["key"], mt_pos0=state0["pos"], mt_key_final=st[1].copy(), mt_pos_final=np.int64(st[2]),
               exploration_rate=np.array(rates_in_force, np.float64), rand=np.array(hk.rands, np.float64),
               explored=np.array([r < e for r, e in zip(hk.rands, rates_in_force)], np.uint8),
               batch_inds=np.stack([r for _, _, r in sized[0::2]]).astype(np.int64), env_indices=np.stack([r for _, _, r in sized[1::2]]).astype(np.int64),
               batch_high=np.array([(a[1] if len(a) > 1 else kw.get("high", a[0])) for a, kw, _ in sized[0::2]], np.int64),
               n_updates=np.int64(model._n_updates), n_calls=np.int64(model._n_calls), num_timesteps=np.int64(model.num_timesteps),
               final_exploration_rate=np.float64(model.exploration_rate))
    print("dqn explore: rates", rates_in_force, "explored", out["explored"].tolist(), "highs", out["batch_high"].tolist())
    save("dqn_explore_kat.npz", **out)


def _gen_dqn_wiring():
    """A synthetic one-step problem (done = 1 everywhere): reward 1 iff the stored index equals a fixed function of the observation's
    sign pattern. The unmodified reference trains on it for seeds 0, 1, 2; the fixture holds the data, the held-out observations and
    how often the greedy action is the rewarded one, trained and untrained."""
    from core.common.logger import Logger
    from core.dqn.dqn import DQN

    K, N, R, B, steps, lr = 3, 8, 256, 64, 600, 1e-3
    rng = np.random.default_rng(4242)
    best = lambda o: ((o[..., 0] > 0).astype(np.int64) + (o[..., 2] > 0)) * K + (o[..., 1] > 0).astype(np.int64) + (o[..., 3] > 0)  # noqa: E731
    obs = rng.uniform(-1, 1, (R, N, 4)).astype(np.float32)
    index = rng.integers(0, K * K, (R, N)).astype(np.int64)
    reward = (index == best(obs)).astype(np.float32)
    held = rng.uniform(-1, 1, (512, 4)).astype(np.float32)
    trained, untrained = [], []
    for seed in (0, 1, 2):
        model = DQN("MlpPolicy", _make_discrete_venv(N, K), seed=seed, device="cpu", batch_size=B, buffer_size=R * N, learning_rate=lr)
        model.set_logger(Logger(folder=None, output_formats=[]))
        for r in range(R):
            model.replay_buffer.add(obs[r], obs[r], index[r].reshape(N, 1), reward[r], np.ones(N, bool), [{} for _ in range(N)])
        untrained.append(float((model.predict(held, deterministic=True)[0] == best(held)).mean()))
        model.train(gradient_steps=steps, batch_size=B)
        trained.append(float((model.predict(held, deterministic=True)[0] == best(held)).mean()))
    print(f"dqn wiring: reference accuracy trained {trained}, untrained {untrained}")
    save("dqn_wiring_kat.npz", obs=obs, index=index, reward=reward, held_obs=held, held_best=best(held), levels=np.int64(K),
         batch_size=np.int64(B), gradient_steps=np.int64(steps), learning_rate=np.float64(lr), reference_accuracy=np.array(trained),
         untrained_accuracy=np.array(untrained))


def gen_dqn():
    small = _gen_dqn_train("small", K=3, B=32, n_steps=3, update_after=1, max_grad_norm=0.05, target_update_interval=1000,
                           policy_kwargs=dict(net_arch=[64, 64]))
    assert small["clip_engaged"]
    save("dqn_train_kat_small.npz", **small)
    save("dqn_train_kat_default.npz", **slim_weights(_gen_dqn_train("default", K=5, B=32, n_steps=2, update_after=0)))
    _gen_dqn_predict()
    _gen_dqn_explore()
    _gen_dqn_wiring()


# ------------------------------------------------------- PPO / A2C on the discretised valve face (Categorical head)
def gen_ppo_discrete():
    """PPO on Discrete(K * K) (core/ppo/ppo.py:127-136, core/common/distributions.py:263-311): ppo_cat_train_kat_small.npz (K = 3, 4
    envs, n_steps 8, batch 12, 3 epochs, nets [32, 32]), ppo_cat_train_kat_default.npz (K = 5, class-default nets as digests, 8 envs,
    n_steps 16, batch 64, 2 epochs) and ppo_cat_predict_kat.npz. The sampled indices are rollout/actions [T, N, 1]."""
    late = ((1, 396), (2, 399), (3, 395))
    small = dict(n_envs=4, n_steps=8, batch_size=12, n_epochs=3, net_arch=[32, 32], late=late)
    for seed in range(7, 120):
        model, out, hk = _ppo_run(seed, venv=_make_discrete_venv(4, 3), **small)
        clipped = max(float(mb["scalars"][5]) for mb in hk.minibatches)
        if clipped > 0 and int(out["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, None):
            break
    else:
        raise RuntimeError("no seed met the conditions of the small categorical PPO fixture")
    out["levels"] = np.int64(3)
    assert out["rollout/actions"].shape == (8, 4, 1) and "policy/log_std" not in "".join(out["state_dict_keys"].tolist())
    print(f"ppo cat small: seed {seed}, max clip_fraction {clipped:.3f}, truncations {int(out['n_truncations'])}")
    save("ppo_cat_train_kat_small.npz", **out)
    for seed_d in range(11, 120):
        _, o, hk_d = _ppo_run(seed_d, n_envs=8, n_steps=16, batch_size=64, n_epochs=2, late=((0, 390), (5, 397), (6, 399)),
                              venv=_make_discrete_venv(8, 5))
        # the conditions of ppo_train_kat_default.npz: four steps at the class-default head gain of 0.01 move no ratio past the clip range
        if int(o["n_truncations"]) >= 2 and _ppo_margins_ok(hk_d, 0.2, None):
            break
    else:
        raise RuntimeError("no seed met the conditions of the default categorical PPO fixture")
    o["levels"] = np.int64(5)
    print(f"ppo cat default: seed {seed_d}")
    save("ppo_cat_train_kat_default.npz", **slim_weights(o))
    # predict: the trained small model on 16 seeded observations; every row's top-two logit gap exceeds 1e-4 * max |logit|
    for pseed in range(99, 200):
        obs = np.random.default_rng(pseed).uniform(-1, 1, (16, 4)).astype(np.float32)
        with th.no_grad():
            logits = model.policy.action_net(model.policy.mlp_extractor.forward_actor(th.as_tensor(obs))).numpy()
        top = np.sort(logits, axis=1)
        if ((top[:, -1] - top[:, -2]) > 1e-4 * np.abs(logits).max()).all():
            break
    else:
        raise RuntimeError("no observation seed met the logit-gap condition")
    p = _flat_sd("policy", model.policy.state_dict())
    p["obs"], p["net_arch"], p["seed"], p["obs_seed"], p["levels"] = obs, np.array([32, 32], np.int64), out["seed"], np.int64(pseed), np.int64(3)
    p["deterministic"], _ = model.predict(obs, deterministic=True)
    assert p["deterministic"].dtype == np.int64 and p["deterministic"].shape == (16,) and np.array_equal(p["deterministic"], logits.argmax(axis=1))
    p["logits"] = logits
    with th.no_grad():
        p["values"] = model.policy.predict_values(th.as_tensor(obs)).numpy()
    save("ppo_cat_predict_kat.npz", **p)


def gen_a2c_discrete():
    """A2C on Discrete(9), two consecutive iterations: a2c_cat_train_kat_small.npz (K = 3, 4 envs, n_steps 5, nets [32, 32])"""
    late = ((1, 396), (2, 399), (3, 392))
    for seed in range(7, 120):
        _, out = _a2c_run(seed, n_envs=4, net_arch=[32, 32], late=late, venv=_make_discrete_venv(4, 3))
        trunc = [int(out[f"it{k}/timeouts"].sum()) for k in range(2)]
        if min(trunc) >= 1:
            break
    else:
        raise RuntimeError("no seed met the conditions of the small categorical A2C fixture")
    assert int(out["n_truncations"]) >= 2 and out["it0/rollout/actions"].shape == (5, 4, 1) and str(out["optimizer"]) == "RMSprop"
    out["levels"] = np.int64(3)
    print(f"a2c cat small: seed {seed}, gradient norms {[float(out[f'it{k}/grad_norm']) for k in range(2)]}, truncations {trunc}")
    save("a2c_cat_train_kat_small.npz", **out)


# ------------------------------------------------------- PPO / A2C on the MultiDiscrete valve face (MultiCategorical head)
def _make_multidiscrete_venv(N, K0, K1):
    """Harness code of ours: the reference's TwoSeriesCSTREnv behind a MultiDiscrete([K0, K1]) action space; the pair (a0, a1) opens
    the two valves to v_0(a0), v_1(a1)."""
    from gymnasium import spaces

    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from twoseriescstr import TwoSeriesCSTREnv

    class MultiDiscreteValveCSTR(TwoSeriesCSTREnv):
        def __init__(self):
            super().__init__()
            self._valve_box, self.action_space = self.action_space, spaces.MultiDiscrete([K0, K1])

        def step(self, action):
            a0, a1 = (int(q) for q in np.asarray(action).reshape(2))
            face, self.action_space = self.action_space, self._valve_box  # the env's own step clips into its Box
            try:
                return super().step(np.array([_valve(a0, K0), _valve(a1, K1)], np.float32))
            finally:
                self.action_space = face

    return DummyVecEnv([lambda: MultiDiscreteValveCSTR() for _ in range(N)])


def gen_ppo_multidiscrete():
    """PPO on MultiDiscrete([K0, K1]) (core/ppo/ppo.py:127-136, core/common/distributions.py:314-368): ppo_mcat_train_kat_small.npz
    (nvec [3, 5], 4 envs, n_steps 8, batch 12, 3 epochs, nets [32, 32]), ppo_mcat_train_kat_default.npz (nvec [5, 5], class-default
    nets as digests, 8 envs, n_steps 16, batch 64, 2 epochs) and ppo_mcat_predict_kat.npz. The sampled pairs are rollout/actions
    [T, N, 2]."""
    late = ((1, 396), (2, 399), (3, 395))
    small = dict(n_envs=4, n_steps=8, batch_size=12, n_epochs=3, net_arch=[32, 32], late=late)
    for seed in range(7, 120):
        model, out, hk = _ppo_run(seed, venv=_make_multidiscrete_venv(4, 3, 5), **small)
        clipped = max(float(mb["scalars"][5]) for mb in hk.minibatches)
        if clipped > 0 and int(out["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, None):
            break
    else:
        raise RuntimeError("no seed met the conditions of the small multi-categorical PPO fixture")
    out["nvec"] = np.array([3, 5], np.int64)
    keys = "".join(out["state_dict_keys"].tolist())
    assert out["rollout/actions"].shape == (8, 4, 2) and "log_std" not in keys and out["before/policy/action_net.weight"].shape == (8, 32)
    print(f"ppo mcat small: seed {seed}, max clip_fraction {clipped:.3f}, truncations {int(out['n_truncations'])}")
    save("ppo_mcat_train_kat_small.npz", **out)
    for seed_d in range(11, 120):
        _, o, hk_d = _ppo_run(seed_d, n_envs=8, n_steps=16, batch_size=64, n_epochs=2, late=((0, 390), (5, 397), (6, 399)),
                              venv=_make_multidiscrete_venv(8, 5, 5))
        # the conditions of ppo_train_kat_default.npz: four steps at the class-default head gain of 0.01 move no ratio past the clip range
        if int(o["n_truncations"]) >= 2 and _ppo_margins_ok(hk_d, 0.2, None):
            break
    else:
        raise RuntimeError("no seed met the conditions of the default multi-categorical PPO fixture")
    o["nvec"] = np.array([5, 5], np.int64)
    print(f"ppo mcat default: seed {seed_d}")
    save("ppo_mcat_train_kat_default.npz", **slim_weights(o))
    # predict: the trained small model on 16 seeded observations; per valve, every row's top-two logit gap exceeds 1e-4 * max |logit|
    for pseed in range(99, 400):
        obs = np.random.default_rng(pseed).uniform(-1, 1, (16, 4)).astype(np.float32)
        with th.no_grad():
            logits = model.policy.action_net(model.policy.mlp_extractor.forward_actor(th.as_tensor(obs))).numpy()
        tops = [np.sort(z, axis=1) for z in (logits[:, :3], logits[:, 3:])]
        if all(((t[:, -1] - t[:, -2]) > 1e-4 * np.abs(logits).max()).all() for t in tops):
            break
    else:
        raise RuntimeError("no observation seed met the logit-gap condition")
    p = _flat_sd("policy", model.policy.state_dict())
    p["obs"], p["net_arch"], p["seed"], p["obs_seed"], p["nvec"] = obs, np.array([32, 32], np.int64), out["seed"], np.int64(pseed), np.array([3, 5], np.int64)
    p["deterministic"], _ = model.predict(obs, deterministic=True)
    expect = np.stack([logits[:, :3].argmax(axis=1), logits[:, 3:].argmax(axis=1)], axis=1)
    assert p["deterministic"].dtype == np.int64 and p["deterministic"].shape == (16, 2) and np.array_equal(p["deterministic"], expect)
    one, _ = model.predict(obs[0], deterministic=True)
    assert one.shape == (2,) and one.dtype == np.int64
    p["logits"] = logits
    with th.no_grad():
        p["values"] = model.policy.predict_values(th.as_tensor(obs)).numpy()
    save("ppo_mcat_predict_kat.npz", **p)


def _a2c_reference_own_error(out, nvec):
    """Harness code of ours: how far the reference's float32 weights after each train() are from the same step taken in float64 (same
    rollout rows, same weights before, same square_avg before), per element in the units the tests hold an implementation to
    (tests/_parity_helpers.check_weights: |got - want| / (2e-5 max|want| + 1e-4 |want|)); the worst over both iterations. RMSprop
    divides by sqrt(square_avg) + eps, so where a gradient element is a cancelling sum near eps its float32 rounding error reaches the
    weight almost undamped: a rollout with such an element measures the summation order, not the statements."""
    keys = [str(k) for k in out["state_dict_keys"]]
    lr, eps, alpha = float(out["learning_rate"]), float(out["rms_prop_eps"]), 0.99
    T, N = int(out["n_steps"]), int(out["n_envs"])
    flat = lambda a: (a if a.ndim > 2 else a[..., None]).swapaxes(0, 1).reshape(T * N, -1)  # noqa: E731  swap_and_flatten
    worst = 0.0
    for it in range(int(out["iterations"])):
        pre, before = f"it{it}/", ("before" if it == 0 else f"it{it - 1}/after")
        P = {k: th.tensor(out[f"{before}/policy/{k}"].astype(np.float64), requires_grad=True) for k in keys}
        f = lambda name: th.tensor(flat(out[f"{pre}rollout/{name}"]).astype(np.float64))  # noqa: E731
        obs = f("observations")

        def mlp(net, head):
            h = obs
            for i in (0, 2):
                h = th.tanh(h @ P[f"mlp_extractor.{net}.{i}.weight"].T + P[f"mlp_extractor.{net}.{i}.bias"])
            return h @ P[f"{head}.weight"].T + P[f"{head}.bias"]

        dists = [th.distributions.Categorical(logits=z) for z in th.split(mlp("policy_net", "action_net"), list(nvec), dim=1)]
        log_prob = sum(d.log_prob(a.long()) for d, a in zip(dists, th.unbind(f("actions"), dim=1)))
        entropy = sum(d.entropy() for d in dists)
        values = mlp("value_net", "value_net").flatten()
        loss = (-(f("advantages").flatten() * log_prob).mean() + float(out["ent_coef"]) * -entropy.mean()
                + float(out["vf_coef"]) * th.nn.functional.mse_loss(f("returns").flatten(), values))
        loss.backward()
        norm = float(th.sqrt(sum((p.grad ** 2).sum() for p in P.values())))
        coef = min(1.0, float(out["max_grad_norm"]) / (norm + 1e-6))
        for k in keys:
            g = P[k].grad.numpy() * coef
            prev = np.zeros_like(g) if it == 0 else out[f"it{it - 1}/opt/square_avg/{k}"].astype(np.float64)
            stepped = P[k].detach().numpy() - lr * g / (np.sqrt(alpha * prev + (1 - alpha) * g * g) + eps)
            ref = out[f"{pre}after/policy/{k}"].astype(np.float64)
            worst = max(worst, float((np.abs(ref - stepped) / (2e-5 * max(np.abs(ref).max(), 1e-3) + 1e-4 * np.abs(ref))).max()))
    return worst


def gen_a2c_multidiscrete():
    """A2C on MultiDiscrete([3, 5]), two consecutive iterations: a2c_mcat_train_kat_small.npz (4 envs, n_steps 5, nets [32, 32]).
    Seed conditions: a truncation in each iteration, as for the Categorical fixture, and a rollout whose step the reference itself
    takes well: its own float32 error (_a2c_reference_own_error) at most a quarter of the bar the tests hold an implementation to, so
    that three quarters of the bar remain for the implementation's own float32 rounding, which is of the same kind and size. (Seed 7
    has a gradient element of 8e-5 in action_net.weight whose float32 value is 2.5e-4 off in the reference itself; its step through
    RMSprop's eps = 1e-5 puts the reference's own weight at 0.6 of the bar.)"""
    late = ((1, 396), (2, 399), (3, 392))
    for seed in range(7, 120):
        _, out = _a2c_run(seed, n_envs=4, net_arch=[32, 32], late=late, venv=_make_multidiscrete_venv(4, 3, 5))
        trunc = [int(out[f"it{k}/timeouts"].sum()) for k in range(2)]
        own = _a2c_reference_own_error(out, (3, 5)) if min(trunc) >= 1 else float("inf")
        print(f"a2c mcat small: seed {seed}: truncations {trunc}, the reference's own float32 error {own:.3f} of the bar")
        if min(trunc) >= 1 and own <= 0.25:
            break
    else:
        raise RuntimeError("no seed met the conditions of the small multi-categorical A2C fixture")
    assert int(out["n_truncations"]) >= 2 and out["it0/rollout/actions"].shape == (5, 4, 2) and str(out["optimizer"]) == "RMSprop"
    out["nvec"] = np.array([3, 5], np.int64)
    print(f"a2c mcat small: seed {seed}, gradient norms {[float(out[f'it{k}/grad_norm']) for k in range(2)]}, truncations {trunc}")
    save("a2c_mcat_train_kat_small.npz", **out)


def gen_callbacks():
    """The reference's training callbacks (core/common/callbacks.py:146-680) on small CPU runs of SAC over
    DummyVecEnv([TwoSeriesCSTREnv] * N). Only STRUCTURE is written -- directory listings, evaluations.npz's timesteps / ep_lengths,
    final counters, the timestep or evaluation count at which a stop callback ends the run -- no learned number."""
    import contextlib
    import io
    import tempfile

    from core.common.callbacks import (BaseCallback, CheckpointCallback, EvalCallback, EveryNTimesteps, StopTrainingOnMaxEpisodes,
                                       StopTrainingOnNoModelImprovement, StopTrainingOnRewardThreshold)
    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from core.sac.sac import SAC
    from twoseriescstr import TwoSeriesCSTREnv

    def venv(n, seed):
        v = DummyVecEnv([lambda: TwoSeriesCSTREnv() for _ in range(n)])
        v.seed(seed)
        return v

    def sac(n, **kw):
        kw = dict(dict(seed=0, device="cpu", batch_size=16, buffer_size=4096, learning_starts=40, policy_kwargs=dict(net_arch=[16, 16])), **kw)
        return SAC("MlpPolicy", venv(n, 3), **kw)

    def learn(model, steps, cb):
        with contextlib.redirect_stdout(io.StringIO()):
            model.learn(steps, callback=cb)

    def names(d):
        return np.array(sorted(os.listdir(d)))

    out = {}
    # (a) EvalCallback + CheckpointCallback: 4 envs, eval_freq 50, save_freq 60, 520 steps
    with tempfile.TemporaryDirectory() as d:
        ev = EvalCallback(venv(2, 7), n_eval_episodes=3, eval_freq=50, log_path=os.path.join(d, "log"), best_model_save_path=os.path.join(d, "best"),
                          verbose=0, warn=False)
        ck = CheckpointCallback(save_freq=60, save_path=os.path.join(d, "ck"), name_prefix="m", save_replay_buffer=True)
        model = sac(4)
        learn(model, 520, [ev, ck])
        e = np.load(os.path.join(d, "log", "evaluations.npz"))
        out.update({"a/dims": np.array([4, 2, 3, 50, 60, 520], np.int64), "a/ck_files": names(os.path.join(d, "ck")),
                    "a/log_files": names(os.path.join(d, "log")), "a/best_files": names(os.path.join(d, "best")),
                    "a/eval_keys": np.array(sorted(e.files)), "a/timesteps": e["timesteps"].astype(np.int64),
                    "a/ep_lengths": e["ep_lengths"].astype(np.int64), "a/results_shape": np.array(e["results"].shape, np.int64),
                    "a/counters": np.array([ev.n_calls, ck.n_calls, ev.num_timesteps, model.num_timesteps, model._n_updates], np.int64)})
    # (b) StopTrainingOnMaxEpisodes(2) on 2 envs: the run ends at the step that closes the 4th episode
    cb = StopTrainingOnMaxEpisodes(max_episodes=2)
    model = sac(2, learning_starts=10 ** 6)
    learn(model, 10 ** 5, cb)
    out["b/stop"] = np.array([2, 2, cb.n_episodes, cb.n_calls, model.num_timesteps], np.int64)
    # (c) StopTrainingOnRewardThreshold(-inf) behind an EvalCallback's new best: ends at the first evaluation
    ev = EvalCallback(venv(2, 7), callback_on_new_best=StopTrainingOnRewardThreshold(-np.inf), n_eval_episodes=2, eval_freq=30, verbose=0, warn=False)
    model = sac(4, learning_starts=10 ** 6)
    learn(model, 2000, ev)
    out["c/stop"] = np.array([4, 30, ev.n_calls, model.num_timesteps], np.int64)

    # (d) StopTrainingOnNoModelImprovement(2, min_evals=1) after every evaluation, predictions from a fixed action tape (the model
    #     never trains: learning_starts beyond the run), so the evaluation results depend on the env alone
    class Tape:
        def __init__(self, actions):
            self.actions, self.t = actions, 0

        def predict(self, observations, state=None, episode_start=None, deterministic=False):
            a = self.actions[self.t % len(self.actions)].copy()
            self.t += 1
            return a, state

    tape = np.random.default_rng(99).uniform(-1, 1, size=(257, 2, 2)).astype(np.float32)
    stop = StopTrainingOnNoModelImprovement(max_no_improvement_evals=2, min_evals=1)
    ev = EvalCallback(venv(2, 7), callback_after_eval=stop, n_eval_episodes=2, eval_freq=20, verbose=0, warn=False)
    model = sac(4, learning_starts=10 ** 6)
    tp = Tape(tape)
    model.predict = tp.predict
    learn(model, 10 ** 5, ev)
    out.update({"d/tape": tape, "d/stop": np.array([4, 20, stop.n_calls, ev.n_calls, model.num_timesteps, stop.no_improvement_evals, tp.t], np.int64)})

    # (e) EveryNTimesteps(100) on 4 envs and on 3 envs (100 is no multiple of 3): the timesteps at which the child is called
    class Rec(BaseCallback):
        def __init__(self):
            super().__init__()
            self.seen = []

        def _on_step(self):
            self.seen.append(self.num_timesteps)
            return True

    for n in (4, 3):
        rec = Rec()
        model = sac(n, learning_starts=10 ** 6)
        learn(model, 650, EveryNTimesteps(n_steps=100, callback=rec))
        out[f"e/fired_{n}"] = np.array(rec.seen, np.int64)
        out[f"e/final_{n}"] = np.array([model.num_timesteps], np.int64)
    save("callbacks_kat.npz", **out)


def _goal_reward(ag, dg):
    """The goal face's float32 reward statement (core/common/vec_env/cstr_vec_env.py states the same): the reference's concentration
    term (twoseriescstr.py:288-291) on (achieved, desired), both normalised."""
    lo2, span2, cs = np.float32(0.0), np.float32(0.7) - np.float32(0.0), np.float32(0.45 - 0.05)
    ag, dg = np.asarray(ag, np.float32).reshape(-1), np.asarray(dg, np.float32).reshape(-1)
    c2 = lo2 + (ag + np.float32(1)) * span2 / np.float32(2)
    t = lo2 + (dg + np.float32(1)) * span2 / np.float32(2)
    ne = np.abs(c2 - t) / cs
    return (np.float32(-5) * (ne * ne) - np.float32(2) * ne).astype(np.float32)


def _make_goal_venv(max_steps, targets):
    """Harness code of ours: a wrapper AROUND the unmodified TwoSeriesCSTREnv (not a subclass: the env's own compute_reward(state,
    action) has another signature) that exposes the Dict face and the reward statement above."""
    import gymnasium
    from gymnasium import spaces

    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from twoseriescstr import TwoSeriesCSTREnv

    class GoalCSTR(gymnasium.Env):
        def __init__(self, steps, target):
            self.inner = TwoSeriesCSTREnv()
            self.inner.max_steps = steps
            box = lambda n: spaces.Box(-np.ones(n, np.float32), np.ones(n, np.float32), dtype=np.float32)  # noqa: E731
            self.observation_space = spaces.Dict({"observation": box(4), "achieved_goal": box(1), "desired_goal": box(1)})
            self.action_space = self.inner.action_space
            self.goal = np.float32(2) * (np.float32(target) - np.float32(0.0)) / np.float32(0.7) - np.float32(1)

        def _face(self, o):
            o = np.asarray(o, np.float32)
            return {"achieved_goal": o[2:3].copy(), "desired_goal": np.array([self.goal], np.float32), "observation": o}

        def reset(self, *, seed=None, options=None):
            o, info = self.inner.reset(seed=seed, options=options)
            return self._face(o), info

        def step(self, action):
            o, _, terminated, truncated, info = self.inner.step(action)
            d = self._face(o)
            return d, float(self.compute_reward(d["achieved_goal"][None], d["desired_goal"][None], [info])[0]), terminated, truncated, info

        def compute_reward(self, achieved_goal, desired_goal, infos):
            return _goal_reward(achieved_goal, desired_goal)

    return DummyVecEnv([lambda s=s, t=t: GoalCSTR(s, t) for s, t in zip(max_steps, targets)])


def gen_her():
    """her_buffer_kat.npz: the unmodified HerReplayBuffer (core/her/her_replay_buffer.py) fed by scripted steps of three goal-face envs
    with per-env episode lengths, into rings of 4 and 12 rows through three wraps: the add inputs, the episode bookkeeping after every
    add, seeded sample(10) / sample(256) for the three strategies and n_sampled_goal 0 / 4 (drawn indices, goal indices, the five
    outputs, the MT19937 state afterwards), and a pickle + truncate_last_trajectory case."""
    import pickle
    import warnings

    from core.her.her_replay_buffer import HerReplayBuffer
    from core.her.goal_selection_strategy import KEY_TO_GOAL_STRATEGY

    N, out = 3, {}
    targets = (0.12, 0.20, 0.33)
    for R, tag, steps in ((4, "r4a", (1, 2, 4)), (4, "r4b", (2, 4, 7)), (12, "r12a", (1, 2, 12)), (12, "r12b", (2, 12, 15))):
        venv = _make_goal_venv(steps, targets)
        venv.seed(40 + R)
        obs = venv.reset()
        buf = HerReplayBuffer(R * N, venv.observation_space, venv.action_space, venv, device="cpu", n_envs=N)
        rng = np.random.default_rng(R)
        T = 3 * R + 2
        rec = {k: [] for k in ("obs", "next", "act", "rew", "done", "timeout", "ep_start", "ep_length", "cur")}
        flat = lambda d: np.concatenate([d["achieved_goal"], d["desired_goal"], d["observation"]], axis=1).astype(np.float32)  # noqa: E731
        for _ in range(T):
            a = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
            nobs, r, d, infos = venv.step(a)
            nxt = {k: v.copy() for k, v in nobs.items()}
            for i in range(N):
                if d[i]:
                    for k in nxt:
                        nxt[k][i] = infos[i]["terminal_observation"][k]
            buf.add(obs, nxt, a, r, d, infos)
            for k, v in (("obs", flat(obs)), ("next", flat(nxt)), ("act", a), ("rew", np.asarray(r, np.float32)), ("done", d.astype(np.float32)),
                         ("timeout", np.array([i.get("TimeLimit.truncated", False) for i in infos], np.float32)),
                         ("ep_start", buf.ep_start.copy()), ("ep_length", buf.ep_length.copy()), ("cur", buf._current_ep_start.copy())):
                rec[k].append(v)
            obs = nobs
        out.update({f"{tag}/{k}": np.stack(v) for k, v in rec.items()})
        out[f"{tag}/meta"] = np.array([R, N, T, buf.pos, int(buf.full)], np.int64)
        # seeded samples; np.random.choice / randint are recorded by hooks around the unmodified sample()
        choice, randint = np.random.choice, np.random.randint
        for strategy in ("future", "final", "episode"):
            for nsg in (0, 4):
                for B in ((10, 256) if tag in ("r4a", "r12b") else (10,)):
                    buf.goal_selection_strategy, buf.n_sampled_goal, buf.her_ratio = KEY_TO_GOAL_STRATEGY[strategy], nsg, 1 - (1.0 / (nsg + 1))
                    drawn = {}

                    def rec_choice(a, **kw):
                        drawn["flat"] = choice(a, **kw)
                        return drawn["flat"]

                    def rec_randint(*a, **kw):
                        drawn["goal"] = randint(*a, **kw)
                        return drawn["goal"]

                    np.random.seed(1000 + B + nsg)
                    np.random.choice, np.random.randint = rec_choice, rec_randint
                    try:
                        s = buf.sample(B)
                    finally:
                        np.random.choice, np.random.randint = choice, randint
                    st = np.random.get_state()
                    key = f"{tag}/{strategy}/{nsg}/{B}"
                    out[key + "/flat_idx"] = np.asarray(drawn["flat"], np.int64)
                    out[key + "/goal_idx"] = np.asarray(drawn.get("goal", np.zeros(0)), np.int64)
                    out[key + "/obs"] = np.concatenate([s.observations[k].numpy() for k in ("achieved_goal", "desired_goal", "observation")], axis=1)
                    out[key + "/next"] = np.concatenate([s.next_observations[k].numpy() for k in ("achieved_goal", "desired_goal", "observation")], axis=1)
                    out[key + "/act"], out[key + "/done"], out[key + "/rew"] = s.actions.numpy(), s.dones.numpy(), s.rewards.numpy()
                    out[key + "/mt_key"], out[key + "/mt_pos"] = st[1].astype(np.uint32), np.array([st[2], st[3]], np.int64)
        # save / load / truncate_last_trajectory (:386-408)
        clone = pickle.loads(pickle.dumps(buf))
        clone.set_env(venv)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            clone.truncate_last_trajectory()
        out[f"{tag}/trunc/warned"] = np.array([len(w)], np.int64)
        out[f"{tag}/trunc/ep_length"], out[f"{tag}/trunc/cur"] = clone.ep_length.copy(), clone._current_ep_start.copy()
        out[f"{tag}/trunc/dones"], out[f"{tag}/trunc/timeouts"] = clone.dones.astype(np.float32), clone.timeouts.astype(np.float32)
    save("her_buffer_kat.npz", **out)


# ------------------------------------------------------------------- PPO / A2C on the goal face
GOAL_ONPOLICY_TARGETS = (0.15, 0.20, 0.25, 0.30, 0.35, 0.18, 0.22, 0.28)  # fixed per-env setpoints, mol/L


def _goal_onpolicy_venv(n_envs):
    return _make_goal_venv((400,) * n_envs, GOAL_ONPOLICY_TARGETS[:n_envs])


def _goal_run_extras(out, n_envs):
    """what a goal-face fixture records beside the Box face's: the per-env targets; init_obs / rollout/observations / last_obs already are
    the flat rows [achieved_goal | desired_goal | observation] (_obs_rows)"""
    out["targets"] = np.array(GOAL_ONPOLICY_TARGETS[:n_envs], np.float32)
    return out


def gen_ppo_goal():
    """PPO("MultiInputPolicy") of the UNMODIFIED reference (MultiInputActorCriticPolicy, CombinedExtractor, DictRolloutBuffer:
    core/common/policies.py:839-910, core/common/buffers.py:696-840) on the goal-face harness env: ppo_goal_train_kat_small.npz (4 envs,
    n_steps 8, batch 12, 3 epochs, nets [32, 32], lr 3e-3), ppo_goal_train_kat_default.npz (class-default nets, 8 envs, n_steps 16,
    batch 64, 2 epochs) and ppo_goal_predict_kat.npz (16 seeded dict observations)."""
    late = ((1, 396), (2, 399), (3, 395))
    small = dict(n_envs=4, n_steps=8, batch_size=12, n_epochs=3, net_arch=[32, 32], late=late, policy="MultiInputPolicy", gaussian=True)
    for seed in range(7, 80):
        model, out, hk = _ppo_run(seed, venv=_goal_onpolicy_venv(4), **small)
        clipped = max(float(mb["scalars"][5]) for mb in hk.minibatches)
        if clipped > 0 and int(out["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, None):
            break
    else:
        raise RuntimeError("no seed met the conditions of the small goal-face PPO fixture")
    assert type(model.rollout_buffer).__name__ == "DictRolloutBuffer" and type(model.policy).__name__ == "MultiInputActorCriticPolicy"
    assert model.policy.features_dim == 6 and tuple(out["before/policy/mlp_extractor.policy_net.0.weight"].shape) == (32, 6)
    print(f"ppo goal small: seed {seed}, max clip_fraction {clipped:.3f}, truncations {int(out['n_truncations'])}")
    save("ppo_goal_train_kat_small.npz", **_goal_run_extras(out, 4))
    model, o, hk = _ppo_run(11, n_envs=8, n_steps=16, batch_size=64, n_epochs=2, late=((0, 390), (5, 397), (6, 399)), venv=_goal_onpolicy_venv(8),
                            policy="MultiInputPolicy", gaussian=True)
    assert int(o["n_truncations"]) >= 2 and _ppo_margins_ok(hk, 0.2, None)
    save("ppo_goal_train_kat_default.npz", **_goal_run_extras(o, 8))
    # predict: the trained small model on seeded dict observations, deterministic and sampled (the draw is recorded), and predict_values
    model, _, _ = _ppo_run(int(out["seed"]), venv=_goal_onpolicy_venv(4), **small)
    rows = np.random.default_rng(99).uniform(-1, 1, (16, 6)).astype(np.float32)
    obs = {"achieved_goal": rows[:, 0:1].copy(), "desired_goal": rows[:, 1:2].copy(), "observation": rows[:, 2:6].copy()}
    p = _flat_sd("policy", model.policy.state_dict())
    p["rows"], p["net_arch"], p["seed"] = rows, np.array([32, 32], np.int64), out["seed"]
    p["deterministic"], _ = model.predict(obs, deterministic=True)
    with _PpoHooks() as hk:
        p["sampled"], _ = model.predict(obs, deterministic=False)
        p["eps"] = hk.draws[0].numpy()
    with th.no_grad():
        p["values"] = model.policy.predict_values({k: th.as_tensor(v) for k, v in obs.items()}).numpy()
    save("ppo_goal_predict_kat.npz", **p)


def gen_a2c_goal():
    """A2C("MultiInputPolicy") of the unmodified reference on the goal-face harness env, two consecutive iterations:
    a2c_goal_train_kat_small.npz (4 envs, n_steps 5, nets [32, 32], ent_coef 0.01, lr 3e-3; the clip engaged in both steps)."""
    late = ((1, 396), (2, 399), (3, 392))
    for seed in range(7, 80):
        model, out = _a2c_run(seed, n_envs=4, net_arch=[32, 32], late=late, venv=_goal_onpolicy_venv(4), policy="MultiInputPolicy", gaussian=True)
        norms = [float(out[f"it{k}/grad_norm"]) for k in range(2)]
        trunc = [int(out[f"it{k}/timeouts"].sum()) for k in range(2)]
        if min(norms) > 1.05 * 0.5 and min(trunc) >= 1:
            break
    else:
        raise RuntimeError("no seed met the conditions of the small goal-face A2C fixture")
    assert type(model.rollout_buffer).__name__ == "DictRolloutBuffer" and str(out["optimizer"]) == "RMSprop"
    print(f"a2c goal small: seed {seed}, gradient norms {norms}, truncations {trunc}")
    save("a2c_goal_train_kat_small.npz", **_goal_run_extras(out, 4))


GENS = {"her": gen_her, "her_learners": gen_her_learners, "ppo_multidiscrete": gen_ppo_multidiscrete, "a2c_multidiscrete": gen_a2c_multidiscrete, "ppo_discrete": gen_ppo_discrete, "a2c_discrete": gen_a2c_discrete, "callbacks": gen_callbacks, "a2c": gen_a2c, "ppo": gen_ppo, "bcq": lambda: (gen_bcq(), gen_bcq_predict()), "maddpg_default": gen_maddpg_default, "maddpg4_default": gen_maddpg4_default, "maddpg4": gen_maddpg4, "ddpg": gen_ddpg, "eval": gen_eval, "evalmodel": gen_evalmodel, "info": gen_info, "config1": gen_config1, "env": gen_env, "resets": gen_resets, "vecnorm": gen_vecnorm, "vecenv": gen_vecenv, "sampler": gen_sampler, "replay": gen_replay, "sac": gen_sac,
        "sac_ncrit": gen_sac_ncrit, "sac_sde": gen_sac_sde, "td3_ncrit": gen_td3_ncrit,
        "td3": gen_td3, "init": gen_init, "maddpg": gen_maddpg, "iddpg": gen_iddpg, "checkpoint": gen_checkpoint, "dqn": gen_dqn,
        "rmsprop_tf": gen_rmsprop_tf, "ppo_goal": gen_ppo_goal, "a2c_goal": gen_a2c_goal}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(GENS))
    args = ap.parse_args()
    for k in args.only.split(","):
        GENS[k]()
