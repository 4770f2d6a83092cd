"""`evaluate_policy` (reference: core/common/evaluation.py:11-140).

Two evaluation loops with the reference's episode accounting (static split of the episodes over the sub-environments,
returns = float64 sums of the float32 step rewards, episodes appended in sub-environment order within a vec-step):

  * device loop -- `model` is one of this stack's algorithms / policies and `env` a `CSTRVecEnv` (optionally wrapped in
    `VecNormalize`), no per-step callback: actor, `predict()`'s action post-processing (policies.py:379-386), env step and the
    accounting all stay in HBM; the host reads one flag per vec-step and the finished episodes' rows;
  * host loop -- any object with `predict(observations, state=, episode_start=, deterministic=)` (evaluation.py:88-93) and any
    `VecEnv` of this package, NumPy in / NumPy out like the reference; also taken when a `callback` wants `locals()` per
    (step, env) (evaluation.py:104-105).

`evaluate_policy_fused` (specific to this package) runs the same evaluation as ONE launch, cstr_eval_episodes_f32: every env's
episodes are walked inside the kernel and the host reads three arrays back. It covers deterministic evaluation of a two-hidden-layer
actor on a bare `CSTRVecEnv`; `supported()` tells whether it applies. On the goal face (`goal_conditioned=True`, SAC / TD3 / DDPG / PPO / A2C on
"MultiInputPolicy") the launch is cstr_eval_goal_episodes_f32, and `evaluate_goal_tracking` returns what it knows per episode beyond the
return: the setpoint that was drawn, how far C2 ended from it and the mean absolute gap on the way.

`evaluate_trajectories` (specific to this package) returns the closed-loop trajectories themselves -- states, applied flows and rewards per
episode -- from ONE launch of the recording kernel, cstr_collect_episodes_f32, into a temporary replay ring; the same launch is what
`core.common.offline_dataset.collect_offline_dataset` and `twoseriescstr.evaluate_model` run.
"""
import warnings
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch as th
from torch import nn

from core.common import hip_ops
from core.common.vec_env import CSTRVecEnv
from core.common.vec_env.base_vec_env import VecEnv


_MONITOR_WARNING = ("Evaluation environment is not wrapped with a ``Monitor`` wrapper. "
                    "This may result in reporting modified episode lengths and rewards, if other wrappers happen to modify these. "
                    "Consider wrapping environment first with ``Monitor`` wrapper.")


def _device_post(policy, dev):
    """`BasePolicy.predict`'s post-processing of the actor output (policies.py:379-386) as device ops with numpy's float32
    rounding points: squashed policies un-scale (`low + 0.5 * (a + 1) * (high - low)`), others clip into the action box.
    MADDPG's per-agent un-scaling (multi_agent_policies.py:605-610) is the same expression on the agent's columns."""
    low = th.as_tensor(np.asarray(policy.action_space.low, np.float32), device=dev)
    high = th.as_tensor(np.asarray(policy.action_space.high, np.float32), device=dev)
    if policy.squash_output:
        span = high - low
        return lambda a: low + (0.5 * (a + 1.0)) * span
    return lambda a: th.minimum(th.maximum(a, low), high)


def _evaluate_on_device(policy, env, targets_h: np.ndarray, deterministic: bool):
    n, dev = env.num_envs, env.unwrapped.device
    targets = th.as_tensor(targets_h, device=dev)
    counts = th.zeros(n, dtype=th.long, device=dev)
    cur_ret = th.zeros(n, dtype=th.float64, device=dev)   # current_rewards = np.zeros(n_envs): float64 (evaluation.py:84)
    cur_len = th.zeros(n, dtype=th.long, device=dev)
    rets, lens = [], []
    obs = env.reset_device()
    policy.set_training_mode(False)
    post = _device_post(policy, dev)
    while bool((counts < targets).any()):
        with th.no_grad():
            act = post(policy._predict(obs, deterministic=deterministic))
        obs, rew, done, _, _ = env.step_device(act.contiguous())
        cur_ret += rew.to(th.float64)
        cur_len += 1
        fin = (done > 0) & (counts < targets)
        if bool(fin.any()):
            rets += cur_ret[fin].cpu().tolist()
            lens += cur_len[fin].cpu().tolist()
            counts += fin.long()
            cur_ret[fin] = 0.0
            cur_len[fin] = 0
    return rets, lens


def _evaluate_on_host(model, env, targets: np.ndarray, deterministic: bool, render: bool, callback):
    n_envs = env.num_envs
    episode_rewards, episode_lengths = [], []
    episode_counts = np.zeros(n_envs, dtype="int")
    episode_count_targets = targets
    current_rewards = np.zeros(n_envs)
    current_lengths = np.zeros(n_envs, dtype="int")
    observations = env.reset()
    states = None
    episode_starts = np.ones((n_envs,), dtype=bool)
    while (episode_counts < episode_count_targets).any():
        actions, states = model.predict(observations, state=states, episode_start=episode_starts, deterministic=deterministic)
        new_observations, rewards, dones, infos = env.step(actions)
        current_rewards += rewards
        current_lengths += 1
        for i in np.nonzero(episode_counts < episode_count_targets)[0]:
            reward, done, info = rewards[i], dones[i], infos[i]
            episode_starts[i] = done
            if callback is not None:  # locals() once per (vec-step, active env), before the episode is closed (:104-105)
                callback(locals(), globals())
            if dones[i]:
                episode_rewards.append(current_rewards[i])
                episode_lengths.append(current_lengths[i])
                episode_counts[i] += 1
                current_rewards[i] = 0
                current_lengths[i] = 0
        observations = new_observations
        if render:
            env.render()
    return episode_rewards, episode_lengths


def evaluate_policy(model, env, n_eval_episodes: int = 10, deterministic: bool = True, render: bool = False,
                    callback: Optional[Callable] = None, reward_threshold: Optional[float] = None,
                    return_episode_rewards: bool = False, warn: bool = True) -> Union[Tuple[float, float], Tuple[list, list]]:
    if not isinstance(env, VecEnv) and not isinstance(getattr(env, "unwrapped", None), CSTRVecEnv):
        raise ValueError("evaluate_policy: pass a VecEnv of this package (CSTRVecEnv, optionally wrapped in VecNormalize)")
    if warn:  # no Monitor / VecMonitor wrapper exists in this stack: the reference's warning always applies (evaluation.py:64-70)
        warnings.warn(_MONITOR_WARNING, UserWarning)
    n = env.num_envs
    targets = np.array([(n_eval_episodes + i) // n for i in range(n)], dtype="int")  # :79-82
    policy = getattr(model, "policy", model)
    on_device = (callback is None and not render and isinstance(getattr(env, "unwrapped", None), CSTRVecEnv)
                 and hasattr(env, "step_device") and hasattr(policy, "_predict") and hasattr(policy, "squash_output")
                 and hasattr(getattr(policy, "action_space", None), "low"))  # a Discrete face (DQN) steps through env.step(indices)
    if on_device:
        rets, lens = _evaluate_on_device(policy, env, targets, deterministic)
    else:
        rets, lens = _evaluate_on_host(model, env, targets, deterministic, render, callback)
    mean_reward, std_reward = np.mean(rets), np.std(rets)
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, "Mean reward below threshold: " f"{mean_reward:.2f} < {reward_threshold:.2f}"
    if return_episode_rewards:
        return rets, lens
    return mean_reward, std_reward


# ---- the whole evaluation in one launch ---------------------------------------------------------------------------------

# What `EvalCallback(fused=None)` picks where `supported()` holds. Decided by measurement (tools/eval_probe.py, profiles/eval_probe.txt,
# DESIGN.md 5): the launch is the default because it is faster than the device loop at both probed env counts (4.3 ms against 98.5 ms
# with 16 evaluation envs, 5.6 ms against 93.4 ms with 256; on the goal face, tools/goal_eval_probe.py, profiles/goal_eval_probe.txt: 4.7 ms
# against 87.2 ms and 6.0 ms against 87.5 ms).
FUSED_BY_DEFAULT = True

_ACTS = {nn.ReLU: 1, nn.Tanh: 2}


def _two_layer_mlp(seq):
    """(l1, l2, act) of nn.Sequential(Linear, act, Linear, act) with one activation class, else None"""
    mods = list(seq)
    if len(mods) != 4 or not (isinstance(mods[0], nn.Linear) and isinstance(mods[2], nn.Linear)):
        return None
    if type(mods[1]) not in _ACTS or type(mods[1]) is not type(mods[3]):
        return None
    return mods[0], mods[2], _ACTS[type(mods[1])]


def _fused_operands(policy) -> Optional[dict]:
    """The policy's deterministic actor as operands of hip_ops.eval_episodes / goal_eval_episodes (cstr_policy_mlp_t), or None if that
    struct cannot describe it: SAC's actor without gSDE (head 0 at its mode), TD3's / DDPG's actor (head 1, tanh), `ActorCriticPolicy`
    with a two-layer `policy_net` and a linear `action_net` (head 1, no output activation, clipped instead of un-scaled). `goal`: the
    actor sits behind a `CombinedExtractor` (MultiInputPolicy of SAC / TD3 / DDPG / PPO / A2C), i.e. its rows are the goal face's flat rows."""
    from core.common.policies import ActorCriticPolicy
    from core.common.torch_layers import CombinedExtractor, FlattenExtractor

    actor = getattr(policy, "actor", None)
    if isinstance(policy, ActorCriticPolicy):
        if getattr(policy, "use_sde", False) or not isinstance(policy.features_extractor, (FlattenExtractor, CombinedExtractor)):
            return None
        net = _two_layer_mlp(policy.mlp_extractor.policy_net)
        if net is None or not isinstance(policy.action_net, nn.Linear):
            return None
        l1, l2, act = net
        return dict(layers=(l1, l2), w3=policy.action_net.weight, b3=policy.action_net.bias, act=act, head=1, out_act=0,
                    goal=isinstance(policy.features_extractor, CombinedExtractor))
    if not isinstance(actor, nn.Module) or not isinstance(getattr(actor, "features_extractor", None), (FlattenExtractor, CombinedExtractor)):
        return None
    goal = isinstance(actor.features_extractor, CombinedExtractor)
    if isinstance(getattr(actor, "latent_pi", None), nn.Sequential):  # SAC
        if getattr(actor, "use_sde", False) or not isinstance(actor.mu, nn.Linear) or not isinstance(actor.log_std, nn.Linear):
            return None
        net = _two_layer_mlp(actor.latent_pi)
        if net is None:
            return None
        l1, l2, act = net
        return dict(layers=(l1, l2), w3=th.cat((actor.mu.weight, actor.log_std.weight), dim=0), b3=th.cat((actor.mu.bias, actor.log_std.bias), dim=0),
                    act=act, head=0, out_act=0, goal=goal)
    if isinstance(getattr(actor, "mu", None), nn.Sequential):  # TD3 / DDPG: create_mlp(..., squash_output=True)
        mods = list(actor.mu)
        if len(mods) != 6 or not isinstance(mods[4], nn.Linear) or not isinstance(mods[5], nn.Tanh):
            return None
        net = _two_layer_mlp(nn.Sequential(*mods[:4]))
        if net is None:
            return None
        l1, l2, act = net
        if getattr(policy, "normalize_states", False):  # TD3+BC: the env's raw observations go through the dataset's statistics
            l1 = _fold_obs_norm(l1, getattr(policy, "obs_norm", None))
        return dict(layers=(l1, l2), w3=mods[4].weight, b3=mods[4].bias, act=act, head=1, out_act=2, goal=goal)
    return None


def _fold_obs_norm(l1: nn.Linear, obs_norm):
    """The first layer on (o - mean) / std as a layer on o: W' = W / std per input column, b' = b - W' @ mean. Temporaries of one
    call (float64 arithmetic, float32 storage); the model's parameters are untouched. A policy trained on normalised observations
    without its statistics is an error, never a launch on the raw network."""
    if obs_norm is None or obs_norm[0] is None or obs_norm[1] is None:
        raise RuntimeError("the policy was trained on normalised observations (normalize_states=True) and its statistics are missing: "
                           "the one-launch evaluation would step the env with a policy that sees raw observations")
    from types import SimpleNamespace

    with th.no_grad():
        mean, std = (t.to(l1.weight.device, th.float64) for t in obs_norm)
        w = l1.weight.detach().to(th.float64) / std
        b = l1.bias.detach().to(th.float64) - w @ mean
        return SimpleNamespace(weight=w.to(th.float32).contiguous(), bias=b.to(th.float32).contiguous(), in_features=l1.in_features,
                               out_features=l1.out_features)


def _why_not_fused(model, env, deterministic: bool) -> Optional[str]:
    if not deterministic:
        return "stochastic evaluation (deterministic=False)"
    if not isinstance(env, CSTRVecEnv):
        return "the evaluation env must be a bare CSTRVecEnv (no VecNormalize or other wrapper)"
    if env.discrete_actions is not None:
        return "the Discrete valve face (DQN)"
    if getattr(env, "multi_discrete_actions", None) is not None:
        return "the MultiDiscrete valve face (one categorical per valve: the launch has no MultiCategorical head)"
    policy = getattr(model, "policy", model)
    if not isinstance(policy, nn.Module) or not hasattr(policy, "squash_output") or not hasattr(getattr(policy, "action_space", None), "low"):
        return f"{type(policy).__name__} is not a single-agent policy over a Box action space"
    ops = _fused_operands(policy)
    if ops is None:
        return f"{type(policy).__name__}: the actor is not a two-hidden-layer MLP that cstr_policy_mlp_t describes (gSDE, other depths, BCQ, MADDPG)"
    if ops["goal"] != env.goal_conditioned:
        return ("a goal-face model (MultiInputPolicy) on an env without goal_conditioned=True" if ops["goal"]
                else "a Box-face model on the goal face (goal_conditioned=True needs a MultiInputPolicy)")
    l1, l2 = ops["layers"]
    k0 = hip_ops.GOAL_ROW if ops["goal"] else env.obs_dim  # the goal face's flat row [achieved | desired | observation]
    shape_ok = (hip_ops.goal_eval_episodes_supported(l1.out_features, l2.out_features, ops["w3"].shape[0], ops["head"]) if ops["goal"] else
                hip_ops.eval_episodes_supported(l1.in_features, l1.out_features, l2.out_features, ops["w3"].shape[0], ops["head"], env.act_dim))
    if not shape_ok:
        return f"network shape ({l1.in_features}, {l1.out_features}, {l2.out_features}, {ops['w3'].shape[0]}) on a ({env.obs_dim}, {env.act_dim}) env"
    if l1.in_features != k0 or l1.weight.device != env.device:
        return "policy and env disagree on the observation width or the device"
    return None


def supported(model, env, deterministic: bool = True) -> bool:
    """Whether `evaluate_policy_fused` applies to this model / policy, env and mode."""
    return _why_not_fused(model, env, deterministic) is None


def _aligned(t: th.Tensor) -> th.Tensor:
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _launch(model, env, n_eval_episodes: int, tracking: bool = False):
    """The one launch behind `evaluate_policy_fused` / `evaluate_goal_tracking` on a supported (model, env): resets the env, runs every
    env's episodes and returns (order, arrays) -- the reference's episode order as (env, slot) pairs
    (an episode is appended at the vec-step it ends, sub-environments in order within a vec-step: evaluation.py:99-126) and the launch's
    per-episode arrays on the host: (ep_return, ep_len) and, with `tracking` on the goal face, (ep_goal, ep_gap, ep_abs_gap) behind them."""
    n = env.num_envs
    targets = np.array([(n_eval_episodes + i) // n for i in range(n)], dtype="int")  # :79-82
    policy = getattr(model, "policy", model)
    ops = _fused_operands(policy)
    l1, l2 = ops["layers"]
    env.reset_device()
    with th.no_grad(), th.cuda.device(env.device):
        w1, w2, w3 = _aligned(l1.weight), _aligned(l2.weight), _aligned(ops["w3"])
        b1, b2, b3 = l1.bias.detach().contiguous(), l2.bias.detach().contiguous(), ops["b3"].detach().contiguous()
        net = (w1, b1, w2, b2, w3, b3, ops["act"], ops["head"], ops["out_act"], hip_ops.policy_swizzle(w2), env.coef, env.integrator)
        low, high = np.asarray(policy.action_space.low, np.float32), np.asarray(policy.action_space.high, np.float32)
        max_vec_steps = int(targets.max()) * int(env.coef.max_steps)
        if ops["goal"]:  # the launch advances obs / step_count / pcg_state / targets / episode in place, as step_device does
            lo_g, hi_g = env.goal_range if env.goal_range is not None else (0.0, 0.0)
            out = hip_ops.goal_eval_episodes(*net, env.obs, env.step_count, env.pcg_state, env.targets, policy.squash_output, low, high, targets,
                                             max_vec_steps, static_init=env.static_init, episode=env.episode, goal_seed=env.goal_seed,
                                             goal_index_offset=env.seed_offset, goal_lo=lo_g, goal_hi=hi_g, tracking=tracking)
            env._refresh_flat(redraw=False)  # the flat rows of the state the launch left
        else:
            out = hip_ops.eval_episodes(*net, env.obs, env.step_count, env.pcg_state, policy.squash_output, low, high, targets, max_vec_steps,
                                        static_init=env.static_init)
        arrays = [t.cpu().numpy() for t in out[:2] + out[3:]]  # (the wrapper has read ep_done back and checked it against the targets)
    len_h = arrays[1]
    order = [(i, j) for _, i, j in sorted((int(len_h[i, :j + 1].sum()), i, j) for i in range(n) for j in range(int(targets[i])))]
    return order, arrays


# ---- recorded rollouts: the same walk, every step left in a replay ring (cstr_collect_episodes_f32) --------------------------------

def _why_not_collected(model, env) -> Optional[str]:
    """Why the recording launch does not cover (model, env), or None: what `_why_not_fused` declines, the goal face and the 8-wide
    observation layouts."""
    why = _why_not_fused(model, env, True)
    if why is None and env.goal_conditioned:
        why = "the goal face (goal_conditioned=True): HerReplayBuffer datasets are not collected by this launch"
    if why is None and (env.obs_dim, env.act_dim) != hip_ops.LAYOUTS[0]:
        why = f"the ({env.obs_dim}, {env.act_dim}) observation layout: the recording launch exists for {hip_ops.LAYOUTS[0]}"
    return why


def _collect_launch(model, env, ring, n_steps: int, explore_prob: float = 0.0, seed: int = 0, ep_stride: int = 0, row0: int = 0,
                    step_offset: int = 0):
    """`n_steps` vec-steps of a supported (model, env) from the env's CURRENT state into rows `row0 ..` of `ring`, one launch.
    Returns (ep_return, ep_len, ep_done) on the host."""
    policy = getattr(model, "policy", model)
    ops = _fused_operands(policy)
    l1, l2 = ops["layers"]
    with th.no_grad(), th.cuda.device(env.device):
        w1, w2, w3 = _aligned(l1.weight), _aligned(l2.weight), _aligned(ops["w3"])
        b1, b2, b3 = l1.bias.detach().contiguous(), l2.bias.detach().contiguous(), ops["b3"].detach().contiguous()
        low, high = np.asarray(policy.action_space.low, np.float32), np.asarray(policy.action_space.high, np.float32)
        out = hip_ops.collect_episodes(w1, b1, w2, b2, w3, b3, ops["act"], ops["head"], ops["out_act"], hip_ops.policy_swizzle(w2), env.coef,
                                       env.integrator, env.obs, env.step_count, env.pcg_state, policy.squash_output, low, high, ring, n_steps,
                                       row0=row0, explore_prob=explore_prob, seed=seed, index_offset=env.seed_offset, step_offset=step_offset,
                                       ep_stride=ep_stride, static_init=env.static_init)
        return tuple(t.cpu().numpy() for t in out)


def segment_episodes(rewards: np.ndarray, dones: np.ndarray):
    """Episodes of recorded [T, N] `rewards` / `dones` that ENDED within the T rows, in `evaluate_policy`'s order (the vec-step an episode
    ends at, then the env index): a list of (env, first row, length) and the float64 sums of the float32 rewards -- what the launch's
    ep_return holds, recomputed on the host."""
    rewards, dones = np.asarray(rewards), np.asarray(dones)
    spans, rets = [], []
    start = np.zeros(rewards.shape[1], np.int64)
    for t, i in zip(*np.nonzero(dones > 0)):  # row-major: by vec-step, then by env
        spans.append((int(i), int(start[i]), int(t + 1 - start[i])))
        rets.append(np.cumsum(rewards[start[i]:t + 1, i], dtype=np.float64)[-1])  # the kernel's order: one f64 add per step
        start[i] = t + 1
    return spans, np.asarray(rets, np.float64)


def pad_episodes(field: np.ndarray, spans, l_max: Optional[int] = None) -> np.ndarray:
    """[E, Lmax, ...] float64 from a recorded [T, N, ...] field and `segment_episodes`' spans; rows past an episode's end are NaN."""
    field = np.asarray(field)
    l_max = max((ln for _, _, ln in spans), default=0) if l_max is None else l_max
    out = np.full((len(spans), l_max) + field.shape[2:], np.nan, np.float64)
    for e, (i, s, ln) in enumerate(spans):
        out[e, :ln] = field[s:s + ln, i]
    return out


def evaluate_trajectories(model, env, n_eval_episodes: int = 10) -> dict:
    """Closed-loop trajectories of deterministic evaluation, from ONE launch (cstr_collect_episodes_f32 without exploration) into a
    temporary ring: the env is reset, every env runs ceil(n_eval_episodes / n_envs) episodes' worth of vec-steps, and the first
    `n_eval_episodes` episodes in `evaluate_policy`'s order (the vec-step an episode ends at, then the env index) are returned as
      episode_rewards [E] float64 (f64 sums of the f32 step rewards), episode_lengths [E] int64,
      states  [E, Lmax, 4] float64 -- the recorded float32 observation BEFORE each step as [C1, T1, C2, T2] in mol/L and K
                                      (low + (o + 1) (high - low) / 2 in float32): row 0 is the reset state, the terminal state is not a row;
      actions [E, Lmax, 2] float64 -- the coolant flows the env applied, L/min;
      rewards [E, Lmax]    float64.
    Episodes shorter than Lmax are padded with NaN (take nanmean over episodes). Raises ValueError where the launch does not apply."""
    why = _why_not_collected(model, env)
    if why is not None:
        raise ValueError(f"evaluate_trajectories does not cover {why}")
    n, limit = env.num_envs, int(env.coef.max_steps)
    n_steps = -(-int(n_eval_episodes) // n) * limit
    if n_steps <= 0:
        raise ValueError("n_eval_episodes must be positive")
    env.reset_device()
    with th.cuda.device(env.device):
        ring = hip_ops.DeviceRing(n_steps, n, env.obs_dim, env.act_dim, env.device)
    _collect_launch(model, env, ring, n_steps)
    return _trajectories(env, ring, n_eval_episodes)


def _trajectories(env, ring, n_episodes: int) -> dict:
    from twoseriescstr import TwoSeriesCSTREnv as E

    rew, done = ring.rewards.cpu().numpy(), ring.dones.cpu().numpy()
    spans, rets = segment_episodes(rew, done)
    spans, rets = spans[:n_episodes], rets[:n_episodes]
    obs, act = ring.observations.cpu().numpy(), ring.actions.cpu().numpy()
    raw = E.raw_state_low + (obs + np.float32(1.0)) * (E.raw_state_high - E.raw_state_low) / np.float32(2.0)   # _denormalize_state
    low, high = np.asarray(env.action_space.low, np.float32), np.asarray(env.action_space.high, np.float32)
    ea = low + (np.float32(0.5) * (act + np.float32(1.0)) * (high - low))  # the env action behind the buffer action (unscale_action)
    flow = E.raw_action_low + (np.clip(ea, -1.0, 1.0) + np.float32(1.0)) * (E.raw_action_high - E.raw_action_low) / np.float32(2.0)
    return dict(episode_rewards=rets, episode_lengths=np.array([ln for _, _, ln in spans], np.int64), states=pad_episodes(raw, spans),
                actions=pad_episodes(flow, spans), rewards=pad_episodes(rew, spans))


def evaluate_policy_fused(model, env, n_eval_episodes: int = 10, deterministic: bool = True, reward_threshold: Optional[float] = None,
                          return_episode_rewards: bool = False, warn: bool = True) -> Union[Tuple[float, float], Tuple[list, list]]:
    """`evaluate_policy` as ONE launch (hip_ops.eval_episodes; on the goal face hip_ops.goal_eval_episodes): same arguments minus `render` /
    `callback`, same return values, the episode lists in the reference's order -- sorted by (vec-step at which the episode ended, env
    index). Raises ValueError where `supported()` is False."""
    why = _why_not_fused(model, env, deterministic)
    if why is not None:
        raise ValueError(f"evaluate_policy_fused does not cover {why}; use evaluate_policy")
    if warn:
        warnings.warn(_MONITOR_WARNING, UserWarning)
    order, (ret_h, len_h) = _launch(model, env, n_eval_episodes)
    rets = [float(ret_h[i, j]) for i, j in order]
    lens = [int(len_h[i, j]) for i, j in order]
    mean_reward, std_reward = np.mean(rets), np.std(rets)
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, "Mean reward below threshold: " f"{mean_reward:.2f} < {reward_threshold:.2f}"
    if return_episode_rewards:
        return rets, lens
    return mean_reward, std_reward


def evaluate_goal_tracking(model, env, n_eval_episodes: int = 10, warn: bool = True) -> dict:
    """Setpoint tracking of a goal-face model, from the same launch as `evaluate_policy_fused` (deterministic actions) with its three
    per-episode tracking outputs. Returns float64 / int arrays with one entry per episode, in the reference's episode order:
      episode_rewards, episode_lengths -- what `evaluate_policy_fused(..., return_episode_rewards=True)` returns;
      target          -- the episode's setpoint in mol/L: the launch's normalised desired goal g through the inverse of the env's affine
                         map in float64, s_lo[2] + (g + 1) s_span[2] / 2;
      final_error     -- C2 - setpoint in mol/L at the episode's terminal observation (signed): the launch's float32 gap times s_span[2] / 2;
      mean_abs_error  -- mean over the episode's steps of |C2 - setpoint| in mol/L, each step's next observation against the episode's setpoint.
    Raises ValueError where `supported(model, env)` is False or the env is not the goal face."""
    why = _why_not_fused(model, env, True)
    if why is None and not env.goal_conditioned:
        why = "an env without the goal face (goal_conditioned=True)"
    if why is not None:
        raise ValueError(f"evaluate_goal_tracking does not cover {why}")
    if warn:
        warnings.warn(_MONITOR_WARNING, UserWarning)
    order, (ret_h, len_h, goal_h, gap_h, abs_h) = _launch(model, env, n_eval_episodes, tracking=True)
    pick = lambda x: np.array([x[i, j] for i, j in order], dtype=np.float64)  # noqa: E731
    lo2, half_span = float(env.coef.s_lo[2]), float(env.coef.s_span[2]) / 2.0
    lens = np.array([int(len_h[i, j]) for i, j in order], dtype=np.int64)
    return dict(episode_rewards=pick(ret_h), episode_lengths=lens, target=lo2 + (pick(goal_h) + 1.0) * half_span,
                final_error=pick(gap_h) * half_span, mean_abs_error=pick(abs_h) / lens * half_span)
