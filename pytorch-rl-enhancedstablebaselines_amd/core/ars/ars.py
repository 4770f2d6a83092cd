"""Augmented Random Search (Mania, Guy & Recht 2018, "Simple random search provides a competitive approach to reinforcement
learning"; sb3_contrib.ARS) with sb3_contrib's constructor, defaults, update arithmetic and logger keys. No backward pass, no critic,
no replay ring, no optimiser: one update evaluates 2 n_delta perturbed copies of a small deterministic policy over whole episodes and
moves the parameters along the best directions.

ONE UPDATE (`_do_one_update`), theta = `weights`, s = delta_std, P = len(theta):
    1. deltas ~ N(0, 1) [n_delta, P]
    2. candidates theta + s delta_k (index k) and theta - s delta_k (index n_delta + k)
    3. R_c = sum of the candidate's episode rewards over its n_eval_episodes episodes + alive_bonus_offset * sum of their lengths
       (a sum, not a mean)
    4. top_k = max(R+_k, R-_k); keep the n_top largest
    5. return_std = unbiased standard deviation over the 2 n_top kept returns
    6. step_size = learning_rate / (n_top * return_std + 1e-6)
    7. theta += step_size * sum over the kept k of (R+_k - R-_k) delta_k
    8. num_timesteps += sum of all episode lengths
ORDERING RULES: ties in top_k go to the lower k; a NaN return counts as the greatest (as torch.argsort(descending=True) orders it)
and the step is then NaN, as published -- this is not "fixed". Steps 5-7 run in float64 with one float32 rounding of theta.

THE DELTAS ARE NEVER STORED: delta[k][p] is a function of (delta seed, update index, k, p) through Philox4x32-10 and Box-Muller
(include/cstr_rl_hip.h, "Augmented Random Search"; `ars_deltas` below is the same statement in NumPy). The delta seed is the model's
`seed` (drawn from the OS when None) and the update index is `_n_updates`.

TWO PATHS, reported by `fused_learner`:
  * kernel path -- a bare `CSTRVecEnv` on the Box face (layouts (4,2), (8,2), (8,4), either integrator, either init_mode) and a policy
    `hip_ops.ars_supported` takes (0, 1 or 2 hidden layers of width <= 64, ReLU or Tanh, n_delta <= 4096): ONE population launch
    (candidate c on env slot c % n_envs, a slot's candidates one after another; each does the env's reset draw, its episodes and the
    auto-reset draws) and ONE update launch per update, then one read of six doubles -- the only host synchronisation.
    `CSTRVecEnv(2 * n_delta)` evaluates every candidate in parallel; `CSTRVecEnv(1)` consumes the env's random stream exactly as the
    published sequential loop does.
  * published statements -- everything else the constructor accepts, and `fused_learner = False`: the candidates in index order
    through `evaluate_policy(model, env, n_eval_episodes, return_episode_rewards=True, deterministic=True)`, then the update in torch.

CALLBACKS: `update_locals` / `on_step()` run ONCE PER UPDATE, after the step, on both paths (the published code calls them per env step
from inside `evaluate_policy`); a `False` return ends `learn()`.

Refused: VecNormalize-wrapped envs, the goal face, the Discrete and MultiDiscrete faces, data-parallel runs, `enable_graph_capture(True)`
(two launches per update need no graph), n_delta < 1, n_eval_episodes < 1, delta_std <= 0, `async_eval` (not built)."""
import sys
import time
import warnings
from typing import Optional, Union

import numpy as np
import torch as th
from torch import nn

from core import _native as nv
from core.ars.policies import ARSLinearPolicy, ARSPolicy
from core.common import hip_ops
from core.common.base_class import BaseAlgorithm
from core.common.evaluation import evaluate_policy
from core.common.utils import get_schedule_fn
from core.common.vec_env import CSTRVecEnv, unwrap_vec_normalize

_ACTS = {nn.ReLU: hip_ops.ACT["relu"], nn.Tanh: hip_ops.ACT["tanh"]}


def ars_deltas(seed: int, update_index: int, n_delta: int, n_params: int) -> np.ndarray:
    """delta [n_delta, n_params] float32 of update `update_index`: the statement of include/cstr_rl_hip.h in NumPy float32 (the
    launches evaluate logf / sincospif on the device: the two agree to a few units in the last place)."""
    from core.common.vec_env.cstr_vec_env import _philox4x32_10

    f = np.float32
    nq = (n_params + 3) // 4
    k, q = np.meshgrid(np.arange(n_delta, dtype=np.uint32), np.arange(nq, dtype=np.uint32), indexing="ij")
    c = np.zeros((n_delta * nq, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = q.reshape(-1), k.reshape(-1), np.uint32(update_index & 0xFFFFFFFF), np.uint32(nv.ARS_TAG)
    w = _philox4x32_10(c, int(seed) & (2**64 - 1))
    u = ((w >> np.uint32(8)).astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    out = np.empty((n_delta * nq, 4), f)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(f(-2.0) * np.log(u[:, a]).astype(f)).astype(f)
        ang = (f(2.0) * u[:, b]).astype(np.float64) * np.pi
        out[:, a], out[:, b] = r * np.cos(ang).astype(f), r * np.sin(ang).astype(f)
    return out.reshape(n_delta, 4 * nq)[:, :n_params].copy()


class ARS(BaseAlgorithm):
    policy_aliases = {"MlpPolicy": ARSPolicy, "LinearPolicy": ARSLinearPolicy}

    def __init__(self, policy, env, n_delta: int = 8, n_top: Optional[int] = None, learning_rate=0.02, delta_std=0.05, zero_policy: bool = True,
                 alive_bonus_offset: float = 0, n_eval_episodes: int = 1, policy_kwargs: Optional[dict] = None, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, seed: Optional[int] = None, verbose: int = 0, device: Union[th.device, str] = "auto",
                 _init_setup_model: bool = True):
        if env is None:
            raise ValueError("ARS needs its environment at construction")
        if int(n_delta) < 1:
            raise ValueError(f"ARS: n_delta must be at least 1, got {n_delta}")
        if int(n_eval_episodes) < 1:
            raise ValueError(f"ARS: n_eval_episodes must be at least 1, got {n_eval_episodes}")
        if not callable(delta_std) and not float(delta_std) > 0:
            raise ValueError(f"ARS: delta_std must be positive, got {delta_std}")
        self._policy_alias = policy if isinstance(policy, str) else None
        super().__init__(policy, env, learning_rate, policy_kwargs=policy_kwargs, stats_window_size=stats_window_size,
                         tensorboard_log=tensorboard_log, verbose=verbose, device=device, support_multi_env=True, seed=seed)
        if unwrap_vec_normalize(self.env) is not None:
            raise NotImplementedError("ARS on a VecNormalize-wrapped env is not built")
        if self.world_size > 1:
            raise NotImplementedError("ARS: data-parallel training (world_size > 1) is not built")
        self.n_delta, self.pop_size = int(n_delta), 2 * int(n_delta)
        self.delta_std_schedule = get_schedule_fn(delta_std)
        self.delta_std = delta_std
        self.n_eval_episodes = int(n_eval_episodes)
        if n_top is None:
            n_top = n_delta
        if n_top > n_delta:  # sb3_contrib/ars/ars.py
            warnings.warn(f"n_top = {n_top} > n_delta = {n_delta}, setting n_top = n_delta")
            n_top = n_delta
        if int(n_top) < 1:
            raise ValueError(f"ARS: n_top must be at least 1, got {n_top}")
        self.n_top = int(n_top)
        self.alive_bonus_offset = alive_bonus_offset
        self.zero_policy = bool(zero_policy)
        self.weights: Optional[th.Tensor] = None
        self.fused_learner = False
        self.delta_seed = int(seed) if seed is not None else int(np.random.SeedSequence().entropy & (2**63 - 1))
        self.last_returns: Optional[th.Tensor] = None  # the last update's candidate returns [2 n_delta] float64, in HBM
        if _init_setup_model:
            self._setup_model()

    # ---- setup -------------------------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        self._setup_lr_schedule()
        self.set_random_seed(self.seed)
        self.policy = self.policy_class(self.observation_space, self.action_space, **self.policy_kwargs)
        self.weights = self.policy.to_device_flat(self.device)
        self.n_params = int(self.weights.numel())
        if self.zero_policy:
            self.weights.zero_()  # the modules view it
        dev, nd = self.device, self.n_delta
        with th.cuda.device(dev):
            self._returns = th.zeros(2 * nd, dtype=th.float64, device=dev)
            self._lengths = th.zeros(2 * nd, dtype=th.int32, device=dev)
            self._block = th.zeros(hip_ops.ARS_STATS_WORDS + 2, dtype=th.float64, device=dev)  # the statistics block, then {step_size, return_std}
            self._kept = th.zeros(self.n_top, dtype=th.int32, device=dev)
        self.last_returns = self._returns
        self.fused_learner = self._kernel_shapes() is not None

    def _kernel_shapes(self):
        """(hidden widths, activation code) when the two launches take this model and env, else None"""
        env, pol = self.env, self.policy
        if not isinstance(env, CSTRVecEnv) or env.goal_conditioned or env.discrete_actions is not None or env.multi_discrete_actions is not None:
            return None
        if env.device != self.device or type(pol) not in (ARSPolicy, ARSLinearPolicy):
            return None
        mods = list(pol.action_net)
        if pol.squash_output:
            if not isinstance(mods[-1], nn.Tanh):
                return None
            mods = mods[:-1]
        linears, acts = mods[0::2], mods[1::2]
        if not all(isinstance(m, nn.Linear) for m in linears) or len(acts) != len(linears) - 1:
            return None
        if any(type(m) not in _ACTS for m in acts) or len({type(m) for m in acts}) > 1:
            return None
        if any((m.bias is not None) != pol.with_bias for m in linears):
            return None
        hidden = [m.out_features for m in linears[:-1]]
        act = _ACTS[type(acts[0])] if acts else hip_ops.ACT["relu"]
        if linears[0].in_features != env.obs_dim or linears[-1].out_features != env.act_dim:
            return None
        if not hip_ops.ars_supported(env.obs_dim, env.act_dim, hidden, act, pol.with_bias, pol.squash_output, self.n_delta, self.n_top):
            return None
        return hidden, act

    def enable_graph_capture(self, enabled: bool = True) -> None:
        if enabled:
            raise NotImplementedError("ARS: hipGraph replay is not built (an update is two launches and one read: there is nothing to fold)")

    # ---- one update ----------------------------------------------------------------------------------------------------------------
    def _update_kernels(self, lr: float, delta_std: float) -> tuple:
        hidden, act = self._kernel_shapes()
        env, pol = self.env, self.policy
        if not env._has_reset:
            raise ValueError("Please call env.reset() to reset the env first!")
        low, high = np.asarray(self.action_space.low, np.float32), np.asarray(self.action_space.high, np.float32)
        stats, out = self._block[:hip_ops.ARS_STATS_WORDS], self._block[hip_ops.ARS_STATS_WORDS:]
        with th.cuda.device(self.device):
            hip_ops.ars_population(self.weights, hidden, act, pol.with_bias, pol.squash_output, delta_std, self.delta_seed, self._n_updates,
                                   self.n_delta, self.n_eval_episodes, float(self.alive_bonus_offset), env.coef, env.integrator, env.obs,
                                   env.step_count, env.pcg_state, low, high, self._returns, self._lengths, stats, static_init=env.static_init)
            hip_ops.ars_update(self.weights, self._returns, self.n_delta, self.n_top, lr, self.delta_seed, self._n_updates, out, self._kept)
            blk = self._block.cpu().numpy()  # the update's one host synchronisation
        return float(blk[4]), float(blk[5]), int(blk[0]), float(blk[1])

    def _update_published(self, lr: float, delta_std: float) -> tuple:
        """the published statements: sequential `evaluate_policy` calls, the update in torch (float64)"""
        nd, dev = self.n_delta, self.device
        deltas = th.as_tensor(ars_deltas(self.delta_seed, self._n_updates, nd, self.n_params), device=dev)
        theta = self.weights.clone()
        policy_deltas = th.tensor(delta_std, dtype=th.float32, device=dev) * deltas
        candidates = th.cat([theta + policy_deltas, theta - policy_deltas])
        returns, lengths = np.zeros(2 * nd, np.float64), np.zeros(2 * nd, np.int64)
        for c in range(2 * nd):
            self.weights.copy_(candidates[c])  # the modules view the vector
            ep_rew, ep_len = evaluate_policy(self, self.env, n_eval_episodes=self.n_eval_episodes, return_episode_rewards=True,
                                             deterministic=True, warn=False)
            returns[c] = sum(ep_rew) + self.alive_bonus_offset * sum(ep_len)
            lengths[c] = sum(ep_len)
        self.weights.copy_(theta)
        r = th.as_tensor(returns, device=dev)
        self._returns.copy_(r)
        self._lengths.copy_(th.as_tensor(lengths.astype(np.int32), device=dev))
        plus, minus = r[:nd], r[nd:]
        top = th.maximum(plus, minus)
        idx = th.sort(top, descending=True, stable=True).indices[:self.n_top]  # NaN first, ties to the lower k
        plus, minus = plus[idx], minus[idx]
        return_std = th.cat([plus, minus]).std()
        step_size = lr / (self.n_top * return_std + 1e-6)
        step = step_size * ((plus - minus) @ deltas[idx].to(th.float64))
        self.weights.copy_((theta.to(th.float64) + step).to(th.float32))
        self._kept.copy_(idx.to(th.int32))
        return float(step_size), float(return_std), int(lengths.sum()), float(returns.sum())

    def _do_one_update(self, callback=None, async_eval=None) -> bool:
        if async_eval is not None:
            raise NotImplementedError("ARS: async_eval is not built")
        lr = float(self.lr_schedule(self._current_progress_remaining))
        delta_std = float(self.delta_std_schedule(self._current_progress_remaining))
        if not delta_std > 0:
            raise ValueError(f"ARS: delta_std must be positive, got {delta_std}")
        step_size, return_std, n_steps, ret_sum = (self._update_kernels if self.fused_learner else self._update_published)(lr, delta_std)
        self.num_timesteps += n_steps
        self._n_updates += 1
        n_ep = 2 * self.n_delta * self.n_eval_episodes
        self._episode_num += n_ep
        self.logger.record("train/iterations", self._n_updates, exclude="tensorboard")
        self.logger.record("train/delta_std", delta_std)
        self.logger.record("train/learning_rate", lr)
        self.logger.record("train/step_size", step_size)
        self.logger.record("rollout/return_std", return_std)
        self.logger.record("rollout/ep_rew_mean", (ret_sum - float(self.alive_bonus_offset) * n_steps) / n_ep)
        self.logger.record("rollout/ep_len_mean", n_steps / n_ep)
        if callback is not None:
            callback.update_locals(locals())
            return bool(callback.on_step())
        return True

    def _log_and_dump(self) -> None:
        time_elapsed = max((time.time_ns() - self.start_time) / 1e9, sys.float_info.epsilon)
        fps = int((self.num_timesteps - self._num_timesteps_at_start) / time_elapsed)
        self.logger.record("time/fps", fps)
        self.logger.record("time/time_elapsed", int(time_elapsed), exclude="tensorboard")
        self.logger.record("time/total_timesteps", self.num_timesteps, exclude="tensorboard")
        self.logger.dump(step=self.num_timesteps)

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 1, tb_log_name: str = "ARS", reset_num_timesteps: bool = True,
              async_eval=None, progress_bar: bool = False):
        if async_eval is not None:
            raise NotImplementedError("ARS: async_eval is not built")
        total_steps, callback = self._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)
        callback.on_training_start(locals(), globals())
        while self.num_timesteps < total_steps:
            self._update_current_progress_remaining(self.num_timesteps, total_steps)
            go_on = self._do_one_update(callback, async_eval)
            if log_interval is not None and self._n_updates % log_interval == 0:
                self._log_and_dump()
            if not go_on:
                break
        callback.on_training_end()
        return self

    def train(self) -> None:
        raise NotImplementedError("ARS has no gradient step: learn() runs `_do_one_update`")

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        d = dict(n_delta=self.n_delta, n_top=self.n_top, zero_policy=self.zero_policy, alive_bonus_offset=self.alive_bonus_offset,
                 n_eval_episodes=self.n_eval_episodes, delta_seed=self.delta_seed, policy_alias=self._policy_alias or "MlpPolicy")
        if not callable(self.delta_std):
            d["delta_std"] = self.delta_std
        return d

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("policy_alias", "n_delta", "n_top", "learning_rate", "delta_std", "zero_policy", "alive_bonus_offset", "n_eval_episodes", "seed",
                "policy_kwargs")

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        ctor = dict(ctor)
        return cls(ctor.pop("policy_alias", "MlpPolicy"), env, device=device, **ctor)

    def _restore_extra(self, data: dict) -> None:
        if "delta_seed" in data:
            self.delta_seed = int(data["delta_seed"])
