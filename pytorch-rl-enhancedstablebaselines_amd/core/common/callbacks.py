"""Callbacks of the reference (core/common/callbacks.py:30-680): the hook points and the training callbacks built on them --
`EventCallback`, `CheckpointCallback`, `EvalCallback`, `EveryNTimesteps`, `StopTrainingOnRewardThreshold`,
`StopTrainingOnMaxEpisodes`, `StopTrainingOnNoModelImprovement` -- with the reference's constructor signatures, attributes, log keys,
file names and assertion / warning texts. `ProgressBarCallback` is left out (tqdm / rich are not dependencies).

Specific to this package: `BaseCallback.calls_until_event()` / `skip_calls()`. A callback that does nothing on most calls says how many
calls away its next event is; graph replay (core/common/graph_replay.py) then replays the iterations in between and only the iteration
that contains an event runs through the eager loop, where the hook fires exactly where the reference fires it. `EvalCallback` takes one
extra keyword, `fused`, that selects `evaluate_policy_fused` (the whole evaluation in one launch).
"""
import math
import os
import warnings
from typing import Callable, Optional, Union

import numpy as np


class BaseCallback:
    def __init__(self, verbose: int = 0):
        self.model = None
        self.n_calls = 0
        self.num_timesteps = 0
        self.verbose = verbose
        self.locals: dict = {}
        self.globals: dict = {}
        self.parent = None

    @property
    def training_env(self):
        return self.model.get_env()

    @property
    def logger(self):
        return self.model.logger

    def init_callback(self, model) -> None:
        self.model = model
        self._init_callback()

    def _init_callback(self) -> None:
        pass

    def on_training_start(self, locals_: dict, globals_: dict) -> None:
        self.locals, self.globals = locals_, globals_
        self.num_timesteps = self.model.num_timesteps
        self._on_training_start()

    def _on_training_start(self) -> None:
        pass

    def on_rollout_start(self) -> None:
        self._on_rollout_start()

    def _on_rollout_start(self) -> None:
        pass

    def _on_step(self) -> bool:
        return True

    def on_step(self) -> bool:
        self.n_calls += 1
        self.num_timesteps = self.model.num_timesteps
        return self._on_step()

    def on_training_end(self) -> None:
        self._on_training_end()

    def _on_training_end(self) -> None:
        pass

    def on_rollout_end(self) -> None:
        self._on_rollout_end()

    def _on_rollout_end(self) -> None:
        pass

    def update_locals(self, locals_: dict) -> None:
        self.locals.update(locals_)
        self.update_child_locals(locals_)

    def update_child_locals(self, locals_: dict) -> None:
        pass

    # ---- this package's extension: events known in advance -----------------------------------------------------------
    def calls_until_event(self):
        """None: "I must see every step" (the default: a subclass may do anything in `_on_step`). An integer k >= 1: the next k - 1
        calls of `on_step()` do nothing but count and return True, call k is the event. math.inf: never."""
        return None

    def skip_calls(self, n: int) -> None:
        """Stand in for `n` calls of `on_step()` that `calls_until_event()` declared eventless."""
        self.n_calls += n
        self.num_timesteps = self.model.num_timesteps


class NoopCallback(BaseCallback):
    """What `callback=None` becomes; lets the loop skip `locals()` snapshots."""
    is_noop = True

    def calls_until_event(self):
        return math.inf


def _keeps_own_step(cb, cls) -> bool:
    """The class's event schedule only describes the class's own `_on_step`: a subclass that overrides it may work on every call."""
    return type(cb)._on_step is cls._on_step


class EventCallback(BaseCallback):
    """A callback with one child that is called when this callback's event happens (reference: callbacks.py:146-187). The child
    shares the model, learns about the start of training and sees the rollout's locals; `_on_event()` is its `on_step()`."""

    def __init__(self, callback: Optional[BaseCallback] = None, verbose: int = 0):
        super().__init__(verbose=verbose)
        self.callback = callback
        if callback is not None:
            callback.parent = self

    def init_callback(self, model) -> None:
        super().init_callback(model)
        child = self.callback
        if child is not None:
            child.init_callback(model)

    def _on_training_start(self) -> None:
        child = self.callback
        if child is not None:
            child.on_training_start(self.locals, self.globals)

    def _on_event(self) -> bool:
        return True if self.callback is None else self.callback.on_step()

    def _on_step(self) -> bool:
        return True

    def update_child_locals(self, locals_: dict) -> None:
        child = self.callback
        if child is not None:
            child.update_locals(locals_)


class CallbackList(BaseCallback):
    def __init__(self, callbacks: list):
        super().__init__()
        assert isinstance(callbacks, list)
        self.callbacks = callbacks

    def calls_until_event(self):
        """The nearest event of any child; None as soon as one child has to see every step."""
        nearest = math.inf
        for cb in self.callbacks:
            k = cb.calls_until_event()
            if k is None:
                return None
            nearest = min(nearest, k)
        return nearest

    def skip_calls(self, n: int) -> None:
        super().skip_calls(n)
        for cb in self.callbacks:
            cb.skip_calls(n)

    def _init_callback(self) -> None:
        for cb in self.callbacks:
            cb.init_callback(self.model)
            cb.parent = self.parent

    def _on_training_start(self) -> None:
        for cb in self.callbacks:
            cb.on_training_start(self.locals, self.globals)

    def _on_rollout_start(self) -> None:
        for cb in self.callbacks:
            cb.on_rollout_start()

    def _on_step(self) -> bool:
        cont = True
        for cb in self.callbacks:
            cont = cb.on_step() and cont
        return cont

    def _on_rollout_end(self) -> None:
        for cb in self.callbacks:
            cb.on_rollout_end()

    def _on_training_end(self) -> None:
        for cb in self.callbacks:
            cb.on_training_end()

    def update_child_locals(self, locals_: dict) -> None:
        for cb in self.callbacks:
            cb.update_locals(locals_)


class ConvertCallback(BaseCallback):
    def __init__(self, callback: Optional[Callable[[dict, dict], bool]], verbose: int = 0):
        super().__init__(verbose)
        self.callback = callback

    def _on_step(self) -> bool:
        if self.callback is not None:
            return self.callback(self.locals, self.globals)
        return True


class CheckpointCallback(BaseCallback):
    """Every `save_freq`-th call of `on_step()` writes `{name_prefix}_{num_timesteps}_steps.zip` into `save_path`; on request also
    the replay buffer (`{name_prefix}_replay_buffer_{n}_steps.pkl`, algorithms that have one) and the `VecNormalize` statistics
    (`{name_prefix}_vecnormalize_{n}_steps.pkl`, when the training env is wrapped). A call is `n_envs` timesteps (reference:
    callbacks.py:244-320)."""

    def __init__(self, save_freq: int, save_path: str, name_prefix: str = "rl_model", save_replay_buffer: bool = False,
                 save_vecnormalize: bool = False, verbose: int = 0):
        super().__init__(verbose)
        self.save_freq, self.save_path, self.name_prefix = save_freq, save_path, name_prefix
        self.save_replay_buffer, self.save_vecnormalize = save_replay_buffer, save_vecnormalize

    def _init_callback(self) -> None:
        if self.save_path is not None:
            os.makedirs(self.save_path, exist_ok=True)

    def _checkpoint_path(self, checkpoint_type: str = "", extension: str = "") -> str:
        """`checkpoint_type`: "" (model), "replay_buffer_" or "vecnormalize_"; the file is named after the current timestep"""
        stem = "_".join((self.name_prefix, f"{checkpoint_type}{self.num_timesteps}", "steps"))
        return os.path.join(self.save_path, stem + "." + extension)

    def calls_until_event(self):
        if not _keeps_own_step(self, CheckpointCallback):
            return None
        return self.save_freq - self.n_calls % self.save_freq

    def _artifacts(self):
        """(what, file, writer) of everything a checkpoint consists of for this model"""
        model = self.model
        yield "model", self._checkpoint_path(extension="zip"), model.save
        if self.save_replay_buffer and getattr(model, "replay_buffer", None) is not None:
            yield "replay buffer", self._checkpoint_path("replay_buffer_", "pkl"), model.save_replay_buffer
        vec_normalize = model.get_vec_normalize_env() if self.save_vecnormalize else None
        if vec_normalize is not None:
            yield "VecNormalize statistics", self._checkpoint_path("vecnormalize_", "pkl"), vec_normalize.save

    def _on_step(self) -> bool:
        if self.n_calls % self.save_freq:
            return True
        for what, file, write in self._artifacts():
            write(file)
            if self.verbose >= 2:
                print(f"checkpoint at {self.num_timesteps} timesteps: {what} -> {file}")
        return True


def sync_envs_normalization(env, eval_env) -> None:
    """Give the evaluation env's `VecNormalize` the running statistics of the training env's (reference:
    core/common/vec_env/__init__.py:sync_envs_normalization): obs_rms and ret_rms, i.e. the whole statistics block. Only the
    outermost wrapper is looked at (this package has no other wrapper). Two bare envs have nothing to synchronise and nothing
    happens; a wrapper on one side only, or wrappers over different observation widths, is an AttributeError, which `EvalCallback`
    reports with the reference's text."""
    from core.common.vec_env import VecNormalize

    wrapped = [isinstance(e, VecNormalize) for e in (env, eval_env)]
    if wrapped[0] != wrapped[1]:
        raise AttributeError("only one of the two envs is wrapped in VecNormalize")
    if not wrapped[0]:
        return
    if tuple(env.observation_space.shape) != tuple(eval_env.observation_space.shape):
        raise AttributeError(f"VecNormalize over observations {tuple(env.observation_space.shape)} and {tuple(eval_env.observation_space.shape)}")
    eval_env._state.copy_(env._state)


class EvalCallback(EventCallback):
    """Every `eval_freq`-th call of `on_step()`: evaluate the model on `eval_env` for `n_eval_episodes` episodes, log
    `eval/mean_reward`, `eval/mean_ep_length` and `time/total_timesteps`, append to `{log_path}/evaluations.npz` (`timesteps`,
    `results`, `ep_lengths`, and `successes` when an env reports `is_success`), save `{best_model_save_path}/best_model.zip` on a new
    best mean reward and call `callback_on_new_best`; `callback_after_eval` runs after every evaluation. Either child can end
    training (reference: callbacks.py:341-540).

    `fused` (specific to this package): None = `evaluate_policy_fused` (the whole evaluation in one launch) where
    `core.common.evaluation.supported` says it applies (the Box faces, and HER models on the goal face), else `evaluate_policy`;
    False = always `evaluate_policy`; True = raise if unsupported."""

    def __init__(self, eval_env, callback_on_new_best: Optional[BaseCallback] = None, callback_after_eval: Optional[BaseCallback] = None,
                 n_eval_episodes: int = 5, eval_freq: int = 10000, log_path: Optional[str] = None,
                 best_model_save_path: Optional[str] = None, deterministic: bool = True, render: bool = False, verbose: int = 1,
                 warn: bool = True, fused: Optional[bool] = None):
        from core.common.vec_env import DummyVecEnv, VecEnv

        super().__init__(callback_after_eval, verbose=verbose)
        if callback_on_new_best is not None:
            callback_on_new_best.parent = self
        self.callback_on_new_best = callback_on_new_best
        self.n_eval_episodes, self.eval_freq = n_eval_episodes, eval_freq
        self.deterministic, self.render, self.warn, self.fused = deterministic, render, warn, fused
        self.best_mean_reward = self.last_mean_reward = -np.inf
        self.eval_env = eval_env if isinstance(eval_env, VecEnv) else DummyVecEnv([lambda: eval_env])  # a single env: one-env VecEnv
        self.best_model_save_path = best_model_save_path
        self.log_path = None if log_path is None else os.path.join(log_path, "evaluations")  # np.savez adds ".npz"
        self.evaluations_timesteps: list = []
        self.evaluations_results: list = []
        self.evaluations_length: list = []
        self.evaluations_successes: list = []
        self._is_success_buffer: list = []

    def _init_callback(self) -> None:
        if not isinstance(self.training_env, type(self.eval_env)):
            warnings.warn(f"Training and eval env are not of the same type{self.training_env} != {self.eval_env}")
        for folder in (self.best_model_save_path, None if self.log_path is None else os.path.dirname(self.log_path)):
            if folder is not None:
                os.makedirs(folder, exist_ok=True)
        if self.callback_on_new_best is not None:
            self.callback_on_new_best.init_callback(self.model)

    def _log_success_callback(self, locals_: dict, globals_: dict) -> None:
        """`evaluate_policy`'s per-(step, env) hook on the host loop: remember `info["is_success"]` of every episode that ends"""
        if not locals_["done"]:
            return
        flag = locals_["info"].get("is_success")
        if flag is not None:
            self._is_success_buffer.append(flag)

    def calls_until_event(self):
        if not _keeps_own_step(self, EvalCallback):
            return None
        if self.eval_freq <= 0:
            return math.inf
        return self.eval_freq - self.n_calls % self.eval_freq

    def _evaluate(self):
        """(episode returns, episode lengths) of one evaluation, through the launch or the loop as `fused` says"""
        from core.common import evaluation

        common = dict(n_eval_episodes=self.n_eval_episodes, deterministic=self.deterministic, return_episode_rewards=True, warn=self.warn)
        launch = self.fused
        if launch is None:
            launch = evaluation.FUSED_BY_DEFAULT and not self.render and evaluation.supported(self.model, self.eval_env, self.deterministic)
        if launch:
            if self.render:
                raise ValueError("EvalCallback(fused=True): evaluate_policy_fused does not render")
            return evaluation.evaluate_policy_fused(self.model, self.eval_env, **common)
        # `is_success` needs `info` per (step, env), which only the host loop has; no device env of this package reports it, so a
        # device env keeps the device loop (whose results are the host loop's, see evaluation.py)
        hook = None if hasattr(self.eval_env, "step_device") else self._log_success_callback
        return evaluation.evaluate_policy(self.model, self.eval_env, render=self.render, callback=hook, **common)

    def _match_normalization(self) -> None:
        if self.model.get_vec_normalize_env() is None:
            return
        try:
            sync_envs_normalization(self.training_env, self.eval_env)
        except AttributeError as e:
            raise AssertionError(
                "Training and eval env are not wrapped the same way, "
                "see https://stable-baselines3.readthedocs.io/en/master/guide/callbacks.html#evalcallback "
                "and warning above."
            ) from e

    def _append_to_log(self, returns: list, lengths: list) -> None:
        assert isinstance(returns, list) and isinstance(lengths, list)
        self.evaluations_timesteps.append(self.num_timesteps)
        self.evaluations_results.append(returns)
        self.evaluations_length.append(lengths)
        arrays = dict(timesteps=self.evaluations_timesteps, results=self.evaluations_results, ep_lengths=self.evaluations_length)
        if self._is_success_buffer:
            self.evaluations_successes.append(self._is_success_buffer)
            arrays["successes"] = self.evaluations_successes
        np.savez(self.log_path, **arrays)

    def _report(self, returns: list, lengths: list) -> float:
        """Logger records of one evaluation, dumped at once so that they carry the evaluation's own timestep; returns the mean"""
        mean_reward, mean_length = float(np.mean(returns)), np.mean(lengths)
        log = self.logger
        log.record("eval/mean_reward", mean_reward)
        log.record("eval/mean_ep_length", mean_length)
        if self._is_success_buffer:
            log.record("eval/success_rate", np.mean(self._is_success_buffer))
        log.record("time/total_timesteps", self.num_timesteps, exclude="tensorboard")
        log.dump(self.num_timesteps)
        if self.verbose >= 1:
            text = (f"evaluation at {self.num_timesteps} timesteps: return {mean_reward:.2f} (std {np.std(returns):.2f}), "
                    f"episode length {mean_length:.2f} (std {np.std(lengths):.2f})")
            if self._is_success_buffer:
                text += f", success rate {100 * np.mean(self._is_success_buffer):.2f}%"
            print(text)
        return mean_reward

    def _on_step(self) -> bool:
        if self.eval_freq <= 0 or self.n_calls % self.eval_freq:
            return True
        self._match_normalization()
        self._is_success_buffer = []
        returns, lengths = self._evaluate()
        if self.log_path is not None:
            self._append_to_log(returns, lengths)
        self.last_mean_reward = self._report(returns, lengths)
        go_on = True
        if self.last_mean_reward > self.best_mean_reward:
            self.best_mean_reward = self.last_mean_reward
            if self.verbose >= 1:
                print(f"best mean return so far: {self.best_mean_reward:.2f}")
            if self.best_model_save_path is not None:
                self.model.save(os.path.join(self.best_model_save_path, "best_model"))
            if self.callback_on_new_best is not None:
                go_on = self.callback_on_new_best.on_step()
        if self.callback is not None:  # evaluated only while training still goes on, as `a and b()` does
            go_on = go_on and self._on_event()
        return go_on

    def update_child_locals(self, locals_: dict) -> None:
        if self.callback:
            self.callback.update_locals(locals_)


class StopTrainingOnRewardThreshold(BaseCallback):
    """A child of `EvalCallback` (usually its `callback_on_new_best`): training goes on only while the parent's best mean reward is
    below `reward_threshold` (reference: callbacks.py:543-570)."""

    def __init__(self, reward_threshold: float, verbose: int = 0):
        super().__init__(verbose=verbose)
        self.reward_threshold = reward_threshold

    def _on_step(self) -> bool:
        assert self.parent is not None, "``StopTrainingOnMinimumReward`` callback must be used with an ``EvalCallback``"
        best = self.parent.best_mean_reward
        reached = not bool(best < self.reward_threshold)
        if reached and self.verbose >= 1:
            print(f"mean reward {best:.2f} has reached the threshold {self.reward_threshold}: training stops")
        return not reached


class EveryNTimesteps(EventCallback):
    """Calls `callback` whenever at least `n_steps` timesteps have passed since it was last called (reference:
    callbacks.py:573-591)."""

    def __init__(self, n_steps: int, callback: BaseCallback):
        super().__init__(callback)
        self.n_steps = n_steps
        self.last_time_trigger = 0

    def calls_until_event(self):
        """A call adds the training env's `num_envs` timesteps: the first call at which `num_timesteps - last_time_trigger` reaches
        `n_steps`, counted from the model's current `num_timesteps`."""
        if not _keeps_own_step(self, EveryNTimesteps):
            return None
        per_call = max(int(self.training_env.num_envs), 1)
        missing = self.n_steps - (self.model.num_timesteps - self.last_time_trigger)
        return max(-(-missing // per_call), 1)

    def _on_step(self) -> bool:
        if self.num_timesteps - self.last_time_trigger < self.n_steps:
            return True
        self.last_time_trigger = self.num_timesteps
        return self._on_event()


class StopTrainingOnMaxEpisodes(BaseCallback):
    """Ends training once `max_episodes` episodes per training env, `max_episodes * n_envs` in total, have finished (reference:
    callbacks.py:594-635). The episodes are counted from `locals["dones"]`, a NumPy array on the host path and a float tensor in HBM
    on the device rollout path."""

    def __init__(self, max_episodes: int, verbose: int = 0):
        super().__init__(verbose=verbose)
        self.max_episodes = max_episodes
        self._total_max_episodes = max_episodes  # for one env; `_init_callback` knows how many there are
        self.n_episodes = 0

    def _init_callback(self) -> None:
        self._total_max_episodes = self.max_episodes * self.training_env.num_envs

    @staticmethod
    def _finished(dones) -> int:
        if hasattr(dones, "is_cuda"):  # torch tensor
            return int((dones != 0).sum().item())
        return int(np.count_nonzero(dones))

    def _on_step(self) -> bool:
        assert "dones" in self.locals, "`dones` variable is not defined, please check your code next to `callback.on_step()`"
        self.n_episodes += self._finished(self.locals["dones"])
        if self.n_episodes < self._total_max_episodes:
            return True
        if self.verbose >= 1:
            n_envs = self.training_env.num_envs
            print(f"{self.n_episodes} episodes played on {n_envs} env(s) after {self.num_timesteps} timesteps "
                  f"({self.n_episodes / n_envs:.2f} per env, max_episodes={self.max_episodes}): training stops")
        return False


class StopTrainingOnNoModelImprovement(BaseCallback):
    """A child of `EvalCallback` (its `callback_after_eval`): ends training after more than `max_no_improvement_evals` evaluations in
    a row without a new best mean reward; the first `min_evals` evaluations are not counted (reference: callbacks.py:638-680)."""

    def __init__(self, max_no_improvement_evals: int, min_evals: int = 0, verbose: int = 0):
        super().__init__(verbose=verbose)
        self.max_no_improvement_evals, self.min_evals = max_no_improvement_evals, min_evals
        self.last_best_mean_reward = -np.inf
        self.no_improvement_evals = 0

    def _on_step(self) -> bool:
        assert self.parent is not None, "``StopTrainingOnNoModelImprovement`` callback must be used with an ``EvalCallback``"
        best, previous = self.parent.best_mean_reward, self.last_best_mean_reward
        self.last_best_mean_reward = best
        if self.n_calls <= self.min_evals:
            return True
        self.no_improvement_evals = 0 if best > previous else self.no_improvement_evals + 1
        stop = self.no_improvement_evals > self.max_no_improvement_evals
        if stop and self.verbose >= 1:
            print(f"no new best model in {self.no_improvement_evals} consecutive evaluations: training stops")
        return not stop


MaybeCallback = Union[None, Callable, list, BaseCallback]


def to_callback(callback: MaybeCallback) -> BaseCallback:
    """reference: core/common/base_class.py:382-404"""
    if callback is None:
        return NoopCallback()
    if isinstance(callback, list):
        return CallbackList(callback)
    if not isinstance(callback, BaseCallback):
        return ConvertCallback(callback)
    return callback
