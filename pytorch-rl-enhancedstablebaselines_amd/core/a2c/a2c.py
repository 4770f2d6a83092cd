"""A2C with the reference's constructor, `train()` arithmetic and logger keys (reference: core/a2c/a2c.py:16-208) on the HIP path.

One gradient step per rollout over the WHOLE buffer. On the kernel path the buffer is evaluated in place: its [T][N][.] field arrays
are B = T * N contiguous rows in storage order, so there is no permutation upload and no gather launch -- the reference's row order
(`rollout_buffer.get(None)`: one permutation of the env-major rows) only reorders the terms of the batch means and of the
weight-gradient sums. The launches of a step: policy forward, value forward, ONE launch for everything between `evaluate_actions` and
`loss.backward()` (:150-171, hip_ops.a2c_loss: the four scalars and d loss / d (action mean, value, log_std)), the backward with one
deferred weight-gradient launch, and `FlatRMSprop.step(max_norm=...)`, which folds clip_grad_norm_ into the optimiser's two launches.
`use_rms_prop=False` runs the same path with FlatAdam (eps 1e-5) behind hip_ops.grad_clip. Nothing synchronises with the host.
`policy_kwargs=dict(optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5))` (core.common.sb2_compat.rmsprop_tf_like, the
original A2C's optimiser) takes the same path and the same number of launches through `FlatRMSpropTFLike.step(max_norm=...)`, in all
its forms (weight decay, momentum, centred).
Another optimiser class, or widths the kernels decline, run the reference's own torch statements on the arena parameters
(`fused_learner` False, `rollout_buffer.get(None)` included); they are also the tests' reference.

NumPy's stream: the reference draws one `permutation(T * N)` per train() from the process-global legacy stream. Where the buffer
draws from that global stream (a VecEnv that is not device-resident) the in-place path still consumes the draw, so the stream's
position matches the reference's; with the algorithm's own `RandomState` (a device env) nothing else reads it and the draw is skipped.

On a Discrete valve face the policy has a Categorical head and the loss launch is hip_ops.categorical_loss (csrc/cstr_categorical.hip);
on a MultiDiscrete one (`CSTRVecEnv(multi_discrete_actions=(K0, K1))`) a MultiCategorical head, one categorical per valve, and the loss
launch is hip_ops.multicategorical_loss (csrc/cstr_multicategorical.hip).

On the goal face (`CSTRVecEnv(goal_conditioned=True)`, "MultiInputPolicy") the observation is the env's flat row [achieved_goal |
desired_goal | observation]: a MultiInputActorCriticPolicy (first layers at K = 6) and a DictRolloutBuffer, whose add and gather launches
are the Box face's kernels instantiated on the 6-float row; the head, GAE, loss, clip and optimiser launches are the Box face's own.

Not built: gSDE, hipGraph replay, data-parallel training, VecNormalize, MultiBinary actions, CNN policies, Dict observation spaces other
than the goal face, the goal face combined with a discrete valve face."""
from typing import Optional, Union

import numpy as np
import torch as th
from torch.nn import functional as F

from core.a2c.policies import MlpPolicy, MultiInputPolicy
from core.common import fused, hip_ops
from core.common.arena import FlatRMSprop, FlatRMSpropTFLike
from core.common.buffers import RolloutBuffer
from core.common.logger import DeviceMean
from core.common.on_policy_algorithm import OnPolicyAlgorithm
from core.common.spaces import Discrete, MultiDiscrete


class A2C(OnPolicyAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy, "MultiInputPolicy": MultiInputPolicy}
    flat_rmsprop = True  # torch.optim.RMSprop in the form below becomes arena.FlatRMSprop, RMSpropTFLike arena.FlatRMSpropTFLike

    def __init__(self, policy, env, learning_rate=7e-4, n_steps: int = 5, gamma: float = 0.99, gae_lambda: float = 1.0,
                 ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm: float = 0.5, rms_prop_eps: float = 1e-5,
                 use_rms_prop: bool = True, use_sde: bool = False, sde_sample_freq: int = -1, rollout_buffer_class=None,
                 rollout_buffer_kwargs: Optional[dict] = None, normalize_advantage: bool = False, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device: Union[th.device, str] = "auto", _init_setup_model: bool = True):
        self._policy_kwargs_arg = dict(policy_kwargs or {})  # what save() stores: the rewrite below is redone by the constructor
        super().__init__(policy, env, learning_rate=learning_rate, n_steps=n_steps, gamma=gamma, gae_lambda=gae_lambda, ent_coef=ent_coef,
                         vf_coef=vf_coef, max_grad_norm=max_grad_norm, use_sde=use_sde, sde_sample_freq=sde_sample_freq,
                         rollout_buffer_class=rollout_buffer_class, rollout_buffer_kwargs=rollout_buffer_kwargs,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs,
                         verbose=verbose, device=device, seed=seed, _init_setup_model=False, supported_action_spaces=("Box", Discrete, MultiDiscrete))
        self.normalize_advantage = normalize_advantage
        self.rms_prop_eps, self.use_rms_prop = rms_prop_eps, use_rms_prop
        self._rewrite_policy_kwargs(self.policy_kwargs, use_rms_prop, rms_prop_eps)
        self.debug_capture = False  # True: train() keeps per-row values / log-probs in buffer order, the scalars and the gradient norm
        self.last_train_capture: Optional[dict] = None
        if _init_setup_model:
            self._setup_model()

    @staticmethod
    def _rewrite_policy_kwargs(policy_kwargs: dict, use_rms_prop: bool, rms_prop_eps: float) -> dict:
        """:123-127: RMSprop (the original implementation) rather than Adam, unless the caller chose an optimiser class"""
        if use_rms_prop and "optimizer_class" not in policy_kwargs:
            policy_kwargs["optimizer_class"] = th.optim.RMSprop
            policy_kwargs["optimizer_kwargs"] = dict(alpha=0.99, eps=rms_prop_eps, weight_decay=0)
        return policy_kwargs

    def _setup_model(self) -> None:
        super()._setup_model()
        dev = self.device
        self._ws = hip_ops.new_ppo_workspace(dev)
        self._scalars = th.zeros(4, dtype=th.float32, device=dev)
        self._grad_norm = th.zeros(1, dtype=th.float32, device=dev)
        self._step_bufs: dict = {}

    # ---- train ----------------------------------------------------------------------------------------------------
    def _bufs(self, rows: int) -> dict:
        b = self._step_bufs.get(rows)
        if b is None:
            e = lambda *sh: th.empty(*sh, dtype=th.float32, device=self.device)  # noqa: E731
            b = self._step_bufs[rows] = dict(g_mean=e(rows, self.policy.action_net.out_features), g_value=e(rows, 1), log_prob=e(rows))
        return b

    def _rows_in_place(self, rb: RolloutBuffer):
        """The buffer's own storage as B = T * N rows (row t * N + n) -> (observations, actions, advantages, returns, order None). On the
        goal face the observations are the DictRolloutBuffer's flat rows, B contiguous 6-float rows."""
        assert rb.full, ""
        total = rb.buffer_size * rb.n_envs
        if rb.forced_permutations:
            rb.forced_permutations.pop(0)  # the teacher-forcing hook stays in step with get()
        elif rb.permutation_rng is None:
            np.random.permutation(total)  # the global stream moves as in the reference (buffers.py:483)
        return (rb.rb.observations.view(total, -1), rb.actions.view(total, -1), rb.advantages.view(total), rb.returns.view(total), None)

    @staticmethod
    def _rows_get(rb: RolloutBuffer):
        """:144, `get(batch_size=None)`: the whole buffer in one permuted minibatch -> (..., storage row of each minibatch row)"""
        rd = next(iter(rb.get(batch_size=None)))
        order = None
        idx = getattr(rb, "last_indices", None)
        if idx is not None:  # flat index i = env i // T, step i % T (swap_and_flatten) -> storage row step * N + env
            order = (idx % rb.buffer_size) * rb.n_envs + idx // rb.buffer_size
        return rd.observations, rd.actions, rd.advantages, rd.returns, order

    def _step_fused(self, obs, actions, advantages, returns):
        """evaluate_actions on the per-layer kernels, the loss launch, loss.backward() from its gradients, clip_grad_norm_ and the step"""
        fast, pol = self._fast, self.policy
        b = self._bufs(obs.shape[0])
        mean = fast.logits(obs, train_params=True) if (fast.discrete or fast.multi_discrete) else fast.mean(obs, train_params=True)
        values = fast.values(obs, train_params=True)
        if fast.discrete or fast.multi_discrete:  # a (Multi)Categorical head: g_mean holds d loss / d logits, there is no log_std
            fast.discrete_loss(hip_ops.CAT_A2C, mean.detach(), actions, values.detach(), advantages, returns, self.normalize_advantage,
                               self.ent_coef, self.vf_coef, b["g_mean"], b["g_value"], self._ws, scalars_out=self._scalars,
                               log_prob_out=b["log_prob"] if self.debug_capture else None)
        else:
            hip_ops.a2c_loss(mean.detach(), pol.log_std.detach(), actions, values.detach(), advantages, returns, self.normalize_advantage,
                             self.ent_coef, self.vf_coef, b["g_mean"], b["g_value"], pol.log_std.grad, self._ws, scalars_out=self._scalars,
                             log_prob_out=b["log_prob"] if self.debug_capture else None)
        with fused.deferred_weight_grads():
            th.autograd.backward([mean, values], [b["g_mean"], b["g_value"]])
        opt = pol.optimizer
        if isinstance(opt, (FlatRMSprop, FlatRMSpropTFLike)):
            opt.step(max_norm=self.max_grad_norm, workspace=self._ws, norm_out=self._grad_norm)
        else:
            hip_ops.grad_clip(pol.arena.grad, self.max_grad_norm, self._ws, self._grad_norm)
            opt.step()
        return values.detach(), b["log_prob"]

    def _step_torch(self, obs, actions, advantages, returns):
        """:150-179 as the reference's own torch statements on the arena parameters"""
        values, log_prob, entropy = self.policy.evaluate_actions(obs, actions)
        values = values.flatten()
        if self.normalize_advantage:
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
        policy_loss = -(advantages * log_prob).mean()
        value_loss = F.mse_loss(returns, values)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss
        self.policy.optimizer.zero_grad()
        loss.backward()
        norm = th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
        self.policy.optimizer.step()
        with th.no_grad():
            self._scalars.copy_(th.stack([policy_loss, value_loss, entropy_loss, loss]).detach())
            self._grad_norm.copy_(norm.detach().reshape(1))
        return values.detach(), log_prob.detach()

    def train(self) -> None:
        """:132-190: one gradient step over the whole rollout buffer"""
        self.policy.set_training_mode(True)
        self._update_learning_rate(self.policy.optimizer)
        rb = self.rollout_buffer
        with th.cuda.device(self.device):
            obs, actions, advantages, returns, order = self._rows_in_place(rb) if self._fused_learner else self._rows_get(rb)
            step = self._step_fused if self._fused_learner else self._step_torch
            values, log_prob = step(obs, actions, advantages, returns)
            if self.debug_capture:
                v, lp = values.reshape(-1).clone(), log_prob.reshape(-1).clone()
                if order is not None:  # back into buffer order
                    at = th.as_tensor(order, device=v.device)
                    v, lp = th.empty_like(v).index_copy_(0, at, v), th.empty_like(lp).index_copy_(0, at, lp)
                self.last_train_capture = dict(values=v, log_prob=lp, scalars=self._scalars.clone(), grad_norm=self._grad_norm.clone())
            # logs (:181-190): device scalars, read when the logger dumps
            with th.no_grad():
                scalars = self._scalars.clone()
                y_pred, y_true = rb.values.flatten(), rb.returns.flatten()
                var_y = y_true.var(unbiased=False)  # explained_variance (utils.py, np.var): NaN where var(y_true) == 0
                explained_var = th.where(var_y == 0, th.full_like(var_y, float("nan")), 1 - (y_true - y_pred).var(unbiased=False) / var_y)
                std = th.exp(self.policy.log_std.detach()).mean() if hasattr(self.policy, "log_std") else None
        self._n_updates += 1
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/explained_variance", DeviceMean(explained_var, 1))
        self.logger.record("train/entropy_loss", DeviceMean(scalars[2], 1))
        self.logger.record("train/policy_loss", DeviceMean(scalars[0], 1))
        self.logger.record("train/value_loss", DeviceMean(scalars[1], 1))
        if std is not None:  # :187-188: a Categorical head has no log_std
            self.logger.record("train/std", DeviceMean(std, 1))

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 100, tb_log_name: str = "A2C", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        return dict(n_steps=self.n_steps, gae_lambda=self.gae_lambda, ent_coef=self.ent_coef, vf_coef=self.vf_coef,
                    max_grad_norm=self.max_grad_norm, normalize_advantage=self.normalize_advantage, rms_prop_eps=self.rms_prop_eps,
                    use_rms_prop=self.use_rms_prop, policy_kwargs=self._policy_kwargs_arg)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "n_steps", "gamma", "gae_lambda", "ent_coef", "vf_coef", "max_grad_norm", "rms_prop_eps", "use_rms_prop",
                "normalize_advantage", "seed", "policy_kwargs")
