"""PPO (clip version) with the reference's constructor, assertions, `train()` arithmetic and logger keys
(reference: core/ppo/ppo.py:19-318) on the HIP path.

A minibatch step on the kernel path: the gather launch (RolloutBuffer.get), the policy and value networks through the per-layer
Linear kernels, ONE launch for everything between `evaluate_actions` and `loss.backward()` (:213-264, hip_ops.ppo_loss: the six logged
scalars and d loss / d (action mean, value, log_std)), the backward with one deferred weight-gradient launch, the gradient clip over
the flat arena (its coefficient stays on the device) and the FlatAdam step. Nothing synchronises with the host unless `target_kl` is
set (the early stop needs approx_kl on the host, as in the reference). Another optimiser class, or widths the kernels decline, run
the reference's own torch statements on the arena parameters (`fused_learner` False); they are also the tests' reference.

On a Discrete valve face (`CSTRVecEnv(discrete_actions=K)`) the policy has a Categorical head: the rollout head and the loss launch
are csrc/cstr_categorical.hip's (hip_ops.categorical_act / categorical_loss), the buffer's action row is the index as one float.

On a MultiDiscrete valve face (`CSTRVecEnv(multi_discrete_actions=(K0, K1))`) it has a MultiCategorical head, one categorical per
valve over K0 + K1 logits: csrc/cstr_multicategorical.hip (hip_ops.multicategorical_act / multicategorical_loss), the buffer's action
row is the level pair as two floats.

Another optimiser class (`RMSpropTFLike` included: its flat kernel form is A2C's alone) runs as itself on the arena's parameter views.

On the goal face (`CSTRVecEnv(goal_conditioned=True)`, "MultiInputPolicy") the observation is the env's flat row [achieved_goal |
desired_goal | observation]: a MultiInputActorCriticPolicy (first layers at K = 6) and a DictRolloutBuffer, whose add and gather launches
are the Box face's kernels instantiated on the 6-float row; the head, GAE, loss, clip and optimiser launches are the Box face's own.

Not built: gSDE, hipGraph replay, data-parallel training, VecNormalize, MultiBinary actions, CNN policies, Dict observation spaces other
than the goal face, the goal face combined with a discrete valve face."""
import warnings
from typing import Optional, Union

import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.logger import DeviceMean
from core.common.on_policy_algorithm import OnPolicyAlgorithm
from core.common.spaces import Discrete, MultiDiscrete
from core.common.utils import get_schedule_fn
from core.ppo.policies import MlpPolicy, MultiInputPolicy


class PPO(OnPolicyAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy, "MultiInputPolicy": MultiInputPolicy}

    def __init__(self, policy, env, learning_rate=3e-4, n_steps: int = 2048, batch_size: int = 64, n_epochs: int = 10, gamma: float = 0.99,
                 gae_lambda: float = 0.95, clip_range=0.2, clip_range_vf=None, normalize_advantage: bool = True, ent_coef: float = 0.0,
                 vf_coef: float = 0.5, max_grad_norm: float = 0.5, use_sde: bool = False, sde_sample_freq: int = -1,
                 rollout_buffer_class=None, rollout_buffer_kwargs: Optional[dict] = None, target_kl: Optional[float] = None,
                 stats_window_size: int = 100, tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None,
                 verbose: int = 0, seed: Optional[int] = None, device: Union[th.device, str] = "auto", _init_setup_model: bool = True):
        super().__init__(policy, env, learning_rate=learning_rate, n_steps=n_steps, gamma=gamma, gae_lambda=gae_lambda, ent_coef=ent_coef,
                         vf_coef=vf_coef, max_grad_norm=max_grad_norm, use_sde=use_sde, sde_sample_freq=sde_sample_freq,
                         rollout_buffer_class=rollout_buffer_class, rollout_buffer_kwargs=rollout_buffer_kwargs,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs,
                         verbose=verbose, device=device, seed=seed, _init_setup_model=False, supported_action_spaces=("Box", Discrete, MultiDiscrete))
        self._check_batch_arguments(batch_size, self.n_steps, None if self.env is None else self.env.num_envs, normalize_advantage)
        self.batch_size = batch_size
        self.n_epochs = n_epochs
        self.clip_range = clip_range
        self.clip_range_vf = clip_range_vf
        self.normalize_advantage = normalize_advantage
        self.target_kl = target_kl
        self.debug_capture = False  # True: train() keeps every minibatch's values / log-probs / scalars / gradient norm (tests)
        self.last_train_minibatches: list = []
        if _init_setup_model:
            self._setup_model()

    @staticmethod
    def _check_batch_arguments(batch_size: int, n_steps: int, n_envs: Optional[int], normalize_advantage: bool) -> None:
        """:138-162: the sanity checks of the advantage normalisation and the truncated-minibatch warning"""
        if normalize_advantage:
            assert batch_size > 1, "`batch_size` must be greater than 1. See https://github.com/DLR-RM/stable-baselines3/issues/440"
        if n_envs is not None:
            buffer_size = n_envs * n_steps
            assert buffer_size > 1 or (not normalize_advantage), \
                f"`n_steps * n_envs` must be greater than 1. Currently n_steps={n_steps} and n_envs={n_envs}"
            untruncated_batches = buffer_size // batch_size
            if buffer_size % batch_size > 0:
                warnings.warn(f"You have specified a mini-batch size of {batch_size},"
                              f" but because the `RolloutBuffer` is of size `n_steps * n_envs = {buffer_size}`,"
                              f" after every {untruncated_batches} untruncated mini-batches,"
                              f" there will be a truncated mini-batch of size {buffer_size % batch_size}\n"
                              f"We recommend using a `batch_size` that is a factor of `n_steps * n_envs`.\n"
                              f"Info: (n_steps={n_steps} and n_envs={n_envs})")

    def _setup_model(self) -> None:
        """:173-182"""
        self._clip_range_arg, self._clip_range_vf_arg = self.clip_range, self.clip_range_vf  # what save() stores
        super()._setup_model()
        self.clip_range = get_schedule_fn(self.clip_range)
        if self.clip_range_vf is not None:
            if isinstance(self.clip_range_vf, (float, int)):
                assert self.clip_range_vf > 0, "`clip_range_vf` must be positive, pass `None` to deactivate vf clipping"
            self.clip_range_vf = get_schedule_fn(self.clip_range_vf)
        dev = self.device
        self._ws = hip_ops.new_ppo_workspace(dev)
        self._scalars = th.zeros(6, dtype=th.float32, device=dev)
        self._sums = th.zeros(max(self.n_epochs, 1), 6, dtype=th.float32, device=dev)
        self._grad_norm = th.zeros(1, dtype=th.float32, device=dev)
        self._step_bufs: dict = {}

    # ---- train ----------------------------------------------------------------------------------------------------
    def _bufs(self, rows: int) -> dict:
        b = self._step_bufs.get(rows)
        if b is None:
            e = lambda *sh: th.empty(*sh, dtype=th.float32, device=self.device)  # noqa: E731
            b = self._step_bufs[rows] = dict(g_mean=e(rows, self.policy.action_net.out_features), g_value=e(rows, 1), log_prob=e(rows))
        return b

    def _minibatch_forward_fused(self, rd, clip_range: float, clip_range_vf: Optional[float], sums: th.Tensor):
        """evaluate_actions on the per-layer kernels and the loss launch; returns what the backward needs"""
        fast, pol = self._fast, self.policy
        obs = getattr(rd, "rows", None)  # the goal face: the flat rows behind the sample's dict (DictRolloutBuffer.get)
        if obs is None:
            obs = rd.observations
        b = self._bufs(obs.shape[0])
        if fast.discrete or fast.multi_discrete:  # a (Multi)Categorical head: g_mean holds d loss / d logits, there is no log_std
            logits = fast.logits(obs, train_params=True)
            values = fast.values(obs, train_params=True)
            fast.discrete_loss(hip_ops.CAT_PPO, logits.detach(), rd.actions, values.detach(), rd.advantages, rd.returns,
                               self.normalize_advantage, self.ent_coef, self.vf_coef, b["g_mean"], b["g_value"], self._ws,
                               old_values=rd.old_values, old_log_prob=rd.old_log_prob, clip_range=clip_range, clip_range_vf=clip_range_vf,
                               scalars_out=self._scalars, scalars_sum=sums, log_prob_out=b["log_prob"] if self.debug_capture else None)
            return logits, values, b
        mean = fast.mean(obs, train_params=True)
        values = fast.values(obs, train_params=True)
        hip_ops.ppo_loss(mean.detach(), pol.log_std.detach(), rd.actions, values.detach(), rd.old_values, rd.old_log_prob, rd.advantages,
                         rd.returns, clip_range, clip_range_vf, self.normalize_advantage, self.ent_coef, self.vf_coef, b["g_mean"],
                         b["g_value"], pol.log_std.grad, self._ws, scalars_out=self._scalars, scalars_sum=sums,
                         log_prob_out=b["log_prob"] if self.debug_capture else None)
        return mean, values, b

    def _minibatch_update_fused(self, mean, values, b) -> None:
        """loss.backward() from the loss launch's gradients, clip_grad_norm_ and the optimiser step (:274-278)"""
        with fused.deferred_weight_grads():
            th.autograd.backward([mean, values], [b["g_mean"], b["g_value"]])
        hip_ops.grad_clip(self.policy.arena.grad, self.max_grad_norm, self._ws, self._grad_norm)
        self.policy.optimizer.step()

    def _minibatch_torch(self, rd, clip_range: float, clip_range_vf: Optional[float], sums: th.Tensor):
        """:213-264 as the reference's own torch statements on the arena parameters; returns (loss, approx_kl tensor, capture)"""
        values, log_prob, entropy = self.policy.evaluate_actions(rd.observations, rd.actions)
        values = values.flatten()
        advantages = rd.advantages
        if self.normalize_advantage and len(advantages) > 1:
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
        ratio = th.exp(log_prob - rd.old_log_prob)
        policy_loss_1 = advantages * ratio
        policy_loss_2 = advantages * th.clamp(ratio, 1 - clip_range, 1 + clip_range)
        policy_loss = -th.min(policy_loss_1, policy_loss_2).mean()
        clip_fraction = th.mean((th.abs(ratio - 1) > clip_range).float())
        if clip_range_vf is None:
            values_pred = values
        else:
            values_pred = rd.old_values + th.clamp(values - rd.old_values, -clip_range_vf, clip_range_vf)
        value_loss = F.mse_loss(rd.returns, values_pred)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss
        with th.no_grad():
            log_ratio = log_prob - rd.old_log_prob
            approx_kl = th.mean((th.exp(log_ratio) - 1) - log_ratio)
            self._scalars.copy_(th.stack([policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction]).detach())
            sums += self._scalars
        return loss, values.detach(), log_prob.detach()

    def train(self) -> None:
        """:184-300"""
        self.policy.set_training_mode(True)
        self._update_learning_rate(self.policy.optimizer)
        clip_range = self.clip_range(self._current_progress_remaining)
        clip_range_vf = None if self.clip_range_vf is None else self.clip_range_vf(self._current_progress_remaining)
        if self._sums.shape[0] != max(self.n_epochs, 1):
            self._sums = th.zeros(max(self.n_epochs, 1), 6, dtype=th.float32, device=self.device)
        self._sums.zero_()
        self.last_train_minibatches = []
        n_minibatches, n_last_epoch, last_epoch = 0, 0, 0
        continue_training = True
        with th.cuda.device(self.device):
            for epoch in range(self.n_epochs):
                n_last_epoch, last_epoch = 0, epoch
                sums = self._sums[epoch]
                for rd in self.rollout_buffer.get(self.batch_size):
                    if self._fused_learner:
                        mean, values, b = self._minibatch_forward_fused(rd, clip_range, clip_range_vf, sums)
                    else:
                        loss, values, log_prob = self._minibatch_torch(rd, clip_range, clip_range_vf, sums)
                    n_minibatches += 1
                    n_last_epoch += 1
                    cap = None
                    if self.debug_capture:
                        cap = dict(values=values.detach().reshape(-1).clone(), scalars=self._scalars.clone(),
                                   log_prob=(b["log_prob"] if self._fused_learner else log_prob).clone(), epoch=epoch)
                        self.last_train_minibatches.append(cap)
                    if self.target_kl is not None:
                        approx_kl_div = float(self._scalars[4])  # the one host read of a minibatch step, as in the reference (:264-267)
                        if approx_kl_div > 1.5 * self.target_kl:
                            continue_training = False
                            if self.verbose >= 1:
                                print(f"Early stopping at step {epoch} due to reaching max kl: {approx_kl_div:.2f}")
                            break
                    if self._fused_learner:
                        self._minibatch_update_fused(mean, values, b)
                    else:
                        self.policy.optimizer.zero_grad()
                        loss.backward()
                        norm = th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
                        self._grad_norm.copy_(norm.detach().reshape(1))
                        self.policy.optimizer.step()
                    if cap is not None:
                        cap["grad_norm"] = self._grad_norm.clone()
                self._n_updates += 1
                if not continue_training:
                    break
            # logs (:284-300): device scalars, read when the logger dumps
            rb = self.rollout_buffer
            with th.no_grad():
                totals = self._sums.sum(dim=0)
                kl_sum = self._sums[last_epoch, 4].clone()
                last_loss = self._scalars[3].clone()
                y_pred, y_true = rb.values.flatten(), rb.returns.flatten()
                var_y = y_true.var(unbiased=False)  # explained_variance (utils.py, np.var): NaN where var(y_true) == 0
                explained_var = th.where(var_y == 0, th.full_like(var_y, float("nan")), 1 - (y_true - y_pred).var(unbiased=False) / var_y)
                std = th.exp(self.policy.log_std.detach()).mean() if hasattr(self.policy, "log_std") else None
        count = max(n_minibatches, 1)
        self.logger.record("train/entropy_loss", DeviceMean(totals[2], count))
        self.logger.record("train/policy_gradient_loss", DeviceMean(totals[0], count))
        self.logger.record("train/value_loss", DeviceMean(totals[1], count))
        self.logger.record("train/approx_kl", DeviceMean(kl_sum, max(n_last_epoch, 1)))
        self.logger.record("train/clip_fraction", DeviceMean(totals[5], count))
        self.logger.record("train/loss", DeviceMean(last_loss, 1))
        self.logger.record("train/explained_variance", DeviceMean(explained_var, 1))
        if std is not None:  # :293-294: a Categorical head has no log_std
            self.logger.record("train/std", DeviceMean(std, 1))
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/clip_range", clip_range)
        if self.clip_range_vf is not None:
            self.logger.record("train/clip_range_vf", clip_range_vf)

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 1, tb_log_name: str = "PPO", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        d = dict(n_steps=self.n_steps, n_epochs=self.n_epochs, gae_lambda=self.gae_lambda, ent_coef=self.ent_coef, vf_coef=self.vf_coef,
                 max_grad_norm=self.max_grad_norm, normalize_advantage=self.normalize_advantage, target_kl=self.target_kl)
        for key, arg in (("clip_range", self._clip_range_arg), ("clip_range_vf", self._clip_range_vf_arg)):
            if arg is None or isinstance(arg, (float, int)):
                d[key] = arg  # a schedule is code: it is not stored, load() takes it as a keyword argument
        return d

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "clip_range_vf",
                "normalize_advantage", "ent_coef", "vf_coef", "max_grad_norm", "target_kl", "seed", "policy_kwargs")
