"""TD3+BC (Fujimoto & Gu 2021, "A Minimalist Approach to Offline Reinforcement Learning"): TD3's gradient step (core/td3/td3.py,
reference td3.py:161-206) on batches of a fixed dataset, with a behaviour-cloning term in the actor loss

    pi = actor(s);  q = Q1(s, pi);  lam = alpha / mean|q|  (a constant: no gradient flows through it)
    actor_loss = -lam * mean(q) + mean((pi - a)^2)          (a = the dataset's action, buffer scaling)

and, by default, observations normalised with the dataset's per-column mean and std (+ 1e-3). It sits on `OfflineAlgorithm` (the
dataset forms, learn(), the hipGraph hooks) and takes everything else from `TD3`: the policy class, the critic step with target
smoothing, `noise_queue` teacher forcing and `debug_capture`, the actor's Adam step and the soft updates. `mean|q| = 0` is not
guarded, as in the published code: lam = inf and the loss is not finite.

On the fused path the actor loss is one launch (cstr_td3bc_actor_loss_f32) where TD3 launches its -mean(Q1) head, and the
behaviour-cloning gradient is added inside the backward launch of the actor's last layer (cstr_td3bc_act_bwd_rows_f32). The row-chain
kernels (core/common/chain.py) have -mean(Q1) built into their actor step and decline this class."""
from typing import List, Optional, Union

import numpy as np
import torch as th
from torch.nn import functional as F

from core.common import fused, hip_ops
from core.common.buffers import ReplayBuffer
from core.common.logger import DeviceMean
from core.common.offline_policy_algorithm import OfflineAlgorithm
from core.common.vec_env import unwrap_vec_normalize
from core.td3.td3 import TD3
from core.td3bc.policies import MlpPolicy

STD_EPS = 1e-3  # added to the per-column std of the dataset's observations (the paper's code)


def dataset_statistics(observations: th.Tensor) -> tuple:
    """(mean, std(ddof=0) + 1e-3) per column of the valid observation rows [R, D]: float64 accumulation, float32 storage."""
    o = observations.to(th.float64)
    return o.mean(dim=0).to(th.float32), (o.std(dim=0, unbiased=False) + STD_EPS).to(th.float32)


class TD3BC(TD3, OfflineAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    goal_face_support = False
    train_batch_size = 256
    chain_type = None

    def __init__(self, policy, env, learning_rate=1e-3, dataset=None, buffer_size: int = 1_000_000, batch_size: int = 256,
                 tau: float = 0.005, gamma: float = 0.99, gradient_steps: int = 1, policy_delay: int = 2,
                 target_policy_noise: float = 0.2, target_noise_clip: float = 0.5, alpha: float = 2.5, normalize_states: bool = True,
                 behavior_cloning_warmup: int = 0, n_eval_episodes: int = 10, policy_kwargs: Optional[dict] = None,
                 stats_window_size: int = 100, tensorboard_log: Optional[str] = None, verbose: int = 0,
                 device: Union[th.device, str] = "auto", seed: Optional[int] = None, _init_setup_model: bool = True, _obs_stats=None):
        if policy_kwargs and policy_kwargs.get("use_sde"):
            raise ValueError("TD3BC does not support gSDE (use_sde=True)")
        if env is not None and unwrap_vec_normalize(env) is not None:
            raise ValueError("TD3BC does not take a VecNormalize-wrapped env: the dataset's own statistics normalise its observations "
                             "(normalize_states=True)")
        if not (alpha >= 0.0):
            raise ValueError(f"TD3BC: alpha must be a non-negative number, got {alpha}")
        OfflineAlgorithm.__init__(self, policy=policy, env=env, dataset=dataset, learning_rate=learning_rate, buffer_size=buffer_size,
                                  batch_size=batch_size, tau=tau, gamma=gamma, gradient_steps=gradient_steps, dataset_buffer_class=None,
                                  dataset_buffer_kwargs=None, n_eval_episodes=n_eval_episodes,
                                  behavior_cloning_warmup=behavior_cloning_warmup, conservative_weight=0.0, policy_kwargs=policy_kwargs,
                                  stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, verbose=verbose, device=device,
                                  seed=seed)
        if self.world_size > 1:
            raise NotImplementedError("data-parallel TD3BC is not built")
        # TD3.__init__ is not run (its base-class call has the online signature): what it sets behind that call -- policy_delay,
        # target_noise_clip, target_policy_noise, debug_capture, last_train_tensors, noise_queue -- is set here and must follow it
        self.policy_delay = policy_delay
        self.target_noise_clip = target_noise_clip
        self.target_policy_noise = target_policy_noise
        self.alpha = float(alpha)
        self.normalize_states = bool(normalize_states)
        self._obs_stats = _obs_stats  # load(): the archive's statistics normalise the dataset, not ones computed again
        self.obs_mean: Optional[th.Tensor] = None
        self.obs_std: Optional[th.Tensor] = None
        self.debug_capture = False
        self.last_train_tensors: dict = {}
        self.last_actor_tensors: dict = {}  # debug_capture, actor steps: Q1(s, pi(s)), pi(s) and {lambda, -lambda mean(q), bc}
        self.noise_queue: List[th.Tensor] = []  # teacher-forcing hook for the target-smoothing noise (td3.py:169)
        if _init_setup_model:
            self._setup_model()

    # ---- dataset: the model's OWN copy, normalised once ----------------------------------------------------------------------
    def _copy_dataset_to_buffer(self, source_buffer) -> None:
        if not self.normalize_states:
            return super()._copy_dataset_to_buffer(source_buffer)
        if source_buffer is self.dataset and isinstance(source_buffer, ReplayBuffer):
            # the caller's object: `to(device)` would hand it back (or move it); normalising in place must not reach it
            st = source_buffer.__getstate__()
            st["device"] = str(self.device)
            source_buffer = type(source_buffer).__new__(type(source_buffer))
            source_buffer.__setstate__(st)
        super()._copy_dataset_to_buffer(source_buffer)
        rb = self.replay_buffer
        if self._obs_stats is not None:
            mean, std = (th.as_tensor(np.asarray(s, np.float32), device=self.device) for s in self._obs_stats)
        else:
            mean, std = dataset_statistics(rb.observations[:rb.size()].reshape(-1, rb.observations.shape[-1]))
        self.obs_mean, self.obs_std = mean.contiguous(), std.contiguous()
        if self.policy is not None:
            self.policy.obs_norm = (self.obs_mean, self.obs_std)
        with th.no_grad():
            for field in (rb.observations, rb.next_observations):
                field.sub_(self.obs_mean).div_(self.obs_std)

    def load_replay_buffer(self, path, truncate_last_traj: bool = True) -> None:
        """A normalising model's networks, `predict()` and the folded evaluation belong to its statistics: rows loaded later go through
        the dataset hook and are normalised with THOSE statistics, never put into the buffer raw."""
        if not self.normalize_states:
            return super().load_replay_buffer(path, truncate_last_traj)
        from core.common.save_util import load_from_pkl

        self._obs_stats = (self.obs_mean.cpu().numpy(), self.obs_std.cpu().numpy())
        self._copy_dataset_to_buffer(load_from_pkl(path, self.verbose))

    def _setup_model(self) -> None:
        super()._setup_model()
        self.policy.normalize_states = self.normalize_states
        self.policy.obs_norm = (self.obs_mean, self.obs_std) if self.normalize_states else None
        act_dim = int(np.prod(self.action_space.shape))
        # the kernel path: TD3's, with two critics and an action width the loss launch takes; otherwise the torch statements
        self.fused_learner = bool(self.fused_learner and len(self.critic.q_networks) == 2 and hip_ops.td3bc_supported(1, act_dim))
        # [actor | critic | lambda | -lambda mean(q) | bc]: the loss launch's aux row is the last three
        self._loss_sum_buf = th.zeros(5, dtype=th.float32, device=self.device)
        b = self._loss_sum_buf
        self._loss_sums = dict(actor=b[0:1], critic=b[1:2], **{"lambda": b[2:3]}, q_term=b[3:4], bc=b[4:5])
        self._aux_now = th.zeros(3, dtype=th.float32, device=self.device)

    def _chain_for(self, batch_size: int):
        return None  # the row-chain actor step has -mean(Q1) built in

    def _graph_eligible(self, callback) -> bool:
        return super()._graph_eligible(callback) and self._use_packed_batch()

    # ---- the actor pass ------------------------------------------------------------------------------------------------------
    def _actor_loss_torch(self, replay_data) -> th.Tensor:
        pi = self.actor(replay_data.observations)
        q = self.critic.q1_forward(replay_data.observations, pi)
        lam = self.alpha / q.abs().mean().detach()
        q_term, bc = -lam * q.mean(), F.mse_loss(pi, replay_data.actions)
        self._loss_sum_buf[2:5] += th.stack([lam, q_term.detach(), bc.detach()])
        if self.debug_capture:
            self.last_actor_tensors = dict(q_pi=q.detach().clone(), pi=pi.detach().clone(), aux=th.stack([lam, q_term.detach(), bc.detach()]))
        return q_term + bc

    def _actor_pass_fused(self, pb, rd, blk) -> th.Tensor:
        B, A = rd.actions.shape
        coef = 2.0 / (B * A)  # d mean_{b,j}((pi - a)^2) / d pi
        if pb is not None and fused.USE_FUSED_LINEAR and A > 1:
            # the action lands in x_pi = (obs | .); the backward of that layer adds the behaviour-cloning gradient where it reads the
            # action columns of the critic's input gradient
            x_pi = self._fast_actor(rd.observations, xbuf=pb.x_pi.detach(), bc=(rd.actions, coef))
            pi = pb.x_pi.detach()[:, pb.obs_dim:]
        else:
            pi = fused.bc_tap(self._fast_actor(rd.observations), rd.actions, coef)
            x_pi = th.cat([rd.observations, pi], dim=1)
        a_out, a_sum = self._loss_slot("actor")
        aux = self._loss_sum_buf[2:5] if self._single_step else self._aux_now
        q_pi = blk.td3bc_pass(x_pi, pi, rd.actions, self.alpha, a_out, a_sum, aux)
        if not self._single_step:
            self._loss_sum_buf[2:5] += self._aux_now
        if self.debug_capture:
            self.last_actor_tensors = dict(q_pi=q_pi.clone(), pi=pi.detach().clone(), aux=aux.clone())
        return a_out

    def _train_host_only(self, gradient_steps: int) -> None:
        n_actor = self._n_delayed_updates(gradient_steps, self.policy_delay)
        super()._train_host_only(gradient_steps)
        if n_actor > 0:  # read lazily, like the losses: no host synchronisation in the step
            self.logger.record("train/bc_loss", DeviceMean(self._loss_sums["bc"], n_actor))
            self.logger.record("train/lambda", DeviceMean(self._loss_sums["lambda"], n_actor))

    # ---- reference odds and ends -----------------------------------------------------------------------------------------------
    def _behavior_cloning_update(self, observations, actions) -> float:
        pass  # accepted, without effect (as BCQ)

    def _behavior_cloning_warmup(self, callback) -> None:
        pass

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "TD3BC",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return OfflineAlgorithm.learn(self, total_timesteps=total_timesteps, callback=callback, log_interval=log_interval,
                                      tb_log_name=tb_log_name, reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        d = dict(super()._extra_save_data(), alpha=self.alpha, normalize_states=self.normalize_states,
                 behavior_cloning_warmup=self.behavior_cloning_warmup, n_eval_episodes=self.n_eval_episodes)
        if self.normalize_states:
            d.update(obs_mean=self.obs_mean.cpu().numpy().astype(np.float64).tolist(), obs_std=self.obs_std.cpu().numpy().astype(np.float64).tolist())
        if isinstance(self.dataset, str):
            d["dataset"] = self.dataset  # load() without dataset= reads it again
        return d

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "buffer_size", "batch_size", "tau", "gamma", "gradient_steps", "seed", "policy_kwargs", "policy_delay",
                "target_policy_noise", "target_noise_clip", "alpha", "normalize_states", "behavior_cloning_warmup", "n_eval_episodes",
                "dataset", "obs_mean", "obs_std")

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        ctor.pop("train_freq", None)  # the base class's (1, "step") placeholder is not a constructor argument here
        mean, std = ctor.pop("obs_mean", None), ctor.pop("obs_std", None)
        if ctor.get("normalize_states", True):
            if mean is None or std is None:
                raise ValueError("TD3BC.load(): the archive says normalize_states=True and holds no statistics")
            ctor["_obs_stats"] = (mean, std)
        return super()._construct_for_load(env, device, ctor)
