"""Policy base classes and the continuous critic (reference: core/common/policies.py:39-414, :912-987)."""
import warnings
from typing import Optional

import numpy as np
import torch as th
from torch import nn

from core.common.spaces import Discrete, MultiDiscrete, as_box, as_discrete, as_multi_discrete, get_action_dim
from core.common.torch_layers import CombinedExtractor, FlattenExtractor, create_mlp


class MultiInputMixin:
    """`MultiInputPolicy` of an algorithm = its own policy class on a Dict observation space with a CombinedExtractor (reference:
    core/sac/policies.py:MultiInputPolicy, core/td3/policies.py:MultiInputPolicy). The extractor concatenates in key order and has no
    parameters, so the networks are the class's own on the flat row: `observation_space` is that row's Box, `goal_space` the Dict.
    `predict()` takes a dict of arrays or flat rows."""

    def __init__(self, observation_space, action_space, lr_schedule, *args, features_extractor_class=CombinedExtractor, **kwargs):
        from core.common.spaces import Box

        if not isinstance(getattr(observation_space, "spaces", None), dict):
            raise ValueError(f"MultiInputPolicy needs a Dict observation space, got {observation_space!r}")
        object.__setattr__(self, "goal_space", observation_space)
        low = np.concatenate([np.asarray(s.low, np.float32).reshape(-1) for s in observation_space.spaces.values()])
        high = np.concatenate([np.asarray(s.high, np.float32).reshape(-1) for s in observation_space.spaces.values()])
        super().__init__(Box(low, high, dtype=np.float32), action_space, lr_schedule, *args, features_extractor_class=features_extractor_class,
                         **kwargs)

    def obs_to_tensor(self, observation) -> tuple:
        """reference: policies.py:240-277, Dict branch: the sub-arrays become one flat row per observation, in key order"""
        if isinstance(observation, dict):
            keys = list(self.goal_space.spaces.keys())
            vectorized = np.ndim(observation[keys[-1]]) == len(self.goal_space.spaces[keys[-1]].shape) + 1
            parts = [np.asarray(observation[k].cpu() if isinstance(observation[k], th.Tensor) else observation[k], dtype=np.float32) for k in keys]
            parts = [p.reshape(-1, int(np.prod(self.goal_space.spaces[k].shape))) for p, k in zip(parts, keys)]
            return th.as_tensor(np.concatenate(parts, axis=1), device=self.device), vectorized
        return super().obs_to_tensor(observation)


class BaseModel(nn.Module):
    """reference: core/common/policies.py:39-277"""

    optimizer = None

    def __init__(self, observation_space, action_space, features_extractor_class=FlattenExtractor,
                 features_extractor_kwargs: Optional[dict] = None, features_extractor: Optional[nn.Module] = None,
                 normalize_images: bool = True, optimizer_class=th.optim.Adam, optimizer_kwargs: Optional[dict] = None):
        super().__init__()
        self.observation_space = as_box(observation_space)
        self.action_space = as_discrete(action_space) or as_multi_discrete(action_space) or as_box(action_space)  # the valve faces
        self.features_extractor = features_extractor
        self.normalize_images = normalize_images
        self.optimizer_class = optimizer_class
        self.optimizer_kwargs = optimizer_kwargs or {}
        self.features_extractor_class = features_extractor_class
        self.features_extractor_kwargs = features_extractor_kwargs or {}

    goal_space = None  # the Dict space of a MultiInputPolicy (MultiInputMixin); `observation_space` is then its flat row

    def make_features_extractor(self) -> nn.Module:
        if self.features_extractor_class is CombinedExtractor and self.goal_space is not None:
            return CombinedExtractor(self.goal_space)
        if self.features_extractor_class is not FlattenExtractor:
            raise NotImplementedError("Only FlattenExtractor and, on a Dict space, CombinedExtractor are built (CNN extractors are out of scope, SURVEY 2)")
        return FlattenExtractor(int(np.prod(self.observation_space.shape)))

    def extract_features(self, obs, features_extractor: nn.Module) -> th.Tensor:
        if isinstance(obs, dict):  # preprocess_obs, Dict branch (preprocessing.py:140-146)
            return features_extractor({k: v.float() for k, v in obs.items()})
        return features_extractor(obs.float())  # preprocess_obs, Box branch (preprocessing.py:118-121)

    @property
    def device(self) -> th.device:
        for p in self.parameters():
            return p.device
        return th.device("cpu")

    def set_training_mode(self, mode: bool) -> None:
        self.train(mode)

    def obs_to_tensor(self, observation) -> tuple:
        """reference: policies.py:240-277 (Box branch)"""
        if isinstance(observation, th.Tensor):
            obs = observation.to(self.device, th.float32)
        else:
            obs = th.as_tensor(np.asarray(observation, dtype=np.float32), device=self.device)
        vectorized = obs.dim() == len(self.observation_space.shape) + 1
        if not vectorized:
            obs = obs.reshape((-1, *self.observation_space.shape))
        return obs, vectorized


class BasePolicy(BaseModel):
    """reference: core/common/policies.py:280-414"""

    def __init__(self, *args, squash_output: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self._squash_output = squash_output

    @property
    def squash_output(self) -> bool:
        return self._squash_output

    @staticmethod
    def _dummy_schedule(progress_remaining: float) -> float:
        return 0.0

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        raise NotImplementedError

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """reference: policies.py:331-386 -> (np.ndarray, None)"""
        self.set_training_mode(False)
        obs_tensor, vectorized = self.obs_to_tensor(observation)
        with th.no_grad():
            actions = self._predict(obs_tensor, deterministic=deterministic)
        actions = actions.cpu().numpy().reshape((-1, *self.action_space.shape))
        if as_discrete(self.action_space) is not None or isinstance(self.action_space, MultiDiscrete):
            pass  # indices: neither unscaled nor clipped (:373-381 are the Box branch)
        elif self.squash_output:
            actions = self.unscale_action(actions)
        else:
            actions = np.clip(actions, self.action_space.low, self.action_space.high)
        if not vectorized:
            actions = actions.squeeze(axis=0)
        return actions, state

    def scale_action(self, action: np.ndarray) -> np.ndarray:
        low, high = self.action_space.low, self.action_space.high
        return 2.0 * ((action - low) / (high - low)) - 1.0

    def unscale_action(self, scaled_action: np.ndarray) -> np.ndarray:
        low, high = self.action_space.low, self.action_space.high
        return low + (0.5 * (scaled_action + 1.0) * (high - low))


class ContinuousCritic(BaseModel):
    """reference: core/common/policies.py:912-987 -- n_critics independent Q networks on cat(obs, action)."""

    def __init__(self, observation_space, action_space, net_arch: list, features_extractor: nn.Module, features_dim: int,
                 activation_fn=nn.ReLU, normalize_images: bool = True, n_critics: int = 2,
                 share_features_extractor: bool = True):
        super().__init__(observation_space, action_space, features_extractor=features_extractor,
                         normalize_images=normalize_images)
        action_dim = get_action_dim(self.action_space)
        self.share_features_extractor = share_features_extractor
        self.n_critics = n_critics
        self.q_networks: list = []
        for idx in range(n_critics):
            q_net = nn.Sequential(*create_mlp(features_dim + action_dim, 1, net_arch, activation_fn))
            self.add_module(f"qf{idx}", q_net)
            self.q_networks.append(q_net)

    def forward(self, obs: th.Tensor, actions: th.Tensor) -> tuple:
        with th.set_grad_enabled(not self.share_features_extractor):
            features = self.extract_features(obs, self.features_extractor)
        qvalue_input = th.cat([features, actions], dim=1)
        return tuple(q_net(qvalue_input) for q_net in self.q_networks)

    def q1_forward(self, obs: th.Tensor, actions: th.Tensor) -> th.Tensor:
        with th.no_grad():
            features = self.extract_features(obs, self.features_extractor)
        return self.q_networks[0](th.cat([features, actions], dim=1))


class ActorCriticPolicy(BasePolicy):
    """reference: core/common/policies.py:416-771 -- policy and value networks of the on-policy algorithms, Box actions (a diagonal
    Gaussian head with a `log_std` parameter), Discrete ones (a Categorical head: `action_net` gives the logits, no `log_std`) or
    MultiDiscrete ones (`multi_discrete`: a MultiCategorical head, `action_net` gives sum(nvec) logits in th.split order) and a
    FlattenExtractor only. Built on the CPU generator in the reference's order (same seed -> the same default initial weights; the
    orthogonal initialisation goes through LAPACK's QR), then `to_device_arenas` moves EVERY parameter, `log_std` included, into one
    flat arena under one optimiser (Adam: eps = 1e-5, :468-472). `fast` (core/common/fused.py FastActorCritic): the kernel form of
    forward / evaluate / predict_values, set by the algorithm."""

    def __init__(self, observation_space, action_space, lr_schedule, net_arch=None, activation_fn=nn.Tanh, ortho_init: bool = True,
                 use_sde: bool = False, log_std_init: float = 0.0, full_std: bool = True, use_expln: bool = False,
                 squash_output: bool = False, features_extractor_class=FlattenExtractor, features_extractor_kwargs: Optional[dict] = None,
                 share_features_extractor: bool = True, normalize_images: bool = True, optimizer_class=th.optim.Adam,
                 optimizer_kwargs: Optional[dict] = None):
        from core.common.distributions import CategoricalDistribution, DiagGaussianDistribution, MultiCategoricalDistribution
        from core.common.torch_layers import MlpExtractor

        if optimizer_kwargs is None:
            optimizer_kwargs = {}
            if optimizer_class == th.optim.Adam:
                optimizer_kwargs["eps"] = 1e-5  # :470-472
        super().__init__(observation_space, action_space, features_extractor_class, features_extractor_kwargs,
                         optimizer_class=optimizer_class, optimizer_kwargs=optimizer_kwargs, squash_output=squash_output,
                         normalize_images=normalize_images)
        if use_sde:
            raise ValueError("ActorCriticPolicy does not support gSDE (use_sde=True): on-policy gSDE is not built")
        assert not squash_output, "squash_output=True is only available when using gSDE (use_sde=True)"  # :519
        if isinstance(net_arch, list) and len(net_arch) > 0 and isinstance(net_arch[0], dict):
            warnings.warn("As shared layers in the mlp_extractor are removed since SB3 v1.8.0, you should now pass directly a dictionary "
                          "and not a list (net_arch=dict(pi=..., vf=...) instead of net_arch=[dict(pi=..., vf=...)])")
            net_arch = net_arch[0]
        if net_arch is None:
            net_arch = dict(pi=[64, 64], vf=[64, 64])
        self.net_arch, self.activation_fn, self.ortho_init = net_arch, activation_fn, ortho_init
        self.share_features_extractor = share_features_extractor
        self.features_extractor = self.make_features_extractor()  # raises for anything but the FlattenExtractor
        self.features_dim = self.features_extractor.features_dim
        self.pi_features_extractor = self.vf_features_extractor = self.features_extractor  # a FlattenExtractor has no parameters
        self.log_std_init, self.use_sde, self.dist_kwargs = log_std_init, False, None
        self.discrete = isinstance(self.action_space, Discrete)  # make_proba_distribution (distributions.py:659-688)
        self.multi_discrete = isinstance(self.action_space, MultiDiscrete)  # `discrete` keeps meaning Discrete only
        if self.discrete:
            self.action_dist = CategoricalDistribution(int(self.action_space.n))
        elif self.multi_discrete:
            self.action_dist = MultiCategoricalDistribution([int(k) for k in self.action_space.nvec])
        else:
            self.action_dist = DiagGaussianDistribution(get_action_dim(self.action_space))
        self._lr_schedule = lr_schedule
        self.fast = None
        # :585-631
        self.mlp_extractor = MlpExtractor(self.features_dim, net_arch=self.net_arch, activation_fn=self.activation_fn)
        if self.discrete or self.multi_discrete:  # the logits layer; a (Multi)Categorical head has no log_std (neither parameter nor attribute)
            self.action_net = self.action_dist.proba_distribution_net(latent_dim=self.mlp_extractor.latent_dim_pi)
        else:
            self.action_net, self.log_std = self.action_dist.proba_distribution_net(latent_dim=self.mlp_extractor.latent_dim_pi,
                                                                                    log_std_init=self.log_std_init)
        self.value_net = nn.Linear(self.mlp_extractor.latent_dim_vf, 1)
        if self.ortho_init:
            for module, gain in ((self.mlp_extractor, np.sqrt(2)), (self.action_net, 0.01), (self.value_net, 1)):
                module.apply(lambda m, gain=gain: self.init_weights(m, gain=gain))
        self.optimizer = None  # to_device_arenas

    @staticmethod
    def init_weights(module: nn.Module, gain: float = 1) -> None:
        """reference: policies.py:312-320"""
        if isinstance(module, nn.Linear):
            nn.init.orthogonal_(module.weight, gain=gain)
            if module.bias is not None:
                module.bias.data.fill_(0.0)

    def to_device_arenas(self, device, flat_rmsprop: bool = False) -> None:
        """flat_rmsprop: torch.optim.RMSprop in A2C's form becomes a FlatRMSprop (arena.make_optimizer); only A2C passes True"""
        from core.common.arena import make_optimizer

        self.arena, self.optimizer = make_optimizer(self.parameters(), device, self._lr_schedule(1), self.optimizer_class, self.optimizer_kwargs,
                                                    flat_rmsprop=flat_rmsprop)

    def flat_optimizers(self) -> list:
        from core.common.arena import FlatAdam, FlatRMSprop, FlatRMSpropTFLike

        return [self.optimizer] if isinstance(self.optimizer, (FlatAdam, FlatRMSprop, FlatRMSpropTFLike)) else []

    # ---- the reference's statements on the arena parameters ----------------------------------------------------------
    def _get_action_dist_from_latent(self, latent_pi: th.Tensor):
        if self.discrete or self.multi_discrete:
            return self.action_dist.proba_distribution(action_logits=self.action_net(latent_pi))
        return self.action_dist.proba_distribution(self.action_net(latent_pi), self.log_std)

    def _fast_index(self, obs: th.Tensor, deterministic: bool, want_value: bool):
        """the kernel head on the discrete face -> (int64 indices [n], values [n, 1] or None, log_prob [n])"""
        index_f32, values, log_prob, _ = self.fast.act(obs.float().contiguous(), deterministic, want_value=want_value)
        return index_f32.reshape(-1).long(), values, log_prob

    def _fast_pairs(self, obs: th.Tensor, deterministic: bool, want_value: bool):
        """the kernel head on the MultiDiscrete face -> (int64 level pairs [n, 2], values [n, 1] or None, log_prob [n])"""
        pair_f32, values, log_prob, _ = self.fast.act(obs.float().contiguous(), deterministic, want_value=want_value)
        return pair_f32.long(), values, log_prob

    def forward(self, obs: th.Tensor, deterministic: bool = False) -> tuple:
        """:636-658 -> (actions, values [n, 1], log_prob [n])"""
        if self.fast is not None and obs.is_cuda and not th.is_grad_enabled():
            if self.discrete:
                return self._fast_index(obs, deterministic, True)
            if self.multi_discrete:
                return self._fast_pairs(obs, deterministic, True)
            return self.fast.act(obs.float().contiguous(), deterministic)[:3]
        features = self.extract_features(obs, self.features_extractor)
        latent_pi, latent_vf = self.mlp_extractor(features)
        values = self.value_net(latent_vf)
        distribution = self._get_action_dist_from_latent(latent_pi)
        actions = distribution.get_actions(deterministic=deterministic)
        log_prob = distribution.log_prob(actions)
        return actions.reshape((-1, *self.action_space.shape)), values, log_prob

    def evaluate_actions(self, obs: th.Tensor, actions: th.Tensor) -> tuple:
        """:719-741 -> (values [n, 1], log_prob [n], entropy [n])"""
        features = self.extract_features(obs, self.features_extractor)
        latent_pi, latent_vf = self.mlp_extractor(features)
        distribution = self._get_action_dist_from_latent(latent_pi)
        if self.discrete:
            actions = actions.long().flatten()  # ppo.py:208-210 / a2c.py:146-148
        elif self.multi_discrete:
            actions = actions.long().reshape(-1, len(self.action_dist.action_dims))  # Categorical.log_prob takes value.long() itself
        log_prob = distribution.log_prob(actions)
        values = self.value_net(latent_vf)
        return values, log_prob, distribution.entropy()

    def get_distribution(self, obs: th.Tensor):
        """:743-752"""
        features = self.extract_features(obs, self.pi_features_extractor)
        return self._get_action_dist_from_latent(self.mlp_extractor.forward_actor(features))

    def predict_values(self, obs: th.Tensor) -> th.Tensor:
        """:754-763 -> [n, 1]"""
        if self.fast is not None and obs.is_cuda and not th.is_grad_enabled():
            return self.fast.values(obs.float().contiguous()).reshape(-1, 1)
        features = self.extract_features(obs, self.vf_features_extractor)
        return self.value_net(self.mlp_extractor.forward_critic(features))

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        """:709-717"""
        if self.fast is not None and observation.is_cuda and not th.is_grad_enabled():
            if self.discrete:
                return self._fast_index(observation, deterministic, False)[0]
            if self.multi_discrete:
                return self._fast_pairs(observation, deterministic, False)[0]
            return self.fast.act(observation.float().contiguous(), deterministic, want_value=False)[0]
        return self.get_distribution(observation).get_actions(deterministic=deterministic)


class MultiInputActorCriticPolicy(MultiInputMixin, ActorCriticPolicy):
    """reference: core/common/policies.py:839-910 -- ActorCriticPolicy behind a CombinedExtractor on a Dict observation space (the goal
    face of the env). The extractor has no parameters: state-dict keys, construction order and seeded initial weights are
    ActorCriticPolicy's on a features_dim = 6 input. On the device the observation already is the flat row, which passes through the
    extractor unchanged; `predict()` takes a dict of arrays or flat rows."""
