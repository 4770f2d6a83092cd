"""DQN's Q network and policy (reference: core/dqn/policies.py:18-214). `MlpPolicy` only: the constructor keywords, the
`state_dict` keys (`q_net.q_net.{0,2,4}.*`, `q_net_target.q_net.{0,2,4}.*`) and the construction order on the CPU generator are the
reference's, so a seeded model starts from bit-equal weights. CnnPolicy / MultiInputPolicy are not built."""
from typing import Optional

import numpy as np
import torch as th
from torch import nn

from core.common.arena import FlatAdam, ParamArena, make_optimizer
from core.common.policies import BasePolicy
from core.common.spaces import as_discrete
from core.common.torch_layers import FlattenExtractor, create_mlp


class QNetwork(BasePolicy):
    """Q(s, .) over a Discrete action space (reference: dqn/policies.py:18-85)"""

    def __init__(self, observation_space, action_space, features_extractor: nn.Module, features_dim: int, net_arch: Optional[list] = None,
                 activation_fn=nn.ReLU, normalize_images: bool = True):
        super().__init__(observation_space, action_space, features_extractor=features_extractor, normalize_images=normalize_images)
        if as_discrete(self.action_space) is None:
            raise ValueError(f"QNetwork needs a Discrete action space, got {self.action_space!r}")
        if net_arch is None:
            net_arch = [64, 64]
        self.net_arch, self.activation_fn, self.features_dim = net_arch, activation_fn, features_dim
        self.q_net = nn.Sequential(*create_mlp(features_dim, int(self.action_space.n), net_arch, activation_fn))

    def forward(self, obs: th.Tensor) -> th.Tensor:
        return self.q_net(self.extract_features(obs, self.features_extractor))

    def _predict(self, observation: th.Tensor, deterministic: bool = True) -> th.Tensor:
        return self(observation).argmax(dim=1).reshape(-1)  # greedy (:68-72)


class DQNPolicy(BasePolicy):
    """reference: dqn/policies.py:88-211; default net_arch [64, 64], ReLU, q_net_target a copy of q_net, one optimiser over q_net"""

    def __init__(self, observation_space, action_space, lr_schedule, net_arch: Optional[list] = None, activation_fn=nn.ReLU,
                 features_extractor_class=FlattenExtractor, features_extractor_kwargs: Optional[dict] = None, normalize_images: bool = True,
                 optimizer_class=th.optim.Adam, optimizer_kwargs: Optional[dict] = None):
        super().__init__(observation_space, action_space, features_extractor_class, features_extractor_kwargs,
                         optimizer_class=optimizer_class, optimizer_kwargs=optimizer_kwargs, normalize_images=normalize_images)
        if net_arch is None:
            net_arch = [64, 64]
        self.net_arch, self.activation_fn = net_arch, activation_fn
        self.net_args = dict(observation_space=self.observation_space, action_space=self.action_space, net_arch=self.net_arch,
                             activation_fn=self.activation_fn, normalize_images=normalize_images)
        self._lr_schedule = lr_schedule
        self._build(lr_schedule)

    def make_q_net(self) -> QNetwork:
        fe = self.make_features_extractor()
        return QNetwork(features_extractor=fe, features_dim=fe.features_dim, **self.net_args)

    def _build(self, lr_schedule) -> None:
        """Creation order of the reference (:153-173): q_net, q_net_target, copy; the optimiser is made with the arenas."""
        self.q_net = self.make_q_net()
        self.q_net_target = self.make_q_net()
        self.q_net_target.load_state_dict(self.q_net.state_dict())
        self.q_net_target.set_training_mode(False)
        self.optimizer = None

    def to_device_arenas(self, device) -> None:
        self.arena, self.optimizer = make_optimizer(self.q_net.parameters(), device, self._lr_schedule(1), self.optimizer_class,
                                                    self.optimizer_kwargs)
        self.target_arena = ParamArena(self.q_net_target.parameters(), device, with_grad=False)
        for p in self.q_net_target.parameters():
            p.requires_grad_(False)

    def flat_optimizers(self) -> list:
        return [self.optimizer] if isinstance(self.optimizer, FlatAdam) else []

    def forward(self, obs: th.Tensor, deterministic: bool = True) -> th.Tensor:
        return self._predict(obs, deterministic=deterministic)

    def _predict(self, obs: th.Tensor, deterministic: bool = True) -> th.Tensor:
        greedy = getattr(self, "greedy_index", None)  # the algorithm's kernel path (per-layer Linear kernels + cstr_dqn_act_f32)
        return self.q_net._predict(obs, deterministic=deterministic) if greedy is None else greedy(obs)

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """reference: policies.py:331-386 for a Discrete space -> (int64 indices [n], or a scalar array for one unvectorised
        observation; None)"""
        self.set_training_mode(False)
        obs_tensor, vectorized = self.obs_to_tensor(observation)
        with th.no_grad():
            actions = self._predict(obs_tensor, deterministic=deterministic)
        actions = actions.cpu().numpy().astype(np.int64).reshape((-1, *self.action_space.shape))
        if not vectorized:
            actions = actions.squeeze(axis=0)
        return actions, state

    def set_training_mode(self, mode: bool) -> None:
        self.q_net.set_training_mode(mode)
        self.training = mode


MlpPolicy = DQNPolicy
