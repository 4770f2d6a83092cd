"""QR-DQN's quantile network and policy (sb3_contrib/qrdqn/policies.py): DQN's policy whose network outputs `n_quantiles` atoms of the
return distribution per action instead of one value. The last Linear layer has n_quantiles * n_actions outputs, atom i of action a
at i * n_actions + a, so `forward` is a view [B, n_quantiles, n_actions]. Attribute names and `state_dict` keys are sb3_contrib's
(`quantile_net.quantile_net.{0,2,4}.*`, `quantile_net_target.quantile_net.{0,2,4}.*`); the construction order on the CPU generator is
network, target, copy, so a seeded model's first two Linear layers are DQNPolicy's bit for bit. Arenas, `flat_optimizers` and
`predict` are DQNPolicy's. `MlpPolicy` only: CnnPolicy / MultiInputPolicy are not built."""
from typing import Optional

import torch as th
from torch import nn

from core.common.arena import ParamArena, make_optimizer
from core.common.policies import BasePolicy
from core.common.spaces import as_discrete
from core.common.torch_layers import FlattenExtractor, create_mlp
from core.dqn.policies import DQNPolicy


class QuantileNetwork(BasePolicy):
    """Z(s, .) [B, n_quantiles, n_actions] over a Discrete action space (sb3_contrib/qrdqn/policies.py QuantileNetwork)"""

    def __init__(self, observation_space, action_space, features_extractor: nn.Module, features_dim: int, n_quantiles: int = 200,
                 net_arch: Optional[list] = None, activation_fn=nn.ReLU, normalize_images: bool = True):
        super().__init__(observation_space, action_space, features_extractor=features_extractor, normalize_images=normalize_images)
        if as_discrete(self.action_space) is None:
            raise ValueError(f"QuantileNetwork needs a Discrete action space, got {self.action_space!r}")
        if int(n_quantiles) < 1:
            raise ValueError(f"QuantileNetwork: n_quantiles must be at least 1, got {n_quantiles}")
        if net_arch is None:
            net_arch = [64, 64]
        self.net_arch, self.activation_fn, self.features_dim, self.n_quantiles = net_arch, activation_fn, features_dim, int(n_quantiles)
        self.n_actions = int(self.action_space.n)
        self.quantile_net = nn.Sequential(*create_mlp(features_dim, self.n_quantiles * self.n_actions, net_arch, activation_fn))

    def forward(self, obs: th.Tensor) -> th.Tensor:
        quantiles = self.quantile_net(self.extract_features(obs, self.features_extractor))
        return quantiles.view(-1, self.n_quantiles, self.n_actions)

    def _predict(self, observation: th.Tensor, deterministic: bool = True) -> th.Tensor:
        return self(observation).mean(dim=1).argmax(dim=1).reshape(-1)  # greedy over the mean of the atoms


class QRDQNPolicy(DQNPolicy):
    """sb3_contrib/qrdqn/policies.py QRDQNPolicy; defaults n_quantiles 200, net_arch [64, 64], ReLU, quantile_net_target a copy of
    quantile_net, one optimiser over quantile_net"""

    def __init__(self, observation_space, action_space, lr_schedule, n_quantiles: int = 200, net_arch: Optional[list] = None,
                 activation_fn=nn.ReLU, features_extractor_class=FlattenExtractor, features_extractor_kwargs: Optional[dict] = None,
                 normalize_images: bool = True, optimizer_class=th.optim.Adam, optimizer_kwargs: Optional[dict] = None):
        if int(n_quantiles) < 1:
            raise ValueError(f"QRDQN: n_quantiles must be at least 1, got {n_quantiles}")
        self.n_quantiles = int(n_quantiles)  # before DQNPolicy.__init__: it builds the modules
        super().__init__(observation_space, action_space, lr_schedule, net_arch, activation_fn, features_extractor_class,
                         features_extractor_kwargs, normalize_images, optimizer_class, optimizer_kwargs)

    def make_quantile_net(self) -> QuantileNetwork:
        fe = self.make_features_extractor()
        return QuantileNetwork(features_extractor=fe, features_dim=fe.features_dim, n_quantiles=self.n_quantiles, **self.net_args)

    def _build(self, lr_schedule) -> None:
        """Creation order of the published code: quantile_net, quantile_net_target, copy; the optimiser is made with the arenas."""
        self.quantile_net = self.make_quantile_net()
        self.quantile_net_target = self.make_quantile_net()
        self.quantile_net_target.load_state_dict(self.quantile_net.state_dict())
        self.quantile_net_target.set_training_mode(False)
        self.optimizer = None

    def to_device_arenas(self, device) -> None:
        self.arena, self.optimizer = make_optimizer(self.quantile_net.parameters(), device, self._lr_schedule(1), self.optimizer_class,
                                                    self.optimizer_kwargs)
        self.target_arena = ParamArena(self.quantile_net_target.parameters(), device, with_grad=False)
        for p in self.quantile_net_target.parameters():
            p.requires_grad_(False)

    def _predict(self, obs: th.Tensor, deterministic: bool = True) -> th.Tensor:
        greedy = getattr(self, "greedy_index", None)  # the algorithm's kernel path (folded head + cstr_dqn_act_f32)
        return self.quantile_net._predict(obs, deterministic=deterministic) if greedy is None else greedy(obs)

    def set_training_mode(self, mode: bool) -> None:
        self.quantile_net.set_training_mode(mode)
        self.training = mode


MlpPolicy = QRDQNPolicy
