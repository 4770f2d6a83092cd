"""C51's categorical network and policy: DQN's policy whose network outputs the logits of a softmax over `n_atoms` atoms of a fixed
support per action instead of one value. The last Linear layer has n_actions * n_atoms outputs, atom i of action a at a * n_atoms + i
(action-major: core/qrdqn's layout is the other way round), so `forward` is a view [B, n_actions, n_atoms]. The construction order on
the CPU generator is network, target, copy, as in core/qrdqn/policies.py, so a seeded model's first two Linear layers are DQNPolicy's
bit for bit. Arenas, `flat_optimizers` and `predict` are DQNPolicy's. `MlpPolicy` only."""
from typing import Optional

import torch as th
from torch import nn

from core.common.arena import ParamArena, make_optimizer
from core.common.policies import BasePolicy
from core.common.spaces import as_discrete
from core.common.torch_layers import FlattenExtractor, create_mlp
from core.dqn.policies import DQNPolicy


class CategoricalNetwork(BasePolicy):
    """the logits of Z(s, .) [B, n_actions, n_atoms] over a Discrete action space, on the support linspace(v_min, v_max, n_atoms)"""

    def __init__(self, observation_space, action_space, features_extractor: nn.Module, features_dim: int, n_atoms: int = 51,
                 v_min: float = -10.0, v_max: float = 10.0, net_arch: Optional[list] = None, activation_fn=nn.ReLU,
                 normalize_images: bool = True):
        super().__init__(observation_space, action_space, features_extractor=features_extractor, normalize_images=normalize_images)
        if as_discrete(self.action_space) is None:
            raise ValueError(f"CategoricalNetwork needs a Discrete action space, got {self.action_space!r}")
        if int(n_atoms) < 2:
            raise ValueError(f"CategoricalNetwork: n_atoms must be at least 2, got {n_atoms}")
        if net_arch is None:
            net_arch = [64, 64]
        self.net_arch, self.activation_fn, self.features_dim, self.n_atoms = net_arch, activation_fn, features_dim, int(n_atoms)
        self.v_min, self.v_max = float(v_min), float(v_max)
        self.n_actions = int(self.action_space.n)
        self.categorical_net = nn.Sequential(*create_mlp(features_dim, self.n_actions * self.n_atoms, net_arch, activation_fn))

    def forward(self, obs: th.Tensor) -> th.Tensor:
        logits = self.categorical_net(self.extract_features(obs, self.features_extractor))
        return logits.view(-1, self.n_actions, self.n_atoms)

    def expected_values(self, obs: th.Tensor) -> th.Tensor:
        """sum_i z_i softmax_i(logits) [B, n_actions]"""
        logits = self(obs)
        support = th.linspace(self.v_min, self.v_max, self.n_atoms, dtype=logits.dtype, device=logits.device)
        return (th.softmax(logits, dim=2) * support).sum(dim=2)

    def _predict(self, observation: th.Tensor, deterministic: bool = True) -> th.Tensor:
        return self.expected_values(observation).argmax(dim=1).reshape(-1)  # greedy over the expected value


class C51Policy(DQNPolicy):
    """defaults n_atoms 51, net_arch [64, 64], ReLU, categorical_net_target a copy of categorical_net, one optimiser over
    categorical_net; v_min / v_max are the algorithm's (core/c51/c51.py hands them over)"""

    def __init__(self, observation_space, action_space, lr_schedule, n_atoms: int = 51, v_min: float = -10.0, v_max: float = 10.0,
                 net_arch: Optional[list] = None, activation_fn=nn.ReLU, features_extractor_class=FlattenExtractor,
                 features_extractor_kwargs: Optional[dict] = None, normalize_images: bool = True, optimizer_class=th.optim.Adam,
                 optimizer_kwargs: Optional[dict] = None):
        if int(n_atoms) < 2:
            raise ValueError(f"C51: n_atoms must be at least 2, got {n_atoms}")
        self.n_atoms, self.v_min, self.v_max = int(n_atoms), float(v_min), float(v_max)  # before DQNPolicy.__init__: it builds the modules
        super().__init__(observation_space, action_space, lr_schedule, net_arch, activation_fn, features_extractor_class,
                         features_extractor_kwargs, normalize_images, optimizer_class, optimizer_kwargs)

    def make_categorical_net(self) -> CategoricalNetwork:
        fe = self.make_features_extractor()
        return CategoricalNetwork(features_extractor=fe, features_dim=fe.features_dim, n_atoms=self.n_atoms, v_min=self.v_min,
                                  v_max=self.v_max, **self.net_args)

    def _build(self, lr_schedule) -> None:
        """Creation order: categorical_net, categorical_net_target, copy; the optimiser is made with the arenas."""
        self.categorical_net = self.make_categorical_net()
        self.categorical_net_target = self.make_categorical_net()
        self.categorical_net_target.load_state_dict(self.categorical_net.state_dict())
        self.categorical_net_target.set_training_mode(False)
        self.optimizer = None

    def to_device_arenas(self, device) -> None:
        self.arena, self.optimizer = make_optimizer(self.categorical_net.parameters(), device, self._lr_schedule(1), self.optimizer_class,
                                                    self.optimizer_kwargs)
        self.target_arena = ParamArena(self.categorical_net_target.parameters(), device, with_grad=False)
        for p in self.categorical_net_target.parameters():
            p.requires_grad_(False)

    def _predict(self, obs: th.Tensor, deterministic: bool = True) -> th.Tensor:
        greedy = getattr(self, "greedy_index", None)  # the algorithm's kernel path (fused atom head + cstr_dqn_act_f32)
        return self.categorical_net._predict(obs, deterministic=deterministic) if greedy is None else greedy(obs)

    def set_training_mode(self, mode: bool) -> None:
        self.categorical_net.set_training_mode(mode)
        self.training = mode


MlpPolicy = C51Policy
