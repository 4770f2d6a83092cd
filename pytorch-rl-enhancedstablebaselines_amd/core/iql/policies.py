"""IQL's policy: SAC's `SACPolicy` (actor, twin critic, target critic: same modules, same construction order, so the same seed gives
SAC's initial actor and critic weights) plus a state-value network `value_net` = Flatten -> MLP(obs_dim -> critic net_arch -> 1) with
the critic's activation and an Adam of its own. `value_net` is constructed AFTER the target critic and draws after it. Its parameters
are part of the policy's state_dict and its optimiser state travels in the archive. `MlpPolicy` only."""
import torch as th
from torch import nn

from core.common.arena import FlatAdam, make_optimizer
from core.common.policies import BaseModel
from core.common.torch_layers import create_mlp
from core.sac.policies import SACPolicy


class ValueNetwork(BaseModel):
    """V(s): one scalar-head MLP on the flattened observation"""

    def __init__(self, observation_space, action_space, net_arch: list, features_extractor: nn.Module, features_dim: int,
                 activation_fn=nn.ReLU, normalize_images: bool = True):
        super().__init__(observation_space, action_space, features_extractor=features_extractor, normalize_images=normalize_images)
        self.v_net = nn.Sequential(*create_mlp(features_dim, 1, net_arch, activation_fn))

    def forward(self, obs: th.Tensor) -> th.Tensor:
        return self.v_net(self.extract_features(obs, self.features_extractor))


class IQLPolicy(SACPolicy):
    def make_value_net(self) -> ValueNetwork:
        fe = self.make_features_extractor()
        return ValueNetwork(self.observation_space, self.action_space, self.critic_arch, fe, fe.features_dim, self.activation_fn)

    def _build(self, lr_schedule) -> None:
        super()._build(lr_schedule)  # actor, critic, critic_target: SACPolicy's order and draws
        self.value_net = self.make_value_net()
        self.value_net.optimizer = None  # created by to_device_arenas()

    def to_device_arenas(self, device) -> None:
        super().to_device_arenas(device)
        self.value_arena, self.value_net.optimizer = make_optimizer(self.value_net.parameters(), device, self._lr_schedule(1),
                                                                    self.optimizer_class, self.optimizer_kwargs)

    def flat_optimizers(self) -> list:
        return super().flat_optimizers() + [o for o in (self.value_net.optimizer,) if isinstance(o, FlatAdam)]

    def set_training_mode(self, mode: bool) -> None:
        super().set_training_mode(mode)
        self.value_net.set_training_mode(mode)


MlpPolicy = IQLPolicy
