"""TQC's policy: SAC's `SACPolicy` (same actor, same construction order: actor, critic, critic target) whose critic is `n_critics`
networks create_mlp(features + action, n_quantiles, net_arch): each Q network outputs `n_quantiles` atoms of the return distribution
instead of one value. The networks are registered as `qf{i}` (state-dict keys critic.qf0.0.weight, ...) and exposed as `q_networks`
(what the arenas, the stacked views and the fused passes of SAC read) and as `quantiles_nets` (sb3_contrib's name). The parameter
arenas and `critic_stack` are SACPolicy's. `MlpPolicy` only."""
import torch as th
from torch import nn

from core.common.policies import BaseModel
from core.common.spaces import get_action_dim
from core.common.torch_layers import create_mlp
from core.sac.policies import SACPolicy


class QuantileCritic(BaseModel):
    """Z(s, a) [B, n_critics, n_quantiles]: n_critics independent quantile networks on cat(obs, action)"""

    def __init__(self, observation_space, action_space, net_arch: list, features_extractor: nn.Module, features_dim: int,
                 activation_fn=nn.ReLU, normalize_images: bool = True, n_quantiles: int = 25, n_critics: int = 2):
        super().__init__(observation_space, action_space, features_extractor=features_extractor, normalize_images=normalize_images)
        action_dim = get_action_dim(self.action_space)
        self.share_features_extractor = False
        self.n_critics, self.n_quantiles = n_critics, n_quantiles
        self.q_networks: list = []
        for idx in range(n_critics):
            qf_net = nn.Sequential(*create_mlp(features_dim + action_dim, n_quantiles, net_arch, activation_fn))
            self.add_module(f"qf{idx}", qf_net)
            self.q_networks.append(qf_net)
        self.quantiles_nets = self.q_networks
        self.quantiles_total = n_critics * n_quantiles

    def forward(self, obs: th.Tensor, actions: th.Tensor) -> th.Tensor:
        x = th.cat([self.extract_features(obs, self.features_extractor), actions], dim=1)
        return th.stack(tuple(qf(x) for qf in self.q_networks), dim=1)


class TQCPolicy(SACPolicy):
    def __init__(self, *args, n_quantiles: int = 25, n_critics: int = 2, **kwargs):
        if int(n_quantiles) < 1:
            raise ValueError(f"TQC: n_quantiles must be at least 1, got {n_quantiles}")
        if int(n_critics) < 1:
            raise ValueError(f"TQC: n_critics must be at least 1, got {n_critics}")
        if kwargs.get("use_sde"):
            raise ValueError("TQC does not support gSDE (use_sde=True)")
        self.n_quantiles = int(n_quantiles)  # before SACPolicy.__init__: it builds the modules
        super().__init__(*args, n_critics=int(n_critics), **kwargs)

    def make_critic(self) -> QuantileCritic:
        fe = self.make_features_extractor()
        return QuantileCritic(self.observation_space, self.action_space, self.critic_arch, fe, fe.features_dim, self.activation_fn,
                              n_quantiles=self.n_quantiles, n_critics=self.n_critics)


MlpPolicy = TQCPolicy
