"""MLP builders (reference: core/common/torch_layers.py:33-46, :110-183, :316-373). Module construction order
is the reference's, so `th.manual_seed(s)` yields the same initial weights (tests/golden/policy_init_kat.npz)."""
from typing import Union

import torch as th
from torch import nn


class FlattenExtractor(nn.Module):
    def __init__(self, features_dim: int):
        super().__init__()
        self.features_dim = features_dim
        self.flatten = nn.Flatten()

    def forward(self, observations: th.Tensor) -> th.Tensor:
        return self.flatten(observations)


class CombinedExtractor(nn.Module):
    """reference: core/common/torch_layers.py:266-316 for a Dict of vector sub-spaces: every key is flattened and the results are
    concatenated in key order. No parameters, so a policy built on it has the state-dict keys and seeded initial weights of the
    reference's MultiInputPolicy. The device-side observation of the goal face already is that concatenation (one flat row per env):
    a tensor passes through unchanged."""

    def __init__(self, observation_space):
        super().__init__()
        self.keys = list(observation_space.spaces.keys())
        self.extractors = nn.ModuleDict({k: nn.Flatten() for k in self.keys})
        self.features_dim = int(observation_space.flat_dim())

    def forward(self, observations) -> th.Tensor:
        if isinstance(observations, dict):
            return th.cat([self.extractors[k](observations[k]) for k in self.keys], dim=1)  # :311-316
        return observations.reshape(observations.shape[0], -1)


def create_mlp(input_dim: int, output_dim: int, net_arch: list, activation_fn=nn.ReLU, squash_output: bool = False,
               with_bias: bool = True) -> list:
    modules: list = []
    last = input_dim
    for width in net_arch:
        modules.append(nn.Linear(last, width, bias=with_bias))
        modules.append(activation_fn())
        last = width
    if output_dim > 0:
        modules.append(nn.Linear(last, output_dim, bias=with_bias))
    if squash_output:
        modules.append(nn.Tanh())
    return modules


def get_actor_critic_arch(net_arch: Union[list, dict]) -> tuple:
    if isinstance(net_arch, list):
        return net_arch, net_arch
    assert isinstance(net_arch, dict), "Error: the net_arch can only contain be a list of ints or a dict"
    assert "pi" in net_arch, "Error: no key 'pi' was provided in net_arch for the actor network"
    assert "qf" in net_arch, "Error: no key 'qf' was provided in net_arch for the critic network"
    return net_arch["pi"], net_arch["qf"]


class MlpExtractor(nn.Module):
    """reference: core/common/torch_layers.py:186-264 -- the policy and the value trunk of an actor-critic policy. Every policy layer
    is created before the first value layer (the reference's order: the same seed gives the same default initial weights)."""

    def __init__(self, feature_dim: int, net_arch: Union[list, dict], activation_fn):
        super().__init__()
        if isinstance(net_arch, dict):
            pi_dims, vf_dims = net_arch.get("pi", []), net_arch.get("vf", [])  # a missing key: a linear network
        else:
            pi_dims = vf_dims = net_arch
        policy_net = create_mlp(feature_dim, 0, list(pi_dims), activation_fn)
        value_net = create_mlp(feature_dim, 0, list(vf_dims), activation_fn)
        self.latent_dim_pi = pi_dims[-1] if len(pi_dims) else feature_dim
        self.latent_dim_vf = vf_dims[-1] if len(vf_dims) else feature_dim
        self.policy_net = nn.Sequential(*policy_net)
        self.value_net = nn.Sequential(*value_net)

    def forward(self, features: th.Tensor) -> tuple:
        return self.forward_actor(features), self.forward_critic(features)

    def forward_actor(self, features: th.Tensor) -> th.Tensor:
        return self.policy_net(features)

    def forward_critic(self, features: th.Tensor) -> th.Tensor:
        return self.value_net(features)
