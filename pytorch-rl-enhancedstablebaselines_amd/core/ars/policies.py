"""ARS policies (sb3_contrib/ars/policies.py): a deterministic `action_net` on the flattened observation. `ARSPolicy` defaults to
net_arch [64, 64] with ReLU and biases; `ARSLinearPolicy` (alias "LinearPolicy") is the same class with net_arch [] and no bias, i.e.
the gain matrix u = K x that Mania, Guy & Recht train. With `squash_output` a Tanh follows the last layer and `predict()` un-scales
its output to [low, high]; without it `predict()` clips. State-dict keys are sb3_contrib's (`action_net.{0,2,4}.*`).

`to_device_flat` moves the parameters into ONE flat float32 device tensor without padding, in `parameters()` order, which the modules
then view (as the arenas of the gradient methods do): that tensor is `ARS.weights` and the `theta` operand of the two ARS launches, so
nothing is copied between "the vector" and "the modules"."""
from typing import Optional

import torch as th
from torch import nn

from core.common.policies import BasePolicy
from core.common.torch_layers import create_mlp


class ARSPolicy(BasePolicy):
    def __init__(self, observation_space, action_space, net_arch: Optional[list] = None, activation_fn=nn.ReLU, with_bias: bool = True,
                 squash_output: bool = True):
        super().__init__(observation_space, action_space, squash_output=bool(squash_output))
        if not hasattr(self.action_space, "low"):
            raise ValueError(f"ARSPolicy is built for Box action spaces, got {action_space!r}")
        if net_arch is None:
            net_arch = [64, 64]
        self.net_arch, self.activation_fn, self.with_bias = list(net_arch), activation_fn, bool(with_bias)
        self.features_extractor = self.make_features_extractor()
        self.features_dim = self.features_extractor.features_dim
        action_dim = int(self.action_space.shape[0])
        self.action_net = nn.Sequential(*create_mlp(self.features_dim, action_dim, self.net_arch, activation_fn, with_bias=self.with_bias,
                                                    squash_output=self.squash_output))
        self.flat: Optional[th.Tensor] = None

    def to_device_flat(self, device) -> th.Tensor:
        params = list(self.parameters())
        flat = th.zeros(sum(p.numel() for p in params), dtype=th.float32, device=device)
        off = 0
        with th.no_grad():
            for p in params:
                view = flat[off:off + p.numel()].view(p.shape)
                view.copy_(p.detach().to(device, th.float32))
                p.data = view
                p.requires_grad_(False)  # no gradient method touches these
                off += p.numel()
        self.flat = flat
        return flat

    def forward(self, obs: th.Tensor) -> th.Tensor:
        return self.action_net(self.extract_features(obs, self.features_extractor))

    def _predict(self, observation: th.Tensor, deterministic: bool = True) -> th.Tensor:
        return self(observation)  # deterministic either way


class ARSLinearPolicy(ARSPolicy):
    def __init__(self, observation_space, action_space, with_bias: bool = False, squash_output: bool = True):
        super().__init__(observation_space, action_space, net_arch=[], with_bias=with_bias, squash_output=squash_output)


MlpPolicy = ARSPolicy
LinearPolicy = ARSLinearPolicy
