"""Squashed diagonal Gaussian (reference: core/common/distributions.py:125-260).

`eps_queue`: teacher-forcing hook. The reference draws eps through `Normal.rsample` on the CPU generator; a
GPU run cannot reproduce those numbers, so parity tests push the recorded eps tensors here and the next
`sample()` calls consume them instead of `randn` (SURVEY 7 "Stochastic parity")."""
import math
from typing import List, Optional

import torch as th
from torch import nn


class SquashedDiagGaussianDistribution:
    def __init__(self, action_dim: int, epsilon: float = 1e-6):
        self.action_dim = action_dim
        self.epsilon = epsilon
        self.mean: Optional[th.Tensor] = None
        self.log_std: Optional[th.Tensor] = None
        self.gaussian_actions: Optional[th.Tensor] = None
        self.eps_queue: List[th.Tensor] = []

    def proba_distribution(self, mean_actions: th.Tensor, log_std: th.Tensor):
        self.mean, self.log_std = mean_actions, log_std  # Normal(mean, log_std.exp()) (:161-165)
        return self

    def draw_eps(self, shape, device, dtype=th.float32) -> th.Tensor:
        """Standard-normal draw of Normal.rsample (distributions.py:183), or the next teacher-forced tensor."""
        if self.eps_queue:
            return self.eps_queue.pop(0).to(device, dtype).reshape(shape)
        return th.randn(shape, dtype=dtype, device=device)

    def _eps(self) -> th.Tensor:
        return self.draw_eps(self.mean.shape, self.mean.device, self.mean.dtype)

    def sample(self) -> th.Tensor:
        """rsample then tanh (:183, :236-239)"""
        self.gaussian_actions = self.mean + self.log_std.exp() * self._eps()
        return th.tanh(self.gaussian_actions)

    def mode(self) -> th.Tensor:
        self.gaussian_actions = self.mean
        return th.tanh(self.gaussian_actions)

    def log_prob(self, actions: th.Tensor, gaussian_actions: Optional[th.Tensor] = None) -> th.Tensor:
        """sum Normal.log_prob(u) - sum log(1 - a^2 + eps) (:170-172, :226-234)"""
        if gaussian_actions is None:
            a = actions.clamp(-1.0 + 1e-6, 1.0 - 1e-6)  # TanhBijector.inverse (:699-712)
            gaussian_actions = 0.5 * (a.log1p() - (-a).log1p())
        std = self.log_std.exp()
        var = std ** 2
        lp = -((gaussian_actions - self.mean) ** 2) / (2 * var) - std.log() - math.log(math.sqrt(2 * math.pi))  # torch Normal.log_prob
        lp = lp.sum(dim=1) if lp.dim() > 1 else lp.sum()
        lp = lp - th.sum(th.log(1 - actions ** 2 + self.epsilon), dim=1)
        return lp

    def actions_from_params(self, mean_actions, log_std, deterministic: bool = False) -> th.Tensor:
        self.proba_distribution(mean_actions, log_std)
        return self.mode() if deterministic else self.sample()

    def log_prob_from_params(self, mean_actions, log_std):
        action = self.actions_from_params(mean_actions, log_std)
        return action, self.log_prob(action, self.gaussian_actions)


class StateDependentNoiseDistribution:
    """Generalized State-Dependent Exploration, squashed (reference: core/common/distributions.py:421-617; SAC passes
    learn_features=True, so gradients reach the latent through the noise and the variance).

    Every reset draws TWO matrices, `exploration_mat` [L, A] and `exploration_matrices` [n, L, A], in that order. After the
    policy has moved to the device they are drawn by one HIP launch (hip_ops.sde_draw) from this distribution's own Philox stream
    into buffers with fixed addresses (one set per n, so captured graphs replay fresh draws); `z_queue` is the teacher-forcing hook:
    the standard-normal tensors queued there are consumed in the reference's draw order (two per reset) instead. With
    `torch_matrices` (the ATen learner path) the matrices are the reference's autograd expressions z * get_std(log_std)."""

    def __init__(self, action_dim: int, full_std: bool = True, use_expln: bool = False, squash_output: bool = True,
                 learn_features: bool = True, epsilon: float = 1e-6):
        if not squash_output or not learn_features:
            raise NotImplementedError("StateDependentNoiseDistribution: only SAC's form (squash_output, learn_features) is built")
        self.action_dim, self.full_std, self.use_expln, self.epsilon = action_dim, full_std, use_expln, epsilon
        self.latent_sde_dim: Optional[int] = None
        self.exploration_mat: Optional[th.Tensor] = None
        self.exploration_matrices: Optional[th.Tensor] = None
        self.z_queue: List[th.Tensor] = []
        self.torch_matrices = True
        self.rng_ctl: Optional[th.Tensor] = None
        self._bufs: dict = {}   # n -> (std [L, A], z [1 + n, L, A], mats [1 + n, L, A])
        self.current = None     # the buffers of the last device draw
        self.mean = self.variance = self._latent_sde = None

    def get_std(self, log_std: th.Tensor) -> th.Tensor:
        """:473-497"""
        if self.use_expln:
            below_threshold = th.exp(log_std) * (log_std <= 0)
            safe_log_std = log_std * (log_std > 0) + self.epsilon
            above_threshold = (th.log1p(safe_log_std) + 1.0) * (log_std > 0)
            std = below_threshold + above_threshold
        else:
            std = th.exp(log_std)
        if self.full_std:
            return std
        return th.ones(self.latent_sde_dim, self.action_dim).to(log_std.device) * std

    def proba_distribution_net(self, latent_dim: int, log_std_init: float = -2.0, latent_sde_dim: Optional[int] = None):
        """:514-539 -- consumes the generator exactly as the reference does: the mean Linear's init, then the two draws."""
        from torch import nn

        mean_actions_net = nn.Linear(latent_dim, self.action_dim)
        self.latent_sde_dim = latent_dim if latent_sde_dim is None else latent_sde_dim
        log_std = th.ones(self.latent_sde_dim, self.action_dim) if self.full_std else th.ones(self.latent_sde_dim, 1)
        log_std = nn.Parameter(log_std * log_std_init, requires_grad=True)
        self.sample_weights(log_std)
        return mean_actions_net, log_std

    def _queued(self, shape, device) -> Optional[th.Tensor]:
        return self.z_queue.pop(0).to(device, th.float32).reshape(shape) if self.z_queue else None

    def sample_weights(self, log_std: th.Tensor, batch_size: int = 1) -> None:
        """:499-512"""
        shape = (self.latent_sde_dim, self.action_dim)
        if not log_std.is_cuda:  # construction, on the CPU generator: Normal(0, std).rsample() then .rsample((n,))
            std = self.get_std(log_std)
            z1 = self._queued(shape, "cpu")
            z1 = th.empty(shape).normal_() if z1 is None else z1
            z2 = self._queued((batch_size,) + shape, "cpu")
            z2 = th.empty((batch_size,) + shape).normal_() if z2 is None else z2
            self.exploration_mat, self.exploration_matrices = z1 * std, z2 * std
            self._host_z = (z1, z2)
            return
        from core.common import hip_ops

        std_b, z, mats = self._buffers(batch_size, log_std.device)
        z1 = self._queued(shape, log_std.device)
        if z1 is not None:
            z2 = self._queued((batch_size,) + shape, log_std.device)
            if z2 is None:
                raise ValueError("z_queue: a reset consumes two tensors ([L, A] then [n, L, A])")
            z[0].copy_(z1)
            z[1:].copy_(z2)
            hip_ops.sde_draw(log_std.detach(), self.action_dim, self.use_expln, z, mats, std_b)
        else:
            if self.rng_ctl is None:
                self.rng_ctl = hip_ops.new_rng_ctl(th.initial_seed(), log_std.device)
            # z of exploration_mat is what a backward needs (dM/dstd = z); with torch_matrices every z is an operand
            hip_ops.sde_draw(log_std.detach(), self.action_dim, self.use_expln, z, mats, std_b, rng_ctl=self.rng_ctl,
                             z_keep=None if self.torch_matrices else 1)
        self.current = (std_b, z, mats, batch_size)
        if self.torch_matrices:
            std = self.get_std(log_std)
            self.exploration_mat, self.exploration_matrices = z[0] * std, z[1:] * std
        else:
            self.exploration_mat, self.exploration_matrices = mats[0], mats[1:]

    def _buffers(self, n: int, device):
        if n not in self._bufs:
            L, a = self.latent_sde_dim, self.action_dim
            e = lambda *sh: th.empty(*sh, dtype=th.float32, device=device)  # noqa: E731
            self._bufs[n] = (e(L, a), e(1 + n, L, a), e(1 + n, L, a))
        return self._bufs[n]

    def to_device(self, log_std: th.Tensor) -> None:
        """The construction draws, on the device (`log_std` already lives there): what predict() uses before the first reset."""
        z1, z2 = self._host_z
        self.z_queue[:0] = [z1, z2]
        self.sample_weights(log_std, z2.shape[0])

    def seed_rng(self, seed: int) -> None:
        if self.rng_ctl is not None:
            from core.common import hip_ops

            self.rng_ctl.copy_(hip_ops.new_rng_ctl(seed, self.rng_ctl.device))

    def noise_rows(self, rows: int) -> bool:
        """get_noise (:593-603): one matrix per row when the batch has the length of exploration_matrices (and is not 1)."""
        return rows != 1 and rows == len(self.exploration_matrices)

    # ---- the reference's statements in torch (ATen path, predict() through the nn.Module) ----------------------------------
    def proba_distribution(self, mean_actions: th.Tensor, log_std: th.Tensor, latent_sde: th.Tensor):
        self._latent_sde = latent_sde
        self.variance = th.mm(self._latent_sde ** 2, self.get_std(log_std) ** 2)
        self.mean, self.scale = mean_actions, th.sqrt(self.variance + self.epsilon)
        return self

    def get_noise(self, latent_sde: th.Tensor) -> th.Tensor:
        if not self.noise_rows(len(latent_sde)):
            return th.mm(latent_sde, self.exploration_mat)
        return th.bmm(latent_sde.unsqueeze(dim=1), self.exploration_matrices).squeeze(dim=1)

    def sample(self) -> th.Tensor:
        return th.tanh(self.mean + self.get_noise(self._latent_sde))

    def mode(self) -> th.Tensor:
        return th.tanh(self.mean)

    def log_prob(self, actions: th.Tensor) -> th.Tensor:
        eps = th.finfo(actions.dtype).eps  # TanhBijector.inverse (:699-712)
        a = actions.clamp(min=-1.0 + eps, max=1.0 - eps)
        gaussian_actions = 0.5 * (a.log1p() - (-a).log1p())
        var = self.scale ** 2
        lp = -((gaussian_actions - self.mean) ** 2) / (2 * var) - self.scale.log() - math.log(math.sqrt(2 * math.pi))
        lp = lp.sum(dim=1)
        return lp - th.sum(th.log(1.0 - th.tanh(gaussian_actions) ** 2 + self.epsilon), dim=1)

    def actions_from_params(self, mean_actions, log_std, latent_sde, deterministic: bool = False) -> th.Tensor:
        self.proba_distribution(mean_actions, log_std, latent_sde)
        return self.mode() if deterministic else self.sample()

    def log_prob_from_params(self, mean_actions, log_std, latent_sde):
        actions = self.actions_from_params(mean_actions, log_std, latent_sde)
        return actions, self.log_prob(actions)


class CategoricalDistribution:
    """reference: core/common/distributions.py:263-311 -- torch's Categorical over the logits of a Discrete action space (torch
    statements: the API and the torch-statement path; the kernel path evaluates the same expressions in csrc/cstr_categorical.hip).
    `action_queue`: teacher-forcing hook, each `sample()` pops its indices from here first (tests)."""

    def __init__(self, action_dim: int):
        self.action_dim = action_dim
        self.distribution = None
        self.action_queue: list = []

    def proba_distribution_net(self, latent_dim: int) -> nn.Module:
        return nn.Linear(latent_dim, self.action_dim)

    def proba_distribution(self, action_logits: th.Tensor) -> "CategoricalDistribution":
        self.distribution = th.distributions.Categorical(logits=action_logits)
        return self

    def log_prob(self, actions: th.Tensor) -> th.Tensor:
        return self.distribution.log_prob(actions)

    def entropy(self) -> th.Tensor:
        return self.distribution.entropy()

    def sample(self) -> th.Tensor:
        if self.action_queue:
            d = self.distribution
            return self.action_queue.pop(0).to(d.logits.device, th.int64).reshape(d.logits.shape[:-1])
        return self.distribution.sample()

    def mode(self) -> th.Tensor:
        return th.argmax(self.distribution.probs, dim=1)

    def get_actions(self, deterministic: bool = False) -> th.Tensor:
        return self.mode() if deterministic else self.sample()

    def actions_from_params(self, action_logits: th.Tensor, deterministic: bool = False) -> th.Tensor:
        self.proba_distribution(action_logits)
        return self.get_actions(deterministic=deterministic)

    def log_prob_from_params(self, action_logits: th.Tensor):
        actions = self.actions_from_params(action_logits)
        return actions, self.log_prob(actions)


class MultiCategoricalDistribution:
    """reference: core/common/distributions.py:314-368 -- one torch Categorical per component of a MultiDiscrete action space, over
    the th.split of the flat logits (torch statements: the API and the torch-statement path; the kernel path evaluates the same
    expressions in csrc/cstr_multicategorical.hip). Log-probs and entropies are summed over the components.
    `action_queue`: teacher-forcing hook, each `sample()` pops its [n, len(action_dims)] levels from here first (tests)."""

    def __init__(self, action_dims):
        self.action_dims = [int(k) for k in action_dims]
        self.distribution = None
        self.action_queue: list = []

    def proba_distribution_net(self, latent_dim: int) -> nn.Module:
        return nn.Linear(latent_dim, sum(self.action_dims))

    def proba_distribution(self, action_logits: th.Tensor) -> "MultiCategoricalDistribution":
        self.distribution = [th.distributions.Categorical(logits=z) for z in th.split(action_logits, self.action_dims, dim=1)]
        return self

    def log_prob(self, actions: th.Tensor) -> th.Tensor:
        per_valve = [d.log_prob(a) for d, a in zip(self.distribution, th.unbind(actions, dim=1))]
        return th.stack(per_valve, dim=1).sum(dim=1)

    def entropy(self) -> th.Tensor:
        return th.stack([d.entropy() for d in self.distribution], dim=1).sum(dim=1)

    def sample(self) -> th.Tensor:
        if self.action_queue:
            z = self.distribution[0].logits
            return self.action_queue.pop(0).to(z.device, th.int64).reshape(z.shape[0], len(self.action_dims))
        return th.stack([d.sample() for d in self.distribution], dim=1)

    def mode(self) -> th.Tensor:
        return th.stack([th.argmax(d.probs, dim=1) for d in self.distribution], dim=1)

    def get_actions(self, deterministic: bool = False) -> th.Tensor:
        return self.mode() if deterministic else self.sample()

    def actions_from_params(self, action_logits: th.Tensor, deterministic: bool = False) -> th.Tensor:
        self.proba_distribution(action_logits)
        return self.get_actions(deterministic=deterministic)

    def log_prob_from_params(self, action_logits: th.Tensor):
        actions = self.actions_from_params(action_logits)
        return actions, self.log_prob(actions)


class DiagGaussianDistribution:
    """reference: core/common/distributions.py:125-204 -- the unsquashed diagonal Gaussian of the on-policy algorithms (torch
    statements: the API and the torch-statement path; the kernel path evaluates the same expressions in csrc/cstr_ppo.hip).
    `eps_queue`: teacher-forcing hook, each `sample()` pops its standard-normal draw from here first (tests)."""

    def __init__(self, action_dim: int):
        self.action_dim = action_dim
        self.distribution = None
        self.eps_queue: list = []

    def proba_distribution_net(self, latent_dim: int, log_std_init: float = 0.0):
        mean_actions = nn.Linear(latent_dim, self.action_dim)
        log_std = nn.Parameter(th.ones(self.action_dim) * log_std_init, requires_grad=True)
        return mean_actions, log_std

    def proba_distribution(self, mean_actions: th.Tensor, log_std: th.Tensor) -> "DiagGaussianDistribution":
        action_std = th.ones_like(mean_actions) * log_std.exp()
        self.distribution = th.distributions.Normal(mean_actions, action_std)
        return self

    def log_prob(self, actions: th.Tensor) -> th.Tensor:
        return self.distribution.log_prob(actions).sum(dim=1)  # sum_independent_dims

    def entropy(self) -> th.Tensor:
        return self.distribution.entropy().sum(dim=1)

    def sample(self) -> th.Tensor:
        d = self.distribution
        if self.eps_queue:
            eps = self.eps_queue.pop(0).to(d.loc.device, d.loc.dtype).reshape(d.loc.shape)
            return d.loc + eps * d.scale  # rsample's statement with the draw given
        return d.rsample()

    def mode(self) -> th.Tensor:
        return self.distribution.mean

    def get_actions(self, deterministic: bool = False) -> th.Tensor:
        return self.mode() if deterministic else self.sample()

    def actions_from_params(self, mean_actions: th.Tensor, log_std: th.Tensor, deterministic: bool = False) -> th.Tensor:
        self.proba_distribution(mean_actions, log_std)
        return self.get_actions(deterministic=deterministic)

    def log_prob_from_params(self, mean_actions: th.Tensor, log_std: th.Tensor):
        actions = self.actions_from_params(mean_actions, log_std)
        return actions, self.log_prob(actions)
