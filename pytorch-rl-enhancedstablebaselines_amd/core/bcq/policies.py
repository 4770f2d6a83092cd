"""BCQ's networks and policy (reference: core/bcq/policies.py:21-124 BehaviorVAE, :127-166 PerturbationNetwork, :169-258 VAEActor,
:261-458 BCQPolicy). `MlpPolicy` only. Constructor signatures, attribute names, assertion messages and `state_dict` keys are the
reference's; the networks are built on the CPU generator in the reference's order (same seed -> bit-equal initial weights) and then
moved into flat arenas: one for the VAE, one for the perturbation net, one for the critics, and identical layouts for the targets."""
import warnings
from typing import Optional, Tuple, Union

import torch as th
from torch import nn

from core.common import distributed as dist_util
from core.common.arena import FlatAdam, ParamArena, make_optimizer
from core.common.policies import BasePolicy, ContinuousCritic
from core.common.spaces import get_action_dim
from core.common.torch_layers import FlattenExtractor

LATENT_CLIP = 0.5  # candidates are decoded from clamp(randn, -0.5, 0.5) (:111, :123)


class BehaviorVAE(nn.Module):
    """Conditional VAE of the behaviour policy (reference :21-124); ReLU / Tanh are hard-coded there."""

    def __init__(self, state_dim: int, action_dim: int, latent_dim: Optional[int] = None, hidden_dim: int = 750):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        if latent_dim is None:
            latent_dim = 2 * action_dim
        self.latent_dim = latent_dim
        self.encoder = nn.Sequential(nn.Linear(state_dim + action_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU())
        self.mean = nn.Linear(hidden_dim, latent_dim)
        self.log_std = nn.Linear(hidden_dim, latent_dim)
        self.decoder = nn.Sequential(nn.Linear(state_dim + latent_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                     nn.Linear(hidden_dim, action_dim), nn.Tanh())

    def forward(self, state: th.Tensor, action: th.Tensor, eps: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor, th.Tensor]:
        """:67-87; `eps`: the draw of :82 when it is teacher-forced."""
        mean, std = self.encode(state, action)
        z = mean + std * (th.randn_like(std) if eps is None else eps)
        return self.decoder(th.cat([state, z], dim=1)), mean, std

    def encode(self, state: th.Tensor, action: th.Tensor) -> Tuple[th.Tensor, th.Tensor]:
        z = self.encoder(th.cat([state, action], dim=1))
        return self.mean(z), self.log_std(z).clamp(-4, 15).exp()

    def decode(self, state: th.Tensor, z: Optional[th.Tensor] = None) -> th.Tensor:
        if z is None:
            z = th.randn((state.shape[0], self.latent_dim), device=state.device).clamp(-LATENT_CLIP, LATENT_CLIP)
        return self.decoder(th.cat([state, z], dim=1))

    def sample_action(self, state: th.Tensor, num_samples: int = 10, noise: Optional[th.Tensor] = None) -> th.Tensor:
        """:114-124; `noise` [num_samples * n, L]: the raw draw of :123 (before the clamp) when it is teacher-forced."""
        state_rep = state.repeat(num_samples, 1)
        if noise is None:
            noise = th.randn((state_rep.shape[0], self.latent_dim), device=state.device)
        return self.decoder(th.cat([state_rep, noise.clamp(-LATENT_CLIP, LATENT_CLIP)], dim=1))


class PerturbationNetwork(nn.Module):
    """reference :127-166"""

    def __init__(self, state_dim: int, action_dim: int, hidden_dim: int, max_perturbation: float = 0.05):
        super().__init__()
        self.max_perturbation = max_perturbation
        self.model = nn.Sequential(nn.Linear(state_dim + action_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                   nn.Linear(hidden_dim, action_dim), nn.Tanh())

    def forward(self, state: th.Tensor, action: th.Tensor) -> th.Tensor:
        perturbation = self.model(th.cat([state, action], dim=1)) * self.max_perturbation
        return (action + perturbation).clamp(-1, 1)


class VAEActor(BasePolicy):
    """reference :169-258"""

    def __init__(self, observation_space, action_space, net_arch, features_extractor: nn.Module, features_dim: int,
                 normalize_images: bool = True):
        super().__init__(observation_space, action_space, features_extractor=features_extractor, normalize_images=normalize_images,
                         squash_output=True)
        self.features_dim = features_dim
        action_dim = get_action_dim(self.action_space)
        if isinstance(net_arch, list) and len(net_arch) > 0 and isinstance(net_arch[0], dict):
            warnings.warn("you should now pass directly a dictionary and not a list "
                          "(net_arch=dict(vae_latent_dim=..., vae_hidden_dim=..., perturbation_hidden_dim=..., "
                          "max_perturbation=...) instead of net_arch=[dict(...)])")
            net_arch = net_arch[0]
        if net_arch is None:  # :215-217 (BCQPolicy always passes its own default)
            net_arch = dict(vae_latent_dim=32, vae_hidden_dim=720, perturbation_hidden_dim=400, max_perturbation=0.05)
        self.net_arch = net_arch
        self.vae = BehaviorVAE(state_dim=features_dim, action_dim=action_dim, latent_dim=net_arch["vae_latent_dim"],
                               hidden_dim=net_arch["vae_hidden_dim"])
        self.perturbation = PerturbationNetwork(state_dim=features_dim, action_dim=action_dim, hidden_dim=net_arch["perturbation_hidden_dim"],
                                                max_perturbation=net_arch["max_perturbation"])
        self.vae_optimizer = self.perturbation_optimizer = None

    def forward(self, obs: th.Tensor, num_samples: int = 10, noise: Optional[th.Tensor] = None) -> th.Tensor:
        """:244-253: num_samples perturbed candidates per observation, row r for observation r % n."""
        features = self.extract_features(obs, self.features_extractor)
        candidates = self.vae.sample_action(features, num_samples, noise)
        return self.perturbation(features.repeat(num_samples, 1), candidates)

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        return self(obs=observation, num_samples=100)


class BCQPolicy(BasePolicy):
    """reference :261-458"""

    def __init__(self, observation_space, action_space, lr_schedule, actor_net_arch: Optional[Union[list, dict]] = None,
                 critic_net_arch: Optional[Union[list, dict]] = None, activation_fn=nn.ReLU, features_extractor_class=FlattenExtractor,
                 features_extractor_kwargs: Optional[dict] = None, normalize_images: bool = True, optimizer_class=th.optim.Adam,
                 optimizer_kwargs: Optional[dict] = None, n_critics: int = 2, share_features_extractor: bool = False):
        super().__init__(observation_space, action_space, features_extractor_class, features_extractor_kwargs,
                         optimizer_class=optimizer_class, optimizer_kwargs=optimizer_kwargs, squash_output=True,
                         normalize_images=normalize_images)
        if share_features_extractor:
            raise NotImplementedError("share_features_extractor=True is not built (FlattenExtractor has no parameters)")
        if actor_net_arch is None:
            actor_net_arch = dict(vae_latent_dim=32, vae_hidden_dim=64, perturbation_hidden_dim=64, max_perturbation=0.05)
        else:
            assert isinstance(actor_net_arch, dict), "Error: the net_arch can only contain be a list of ints or a dict"
            assert "vae_latent_dim" in actor_net_arch, "Error: no key 'vae_latent_dim' was provided in net_arch for the actor network"
            assert "vae_hidden_dim" in actor_net_arch, "Error: no key 'vae_hidden_dim' was provided in net_arch for the actor network"
            assert "perturbation_hidden_dim" in actor_net_arch, "Error: no key 'perturbation_hidden_dim' was provided in net_arch for the actor network"
            assert "max_perturbation" in actor_net_arch, "Error: no key 'max_perturbation' was provided in net_arch for the actor network"
        if critic_net_arch is None:
            critic_net_arch = [400, 300]
        self.actor_arch, self.critic_arch = actor_net_arch, critic_net_arch
        self.activation_fn = activation_fn  # stored and never used, as in the reference (:336)
        self.n_critics = n_critics
        self.share_features_extractor = share_features_extractor
        self._lr_schedule = lr_schedule
        self.fast = None
        self.predict_noise_queue: list = []  # teacher-forcing hook: raw [100 n, L] draws of _predict (tests)
        self.debug_capture, self.last_predict = False, {}  # debug_capture: _predict keeps its candidates and their q1
        self._build(lr_schedule)

    def make_actor(self) -> VAEActor:
        fe = self.make_features_extractor()
        return VAEActor(self.observation_space, self.action_space, self.actor_arch, fe, fe.features_dim, self.normalize_images)

    def make_critic(self) -> ContinuousCritic:
        fe = self.make_features_extractor()
        return ContinuousCritic(self.observation_space, self.action_space, self.critic_arch, fe, fe.features_dim,
                                n_critics=self.n_critics, share_features_extractor=False)

    def _build(self, lr_schedule) -> None:
        """Creation order of the reference (:359-401): actor, actor_target, critic, critic_target."""
        self.actor = self.make_actor()
        self.actor_target = self.make_actor()
        self.actor_target.load_state_dict(self.actor.state_dict())
        self.critic = self.make_critic()
        self.critic_target = self.make_critic()
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.actor_target.set_training_mode(False)
        self.critic_target.set_training_mode(False)
        self.critic.optimizer = None

    @staticmethod
    def _vae_params(actor: VAEActor) -> list:
        """The VAE optimiser's parameters in the reference's order (:373-377): the actor's, without the perturbation net's."""
        skip = {id(p) for p in actor.perturbation.parameters()}
        return [p for p in actor.parameters() if id(p) not in skip]

    @staticmethod
    def _head_groups(vae: BehaviorVAE) -> list:
        """mean | log_std heads back to back: ONE [2L, H] weight for the merged head GEMM"""
        return [[vae.mean.weight, vae.log_std.weight], [vae.mean.bias, vae.log_std.bias]]

    def to_device_arenas(self, device) -> None:
        from core.common import fused

        lr = self._lr_schedule(1)
        a, at = self.actor, self.actor_target
        self.pert_arena, a.perturbation_optimizer = make_optimizer(a.perturbation.parameters(), device, lr, self.optimizer_class,
                                                                   self.optimizer_kwargs)
        self.vae_arena, a.vae_optimizer = make_optimizer(self._vae_params(a), device, lr, self.optimizer_class, self.optimizer_kwargs,
                                                         groups=self._head_groups(a.vae))
        self.critic_arena, self.critic.optimizer = make_optimizer(self.critic.parameters(), device, lr, self.optimizer_class,
                                                                  self.optimizer_kwargs, groups=fused.twin_groups(self.critic.q_networks))
        self.pert_target_arena = ParamArena(at.perturbation.parameters(), device, with_grad=False)
        self.vae_target_arena = ParamArena(self._vae_params(at), device, with_grad=False, groups=self._head_groups(at.vae))
        self.critic_target_arena = ParamArena(self.critic_target.parameters(), device, with_grad=False,
                                              groups=fused.twin_groups(self.critic_target.q_networks))
        self.critic_stack = fused.twin_stack(self.critic_arena)
        self.critic_target_stack = fused.twin_stack(self.critic_target_arena)
        for p in list(at.parameters()) + list(self.critic_target.parameters()):
            p.requires_grad_(False)
        w, wg = self.vae_arena.stacked(0)
        b, bg = self.vae_arena.stacked(1)
        l2 = 2 * a.vae.latent_dim
        self.vae_head = (w.view(l2, -1), b.view(l2), wg.view(l2, -1), bg.view(l2))

    def flat_optimizers(self) -> list:
        return [o for o in (self.actor.vae_optimizer, self.actor.perturbation_optimizer, self.critic.optimizer) if isinstance(o, FlatAdam)]

    def broadcast_from_rank0(self) -> None:
        for arena in (self.vae_arena, self.pert_arena, self.critic_arena, self.vae_target_arena, self.pert_target_arena,
                      self.critic_target_arena):
            dist_util.broadcast_(arena.flat, 0)

    def forward(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        return self._predict(observation, deterministic=deterministic)

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        """:426-435: 100 candidates, the one with the largest q1. `deterministic` is ignored, as in the reference. One observation:
        the reference's statements or their kernel form; several observations: the per-observation argmax, [n, A] (the reference
        returns ONE row, the argmax over all 100 n candidates)."""
        num_samples = 100
        n = observation.shape[0]
        noise = self.predict_noise_queue.pop(0).to(observation.device, th.float32).contiguous() if self.predict_noise_queue else None
        if self.fast is not None and observation.is_cuda:
            return self.fast.predict(observation.contiguous(), num_samples, noise)
        candidates = self.actor(observation, num_samples=num_samples, noise=noise)
        q1 = self.critic.q1_forward(observation.repeat(num_samples, 1), candidates)
        if self.debug_capture:
            self.last_predict = dict(q1=q1.detach().clone(), candidates=candidates.detach().clone())
        ind = q1.reshape(num_samples, n).argmax(0) * n + th.arange(n, device=q1.device)
        return candidates[ind]

    def set_training_mode(self, mode: bool) -> None:
        self.actor.set_training_mode(mode)
        self.critic.set_training_mode(mode)
        self.training = mode


MlpPolicy = BCQPolicy
