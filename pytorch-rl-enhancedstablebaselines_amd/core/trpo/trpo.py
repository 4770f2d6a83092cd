"""TRPO (Schulman et al. 2015) with the constructor, defaults, `train()` arithmetic and logger keys of `sb3_contrib.TRPO` on the HIP path.

`train()`: ONE full-batch pass over the rollout buffer (`rollout_buffer.get(None)`, every `sub_sampling_factor`-th row of the permuted
batch), the policy objective mean(adv * ratio) and its gradient g, the natural-gradient direction s = F^-1 g by conjugate gradient on
Fisher-vector products, the step sqrt(2 target_kl / (s . F s)), a backtracking line search against the hard KL bound, then
`n_critic_updates` passes of minibatch regression of the critic with Adam. The actor parameters are every policy parameter whose name
does not contain "value"; vectors over them are flattened in `policy.named_parameters()` order.

The kernel path (`fused_learner` True: a flat Adam, widths the kernels take), csrc/cstr_trpo.hip:
  * the actor's forward at theta0 through the per-layer Linear kernels, its activations kept for all 17 products of the class defaults;
  * hip_ops.trpo_objective: advantage normalisation, log-prob, ratio, objective, KL and the objective's gradients in one launch;
  * a Fisher-vector product = a tangent (forward-mode) pass through the actor's three Linear layers (hip_ops.linear_tangent_fwd), the
    head's Fisher metric (hip_ops.trpo_fisher_head), the per-layer backward (two input-gradient launches, ONE weight-gradient launch)
    and the conjugate-gradient launch (hip_ops.trpo_cg_step), which adds the damping term: 8 launches. At theta0 the new and the old
    distribution coincide, so the Hessian of the mean KL IS the Fisher matrix J^T M J / R: no double backward;
  * the conjugate gradient's scalars (rr, alpha, beta), its `residual_tol` exits and the last-iteration rule live in a device control
    block: the host reads nothing while it runs;
  * a line-search iteration = hip_ops.trpo_apply_step, the actor's forward, the objective launch in line-search mode (it decides, and
    shrinks the device-resident coefficient on a rejection) and ONE 4-byte read of `accepted`, the only host synchronisation of train();
  * a critic minibatch = the gather launch, the value forward, hip_ops.trpo_value_loss, the value backward with one weight-gradient
    launch and `FlatAdam.step`; the actor segments of the gradient arena are exactly zero then, so the step leaves the actor's weights
    and moments bit-identical.
Vectors (g, x, r, p) are arena-sized with zeros outside the actor's tensors, so the backward's output (the gradient arena) is a vector
as it stands. Otherwise (another optimiser class, widths the kernels decline, `fused_learner = False`) the published statements run as
plain torch autograd on the arena parameters, the Fisher-vector product by double backward: the A/B baseline and the tests' reference.

Noise: the conjugate gradient starts from x = 1e-4 * N(0, 1), drawn by hip_ops.trpo_x0 on a Philox stream of TRPO's own tag keyed by
`seed`; `cg_init_queue` (float32 vectors in the flat order, tests) is consumed first. Both paths use the same draws.

Not built: the goal face ("MultiInputPolicy"), gSDE, VecNormalize, hipGraph replay, data-parallel training, a line search without the
per-iteration read, Categorical heads of more than 64 logits on the kernel path (`discrete_actions` of 9 to 16 levels per valve:
`fused_learner` is False, so train() runs the torch statements and the rollout the NumPy loop)."""
from typing import Optional, Union

import torch as th
from torch.nn import functional as F

from core import _native as nv
from core.common import fused, hip_ops
from core.common.logger import DeviceMean
from core.common.on_policy_algorithm import OnPolicyAlgorithm
from core.common.spaces import Discrete, MultiDiscrete
from core.ppo.ppo import PPO
from core.trpo.policies import MlpPolicy

RESIDUAL_TOL = 1e-10
X0_SCALE = 1e-4


class TRPO(OnPolicyAlgorithm):
    policy_aliases = {"MlpPolicy": MlpPolicy}
    goal_face_support = False

    def __init__(self, policy, env, learning_rate=1e-3, n_steps: int = 2048, batch_size: int = 128, gamma: float = 0.99,
                 cg_max_steps: int = 15, cg_damping: float = 0.1, line_search_shrinking_factor: float = 0.8,
                 line_search_max_iter: int = 10, n_critic_updates: int = 10, gae_lambda: float = 0.95, use_sde: bool = False,
                 sde_sample_freq: int = -1, rollout_buffer_class=None, rollout_buffer_kwargs: Optional[dict] = None,
                 normalize_advantage: bool = True, target_kl: float = 0.01, sub_sampling_factor: int = 1, stats_window_size: int = 100,
                 tensorboard_log: Optional[str] = None, policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None,
                 device: Union[th.device, str] = "auto", _init_setup_model: bool = True):
        if cg_max_steps < 1:
            raise ValueError(f"`cg_max_steps` must be at least 1, got {cg_max_steps}")
        if line_search_max_iter < 1:
            raise ValueError(f"`line_search_max_iter` must be at least 1, got {line_search_max_iter}")
        if not 0.0 < line_search_shrinking_factor < 1.0:
            raise ValueError(f"`line_search_shrinking_factor` must lie in (0, 1), got {line_search_shrinking_factor}")
        if not target_kl > 0.0:
            raise ValueError(f"`target_kl` must be positive, got {target_kl}")
        if sub_sampling_factor < 1:
            raise ValueError(f"`sub_sampling_factor` must be at least 1, got {sub_sampling_factor}")
        if n_critic_updates < 0:
            raise ValueError(f"`n_critic_updates` must not be negative, got {n_critic_updates}")
        super().__init__(policy, env, learning_rate=learning_rate, n_steps=n_steps, gamma=gamma, gae_lambda=gae_lambda, ent_coef=0.0,
                         vf_coef=0.0, max_grad_norm=0.0, use_sde=use_sde, sde_sample_freq=sde_sample_freq,
                         rollout_buffer_class=rollout_buffer_class, rollout_buffer_kwargs=rollout_buffer_kwargs,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs,
                         verbose=verbose, device=device, seed=seed, _init_setup_model=False, supported_action_spaces=("Box", Discrete, MultiDiscrete))
        PPO._check_batch_arguments(batch_size, self.n_steps, None if self.env is None else self.env.num_envs, normalize_advantage)
        self.batch_size = batch_size
        self.cg_max_steps, self.cg_damping = int(cg_max_steps), float(cg_damping)
        self.line_search_shrinking_factor, self.line_search_max_iter = float(line_search_shrinking_factor), int(line_search_max_iter)
        self.n_critic_updates = int(n_critic_updates)
        self.normalize_advantage = normalize_advantage
        self.target_kl = float(target_kl)
        self.sub_sampling_factor = int(sub_sampling_factor)
        self.cg_init_queue: list = []  # teacher-forced x0 draws: float32 vectors over the actor parameters in the flat order (tests)
        self.debug_capture = False  # True: train() keeps g, x0, s, step, sFs, the line search's iterations and the CG's rr history
        self.last_train_tensors: dict = {}
        if _init_setup_model:
            self._setup_model()

    def _get_policy_from_name(self, policy_name: str):
        if policy_name == "MultiInputPolicy":
            raise ValueError("TRPO does not support a Dict observation space (the goal face of the env): `MultiInputPolicy` is not built")
        return super()._get_policy_from_name(policy_name)

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        super()._setup_model()
        pol, dev = self.policy, self.device
        fast = self._fast
        if fast is not None:  # the TRPO launches' own widths: a Categorical head of more than 64 logits has no kernel path at all --
            # `fused_learner` is one switch for train() and the rollout, so its rollout is the NumPy loop too
            head = self._head_of(fast)
            if not hip_ops.trpo_supported(*head):
                self._fast, self._fused_learner, pol.fast = None, False, None
        arena = pol.arena
        self._actor_params = [(name, p) for name, p in pol.named_parameters() if "value" not in name]
        self._actor_spans = [(arena.offset_of[id(p)], p.numel()) for _, p in self._actor_params]
        self._n_actor = sum(n for _, n in self._actor_spans)
        with th.cuda.device(dev):
            self._mask = th.zeros(arena.numel, dtype=th.float32, device=dev)
            for o, n in self._actor_spans:
                self._mask[o:o + n] = 1.0
            self._ctl = hip_ops.new_trpo_ctl(dev)
            self._ws = hip_ops.new_ppo_workspace(dev)
            self._x0_rng = None if self.seed is None else hip_ops.new_rng_ctl(int(self.seed), dev)
            self._accepted = th.zeros(1, dtype=th.int32, device=dev)
            self._scalars0 = th.zeros(2, dtype=th.float32, device=dev)  # objective, kl of the gradient-mode launch
            self._scalars_ls = th.zeros(2, dtype=th.float32, device=dev)  # ... of the last line-search launch
            self._vl = th.zeros(1, dtype=th.float32, device=dev)
            self._vl_sum = th.zeros(1, dtype=th.float32, device=dev)
            self._vec = {k: th.zeros(arena.numel, dtype=th.float32, device=dev) for k in ("g", "x", "r", "p", "theta0")}
        self._row_bufs: dict = {}
        self._g_value: dict = {}

    @staticmethod
    def _head_of(fast) -> tuple:
        """(head, k0, k1) of the TRPO launches for a FastActorCritic"""
        if fast.discrete:
            return nv.TRPO_HEAD_CATEGORICAL, fast.n_actions, 0
        if fast.multi_discrete:
            return nv.TRPO_HEAD_MULTICATEGORICAL, fast.nvec[0], fast.nvec[1]
        return nv.TRPO_HEAD_GAUSSIAN, fast.act_dim, 0

    def _x0_stream(self) -> th.Tensor:
        if self._x0_rng is None:  # no seed given: keyed by torch's initial seed, as the rollout's stream is
            self._x0_rng = hip_ops.new_rng_ctl(th.initial_seed(), self.device)
        return self._x0_rng

    # ---- flat vectors ---------------------------------------------------------------------------------------------
    def _flat(self, vec: th.Tensor) -> th.Tensor:
        """the actor entries of an arena-sized vector in `policy.named_parameters()` order"""
        return th.cat([vec[o:o + n] for o, n in self._actor_spans])

    def _scatter(self, flat: th.Tensor, out: th.Tensor) -> th.Tensor:
        """the inverse: `out` (arena-sized) gets the flat vector's entries, zeros elsewhere"""
        flat = flat.to(out.device, th.float32).reshape(-1)
        if flat.numel() != self._n_actor:
            raise ValueError(f"a vector over the actor parameters holds {self._n_actor} floats, got {flat.numel()}")
        out.zero_()
        at = 0
        for o, n in self._actor_spans:
            out[o:o + n] = flat[at:at + n]
            at += n
        return out

    def _draw_x0(self, out: th.Tensor) -> th.Tensor:
        """x0 = 1e-4 * N(0, 1) over the actor parameters (arena-sized, zeros elsewhere): a queued vector first, the Philox stream otherwise"""
        if self.cg_init_queue:
            return self._scatter(th.as_tensor(self.cg_init_queue.pop(0)), out)
        hip_ops.trpo_x0(out, self._mask, X0_SCALE, self._x0_stream())
        return out

    # ---- the batch ------------------------------------------------------------------------------------------------
    def _batch(self):
        """one full-batch pass (one permutation of the buffer's stream), every `sub_sampling_factor`-th row of it"""
        rd = next(iter(self.rollout_buffer.get(batch_size=None)))
        k = self.sub_sampling_factor
        if k == 1:
            return rd.observations, rd.actions, rd.old_log_prob, rd.advantages
        return tuple(t[::k].contiguous() for t in (rd.observations, rd.actions, rd.old_log_prob, rd.advantages))

    # ---- the kernel path ------------------------------------------------------------------------------------------
    def _rows(self, rows: int) -> dict:
        b = self._row_bufs.get(rows)
        if b is None:
            e = lambda *sh: th.empty(*sh, dtype=th.float32, device=self.device)  # noqa: E731
            layers = self._fast.pi_layers
            b = self._row_bufs[rows] = dict(tan=[e(rows, lin.out_features) for lin, _ in layers], up=e(rows, layers[-1][0].out_features),
                                            g_dist=e(rows, layers[-1][0].out_features))
        return b

    def _actor_forward(self, obs: th.Tensor) -> list:
        """[obs, y1, y2, dist]: the actor's layers through the per-layer Linear kernels, no autograd"""
        acts = [obs]
        for lin, act in self._fast.pi_layers:
            acts.append(fused._linear_fwd(acts[-1], lin.weight.detach(), lin.bias.detach(), act))
        return acts

    def _actor_backward(self, acts: list, g_dist: th.Tensor) -> None:
        """the per-layer backward from d / d (mean | logits): dW and db of every actor layer land in the gradient arena (ONE
        weight-gradient launch); log_std's entry is the caller's"""
        layers = self._fast.pi_layers
        gz, sets = g_dist, []
        for i in range(len(layers) - 1, -1, -1):
            lin, _ = layers[i]
            sets.append((gz, acts[i], lin.weight.grad, lin.bias.grad))
            if i > 0:
                gz = hip_ops.linear_bwd_input(gz, lin.weight.detach(), acts[i], layers[i - 1][1])
        for i in range(0, len(sets), nv.MAX_LINEAR_SETS):
            hip_ops.linear_bwd_weight_sets(sets[i:i + nv.MAX_LINEAR_SETS])

    def _fvp_fused(self, v: th.Tensor, acts: list, head: tuple, b: dict) -> None:
        """F v (without the damping term) into the gradient arena: tangent pass, head metric, backward"""
        pol, arena = self.policy, self.policy.arena
        x_dot = None
        for i, (lin, act) in enumerate(self._fast.pi_layers):
            ow, ob = arena.offset_of[id(lin.weight)], arena.offset_of[id(lin.bias)]
            x_dot = hip_ops.linear_tangent_fwd(acts[i], x_dot, lin.weight.detach(), v[ow:ow + lin.weight.numel()].view_as(lin.weight),
                                               v[ob:ob + lin.bias.numel()], acts[i + 1], act, out=b["tan"][i])
        if head[0] == nv.TRPO_HEAD_GAUSSIAN:
            o = arena.offset_of[id(pol.log_std)]
            a = pol.log_std.numel()
            hip_ops.trpo_fisher_head(*head, x_dot, None, pol.log_std.detach(), v[o:o + a], b["up"], arena.grad[o:o + a])
        else:
            hip_ops.trpo_fisher_head(*head, x_dot, acts[-1], None, None, b["up"], None)
        self._actor_backward(acts, b["up"])

    def _objective_launch(self, head, dist, old_dist, old_log_std, actions, old_log_prob, adv, b, line_search: bool) -> None:
        pol = self.policy
        gauss = head[0] == nv.TRPO_HEAD_GAUSSIAN
        log_std = pol.log_std.detach() if gauss else None
        if line_search:
            hip_ops.trpo_objective(*head, dist, log_std, old_dist, old_log_std, actions, old_log_prob, adv, self.normalize_advantage,
                                   self._ctl, self._ws, scalars_out=self._scalars_ls, accepted=self._accepted, target_kl=self.target_kl,
                                   shrink=self.line_search_shrinking_factor)
        else:
            hip_ops.trpo_objective(*head, dist, log_std, old_dist, old_log_std, actions, old_log_prob, adv, self.normalize_advantage,
                                   self._ctl, self._ws, g_dist=b["g_dist"], g_log_std=pol.log_std.grad if gauss else None,
                                   scalars_out=self._scalars0)

    def _actor_step_fused(self, obs, actions, old_log_prob, adv) -> bool:
        pol, arena, vec, ctl = self.policy, self.policy.arena, self._vec, self._ctl
        head = self._head_of(self._fast)
        gauss = head[0] == nv.TRPO_HEAD_GAUSSIAN
        b = self._rows(obs.shape[0])
        cap = self.last_train_tensors if self.debug_capture else None
        actions = actions.reshape(-1) if not gauss else actions
        theta0 = vec["theta0"].copy_(arena.flat)
        old_log_std = None
        if gauss:
            o = arena.offset_of[id(pol.log_std)]
            old_log_std = theta0[o:o + pol.log_std.numel()]
        arena.grad.zero_()  # the value segments stay zero through the actor phase: the gradient arena is a vector over the actor
        acts = self._actor_forward(obs)
        old_dist = acts[-1]
        self._objective_launch(head, old_dist, old_dist, old_log_std, actions, old_log_prob, adv, b, line_search=False)
        self._actor_backward(acts, b["g_dist"])
        g = vec["g"].copy_(arena.grad)
        # conjugate gradient: x = F^-1 g, 1 + cg_max_steps + 1 products, nothing read by the host
        x, r, p = self._draw_x0(vec["x"]), vec["r"], vec["p"]
        if cap is not None:
            cap.update(g=self._flat(g), x0=self._flat(x), rr=[])
        self._fvp_fused(x, acts, head, b)
        hip_ops.trpo_cg_step(nv.TRPO_CG_INIT, x, r, p, arena.grad, g, self.cg_damping, RESIDUAL_TOL, ctl)
        if cap is not None:
            cap["rr"].append(ctl[nv.TRPO_CTL["rr"]].clone())
        for i in range(self.cg_max_steps):
            self._fvp_fused(p, acts, head, b)
            hip_ops.trpo_cg_step(nv.TRPO_CG_STEP, x, r, p, arena.grad, None, self.cg_damping, RESIDUAL_TOL, ctl, last=i == self.cg_max_steps - 1)
            if cap is not None:
                cap["rr"].append(ctl[nv.TRPO_CTL["rr"]].clone())
        self._fvp_fused(x, acts, head, b)
        hip_ops.trpo_cg_step(nv.TRPO_CG_FINISH, x, None, None, arena.grad, None, self.cg_damping, RESIDUAL_TOL, ctl, target_kl=self.target_kl)
        if cap is not None:
            cap.update(s=self._flat(x), step=ctl[nv.TRPO_CTL["step"]].clone(), sFs=ctl[nv.TRPO_CTL["sfs"]].clone(), line_search=[])
        # line search: one 4-byte read per iteration
        success = False
        for _ in range(self.line_search_max_iter):
            if cap is not None:
                coeff = float(ctl[nv.TRPO_CTL["coeff"]])
            hip_ops.trpo_apply_step(arena.flat, theta0, x, self._mask, ctl)
            dist = self._actor_forward(obs)[-1]
            self._objective_launch(head, dist, old_dist, old_log_std, actions, old_log_prob, adv, b, line_search=True)
            success = bool(int(self._accepted.item()))
            if cap is not None:
                cap["line_search"].append((coeff, float(self._scalars_ls[0]), float(self._scalars_ls[1]), success))
            if success:
                break
        if not success:
            arena.flat.copy_(theta0)
        arena.grad.zero_()  # the critic phase starts from exactly zero actor gradients
        return success

    # ---- the torch path: the published statements on the arena parameters -------------------------------------------
    def _torch_distributions(self, obs: th.Tensor) -> list:
        d = self.policy.get_distribution(obs).distribution
        return list(d) if isinstance(d, (list, tuple)) else [d]

    def _torch_log_prob(self, actions: th.Tensor) -> th.Tensor:
        pol = self.policy
        if pol.discrete:
            actions = actions.long().flatten()
        elif pol.multi_discrete:
            actions = actions.long().reshape(-1, len(pol.action_dist.action_dims))
        return pol.action_dist.log_prob(actions)

    @staticmethod
    def _torch_kl(new: list, old: list) -> th.Tensor:
        per = [th.distributions.kl_divergence(n, o) for n, o in zip(new, old)]
        per = [k.sum(dim=1) if k.dim() > 1 else k for k in per]  # the Gaussian's action dimensions
        return th.stack(per, dim=1).sum(dim=1).mean()

    def _torch_objective_kl(self, obs, actions, old_log_prob, adv, old: list):
        new = self._torch_distributions(obs)
        log_prob = self._torch_log_prob(actions)
        ratio = th.exp(log_prob - old_log_prob)
        return (adv * ratio).mean(), self._torch_kl(new, old)

    def _actor_step_torch(self, obs, actions, old_log_prob, adv) -> bool:
        params = [p for _, p in self._actor_params]
        cap = self.last_train_tensors if self.debug_capture else None
        if self.normalize_advantage:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        with th.no_grad():
            old = []
            for d in self._torch_distributions(obs):
                if isinstance(d, th.distributions.Normal):
                    old.append(th.distributions.Normal(d.loc.clone(), d.scale.clone()))
                else:
                    old.append(th.distributions.Categorical(logits=d.logits.clone()))
        objective, kl = self._torch_objective_kl(obs, actions, old_log_prob, adv, old)
        flat = lambda ts: th.cat([t.reshape(-1) for t in ts])  # noqa: E731
        g = flat(th.autograd.grad(objective, params, retain_graph=True)).detach()
        grad_kl = flat(th.autograd.grad(kl, params, create_graph=True))

        def fvp(v):
            return flat(th.autograd.grad(grad_kl @ v, params, retain_graph=True)).detach() + self.cg_damping * v

        x = self._flat(self._draw_x0(self._vec["x"])).clone()
        if cap is not None:
            cap.update(g=g.clone(), x0=x.clone(), rr=[])
        # conjugate_gradient_solver(fvp, g, max_iter=cg_max_steps, residual_tol=1e-10)
        r = g - fvp(x)
        p = r.clone()
        rr = r @ r
        if cap is not None:
            cap["rr"].append(rr.clone())
        if not bool(rr < RESIDUAL_TOL):
            for i in range(self.cg_max_steps):
                ap = fvp(p)
                alpha = rr / (p @ ap)
                x = x + alpha * p
                if i == self.cg_max_steps - 1:
                    break
                r = r - alpha * ap
                new_rr = r @ r
                if bool(new_rr < RESIDUAL_TOL):
                    break
                beta = new_rr / rr
                rr = new_rr
                p = r + beta * p
                if cap is not None:
                    cap["rr"].append(rr.clone())
        s = x
        sfs = s @ fvp(s)
        step = th.sqrt(2 * self.target_kl / sfs)
        if cap is not None:
            cap.update(s=s.clone(), step=step.clone(), sFs=sfs.clone(), line_search=[])
        theta0 = [p_.detach().clone() for p_ in params]
        coeff, success = 1.0, False
        objective = objective.detach()
        with th.no_grad():
            for _ in range(self.line_search_max_iter):
                at = 0
                for p_, o in zip(params, theta0):
                    n = p_.numel()
                    p_.copy_(o + coeff * step * s[at:at + n].view_as(p_))
                    at += n
                new_objective, new_kl = self._torch_objective_kl(obs, actions, old_log_prob, adv, old)
                success = bool((new_kl < self.target_kl) & (new_objective > objective))
                if cap is not None:
                    cap["line_search"].append((coeff, float(new_objective), float(new_kl), success))
                if success:
                    self._scalars_ls.copy_(th.stack([new_objective, new_kl]))
                    break
                coeff *= self.line_search_shrinking_factor
            if not success:
                for p_, o in zip(params, theta0):
                    p_.copy_(o)
            self._scalars0.copy_(th.stack([objective, kl.detach()]))
        return success

    # ---- the critic -----------------------------------------------------------------------------------------------
    def _critic_minibatch_fused(self, rd) -> None:
        values = self._fast.values(rd.observations, train_params=True)
        g = self._g_value.get(values.shape[0])
        if g is None:
            g = self._g_value[values.shape[0]] = th.empty(values.shape[0], 1, dtype=th.float32, device=self.device)
        hip_ops.trpo_value_loss(values.detach().reshape(-1), rd.returns, g.reshape(-1), self._vl, self._vl_sum)
        with fused.deferred_weight_grads():
            th.autograd.backward([values], [g])
        self.policy.optimizer.step()

    def _critic_minibatch_torch(self, rd) -> None:
        pol = self.policy
        values = pol.predict_values(rd.observations)
        value_loss = F.mse_loss(rd.returns, values.flatten())
        pol.optimizer.zero_grad()
        value_loss.backward()  # the actor parameters receive no gradient: they are no part of the critic's graph
        pol.optimizer.step()
        with th.no_grad():
            self._vl.copy_(value_loss.detach().reshape(1))
            self._vl_sum += self._vl

    def train(self) -> None:
        self.policy.set_training_mode(True)
        self._update_learning_rate(self.policy.optimizer)
        rb = self.rollout_buffer
        self.last_train_tensors = {}
        n_minibatches = 0
        with th.cuda.device(self.device):
            obs, actions, old_log_prob, adv = self._batch()
            step = self._actor_step_fused if self._fused_learner else self._actor_step_torch
            success = step(obs, actions, old_log_prob, adv)
            with th.no_grad():
                if success:
                    policy_objective, kl_div = self._scalars_ls[0].clone(), self._scalars_ls[1].clone()
                else:
                    policy_objective, kl_div = self._scalars0[0].clone(), th.zeros((), dtype=th.float32, device=self.device)
            self._vl_sum.zero_()
            critic = self._critic_minibatch_fused if self._fused_learner else self._critic_minibatch_torch
            for _ in range(self.n_critic_updates):
                for rd in rb.get(self.batch_size):
                    critic(rd)
                    n_minibatches += 1
            with th.no_grad():
                value_loss_sum = self._vl_sum[0].clone()
                y_pred, y_true = rb.values.flatten(), rb.returns.flatten()
                var_y = y_true.var(unbiased=False)  # explained_variance (np.var): NaN where var(y_true) == 0
                explained_var = th.where(var_y == 0, th.full_like(var_y, float("nan")), 1 - (y_true - y_pred).var(unbiased=False) / var_y)
                std = th.exp(self.policy.log_std.detach()).mean() if hasattr(self.policy, "log_std") else None
        self._n_updates += 1
        self.logger.record("train/policy_objective", DeviceMean(policy_objective, 1))
        self.logger.record("train/value_loss", DeviceMean(value_loss_sum, max(n_minibatches, 1)))
        self.logger.record("train/kl_divergence_loss", DeviceMean(kl_div, 1))
        self.logger.record("train/explained_variance", DeviceMean(explained_var, 1))
        self.logger.record("train/is_line_search_success", float(success))
        if std is not None:
            self.logger.record("train/std", DeviceMean(std, 1))
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 1, tb_log_name: str = "TRPO", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def _extra_save_data(self) -> dict:
        return dict(n_steps=self.n_steps, gae_lambda=self.gae_lambda, cg_max_steps=self.cg_max_steps, cg_damping=self.cg_damping,
                    line_search_shrinking_factor=self.line_search_shrinking_factor, line_search_max_iter=self.line_search_max_iter,
                    n_critic_updates=self.n_critic_updates, normalize_advantage=self.normalize_advantage, target_kl=self.target_kl,
                    sub_sampling_factor=self.sub_sampling_factor)

    @classmethod
    def _ctor_keys(cls) -> tuple:
        return ("learning_rate", "n_steps", "batch_size", "gamma", "cg_max_steps", "cg_damping", "line_search_shrinking_factor",
                "line_search_max_iter", "n_critic_updates", "gae_lambda", "normalize_advantage", "target_kl", "sub_sampling_factor", "seed",
                "policy_kwargs")
