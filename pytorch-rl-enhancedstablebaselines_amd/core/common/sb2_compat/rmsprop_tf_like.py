"""RMSprop as TensorFlow (and so the original stable-baselines' A2C) computes it, with the reference's public surface
(core/common/sb2_compat/rmsprop_tf_like.py): the same constructor, messages, state keys and module path, so a `policy_kwargs` holding
the class and a `policy.optimizer.pth` written by it are interchangeable with the reference's.

It differs from `torch.optim.RMSprop` in two places: `square_avg` starts at ones, not zeros, and epsilon is added inside the square
root, `sqrt(square_avg + eps)`, not behind it. Per tensor, with g the gradient (plus `weight_decay * p` where set):

    square_avg = alpha * square_avg + (1 - alpha) * g * g
    centred:   grad_avg = alpha * grad_avg + (1 - alpha) * g;  avg = sqrt(square_avg - grad_avg^2 + eps)
    otherwise: avg = sqrt(square_avg + eps)
    momentum:  buf = momentum * buf + g / avg;  p -= lr * buf
    otherwise: p -= lr * g / avg

This class is the public one, the optimiser of every algorithm that is not A2C (it then runs on the arena's parameter views, as any
optimiser class a caller passes does) and the tests' CPU statement. A2C takes the same arithmetic as one flat kernel:
`arena.FlatRMSpropTFLike` over `cstr_rmsprop_tf_f32` (csrc/cstr_a2c.hip), which writes and reads this class's `state_dict` layout."""
from typing import Any, Callable, Iterable, Optional

import torch
from torch.optim import Optimizer


class RMSpropTFLike(Optimizer):
    """:param params: parameters or parameter-group dicts
    :param lr: learning rate
    :param alpha: smoothing constant of the running averages
    :param eps: added to the running average INSIDE the square root
    :param weight_decay: L2 penalty, added to the gradient
    :param momentum: momentum factor (0: none, and no `momentum_buffer` in the state)
    :param centered: normalise by an estimate of the gradient's variance (keeps `grad_avg` in the state)"""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-2, alpha: float = 0.99, eps: float = 1e-8,
                 weight_decay: float = 0, momentum: float = 0, centered: bool = False):
        for value, message in ((lr, "learning rate"), (eps, "epsilon value"), (momentum, "momentum value"),
                               (weight_decay, "weight_decay value"), (alpha, "alpha value")):
            if not 0.0 <= value:  # a NaN is refused as well
                raise ValueError(f"Invalid {message}: {value}")
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay))

    def __setstate__(self, state: dict[str, Any]) -> None:
        super().__setstate__(state)
        for group in self.param_groups:  # pickles older than the two options
            group.setdefault("momentum", 0)
            group.setdefault("centered", False)

    @staticmethod
    def _init_state(state: dict, p: torch.Tensor, group: dict) -> None:
        state["step"] = 0
        state["square_avg"] = torch.ones_like(p, memory_format=torch.preserve_format)  # torch.optim.RMSprop: zeros
        if group["momentum"] > 0:
            state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if group["centered"]:
            state["grad_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    @torch.no_grad()
    def step(self, closure: Optional[Callable[[], float]] = None) -> Optional[float]:  # type: ignore[override]
        """One step over every parameter that has a gradient; returns the closure's loss, if a closure is given."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            alpha, eps, lr, momentum, wd = group["alpha"], group["eps"], group["lr"], group["momentum"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("RMSpropTF does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    self._init_state(state, p, group)
                state["step"] += 1
                if wd != 0:
                    g = g.add(p, alpha=wd)
                sq = state["square_avg"]
                sq.mul_(alpha).addcmul_(g, g, value=1 - alpha)
                if group["centered"]:
                    ga = state["grad_avg"]
                    ga.mul_(alpha).add_(g, alpha=1 - alpha)
                    avg = sq.addcmul(ga, ga, value=-1).add_(eps).sqrt_()  # torch.optim.RMSprop: .sqrt_().add_(eps)
                else:
                    avg = sq.add(eps).sqrt_()  # torch.optim.RMSprop: .sqrt().add_(eps)
                if momentum > 0:
                    buf = state["momentum_buffer"]
                    buf.mul_(momentum).addcdiv_(g, avg)
                    p.add_(buf, alpha=-lr)
                else:
                    p.addcdiv_(g, avg, value=-lr)
        return loss
