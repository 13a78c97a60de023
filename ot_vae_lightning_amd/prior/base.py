"""``Prior``: what sits between the encoder output and the decoder input (reference contract: prior/base.py:26-78).

A prior turns the encoder's tensor ``x`` into the latent ``z`` and charges a per-sample regulariser for it:

    prior(x, step, **kw) -> (z, loss[B], artifacts)     ``encode`` result with the loss weighted (below)
    prior.sample(shape, device) -> z                    draw latents without an encoder
    prior.out_size(size)                                shape of ``z`` for an ``x`` of ``size`` (batch axis excluded)

Weighting: ``loss_coeff`` times a half-cosine ramp that rises from 0 at step 0 to 1 at ``annealing_steps`` and stays
there (``annealing_steps=0`` disables the ramp).

Rules the subclasses of this package follow so that a step can be captured into a hipGraph by ``engine.HipTrainer``:
``encode`` launches kernels only (no ``.item()``, no host-side branching on device values), returns ``loss`` as a
device tensor of shape [B], and puts anything expensive to build on the host (``torch.distributions`` objects) behind a
lazy proxy in ``artifacts``.  ``step`` is a host integer; under graph capture the weight is therefore frozen at capture
time, which is exact whenever ``annealing_steps == 0`` (every shipped config).
"""
import math
from abc import ABC, abstractmethod
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Distribution

__all__ = ["Prior", "MinibatchPrior"]


def _half_cosine(progress: float) -> float:
    """0 at progress=0, 1 at progress>=1, cosine-shaped in between"""
    return 1.0 if progress >= 1.0 else 0.5 - 0.5 * math.cos(math.pi * progress)


class Prior(nn.Module, ABC):
    EncodingResults = Tuple[Tensor, Tensor, Dict[str, Union[Tensor, Distribution]]]

    def __init__(self, loss_coeff: float = 1., annealing_steps: int = 0):
        super().__init__()
        self._loss_coeff, self.annealing_steps = loss_coeff, annealing_steps

    @property
    def loss_coeff(self):
        return self._loss_coeff

    def annealing(self, step: int) -> float:
        return _half_cosine(step / self.annealing_steps) if self.annealing_steps > step else 1

    def forward(self, x: Tensor, step: int, **kwargs) -> "Prior.EncodingResults":
        z, loss, artifacts = self.encode(x, **kwargs)
        return z, loss * (self.loss_coeff * self.annealing(step)), artifacts

    @staticmethod
    def empirical_reverse_kl(p: Distribution, q: Distribution, z: Tensor) -> Tensor:
        """single-sample estimate of KL(q || p) at z ~ q, summed over everything but the batch axis"""
        gap = q.log_prob(z) - p.log_prob(z)
        return gap.flatten(1).sum(1) if gap.dim() > 1 else gap

    # ---- to be provided
    @abstractmethod
    def encode(self, x: Tensor) -> "Prior.EncodingResults":
        ...

    @abstractmethod
    def sample(self, shape, device) -> Tensor:
        ...

    @abstractmethod
    def out_size(self, size):
        ...


class _LatentLossFn(torch.autograd.Function):
    """The one autograd node of the minibatch priors: ``z_out, loss, *extras = _LatentLossFn.apply(z, run, grad, *held)``.

    ``run()`` issues the prior's forward op (and whatever must be ordered behind it) and returns ``(loss, saved, extras)``, tuples of
    tensors; ``grad(g, gz_out, *saved)`` is the call of its ``*_backward`` op, constants bound by the caller.

    Why the latents leave through this node too (``z_out``, an alias of z): z has two consumers, the decoder and the loss.  With both
    behind one node the gradient the decoder sends back (``gz_out``) reaches the prior's backward kernel as its ``gadd`` operand and
    is summed with the loss term's own gradient there, instead of by an autograd accumulation kernel.

    Inside a training engine's step (``functional.PriorLane.active``) ``run`` is issued on the prior lane, beside the decoder.  The
    lane's kernels then read z and ``held`` -- tensors of the LAUNCH stream's pool -- so the lane keeps them alive until the join
    (``PriorLane.hold`` has the bug that taught this); the backward joins the lane first: what ``run`` produced is complete from
    there on."""

    @staticmethod
    def forward(ctx, z, run, grad, *held):
        from ..functional import PriorLane
        ctx.lane = PriorLane.active(z.device)
        loss, saved, extras = PriorLane.issue(z.device, run, z, *held) if ctx.lane else run()
        ctx.save_for_backward(*saved)
        ctx.grad, ctx.device, ctx.n_rest = grad, z.device, 2 + len(held)
        ctx.mark_non_differentiable(*extras)
        ctx.set_materialize_grads(False)  # a missing cotangent arrives as None: no zeros tensor, gadd=None
        return (z.view_as(z), loss, *extras)

    @staticmethod
    def backward(ctx, gz_out, g, *_):
        if ctx.lane:
            from ..functional import PriorLane
            PriorLane.join(ctx.device)
        if g is not None:  # (otherwise only the latents were used downstream)
            gz_out = ctx.grad(g, gz_out, *ctx.saved_tensors)
        return (gz_out,) + (None,) * ctx.n_rest


class MinibatchPrior(Prior):
    """Deterministic encoder (z = x) + a distance between the minibatch of latents and the prior, computed by one forward / backward
    op pair behind ``_LatentLossFn``.  Subclasses provide ``encode(x, ..., _scale)``: ``loss_coeff`` x annealing is folded into the
    loss kernel (and the backward's scale) instead of a separate multiply."""
    seed: Optional[int] = None

    def out_size(self, size):
        return size

    def sample(self, shape, device) -> Tensor:
        return torch.randn(*shape, device=device)

    def _key(self, device) -> Tensor:
        """key of the device-side counter-based generator, made from ``seed`` on first use (again when the device changes); kept in
        ``__dict__``: no buffer, not in ``state_dict()``"""
        from .. import functional as HF
        key = self.__dict__.get("_rng_key")
        if key is None or key.device != device:
            key = self.__dict__["_rng_key"] = HF.new_rng_key(device, self.seed)
        return key

    def forward(self, x: Tensor, step: int, **kwargs) -> Prior.EncodingResults:
        # a subclass that takes keywords (``prior_samples``) declares them in a ``forward`` of its own and calls this one: ``VAE`` hands a
        # keyword only to a plug-in whose signature names it (utils.FilterKwargs)
        return self.encode(x, **kwargs, _scale=float(self.loss_coeff * self.annealing(step)))
