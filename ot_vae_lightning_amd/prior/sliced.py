"""Sliced Wasserstein-2 prior: the third member of the minibatch optimal-transport family (``SinkhornPrior``, ``GaussianW2Prior``).
The reference has no such class; the construction is the sliced-Wasserstein auto-encoder's: project latents and prior
draws on L random unit directions, sort each projection, match by rank.

    theta_l = g_l / |g_l|,  p = z theta^T,  q = y theta^T                              [N, L] each
    SW(z, y) = 1 / (L N) sum_l sum_k (p_l,(k) - q_l,(k))^2                              ties: the smaller original row first
    d SW / d z_i = 2 / (L N) sum_l (p_l,i - q_l,(rank_l(i))) theta_l                    exact: the matching is piecewise constant

No regulariser, no iteration count, no starvation mode, any N against D."""
from typing import Optional

import torch
from torch import Tensor

from .base import Prior

__all__ = ["SlicedWassersteinPrior"]


class _SlicedLossFn(torch.autograd.Function):
    """Forward = ``torch.ops.otvae.sliced_w2`` -> ``otvae_sliced_w2_fwd`` (projection, per-projection sort-and-match in LDS, residuals
    in original row order, fixed-order loss), backward = ``otvae_sliced_w2_bwd`` (residuals x directions on the matrix cores): no
    library GEMM, no library sort and no ATen kernel on either side."""

    @staticmethod
    def forward(ctx, z, y, dirs, scale):
        from ..functional import PriorLane
        ctx.lane = PriorLane.active(z.device)
        if ctx.lane:  # beside the decoder, on the prior lane of a training engine's step (functional.PriorLane)
            PriorLane.hold(z.device, z, y, dirs)
            with PriorLane.section(z.device):
                loss, resid, theta = torch.ops.otvae.sliced_w2(z, y, dirs, float(scale))
        else:
            loss, resid, theta = torch.ops.otvae.sliced_w2(z, y, dirs, float(scale))
        ctx.save_for_backward(resid, theta)
        ctx.scale = float(scale)
        ctx.set_materialize_grads(False)
        # the latents leave through this node too (an alias of z, see prior/sinkhorn.py): the gradient the decoder sends back is added
        # inside otvae_sliced_w2_bwd instead of by an autograd accumulation kernel
        return z.view_as(z), loss

    @staticmethod
    def backward(ctx, gz_out, g):
        resid, theta = ctx.saved_tensors
        if ctx.lane:
            from ..functional import PriorLane
            PriorLane.join(resid.device)  # the residuals (and the loss vector behind them) are complete from here on
        if g is None:  # only the latents were used downstream
            return gz_out, None, None, None
        return torch.ops.otvae.sliced_w2_backward(g, gz_out, resid, theta, ctx.scale), None, None, None


class SlicedWassersteinPrior(Prior):
    """Deterministic encoder + sliced W2 between the minibatch of latents and as many N(0, I) draws.  ``forward`` returns
    (z, loss[B], artifacts) with loss[b] = loss_coeff x annealing x SW (identical for every b, so that the VAE's ``prior_loss.mean()``
    equals it); artifacts = {"prior_samples", "projections"}: the draws y [B, D] and the raw (un-normalised) directions g [L, D].

    Both come from the device-side counter-based generator under one key, on two stream ids, so every replay of a captured step draws
    fresh ones.  The loss is bit-reproducible for given inputs; a latent or draw that is not finite makes it NaN."""

    def __init__(self, n_projections: int = 128, loss_coeff: float = 1., annealing_steps: int = 0, seed: int = None):
        super().__init__(loss_coeff, annealing_steps)
        if isinstance(n_projections, bool) or not isinstance(n_projections, int) or n_projections < 1:
            raise ValueError(f"n_projections must be a positive integer, got {n_projections!r}")
        self.n_projections = n_projections
        self.seed = seed

    def out_size(self, size):
        return size

    def sample(self, shape, device) -> Tensor:
        return torch.randn(*shape, device=device)

    def _key(self, device) -> Tensor:
        from .. import functional as HF
        key = self.__dict__.get("_rng_key")
        if key is None or key.device != device:
            key = self.__dict__["_rng_key"] = HF.new_rng_key(device, self.seed)
        return key

    def forward(self, x: Tensor, step: int, prior_samples: Optional[Tensor] = None,
                projections: Optional[Tensor] = None) -> Prior.EncodingResults:
        # loss_coeff x annealing is folded into the loss kernel (and the backward's scale): no separate multiply
        return self.encode(x, prior_samples=prior_samples, projections=projections,
                           _scale=float(self.loss_coeff * self.annealing(step)))

    def encode(self, x: Tensor, prior_samples: Optional[Tensor] = None, projections: Optional[Tensor] = None,
               _scale: float = 1.0) -> Prior.EncodingResults:
        from .. import _lib
        from .. import functional as HF
        z = x
        zf = z.flatten(1)
        n, d = zf.shape
        if prior_samples is not None and (prior_samples.dim() < 2 or tuple(prior_samples.flatten(1).shape) != (n, d)):
            raise ValueError(f"prior_samples are {tuple(prior_samples.shape)}, the latents flatten to {(n, d)}: the sliced distance "
                             "matches sorted projections one to one")
        if projections is not None and (projections.dim() != 2 or projections.shape[1] != d or projections.shape[0] < 1):
            raise ValueError(f"projections are {tuple(projections.shape)}, expected [L, {d}]")
        if zf.dtype != torch.float32:
            raise NotImplementedError(f"SlicedWassersteinPrior computes in float32, got {zf.dtype} latents")
        _lib.require_cuda(zf, "latents")
        if prior_samples is None:
            prior_samples = HF.normal_like(zf, self._key(zf.device), stream_id=1)
        if projections is None:
            projections = HF.normal_fill_(torch.empty((self.n_projections, d), device=zf.device, dtype=torch.float32),
                                          self._key(zf.device), stream_id=2)
        z_out, loss = _SlicedLossFn.apply(zf, prior_samples.flatten(1), projections, _scale)
        return z_out.view(z.shape), loss, {"prior_samples": prior_samples, "projections": projections}
