"""Sliced Wasserstein-2 prior: the third member of the minibatch optimal-transport family (``SinkhornPrior``, ``GaussianW2Prior``).
The reference has no such class; the construction is the sliced-Wasserstein auto-encoder's: project latents and prior
draws on L random unit directions, sort each projection, match by rank.

    theta_l = g_l / |g_l|,  p = z theta^T,  q = y theta^T                              [N, L] each
    SW(z, y) = 1 / (L N) sum_l sum_k (p_l,(k) - q_l,(k))^2                              ties: the smaller original row first
    d SW / d z_i = 2 / (L N) sum_l (p_l,i - q_l,(rank_l(i))) theta_l                    exact: the matching is piecewise constant

No regulariser, no iteration count, no starvation mode, any N against D.

Forward = ``torch.ops.otvae.sliced_w2`` -> ``otvae_sliced_w2_fwd`` (projection, per-projection sort-and-match in LDS, residuals in
original row order, fixed-order loss), backward = ``otvae_sliced_w2_bwd`` (residuals x directions on the matrix cores): no library
GEMM, no library sort and no ATen kernel on either side."""
from typing import Optional

import torch
from torch import Tensor

from .base import MinibatchPrior, Prior, _LatentLossFn

__all__ = ["SlicedWassersteinPrior"]


class SlicedWassersteinPrior(MinibatchPrior):
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

    def forward(self, x: Tensor, step: int, prior_samples: Optional[Tensor] = None,
                projections: Optional[Tensor] = None) -> Prior.EncodingResults:
        return super().forward(x, step, prior_samples=prior_samples, projections=projections)

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
        y, scale = prior_samples.flatten(1), float(_scale)

        def run():
            loss, resid, theta = torch.ops.otvae.sliced_w2(zf, y, projections, scale)
            return loss, (resid, theta), ()

        z_out, loss = _LatentLossFn.apply(
            zf, run, lambda g, gadd, resid, theta: torch.ops.otvae.sliced_w2_backward(g, gadd, resid, theta, scale), y, projections)
        return z_out.view(z.shape), loss, {"prior_samples": prior_samples, "projections": projections}
