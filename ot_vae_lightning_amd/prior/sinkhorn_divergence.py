"""Sinkhorn-divergence prior: the debiased form of ``SinkhornPrior``'s loss (Genevay, Peyre, Cuturi 2018), beside the other minibatch
priors (``SinkhornPrior``, ``GaussianW2Prior``, ``SlicedWassersteinPrior``, ``MMDPrior``).  The reference has no such class.

    S(z, y) = W(z, y) - W(z, z) / 2 - W(y, y) / 2,   W(p, q) = sum_ij C_pq,ij pi_pq,ij,   C_pq,ij = |p_i - q_j|^2
    pi_pq the (detached) entropic plan of C_pq / max C_zy with uniform marginals: ONE absolute epsilon for the three problems
    d S / d z_i = 2 sum_j pi_zy,ij (z_i - y_j) - sum_j (pi_zz,ij + pi_zz,ji) (z_i - z_j)      envelope form: the plans are constants

``SinkhornPrior`` minimises the raw entropic cost W(z, y), whose minimiser is a shrunken copy of the prior; the two self terms remove that
bias, and S(z, z) = 0.  The effect is large at moderate latent widths and larger ``reg``; at D = 128 and reg = 0.05 the plans are almost
permutations and the two losses nearly coincide (README.md).

Forward = ``torch.ops.otvae.sinkhorn_divergence`` -> ``otvae_sinkhorn_div_fwd`` (all three cost matrices from one launch, the solver of
``sinkhorn_log`` on the batch of three, the read-out), backward = ``otvae_sinkhorn_div_grad`` (one launch on the matrix cores): no library
GEMM and no ATen kernel on either side."""
from typing import Optional

import torch
from torch import Tensor

from ..ot import w2_utils as W
from .base import MinibatchPrior, Prior, _LatentLossFn

__all__ = ["SinkhornDivergencePrior"]


class SinkhornDivergencePrior(MinibatchPrior):
    """Deterministic encoder + Sinkhorn divergence between the minibatch of latents and M draws of N(0, I).  ``forward`` returns
    (z, loss[B], artifacts) with loss[b] = loss_coeff x annealing x S(z, y) (identical for every b, so that the VAE's
    ``prior_loss.mean()`` equals it); artifacts = {"prior_samples", "terms"}: the draws y [M, D] and (W(z, y), W(z, z), W(y, y)) in
    float64, unscaled.

    There is no ``threshold``: the three solves run exactly ``max_iter`` iterations each, because the bias terms cancel only between
    plans of the same iteration count.  The draws come from the device-side counter-based generator, so every replay of a captured
    step draws fresh ones; ``prior_samples`` handed in may have any M.  A latent or draw that is not finite makes the loss NaN."""

    def __init__(self, reg: float = 0.05, max_iter: int = 50, loss_coeff: float = 1., annealing_steps: int = 0, seed: int = None):
        super().__init__(loss_coeff, annealing_steps)
        if not float(reg) > 0:
            raise ValueError(f"sinkhorn_divergence: reg must be positive, got {reg!r}")
        if int(max_iter) < 0:
            raise ValueError(f"sinkhorn_divergence: max_iter must not be negative, got {max_iter!r}")
        self.reg, self.max_iter = reg, max_iter
        self.seed = seed
        self.last_iters = None  # device int32: iterations of the last solves (-1: a solver was starved, the loss is NaN)

    def raise_if_starved(self) -> None:
        """Host check of the last forward (one device read): raises ``SinkhornSolverStarved`` if a single-launch solve gave up
        waiting for its other workgroups.  The training step itself never synchronises for this: a starved solve makes the loss NaN."""
        if self.last_iters is not None:
            W.raise_if_solver_starved(self.last_iters)

    def _draw(self, like: Tensor) -> Tensor:
        """prior samples N(0, I) from the device-side counter-based generator (``SinkhornPrior._draw``)"""
        from .. import functional as HF
        return HF.normal_like(like, self._key(like.device), stream_id=1)

    def forward(self, x: Tensor, step: int, prior_samples: Optional[Tensor] = None) -> Prior.EncodingResults:
        return super().forward(x, step, prior_samples=prior_samples)

    def encode(self, x: Tensor, prior_samples: Optional[Tensor] = None, _scale: float = 1.0) -> Prior.EncodingResults:
        from .. import ops
        z = x
        if z.dim() < 2:
            raise ValueError(f"SinkhornDivergencePrior takes latents [B, ...], got {tuple(z.shape)}")
        zf = z.flatten(1)
        if prior_samples is not None and prior_samples.dim() < 2:
            raise ValueError(f"prior_samples are {tuple(prior_samples.shape)}, expected [M, {zf.shape[1]}]")
        ops.sinkhorn_div_check(zf, prior_samples.flatten(1) if prior_samples is not None else zf, self.reg, self.max_iter)
        if prior_samples is None:
            prior_samples = self._draw(zf) if zf.dtype == torch.float32 else torch.randn_like(zf)
        y = prior_samples.flatten(1)
        cfg, scale = (float(self.reg), int(self.max_iter)), float(_scale)

        def run():
            loss, terms, pi_zy, pi_zz, iters = torch.ops.otvae.sinkhorn_divergence(zf, y, *cfg, scale)
            return loss, (zf, y, pi_zy, pi_zz), (terms, iters)

        z_out, loss, terms, self.last_iters = _LatentLossFn.apply(
            zf, run, lambda g, gadd, z_, y_, pzy, pzz: torch.ops.otvae.sinkhorn_divergence_backward(g, gadd, z_, y_, pzy, pzz, scale), y)
        return z_out.view(z.shape), loss, {"prior_samples": prior_samples, "terms": terms}
