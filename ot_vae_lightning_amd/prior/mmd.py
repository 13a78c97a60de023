"""Kernel two-sample (maximum mean discrepancy) prior: the WAE-MMD / InfoVAE regulariser beside the minibatch optimal-transport priors
(``SinkhornPrior``, ``GaussianW2Prior``, ``SlicedWassersteinPrior``).  The reference has no such class.

    r(a, b) = |a - b|^2,   C_k = 2 D sigma2 s_k   for the scales s_k
    imq:  k(r) = sum_k C_k / (C_k + r)            rbf:  k(r) = sum_k exp(-r / C_k)
    MMD2 = 1/(N(N-1)) sum_{i != j} k(r(z_i, z_j)) + 1/(M(M-1)) sum_{i != j} k(r(y_i, y_j)) - 2/(N M) sum_{i, j} k(r(z_i, y_j))
    (unbiased=False: 1/N^2, 1/M^2 and the diagonal k(0) in the sums)

No iteration, no sort, any N against any M, nothing of size N x M in memory.

Forward = ``torch.ops.otvae.mmd_prior`` -> ``otvae_mmd_fwd`` (Gram tile, kernel function and gradient product in one launch, fixed-order
finish), backward = ``otvae_mmd_bwd`` (one element-wise launch that also adds the decoder's gradient): no library GEMM and no ATen
kernel on either side."""
from typing import Optional, Sequence

import torch
from torch import Tensor

from .base import MinibatchPrior, Prior, _LatentLossFn

__all__ = ["MMDPrior"]

DEFAULT_SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


class MMDPrior(MinibatchPrior):
    """Deterministic encoder + MMD2 between the minibatch of latents and M draws of N(0, sigma2 I).  ``forward`` returns
    (z, loss[B], artifacts) with loss[b] = loss_coeff x annealing x MMD2 (identical for every b, so that the VAE's ``prior_loss.mean()``
    equals it; MMD2 of the unbiased estimator may be negative); artifacts = {"prior_samples", "mmd_terms"}: the draws y [M, D] and
    (Ezz, Eyy, Ezy), unscaled.

    The draws come from the device-side counter-based generator, so every replay of a captured step draws fresh ones;
    ``prior_samples`` handed in may have any M.  The loss is bit-reproducible for given inputs; a latent or draw that is not finite
    makes it NaN."""

    def __init__(self, kernel: str = "imq", scales: Sequence[float] = DEFAULT_SCALES, sigma2: float = 1.0, unbiased: bool = True,
                 loss_coeff: float = 1., annealing_steps: int = 0, seed: int = None):
        super().__init__(loss_coeff, annealing_steps)
        from .. import ops
        ops.mmd_kernel_id(kernel)
        self.kernel = kernel
        self.scales = ops.mmd_check_config(scales, sigma2)
        self.sigma2 = float(sigma2)
        self.unbiased = bool(unbiased)
        self.seed = seed

    def sample(self, shape, device) -> Tensor:
        return torch.randn(*shape, device=device) * self.sigma2 ** 0.5

    def forward(self, x: Tensor, step: int, prior_samples: Optional[Tensor] = None) -> Prior.EncodingResults:
        return super().forward(x, step, prior_samples=prior_samples)

    def encode(self, x: Tensor, prior_samples: Optional[Tensor] = None, _scale: float = 1.0) -> Prior.EncodingResults:
        from .. import _lib, ops
        from .. import functional as HF
        z = x
        if z.dim() < 2:
            raise ValueError(f"MMDPrior takes latents [B, ...], got {tuple(z.shape)}")
        zf = z.flatten(1)
        if prior_samples is not None and prior_samples.dim() < 2:
            raise ValueError(f"prior_samples are {tuple(prior_samples.shape)}, expected [M, {zf.shape[1]}]")
        ys = prior_samples.flatten(1) if prior_samples is not None else None
        ops.mmd_check_inputs(zf, ys if ys is not None else zf, self.unbiased)
        if zf.shape[1] > ops.MMD_MAX_D:
            raise NotImplementedError(f"MMDPrior is built for latents of 1 <= D <= {ops.MMD_MAX_D} entries, got D = {zf.shape[1]}")
        _lib.require_cuda(zf, "latents")
        if prior_samples is None:
            prior_samples = ys = HF.normal_like(zf, self._key(zf.device), stream_id=1)
            if self.sigma2 != 1.0:   # N(0, sigma2 I): the draws scaled by the library's own kernel
                e, prior_samples = ys, torch.empty_like(ys)
                _lib.check(_lib.load().otvae_scale_f32(_lib.ptr(e), self.sigma2 ** 0.5, e.numel(), _lib.ptr(prior_samples),
                                                       _lib.stream()), "otvae_scale_f32")
                ys = prior_samples
        cfg = (ops.MMD_KERNELS[self.kernel], list(self.scales), self.sigma2, self.unbiased)
        need_grad = bool(torch.is_grad_enabled() and zf.requires_grad)   # validation / no_grad: the gradient product is skipped

        def run():
            loss, G, terms = torch.ops.otvae.mmd_prior(zf, ys, *cfg, float(_scale), need_grad)
            return loss, (G,), (terms,)

        z_out, loss, terms = _LatentLossFn.apply(zf, run, torch.ops.otvae.mmd_prior_backward, ys)
        return z_out.view(z.shape), loss, {"prior_samples": prior_samples, "mmd_terms": terms}
