"""``SSIMLoss`` / ``ssim_loss``: ``1 - SSIM`` per image as a training loss -- the structural term that takes the blur off an MSE-only
reconstruction loss (``VAE(..., ssim_loss=SSIMLoss(data_range=1.0))``: ``recon = mse + ssim_weight (1 - SSIM)``).

The forward is the metric's kernel (``otvae_ssim_accum``, ``csrc/ssim.hip``: the values have the bits of
``metrics.structural_similarity``), the backward one launch of ``otvae_ssim_grad`` (``csrc/ssim_grad.hip``) per image that wants a
gradient; both behind ``torch.ops.otvae.ssim_loss``.  Options, their checks and the windows are ``metrics.ssim._Options``.

``MSSSIMLoss`` / ``ms_ssim_loss``: ``1 - MS-SSIM`` per image, the same way: the forward is ``otvae_ms_ssim_accum`` (``csrc/ssim.hip``: the
bits of ``metrics.multiscale_structural_similarity``), which keeps the pooled pyramid and the scale weights, the backward one launch
of ``otvae_ms_ssim_grad`` (``csrc/ssim_grad.hip``, the SSIM gradient's tile kernel) per scale, coarsest first; both behind ``torch.ops.otvae.ms_ssim``.  ``losses.__all__`` is the pair of names the
module began with (``tests/test_ssim_loss_host.py`` holds it to exactly that); the package exports the two new names itself."""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import ops as _ops  # noqa: F401  (registers torch.ops.otvae.*)
from .metrics.ms_ssim import DEFAULT_BETAS, _MSOptions
from .metrics.ssim import _RANGE_BATCH, _Options, _Pair

__all__ = ["SSIMLoss", "ssim_loss"]

_REDUCTIONS = ("mean", "sum", "none")


def _options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, reduction) -> _Options:
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    options = _Options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2)
    if options.range_mode == _RANGE_BATCH:
        raise ValueError("SSIMLoss needs data_range as a value or a pair (low, high): with data_range=None the range comes from each "
                         "batch, so the constants c1, c2 would depend on the data and the loss would have no fixed scale")
    return options


def _loss(options: _Options, reduction: str, preds: Tensor, target: Tensor) -> Tensor:
    out_dtype = preds.dtype if preds.dtype in (torch.float32, torch.float64) else torch.float32
    preds, target = options.prepare(preds, target, detach=False)
    ssim = torch.ops.otvae.ssim_loss(preds, target, options.window[0], options.window[1], options.k1, options.k2, options.range_mode,
                                     options.range_lo, options.range_hi)
    loss = (1.0 - ssim).to(out_dtype)   # [B]; the kernel's float64 cast down, so that it adds to a float32 loss vector
    if reduction == "mean":
        return loss.mean()
    return loss.sum() if reduction == "sum" else loss


class SSIMLoss(nn.Module):
    """``forward(preds, target)``: ``1 - ssim_b`` of the ``[B, C, H, W]`` pairs, reduced by ``"mean"``, ``"sum"`` or ``"none"`` (``[B]``), in
    ``preds.dtype``.  Differentiable once for ``preds`` and for ``target``.  ``data_range`` is a value ``R`` or a pair ``(low, high)`` that
    both images are clamped to first (the gradient is zero where a pixel lies strictly outside it); ``None`` is refused.  Windows of up
    to 15 taps per axis (``sigma <= 2``).  No parameters, no buffers: ``state_dict()`` is empty."""

    def __init__(self, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11, data_range=1.0, k1: float = 0.01,
                 k2: float = 0.03, reduction: str = "mean"):
        super().__init__()
        self.options = _options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, reduction)
        self.reduction = reduction

    @property
    def window_size(self) -> Tuple[int, int]:
        return self.options.window_size

    def forward(self, preds: Tensor, target: Tensor) -> Tensor:
        return _loss(self.options, self.reduction, preds, target)

    def extra_repr(self) -> str:
        o = self.options
        return f"window={o.window_size}, data_range={o.data_range!r}, k1={o.k1}, k2={o.k2}, reduction={self.reduction!r}"


def ssim_loss(preds: Tensor, target: Tensor, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11, data_range=1.0,
              k1: float = 0.01, k2: float = 0.03, reduction: str = "mean") -> Tensor:
    """the functional form of ``SSIMLoss``"""
    return _loss(_options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, reduction), reduction, preds, target)


def _ms_options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas, normalize, reduction) -> _MSOptions:
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    options = _MSOptions(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas, normalize)
    if options.range_mode == _RANGE_BATCH:
        raise ValueError("MSSSIMLoss needs data_range as a value or a pair (low, high): with data_range=None the range comes from each "
                         "batch, so the constants c1, c2 would depend on the data and the loss would have no fixed scale")
    return options


def _ms_loss(options: _MSOptions, reduction: str, preds: Tensor, target: Tensor) -> Tensor:
    out_dtype = preds.dtype if preds.dtype in (torch.float32, torch.float64) else torch.float32
    preds, target = options.prepare(preds, target, detach=False)
    msssim, _, _ = torch.ops.otvae.ms_ssim(preds, target, options.window[0], options.window[1], options.k1, options.k2, options.range_mode,
                                           options.range_lo, options.range_hi, options.betas, options.normalize_mode)
    loss = (1.0 - msssim).to(out_dtype)   # [B]; the kernel's float64 cast down, so that it adds to a float32 loss vector
    if reduction == "mean":
        return loss.mean()
    return loss.sum() if reduction == "sum" else loss


class MSSSIMLoss(nn.Module):
    """``forward(preds, target)``: ``1 - msssim_b`` of the ``[B, C, H, W]`` pairs (``metrics.multiscale_structural_similarity``), reduced by
    ``"mean"``, ``"sum"`` or ``"none"`` (``[B]``), in ``preds.dtype``.  Differentiable once for ``preds`` and for ``target``.  ``data_range`` is a
    value ``R`` or a pair ``(low, high)`` that each scale's images are clamped to (a scale's own gradient term is zero where its pixel lies
    strictly outside it; what arrives from the coarser scales passes, the pooling having taken the unclamped values); ``None`` is
    refused.  Windows of up to 15 taps per axis (``sigma <= 2``), up to 8 scales, and every scale must hold one window.

    A dead image passes no gradient: under ``normalize="relu"`` an image one of whose scale means ``v_s`` is not positive has
    ``msssim_b = 0`` and a gradient of exactly zero everywhere (likewise ``"simple"`` at ``v_s = -1``).  Autograd of the composed formula
    meets ``0 * inf`` there (``d x^beta / dx`` at 0) and returns NaN or 0 depending on how the derivative of ``relu`` is written; here the
    zero is the rule.

    No parameters, no buffers: ``state_dict()`` is empty."""

    def __init__(self, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11, data_range=1.0, k1: float = 0.01,
                 k2: float = 0.03, betas: Tuple[float, ...] = DEFAULT_BETAS, normalize: Optional[str] = "relu", reduction: str = "mean"):
        super().__init__()
        self.options = _ms_options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas, normalize, reduction)
        self.reduction = reduction

    @property
    def window_size(self) -> Tuple[int, int]:
        return self.options.window_size

    def forward(self, preds: Tensor, target: Tensor) -> Tensor:
        return _ms_loss(self.options, self.reduction, preds, target)

    def extra_repr(self) -> str:
        o = self.options
        return (f"window={o.window_size}, betas={o.betas}, normalize={o.normalize!r}, data_range={o.data_range!r}, k1={o.k1}, k2={o.k2}, "
                f"reduction={self.reduction!r}")


def ms_ssim_loss(preds: Tensor, target: Tensor, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11, data_range=1.0,
                 k1: float = 0.01, k2: float = 0.03, betas: Tuple[float, ...] = DEFAULT_BETAS, normalize: Optional[str] = "relu",
                 reduction: str = "mean") -> Tensor:
    """the functional form of ``MSSSIMLoss``"""
    return _ms_loss(_ms_options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas, normalize, reduction), reduction, preds,
                    target)
