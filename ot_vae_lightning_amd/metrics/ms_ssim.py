"""``MultiScaleStructuralSimilarityIndexMeasure`` and ``multiscale_structural_similarity``: torchmetrics' MS-SSIM over everything seen
since ``reset()``, by ``otvae_ms_ssim_accum`` (``csrc/ssim.hip``): one launch per scale that reads the scale's pair once, reduces the
contrast term and the full map and writes the 2 x 2 pooled pair of the next scale, then one fold over all scales.

As for SSIM, only the positions whose window lies inside the image are evaluated (what torchmetrics keeps after its reflect padding
and crop).  Every scale must hold one window: ``H >> (S - 1) >= kh`` and ``W >> (S - 1) >= kw`` (torchmetrics' ``(S - 1)^2`` heuristic
is not reproduced)."""
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .base import Metric
from .ssim import _COUNT, _STATE_WORDS, _SUM, _Options, _Pair

__all__ = ["MultiScaleStructuralSimilarityIndexMeasure", "multiscale_structural_similarity"]

DEFAULT_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_NORMALIZE = {None: 0, "relu": 1, "simple": 2}   # otvae_ms_ssim_accum's normalize


class _MSOptions(_Options):
    """``_Options`` (window, range) and the two multi-scale options, checked once"""

    def __init__(self, gaussian_kernel: bool, sigma: _Pair, kernel_size, data_range, k1: float, k2: float, betas: Sequence[float],
                 normalize: Optional[str]):
        super().__init__(gaussian_kernel, sigma, kernel_size, data_range, k1, k2)
        if not isinstance(betas, tuple) or len(betas) == 0 or not all(isinstance(v, float) for v in betas):
            raise ValueError(f"betas must be a non-empty tuple of floats, got {betas!r}")
        if normalize not in _NORMALIZE:
            raise ValueError(f"normalize must be 'relu', 'simple' or None, got {normalize!r}")
        self.betas, self.normalize = betas, normalize
        self.normalize_mode = _NORMALIZE[normalize]

    def prepare(self, preds: Tensor, target: Tensor, detach: bool = True) -> Tuple[Tensor, Tensor]:
        preds, target = super().prepare(preds, target, detach)
        kh, kw = self.window_size
        scales = len(self.betas)
        h, w = preds.shape[2:]
        if (h >> (scales - 1)) < kh or (w >> (scales - 1)) < kw:
            raise ValueError(f"{h} x {w} images are too small for {scales} scales of the {kh} x {kw} window: every scale must hold one "
                             f"window, so the smallest admissible size is {kh << (scales - 1)} x {kw << (scales - 1)}")
        return preds, target

    def accumulate(self, preds: Tensor, target: Tensor, state: Tensor, per_image: Optional[Tensor]) -> None:
        torch.ops.otvae.ms_ssim_accum(preds, target, self.window[0], self.window[1], self.k1, self.k2, self.range_mode, self.range_lo,
                                      self.range_hi, self.betas, self.normalize_mode, state, per_image)


class MultiScaleStructuralSimilarityIndexMeasure(Metric):
    """``update(preds, target)``: ``msssim_b = prod_s f(v_s[b])^betas[s]`` of each ``[B, C, H, W]`` pair, where ``v_s`` is the mean contrast
    term of scale ``s`` (the mean SSIM at the last one), scale ``s + 1`` the 2 x 2 average pooling of scale ``s`` and ``f`` is ``relu``,
    ``(v + 1) / 2`` (``"simple"``) or the identity (``None``; a negative ``v_s`` then gives NaN, as in torch).  ``data_range=None`` takes the
    range per scale from that scale's images of that call; ``(low, high)`` clamps each scale's images, while the pooling always takes the
    unclamped values.  ``compute()`` returns a 0-d float64 tensor: the mean (``"elementwise_mean"``) or the sum (``"sum"``)."""
    higher_is_better = True

    def __init__(self, gaussian_kernel: bool = True, kernel_size=11, sigma: _Pair = 1.5, reduction: Optional[str] = "elementwise_mean",
                 data_range=None, k1: float = 0.01, k2: float = 0.03, betas: Tuple[float, ...] = DEFAULT_BETAS,
                 normalize: Optional[str] = "relu", **metric_kwargs):
        super().__init__(**metric_kwargs)
        if reduction in ("none", None):
            raise ValueError("reduction='none' keeps no running state: call multiscale_structural_similarity(preds, target, ...) for the "
                             "per-image values")
        if reduction not in ("elementwise_mean", "sum"):
            raise ValueError(f"reduction must be 'elementwise_mean' or 'sum', got {reduction!r}")
        self.reduction = reduction
        self.options = _MSOptions(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas, normalize)
        self.add_state("ms_ssim_state", torch.zeros(_STATE_WORDS, dtype=torch.float64), dist_reduce_fx=[(_SUM, _COUNT + 1, "sum")])

    # torchmetrics' state names, as views of the one buffer the kernel writes
    @property
    def similarity(self) -> Tensor:
        return self.ms_ssim_state[_SUM]

    @property
    def total(self) -> Tensor:
        return self.ms_ssim_state[_COUNT]

    @property
    def window_size(self) -> Tuple[int, int]:
        return self.options.window_size

    def update(self, preds: Tensor, target: Tensor) -> None:
        preds, target = self.options.prepare(preds, target)
        self.options.accumulate(preds, target, self.ms_ssim_state, None)

    def compute(self) -> Tensor:
        s = self.ms_ssim_state
        return s[_SUM] / s[_COUNT] if self.reduction == "elementwise_mean" else s[_SUM].clone()


def multiscale_structural_similarity(preds: Tensor, target: Tensor, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11,
                                     data_range=None, k1: float = 0.01, k2: float = 0.03, betas: Tuple[float, ...] = DEFAULT_BETAS,
                                     normalize: Optional[str] = "relu") -> Tensor:
    """the per-image values ``[B]`` (float64) of one batch, by the same kernels; no state is kept"""
    options = _MSOptions(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, betas, normalize)
    preds, target = options.prepare(preds, target)
    state = torch.zeros(_STATE_WORDS, dtype=torch.float64, device=preds.device)
    per_image = torch.empty(preds.shape[0], dtype=torch.float64, device=preds.device)
    options.accumulate(preds, target, state, per_image)
    return per_image
