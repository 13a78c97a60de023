"""``StructuralSimilarityIndexMeasure`` and ``structural_similarity``: torchmetrics' SSIM over everything seen since ``reset()``, one
pass of ``otvae_ssim_accum`` (``csrc/ssim.hip``) over each image pair.

torchmetrics reflect-pads by ``k // 2``, convolves and crops ``k // 2`` off again: what is left are exactly the positions whose
window never touched the padding, so nothing is padded here and only those ``(H - kh + 1) (W - kw + 1)`` positions are evaluated."""
import math
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from .base import Metric

__all__ = ["StructuralSimilarityIndexMeasure", "structural_similarity"]

# layout of the device state (include/otvae.h, otvae_ssim_accum): the two accumulators, then the range pass's scratch
_SUM, _COUNT = 0, 1
_STATE_WORDS = 4 + 4 * 256   # otvae_ssim_state_words(); the operator checks it against the library
_RANGE_FIXED, _RANGE_CLAMP, _RANGE_BATCH = 0, 1, 2   # otvae_ssim_accum's range_mode

_Pair = Union[float, Sequence[float]]


def _pair(value, name: str) -> Tuple:
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(f"{name} must be one value or a pair (h, w), got {value!r}")
        return tuple(value)
    return (value, value)


def gaussian_window(sigma: float) -> list:
    """``g[i] = exp(-((i - (k - 1) / 2) / sigma)^2 / 2)`` over ``k = 2 int(3.5 sigma + 0.5) + 1`` taps, normalised to sum 1 (float64)"""
    k = 2 * int(3.5 * sigma + 0.5) + 1
    g = [math.exp(-(((i - (k - 1) / 2) / sigma) ** 2) / 2) for i in range(k)]
    total = math.fsum(g)
    return [v / total for v in g]


class _Options:
    """the options ``StructuralSimilarityIndexMeasure`` and ``structural_similarity`` share, checked once"""

    def __init__(self, gaussian_kernel: bool, sigma: _Pair, kernel_size, data_range, k1: float, k2: float,
                 return_full_image: bool = False, return_contrast_sensitivity: bool = False):
        if return_full_image or return_contrast_sensitivity:
            raise ValueError("return_full_image / return_contrast_sensitivity are not available: the map is reduced inside the kernel "
                             "and never stored")
        sigma, kernel_size = _pair(sigma, "sigma"), _pair(kernel_size, "kernel_size")
        if any(not (float(s) > 0) for s in sigma):
            raise ValueError(f"sigma must be positive, got {sigma}")
        if any(int(k) != k or k <= 0 or k % 2 == 0 for k in kernel_size):
            raise ValueError(f"kernel_size must be odd and positive, got {kernel_size}")
        if k1 < 0 or k2 < 0:
            raise ValueError(f"k1 and k2 must not be negative, got {k1}, {k2}")
        self.gaussian_kernel = bool(gaussian_kernel)
        self.sigma = tuple(float(s) for s in sigma)
        self.kernel_size = tuple(int(k) for k in kernel_size)
        self.k1, self.k2 = float(k1), float(k2)
        if self.gaussian_kernel:     # kernel_size is ignored, as in torchmetrics
            self.window = tuple(gaussian_window(s) for s in self.sigma)
        else:
            self.window = tuple([1.0 / k] * k for k in self.kernel_size)
        self.data_range = data_range
        if data_range is None:
            self.range_mode, self.range_lo, self.range_hi = _RANGE_BATCH, 0.0, 0.0
        elif isinstance(data_range, (tuple, list)):
            if len(data_range) != 2 or not float(data_range[1]) > float(data_range[0]):
                raise ValueError(f"data_range must be a value or a pair (low, high) with high > low, got {data_range!r}")
            self.range_mode, self.range_lo, self.range_hi = _RANGE_CLAMP, float(data_range[0]), float(data_range[1])
        else:
            if not float(data_range) > 0:
                raise ValueError(f"data_range must be positive, got {data_range!r}")
            self.range_mode, self.range_lo, self.range_hi = _RANGE_FIXED, 0.0, float(data_range)

    @property
    def window_size(self) -> Tuple[int, int]:
        return len(self.window[0]), len(self.window[1])

    def prepare(self, preds: Tensor, target: Tensor, detach: bool = True) -> Tuple[Tensor, Tensor]:
        """shape checks, then both images as contiguous float32 / float64; ``detach=False`` (``losses.SSIMLoss``) keeps them in the graph"""
        if preds.dim() != 4 or target.dim() != 4:
            raise ValueError(f"SSIM takes [B, C, H, W] images, got {tuple(preds.shape)} and {tuple(target.shape)}")
        if preds.shape != target.shape:
            raise ValueError(f"preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
        kh, kw = self.window_size
        if preds.shape[2] < kh or preds.shape[3] < kw:
            raise ValueError(f"{preds.shape[2]} x {preds.shape[3]} images are smaller than the {kh} x {kw} window")
        if preds.dtype not in (torch.float32, torch.float64):
            preds = preds.float()
        if detach:
            preds, target = preds.detach(), target.detach()
        return preds.contiguous(), target.to(preds.dtype).contiguous()

    def accumulate(self, preds: Tensor, target: Tensor, state: Tensor, per_image: Optional[Tensor]) -> None:
        torch.ops.otvae.ssim_accum(preds, target, self.window[0], self.window[1], self.k1, self.k2, self.range_mode, self.range_lo,
                                   self.range_hi, state, per_image)


class StructuralSimilarityIndexMeasure(Metric):
    """``update(preds, target)`` reads each ``[B, C, H, W]`` pair once: the five window moments are formed in LDS, the map is evaluated
    and summed per image in fp64, all on the device.  ``data_range=None`` takes the range from THAT call's batch (torchmetrics' rule
    for SSIM; ``PeakSignalNoiseRatio`` tracks a running range instead), ``(low, high)`` clamps both inputs first.  ``compute()``
    returns a 0-d float64 tensor: the mean (``"elementwise_mean"``) or the sum (``"sum"``) of the per-image values."""
    higher_is_better = True

    def __init__(self, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11, reduction: Optional[str] = "elementwise_mean",
                 data_range=None, k1: float = 0.01, k2: float = 0.03, return_full_image: bool = False,
                 return_contrast_sensitivity: bool = False, **metric_kwargs):
        super().__init__(**metric_kwargs)
        if reduction in ("none", None):
            raise ValueError("reduction='none' keeps no running state: call structural_similarity(preds, target, ...) for the per-image "
                             "values")
        if reduction not in ("elementwise_mean", "sum"):
            raise ValueError(f"reduction must be 'elementwise_mean' or 'sum', got {reduction!r}")
        self.reduction = reduction
        self.options = _Options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, return_full_image, return_contrast_sensitivity)
        self.add_state("ssim_state", torch.zeros(_STATE_WORDS, dtype=torch.float64), dist_reduce_fx=[(_SUM, _COUNT + 1, "sum")])

    # torchmetrics' state names, as views of the one buffer the kernel writes
    @property
    def similarity(self) -> Tensor:
        return self.ssim_state[_SUM]

    @property
    def total(self) -> Tensor:
        return self.ssim_state[_COUNT]

    @property
    def window_size(self) -> Tuple[int, int]:
        return self.options.window_size

    def update(self, preds: Tensor, target: Tensor) -> None:
        preds, target = self.options.prepare(preds, target)
        self.options.accumulate(preds, target, self.ssim_state, None)

    def compute(self) -> Tensor:
        s = self.ssim_state
        return s[_SUM] / s[_COUNT] if self.reduction == "elementwise_mean" else s[_SUM].clone()


def structural_similarity(preds: Tensor, target: Tensor, gaussian_kernel: bool = True, sigma: _Pair = 1.5, kernel_size=11,
                          data_range=None, k1: float = 0.01, k2: float = 0.03, return_full_image: bool = False,
                          return_contrast_sensitivity: bool = False) -> Tensor:
    """the per-image values ``[B]`` (float64) of one batch, by the same kernel; no state is kept"""
    options = _Options(gaussian_kernel, sigma, kernel_size, data_range, k1, k2, return_full_image, return_contrast_sensitivity)
    preds, target = options.prepare(preds, target)
    state = torch.zeros(_STATE_WORDS, dtype=torch.float64, device=preds.device)
    per_image = torch.empty(preds.shape[0], dtype=torch.float64, device=preds.device)
    options.accumulate(preds, target, state, per_image)
    return per_image
