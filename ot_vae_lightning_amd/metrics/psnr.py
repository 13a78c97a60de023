"""``PeakSignalNoiseRatio``: 10 log_base(range^2 / mse) over everything seen since ``reset()`` -- the monitored key of the
reference's default run (``configs/vae/defaults.yaml``: ``psnr``; ``VAE(monitor="psnr", mode="max")``)."""
import math
from typing import Optional

import torch
from torch import Tensor

from .base import Metric

__all__ = ["PeakSignalNoiseRatio"]

# layout of the device state (include/otvae.h, otvae_sqerr_accum): the four accumulators, then the kernel's reduction scratch
_SSE, _COUNT, _MIN, _MAX, _HEAD = 0, 1, 2, 3, 4
_STATE_WORDS = 4 + 3 * 256   # otvae_sqerr_state_words(); checked against the library at the first update


class PeakSignalNoiseRatio(Metric):
    """``update(preds, target)`` is one pass of ``otvae_sqerr_accum`` over both tensors: sum of squared differences (fp64), element
    count and the target's running minimum / maximum, all on the device.  ``data_range=None`` takes the range from the targets seen
    (max - min, as torchmetrics does); ``compute()`` returns a 0-d float64 tensor, ``inf`` for identical tensors."""
    higher_is_better = True

    def __init__(self, data_range: Optional[float] = None, base: float = 10.0, **metric_kwargs):
        super().__init__(**metric_kwargs)
        self.data_range = None if data_range is None else float(data_range)
        self.base = float(base)
        default = torch.zeros(_STATE_WORDS, dtype=torch.float64)
        default[_MIN], default[_MAX] = math.inf, -math.inf
        self.add_state("sqerr_state", default, dist_reduce_fx=[(_SSE, _COUNT + 1, "sum"), (_MIN, _MIN + 1, "min"), (_MAX, _MAX + 1, "max")])

    # torchmetrics' state names, as views of the one buffer the kernel writes
    @property
    def sum_squared_error(self) -> Tensor:
        return self.sqerr_state[_SSE]

    @property
    def total(self) -> Tensor:
        return self.sqerr_state[_COUNT]

    @property
    def min_target(self) -> Tensor:
        return self.sqerr_state[_MIN]

    @property
    def max_target(self) -> Tensor:
        return self.sqerr_state[_MAX]

    def update(self, preds: Tensor, target: Tensor) -> None:
        if preds.dtype not in (torch.float32, torch.float64):
            preds = preds.float()
        torch.ops.otvae.sqerr_accum(preds.detach(), target.detach(), self.sqerr_state)

    def compute(self) -> Tensor:
        s = self.sqerr_state
        rng = (s[_MAX] - s[_MIN]) if self.data_range is None else torch.as_tensor(self.data_range, dtype=s.dtype, device=s.device)
        mse = s[_SSE] / s[_COUNT]
        return (10.0 / math.log(self.base)) * torch.log(rng * rng / mse)
