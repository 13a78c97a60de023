"""What the feature-level metrics share.  ``ImageFeatureMixin`` (``FrechetInceptionDistance``, ``KernelInceptionDistance``,
``InceptionPrecisionRecall``): images -> features through a network that never trains (the reference's
``FrechetInceptionDistance._extract_features``, metrics/fid.py:99-111).  ``FeatureStore`` (``KernelDistance``, ``PrecisionRecall``): the
device-side append-only store of the features themselves, for the metrics that no running moment can stand in for."""
import warnings
from collections import OrderedDict
from typing import Any, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .base import Metric

__all__ = ["ImageFeatureMixin", "FeatureStore"]


def _default_inception(feature_size: int) -> nn.Module:
    valid = [64, 192, 768, 2048]
    if feature_size not in valid:
        raise ValueError(f"Integer input to argument `feature` must be one of {valid}, but got {feature_size}.")
    try:
        from torchmetrics.image.fid import NoTrainInceptionV3
    except ImportError as e:
        raise ImportError("FrechetInceptionDistance(net=None) builds torchmetrics' Inception-v3 feature extractor, and `torchmetrics` "
                          "(with torch-fidelity) is not importable here: install it, or pass a feature network of your own as `net=`") from e

    class NoTrainInceptionV3NoStateDict(NoTrainInceptionV3):   # the extractor's weights stay out of every checkpoint
        def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
            return destination if destination is not None else OrderedDict()

    return NoTrainInceptionV3NoStateDict(name="inception-v3-compat", features_list=[str(feature_size)])


class ImageFeatureMixin:
    """Mixed into a ``Metric`` in front of it.  ``_init_features`` after the metric's own ``__init__``; grey images are tiled to three
    channels, ``to_255`` maps ``data_range`` onto 0 ... 255 and casts to uint8, ``net`` turns them into features that are flattened to
    ``[B, feature_size]``.  ``net=None`` builds torchmetrics' Inception-v3 (``ImportError`` when that package is missing) and then
    converts to uint8 unless ``data_range`` already is (0, 255)."""

    def _init_features(self, net: Optional[nn.Module], feature_size: int, to_255: bool, data_range: Tuple[float, float]) -> None:
        self.data_range = data_range[1] - data_range[0]
        self.data_low = data_range[0]
        if net is None:
            self.net = _default_inception(feature_size)
            self.to_255 = tuple(data_range) != (0., 255.)
        else:
            self.net = net
            self.net.eval()
            self.to_255 = to_255

    def train(self, mode: bool = True):
        """the feature network never leaves evaluation mode (the model's ``.train()`` reaches the metrics it owns)"""
        super().train(mode)
        self.net.eval()
        return self

    def _extract_features(self, img: Tensor) -> Tensor:
        if img.size(1) == 1:
            img = torch.cat([img, img, img], dim=1)
        if self.to_255:
            img = (255 * (img - self.data_low) / self.data_range).type(torch.uint8)
        return self.net(img).reshape(img.shape[0], -1)


class FeatureStore(Metric):
    """Two sides, ``real`` and ``fake``.  Per side the states are ``*_features`` ``[max_observations, feature_size]`` float32 and
    ``num_*`` int64 ``[2]`` = (rows stored, rows seen); ``_append`` is one ``otvae::feature_append`` (float64 features are ROUNDED to
    float32, the offset is read on the device: it can be captured), rows beyond ``max_observations`` are dropped and
    ``_warn_dropped`` says so once.  Which ``update`` keyword feeds which side is the subclass's business."""
    _store_name = "FeatureStore"   # the class named in the dropped-rows warning

    def _init_store(self, feature_size: int, max_observations: int) -> None:
        self.feature_size, self.max_observations = feature_size, max_observations
        self._warned_dropped = False
        for side in ("real", "fake"):
            self.add_state(f"{side}_features", torch.zeros(max_observations, feature_size, dtype=torch.float32), dist_reduce_fx="sum")
            self.add_state(f"num_{side}", torch.zeros(2, dtype=torch.int64), dist_reduce_fx="sum")

    def reset(self) -> None:
        """the counts go to zero in place; the feature buffers keep their contents (rows beyond the count are never read) and, after a
        ``sync`` enlarged them, return to their own size"""
        for side in ("real", "fake"):
            getattr(self, f"num_{side}").zero_()
            buf = getattr(self, f"{side}_features")
            if buf.shape[0] != self.max_observations:
                setattr(self, f"{side}_features", buf[:self.max_observations].clone())

    def _append(self, feats: Tensor, side: str) -> None:
        feats = feats.detach().reshape(feats.shape[0], -1)
        if feats.shape[1] != self.feature_size:
            raise ValueError(f"features have width {feats.shape[1]}, the metric was built for {self.feature_size}")
        if feats.dtype not in (torch.float32, torch.float64):
            feats = feats.float()
        torch.ops.otvae.feature_append(feats, getattr(self, f"{side}_features"), getattr(self, f"num_{side}"))

    def _read_counts(self) -> List[List[int]]:
        """``[[stored_real, seen_real], [stored_fake, seen_fake]]``, read on the host"""
        return [self.num_real.tolist(), self.num_fake.tolist()]

    def _warn_dropped(self, counts: List[List[int]]) -> None:
        (stored_real, seen_real), (stored_fake, seen_fake) = counts
        if (seen_real > stored_real or seen_fake > stored_fake) and not self._warned_dropped:
            self._warned_dropped = True
            warnings.warn(f"{self._store_name} keeps the first max_observations = {self.max_observations} feature rows per side: "
                          f"{seen_real - stored_real} real and {seen_fake - stored_fake} fake rows were dropped", UserWarning)

    def sync(self, process_group: Any = None) -> None:
        """the union of every rank's stored rows, rank 0's first, in the front of buffers of ``world x max_observations`` rows (the
        fixed-size buffers and the counts are all-gathered: features cannot be sum-reduced); nothing to do without a process group"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        group = process_group if process_group is not None else self.process_group
        world = dist.get_world_size(group)
        if world == 1:
            return
        for side in ("real", "fake"):
            buf, num = getattr(self, f"{side}_features"), getattr(self, f"num_{side}")
            rows = buf.shape[0]
            nums = [torch.empty_like(num) for _ in range(world)]
            bufs = [torch.empty_like(buf) for _ in range(world)]
            dist.all_gather(nums, num.contiguous(), group=group)
            dist.all_gather(bufs, buf.contiguous(), group=group)
            counts = torch.stack(nums).tolist()
            merged = buf.new_zeros(world * rows, buf.shape[1])
            at = 0
            for (stored, _), part in zip(counts, bufs):
                merged[at:at + stored] = part[:stored]
                at += stored
            setattr(self, f"{side}_features", merged)
            num.copy_(torch.tensor([at, sum(seen for _, seen in counts)], dtype=num.dtype))
