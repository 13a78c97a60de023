"""What the image-level metrics (``FrechetInceptionDistance``, ``KernelInceptionDistance``) share: images -> features through a
network that never trains (the reference's ``FrechetInceptionDistance._extract_features``, metrics/fid.py:99-111)."""
from collections import OrderedDict
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

__all__ = ["ImageFeatureMixin"]


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
