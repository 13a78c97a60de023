"""Streaming Frechet distance between two feature streams (the reference's ``metrics/fid.py``): per side only
(n, sum f, sum f f^T) in fp64 is kept, accumulated by ``otvae_moments_accum`` on the fp64 matrix cores; ``compute`` is ``mean_cov``
and the Gaussian 2-Wasserstein distance through the library's eigensolver."""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from ..ot import matrix_utils as MU
from .base import Metric
from .features import ImageFeatureMixin

__all__ = ["frechet_distance", "FrechetDistance", "FrechetInceptionDistance"]

MIN_OBSERVATIONS = 1000   # reference metrics/fid.py:126: below this many observations on either side the distance is reported as inf


def frechet_distance(mean1: Tensor, cov1: Tensor, mean2: Tensor, cov2: Tensor) -> Tensor:
    """|mu1 - mu2|^2 + Tr cov1 + Tr cov2 - 2 Tr (cov1 cov2)^1/2 in fp64 on the device (0-d tensor).

    The cross term is taken as Tr (cov1^1/2 cov2 cov1^1/2)^1/2 = sum_k sqrt(lambda_k) of a SYMMETRIC matrix (two symmetric
    eigendecompositions, the library's block driver up to D = 2048).  Covariances of fewer samples than features are singular and
    round-off makes their smallest eigenvalues slightly negative: such eigenvalues are clamped to zero in cov1^1/2, and in the final
    sum everything below the eigenvalues' own uncertainty (D eps lambda_max) counts as zero, instead of going through ``w2_gaussian``'s positive-definiteness validation (which raises)."""
    m1, m2 = mean1.to(torch.float64).reshape(-1), mean2.to(torch.float64).reshape(-1)
    c1, c2 = cov1.to(torch.float64), cov2.to(torch.float64)
    if c1.is_cuda:
        lam, vt = MU.eigh_vectors(c1)
        root = MU.spectral_fn(lam.clamp(min=0).sqrt(), vt)
        inner = MU.matmul64(MU.matmul64(root, c2), root)[0]
        ev, _ = MU.eigvals_and_fn(inner, 0)
    else:   # moments that live on the host (gathered or pre-filled states): the same two decompositions by LAPACK
        lam, v = torch.linalg.eigh(c1)
        root = (v * lam.clamp(min=0).sqrt()) @ v.T
        ev = torch.linalg.eigvalsh(root @ c2 @ root)
    # an eigenvalue of a D x D fp64 problem is known to about D eps lambda_max: below that it is round-off around an exact zero (rank
    # deficiency), and its square root would enter the trace as sqrt(noise) -- the cut-off of torch.linalg.matrix_rank / ``pinv_sym``
    cut = ev.shape[-1] * torch.finfo(torch.float64).eps * ev.abs().max()
    cross = torch.where(ev > cut, ev, torch.zeros_like(ev)).sqrt().sum()
    diff = m1 - m2
    return (diff * diff).sum() + torch.diagonal(c1).sum() + torch.diagonal(c2).sum() - 2.0 * cross


def _mean_cov(total: Tensor, correlation: Tensor, n: Tensor):
    if total.is_cuda:
        return MU.mean_cov(total, correlation, n)
    mean = total / n
    return mean, correlation / n - torch.outer(mean, mean)


class FrechetDistance(Metric):
    """The metric on features the caller already has: ``update(generated_feats, sample_feats)``, each ``[B, feature_size]`` (more
    dimensions are flattened), float32 or float64, either may be None.  State names and their pairing are the reference's
    (metrics/fid.py:90-97,113-122): ``generated`` feeds ``real_sum`` / ``real_correlation`` / ``num_real_obs`` and ``samples`` the
    ``fake_*`` ones -- the distance is symmetric, so the swapped-looking names change nothing.  (The counts are float64 here, like
    the sums: the kernel adds to all three in one launch.)  ``compute()`` is ``inf`` until both sides have seen 1000 observations; it reads the two
    counts on the host (``update`` never does) and works where the states live -- on the device through the library's kernels, and for
    host-resident states (gathered or pre-filled ones) through LAPACK.  ``update`` has no host path."""
    higher_is_better = False

    def __init__(self, feature_size: int = 2048, **metric_kwargs):
        super().__init__(**metric_kwargs)
        if not 1 <= int(feature_size) <= 2048:
            raise ValueError(f"feature_size must be in 1 ... 2048 (the moments kernel's widths), got {feature_size}")
        d = self.feature_size = int(feature_size)
        for side in ("real", "fake"):
            self.add_state(f"{side}_sum", torch.zeros(d, dtype=torch.double), dist_reduce_fx="sum")
            self.add_state(f"{side}_correlation", torch.zeros(d, d, dtype=torch.double), dist_reduce_fx="sum")
            self.add_state(f"num_{side}_obs", torch.zeros(1, dtype=torch.double), dist_reduce_fx="sum")

    def _accumulate(self, feats: Tensor, side: str) -> None:
        feats = feats.detach().reshape(feats.shape[0], -1)
        if feats.shape[1] != self.feature_size:
            raise ValueError(f"features have width {feats.shape[1]}, the metric was built for {self.feature_size}")
        if feats.dtype not in (torch.float32, torch.float64):
            feats = feats.float()
        torch.ops.otvae.moments_accum(feats, getattr(self, f"num_{side}_obs"), getattr(self, f"{side}_sum"),
                                      getattr(self, f"{side}_correlation"))

    def update(self, generated: Optional[Tensor] = None, samples: Optional[Tensor] = None) -> None:
        if generated is not None:
            self._accumulate(generated, "real")
        if samples is not None:
            self._accumulate(samples, "fake")

    def compute(self) -> Tensor:
        if float(self.num_fake_obs) < MIN_OBSERVATIONS or float(self.num_real_obs) < MIN_OBSERVATIONS:
            return torch.ones(1) * float("inf")
        real_mean, real_cov = _mean_cov(self.real_sum, self.real_correlation, self.num_real_obs[0])
        fake_mean, fake_cov = _mean_cov(self.fake_sum, self.fake_correlation, self.num_fake_obs[0])
        return frechet_distance(real_mean, real_cov, fake_mean, fake_cov)


class FrechetInceptionDistance(ImageFeatureMixin, FrechetDistance):
    """The reference's ``FrechetInceptionDistance`` (metrics/fid.py): ``update(generated=None, samples=None)`` takes IMAGES; grey images
    are tiled to three channels, ``to_255`` maps ``data_range`` onto 0 ... 255 and casts to uint8, ``net`` turns them into features that
    are flattened to ``[B, feature_size]`` and accumulated as in ``FrechetDistance``.  ``net=None`` builds torchmetrics' Inception-v3
    (``ImportError`` when that package is missing) and then converts to uint8 unless ``data_range`` already is (0, 255)."""

    def __init__(self, net: Optional[nn.Module] = None, feature_size: int = 2048, to_255: bool = False,
                 data_range: Tuple[float, float] = (0., 1.), **metric_kwargs):
        super().__init__(feature_size=feature_size, **metric_kwargs)
        self._init_features(net, feature_size, to_255, data_range)

    @torch.no_grad()
    def update(self, generated: Optional[Tensor] = None, samples: Optional[Tensor] = None) -> None:
        if generated is not None:
            self._accumulate(self._extract_features(generated), "real")
        if samples is not None:
            self._accumulate(self._extract_features(samples), "fake")
