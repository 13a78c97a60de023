"""Precision, recall, density and coverage of a model's samples against the data, from k-nearest-neighbour manifolds: *improved
precision and recall* (Kynkaanniemi et al. 2019) and *density and coverage* (Naeem et al. 2020).  Where the Frechet and kernel
distances fold fidelity and diversity into one number, these say which of the two moved.

With data features ``R [N, D]`` ("real"), model features ``F [M, D]`` ("fake"), squared Euclidean distances ``d2`` and
``r2_k(x_i)`` = the k-th smallest of ``{ d2(x_i, x_j) : j != i }`` within a row's own set -- self excluded by INDEX, so a duplicate row
is a neighbour at distance 0 and a radius may be 0:

    precision = (1 / M)   #{ j : some i has d2(F_j, R_i) <= r2_k(R_i) }        fake samples inside the real manifold
    recall    = (1 / N)   #{ i : some j has d2(R_i, F_j) <= r2_k(F_j) }        real samples inside the fake manifold
    density   = (1 / k M) sum_j #{ i : d2(F_j, R_i) <= r2_k(R_i) }             real balls per fake sample, in units of k
    coverage  = (1 / N)   #{ i : min_j d2(R_i, F_j) <= r2_k(R_i) }             real balls that hold a fake sample

Balls are CLOSED (``<=``), as in the 2019 paper; implementations that compare strictly differ only where a distance equals a radius
exactly.  Device features go through ``torch.ops.otvae.knn_sq_radii`` / ``manifold_counts`` (csrc/knn_manifold.hip: fp32 features,
Gram-form distances ``|a|^2 + |b|^2 - 2 <a, b>`` in fp64 on the matrix cores, clamped at 0; no n x n array exists) and the four values
are integer reductions of their per-row outputs: identical from run to run, and precision(R, F) == recall(F, R) bit for bit.  Host
features take an fp64 torch path.  Finite features are a precondition."""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .features import FeatureStore, ImageFeatureMixin

__all__ = ["knn_radii", "precision_recall_density_coverage", "PrecisionRecall", "InceptionPrecisionRecall"]

MAX_FEATURE_SIZE, MAX_K = 2048, 16   # the kernels' envelope
_HOST_BLOCK = 1024                   # rows per block of the host path's distance matrix


def _check_k(k: int) -> int:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"Argument `k` must be an integer in 1 ... {MAX_K}, got {k!r}")
    return k


def _features_2d(t: Tensor, name: str, k: int) -> Tensor:
    if not isinstance(t, Tensor) or t.dim() < 2:
        raise ValueError(f"{name}: expected [n, D] features, got {tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
    t = t.detach().reshape(t.shape[0], -1)
    if not 1 <= t.shape[1] <= MAX_FEATURE_SIZE:
        raise ValueError(f"{name}: feature width {t.shape[1]} is outside 1 ... {MAX_FEATURE_SIZE}")
    if t.shape[0] <= k:
        raise ValueError(f"{name}: k = {k} nearest neighbours need more than {k} rows, got {t.shape[0]}")
    return t


def _host_sq_dists(a: Tensor, b: Tensor, nb: Tensor) -> Tensor:
    """the kernel's Gram form for a block of rows ``a`` against all of ``b`` (fp64, clamped at 0)"""
    return ((a * a).sum(1)[:, None] + nb[None, :] - 2.0 * (a @ b.T)).clamp_min_(0.0)


def _host_sq_radii(x: Tensor, k: int) -> Tensor:
    x = x.double()
    nx = (x * x).sum(1)
    out = []
    for lo in range(0, x.shape[0], _HOST_BLOCK):
        d2 = _host_sq_dists(x[lo:lo + _HOST_BLOCK], x, nx)
        rows = torch.arange(d2.shape[0])
        d2[rows, lo + rows] = float("inf")                           # self, by index
        out.append(d2.topk(k, dim=1, largest=False).values[:, k - 1])
    return torch.cat(out)


def _host_counts(real: Tensor, r2_real: Tensor, fake: Tensor, r2_fake: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    real, fake = real.double(), fake.double()
    nf = (fake * fake).sum(1)
    count_fake = torch.zeros(fake.shape[0], dtype=torch.int32)
    hit, low = [], []
    for lo in range(0, real.shape[0], _HOST_BLOCK):
        d2 = _host_sq_dists(real[lo:lo + _HOST_BLOCK], fake, nf)
        count_fake += (d2 <= r2_real[lo:lo + _HOST_BLOCK, None]).sum(0, dtype=torch.int32)
        hit.append((d2 <= r2_fake[None, :]).any(1).to(torch.int32))
        low.append(d2.min(1).values)
    return count_fake, torch.cat(hit), torch.cat(low)


def _sq_radii(x: Tensor, k: int) -> Tensor:
    if x.is_cuda:
        return torch.ops.otvae.knn_sq_radii(x.float().contiguous(), k)
    return _host_sq_radii(x, k)


def knn_radii(x: Tensor, k: int = 5) -> Tensor:
    """``[n]`` float64: the Euclidean distance from every row of ``x [n, D]`` to its k-th nearest OTHER row (``1 <= k <= 16``,
    ``k < n``).  Device features are used as float32 (float64 ones are rounded)."""
    k = _check_k(k)
    return _sq_radii(_features_2d(x, "x", k), k).sqrt()


def _evaluate(real: Tensor, fake: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    if real.is_cuda:
        real, fake = real.float().contiguous(), fake.float().contiguous()
        r2_real, r2_fake = torch.ops.otvae.knn_sq_radii(real, k), torch.ops.otvae.knn_sq_radii(fake, k)
        count_fake, hit_real, min_real = torch.ops.otvae.manifold_counts(real, r2_real, fake, r2_fake)
    else:
        r2_real, r2_fake = _host_sq_radii(real, k), _host_sq_radii(fake, k)
        count_fake, hit_real, min_real = _host_counts(real, r2_real, fake, r2_fake)
    n, m = real.shape[0], fake.shape[0]
    counts = torch.stack([(count_fake > 0).sum(), hit_real.sum(dtype=torch.int64), count_fake.sum(dtype=torch.int64),
                          (min_real <= r2_real).sum()])
    # tensor / tensor: a correctly rounded quotient of two integers (tensor / number multiplies by a rounded reciprocal on the device)
    values = counts.double() / torch.tensor([m, n, k * m, n], dtype=torch.float64, device=counts.device)
    precision, recall, density, coverage = values.unbind()
    return precision, recall, density, coverage


def precision_recall_density_coverage(real: Tensor, fake: Tensor, k: int = 5) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(precision, recall, density, coverage)`` (0-d float64 tensors) of the model's features ``fake [M, D]`` against the data's
    ``real [N, D]`` with k-nearest-neighbour balls (module docstring).  Device features are used as float32."""
    k = _check_k(k)
    real, fake = _features_2d(real, "real", k), _features_2d(fake, "fake", k)
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise ValueError(f"precision_recall_density_coverage: real {tuple(real.shape)} on {real.device} and fake {tuple(fake.shape)} on "
                         f"{fake.device} must share the feature width and the device")
    return _evaluate(real, fake, k)


class PrecisionRecall(FeatureStore):
    """The metric on features the caller already has: ``update(generated=None, samples=None)``, each ``[B, feature_size]`` (more
    dimensions are flattened), float32 or float64 (ROUNDED to float32 when stored), either may be None.

    WHICH SIDE IS WHICH -- unlike the Frechet and kernel distances these values are not symmetric.  ``samples`` (the data of a
    validation batch) is the REAL manifold and feeds the ``real_*`` states; ``generated`` (the model's samples) is the FAKE manifold
    and feeds the ``fake_*`` states.  (``KernelDistance`` stores ``generated`` in its ``real_*`` states: FID's historical pairing,
    harmless for a symmetric distance, and NOT followed here.)  Precision is then the share of generated samples that fall inside the
    data manifold, recall the share of data samples inside the generated one.

    The store is ``features.FeatureStore`` (fixed-size buffers, ``otvae::feature_append``, rows beyond ``max_observations`` dropped
    with one warning).  ``compute()`` returns ``(precision, recall, density, coverage)``, all from one ``k``, reads the two counts on
    the host and raises ``ValueError`` while a side holds ``k`` rows or fewer.  Host-resident states take the fp64 torch path."""
    higher_is_better = True
    compute_names = ("precision", "recall", "density", "coverage")
    _store_name = "PrecisionRecall"

    def __init__(self, feature_size: int = 2048, max_observations: int = 10000, k: int = 5, **metric_kwargs):
        super().__init__(**metric_kwargs)
        if not isinstance(feature_size, int) or not 1 <= feature_size <= MAX_FEATURE_SIZE:
            raise ValueError(f"feature_size must be an integer in 1 ... {MAX_FEATURE_SIZE} (the kernel's widths), got {feature_size!r}")
        self.k = _check_k(k)
        if not isinstance(max_observations, int) or max_observations <= k:
            raise ValueError(f"max_observations ({max_observations!r}) must be an integer above k ({k})")
        self._init_store(feature_size, max_observations)

    def update(self, generated: Optional[Tensor] = None, samples: Optional[Tensor] = None) -> None:
        if samples is not None:
            self._append(samples, "real")
        if generated is not None:
            self._append(generated, "fake")

    def compute(self) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        counts = self._read_counts()
        stored_real, stored_fake = counts[0][0], counts[1][0]
        if min(stored_real, stored_fake) <= self.k:
            raise ValueError(f"PrecisionRecall with k = {self.k} needs more than {self.k} rows per side, holds {stored_real} data and "
                             f"{stored_fake} generated rows")
        self._warn_dropped(counts)
        return _evaluate(self.real_features[:stored_real], self.fake_features[:stored_fake], self.k)


class InceptionPrecisionRecall(ImageFeatureMixin, PrecisionRecall):
    """``update(generated=None, samples=None)`` takes IMAGES, turned into features exactly as ``FrechetInceptionDistance`` does (grey
    images tiled to three channels, ``to_255``, ``net``, flattened to ``[B, feature_size]``); everything else, the mapping of
    ``samples`` to the real and ``generated`` to the fake manifold included, is ``PrecisionRecall``.  ``net=None`` builds
    torchmetrics' Inception-v3 (``ImportError`` when that package is missing)."""

    def __init__(self, net: Optional[nn.Module] = None, feature_size: int = 2048, to_255: bool = False,
                 data_range: Tuple[float, float] = (0., 1.), **precision_recall_kwargs):
        super().__init__(feature_size=feature_size, **precision_recall_kwargs)
        self._init_features(net, feature_size, to_255, data_range)

    @torch.no_grad()
    def update(self, generated: Optional[Tensor] = None, samples: Optional[Tensor] = None) -> None:
        if samples is not None:
            self._append(self._extract_features(samples), "real")
        if generated is not None:
            self._append(self._extract_features(generated), "fake")
