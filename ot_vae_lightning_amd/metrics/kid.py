"""Kernel Inception Distance (Binkowski et al. 2018; ``torchmetrics.image.kid.KernelInceptionDistance``): the unbiased MMD^2 between
two feature sets under the polynomial kernel ``k(a, b) = (gamma <a, b> + coef)^degree``, reported as mean and standard deviation over
random subsets.  Unlike the Frechet distance it is usable from a few dozen samples and assumes nothing about the features.

The metric keeps the features themselves (fp32, a fixed-size buffer per side, appended to by ``otvae_feature_append`` with the offset
read on the device); ``compute`` draws the subsets' row indices on the device and evaluates every subset in ONE call of
``otvae_poly_mmd_subsets`` (csrc/kid.hip): fp64 on the matrix cores, rows gathered at the load, fixed summation order."""
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .features import FeatureStore, ImageFeatureMixin

__all__ = ["poly_mmd2", "kernel_distance", "KernelDistance", "KernelInceptionDistance"]

_SUBSET_SIZE_ERROR = "Argument `subset_size` should be smaller than the number of samples"   # torchmetrics' wording
MAX_FEATURE_SIZE, MAX_DEGREE, MAX_SUBSETS = 2048, 8, 65535                                    # the kernel's envelope


def _check_kernel(degree: int, gamma: Optional[float], coef: float, width: int) -> Tuple[int, float, float]:
    if not isinstance(degree, int) or not 1 <= degree <= MAX_DEGREE:
        raise ValueError(f"Argument `degree` must be an integer in 1 ... {MAX_DEGREE}, got {degree!r}")
    if gamma is not None and not float(gamma) > 0:
        raise ValueError(f"Argument `gamma` must be None (1 / feature width) or a positive number, got {gamma!r}")
    return degree, (1.0 / width if gamma is None else float(gamma)), float(coef)


def _check_subsets(subsets: int, subset_size: int) -> None:
    if not isinstance(subsets, int) or not 1 <= subsets <= MAX_SUBSETS:
        raise ValueError(f"Argument `subsets` must be an integer in 1 ... {MAX_SUBSETS}, got {subsets!r}")
    if not isinstance(subset_size, int) or subset_size < 2:
        raise ValueError(f"Argument `subset_size` must be an integer of at least 2 (the estimator divides by m - 1), got {subset_size!r}")


def _host_mmd2(x: Tensor, y: Tensor, degree: int, gamma: float, coef: float) -> Tensor:
    """torchmetrics' ``poly_kernel`` / ``maximum_mean_discrepancy`` in fp64 torch, for features that live on the host"""
    x, y = x.double(), y.double()
    m = x.shape[0]
    k_xx, k_yy, k_xy = ((a @ b.T * gamma + coef) ** degree for a, b in ((x, x), (y, y), (x, y)))
    within = (k_xx.sum() - torch.diagonal(k_xx).sum()) + (k_yy.sum() - torch.diagonal(k_yy).sum())
    return within / (m * (m - 1)) - 2.0 * k_xy.sum() / (m * m)


def _features_2d(t: Tensor, name: str) -> Tensor:
    if t.dim() < 2:
        raise ValueError(f"{name}: expected [n, D] features, got {tuple(t.shape)}")
    t = t.detach().reshape(t.shape[0], -1)
    if not 1 <= t.shape[1] <= MAX_FEATURE_SIZE:
        raise ValueError(f"{name}: feature width {t.shape[1]} is outside 1 ... {MAX_FEATURE_SIZE}")
    return t


def _evaluate(real: Tensor, fake: Tensor, idx_real: Optional[Tensor], idx_fake: Optional[Tensor], m: int, degree: int, gamma: float,
              coef: float) -> Tuple[Tensor, Tensor]:
    """(per_subset [S], stats [2]) where the features live: the kernel on the device (features as fp32), fp64 torch on the host"""
    if real.is_cuda:
        return torch.ops.otvae.poly_mmd_subsets(real.float().contiguous(), fake.float().contiguous(), idx_real, idx_fake, m, degree,
                                                gamma, coef)
    if idx_real is None:
        per = _host_mmd2(real[:m], fake[:m], degree, gamma, coef).reshape(1)
    else:
        per = torch.stack([_host_mmd2(real[ir.long()], fake[jf.long()], degree, gamma, coef) for ir, jf in zip(idx_real, idx_fake)])
    return per, torch.stack([per.mean(), per.std(unbiased=False)])


def draw_subsets(n: int, subsets: int, subset_size: int, generator: torch.Generator, device) -> Tensor:
    """``[subsets, subset_size]`` int32 row indices in [0, n): every row is the head of an independent random permutation of 0 ... n - 1
    (no replacement within a subset), drawn on ``device``; nothing is read on the host"""
    keys = torch.rand(subsets, n, generator=generator, device=device)
    return keys.argsort(dim=1)[:, :subset_size].to(torch.int32).contiguous()


def _generator(device, seed: Optional[int], call: int) -> torch.Generator:
    if seed is None:
        seed = int(torch.empty((), dtype=torch.int64).random_())   # from torch's global generator: torch.manual_seed reproduces it
    g = torch.Generator(device=device)
    g.manual_seed((int(seed) * 0x9E3779B1 + call) & 0x7FFFFFFFFFFFFFFF)
    return g


def poly_mmd2(x: Tensor, y: Tensor, degree: int = 3, gamma: Optional[float] = None, coef: float = 1.0) -> Tensor:
    """the unbiased polynomial-kernel MMD^2 of two equally sized feature sets ``[n, D]``: a 0-d float64 tensor.  Device features are
    used as float32 (float64 ones are rounded)."""
    x, y = _features_2d(x, "x"), _features_2d(y, "y")
    if x.shape != y.shape:
        raise ValueError(f"poly_mmd2 takes two feature sets of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[0] < 2:
        raise ValueError("poly_mmd2 needs at least two samples per side")
    degree, gamma, coef = _check_kernel(degree, gamma, coef, x.shape[1])
    return _evaluate(x, y, None, None, x.shape[0], degree, gamma, coef)[0][0]


def kernel_distance(real: Tensor, fake: Tensor, subsets: int = 100, subset_size: int = 1000, degree: int = 3,
                    gamma: Optional[float] = None, coef: float = 1.0, seed: Optional[int] = None, return_subsets: bool = False):
    """KID of two feature sets ``[n_real, D]`` / ``[n_fake, D]``: ``(mean, std)`` (0-d float64 tensors) of the MMD^2 over ``subsets``
    random subsets of ``subset_size`` rows per side; with ``return_subsets`` also ``(per_subset [S], idx_real, idx_fake)``."""
    real, fake = _features_2d(real, "real"), _features_2d(fake, "fake")
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise ValueError(f"kernel_distance: real {tuple(real.shape)} on {real.device} and fake {tuple(fake.shape)} on {fake.device} "
                         "must share the feature width and the device")
    _check_subsets(subsets, subset_size)
    degree, gamma, coef = _check_kernel(degree, gamma, coef, real.shape[1])
    if subset_size > min(real.shape[0], fake.shape[0]):
        raise ValueError(_SUBSET_SIZE_ERROR)
    g = _generator(real.device, seed, 0)
    idx_real = draw_subsets(real.shape[0], subsets, subset_size, g, real.device)
    idx_fake = draw_subsets(fake.shape[0], subsets, subset_size, g, real.device)
    per, stats = _evaluate(real, fake, idx_real, idx_fake, subset_size, degree, gamma, coef)
    if return_subsets:
        return stats[0], stats[1], per, idx_real, idx_fake
    return stats[0], stats[1]


class KernelDistance(FeatureStore):
    """The metric on features the caller already has: ``update(generated_feats, sample_feats)``, each ``[B, feature_size]`` (more
    dimensions are flattened), float32 or float64 (ROUNDED to float32 when stored), either may be None; the store itself is
    ``features.FeatureStore``.  The keyword names and their pairing are ``FrechetDistance``'s (``generated`` feeds the ``real_*``
    states, ``samples`` the ``fake_*`` ones; the distance is symmetric).  Per side the states are ``*_features`` ``[max_observations, feature_size]`` float32 and ``num_*`` int64 ``[2]`` =
    (rows stored, rows seen); rows beyond ``max_observations`` are dropped (``compute`` warns once).  ``update`` is one
    ``otvae::feature_append`` per side and reads nothing on the host, so it can be captured.

    ``compute()`` returns ``(mean, std)`` over ``subsets`` random subsets of ``subset_size`` rows per side, reads the two counts on the
    host (as the Frechet distance's does) and raises ``ValueError`` while a side holds fewer rows than ``subset_size``.  The indices
    come from a generator seeded by ``seed`` and the number of ``compute`` calls so far; ``last_subsets = (idx_real, idx_fake,
    per_subset)`` keeps what the last call used.  Host-resident states (gathered or pre-filled) take an fp64 torch path."""
    higher_is_better = False
    compute_names = ("mean", "std")
    _store_name = "KernelDistance"

    def __init__(self, feature_size: int = 2048, max_observations: int = 10000, subsets: int = 100, subset_size: int = 1000,
                 degree: int = 3, gamma: Optional[float] = None, coef: float = 1.0, seed: Optional[int] = None, **metric_kwargs):
        super().__init__(**metric_kwargs)
        if not isinstance(feature_size, int) or not 1 <= feature_size <= MAX_FEATURE_SIZE:
            raise ValueError(f"feature_size must be an integer in 1 ... {MAX_FEATURE_SIZE} (the kernel's widths), got {feature_size!r}")
        _check_subsets(subsets, subset_size)
        self.degree, self.gamma, self.coef = _check_kernel(degree, gamma, coef, feature_size)
        if not isinstance(max_observations, int) or max_observations < subset_size:
            raise ValueError(f"max_observations ({max_observations!r}) must be an integer of at least subset_size ({subset_size})")
        self.feature_size, self.max_observations = feature_size, max_observations
        self.subsets, self.subset_size, self.seed = subsets, subset_size, seed
        self.last_subsets: Optional[Tuple[Tensor, Tensor, Tensor]] = None
        self._compute_calls = 0
        self._init_store(feature_size, max_observations)

    def update(self, generated: Optional[Tensor] = None, samples: Optional[Tensor] = None) -> None:
        if generated is not None:
            self._append(generated, "real")
        if samples is not None:
            self._append(samples, "fake")

    def compute(self) -> Tuple[Tensor, Tensor]:
        counts = self._read_counts()
        stored_real, stored_fake = counts[0][0], counts[1][0]
        if min(stored_real, stored_fake) < self.subset_size:
            raise ValueError(_SUBSET_SIZE_ERROR)
        self._warn_dropped(counts)
        device = self.real_features.device
        g = _generator(device, self.seed, self._compute_calls)
        self._compute_calls += 1
        idx_real = draw_subsets(stored_real, self.subsets, self.subset_size, g, device)
        idx_fake = draw_subsets(stored_fake, self.subsets, self.subset_size, g, device)
        per, stats = _evaluate(self.real_features[:stored_real], self.fake_features[:stored_fake], idx_real, idx_fake, self.subset_size,
                               self.degree, self.gamma, self.coef)
        self.last_subsets = (idx_real, idx_fake, per)
        return stats[0], stats[1]


class KernelInceptionDistance(ImageFeatureMixin, KernelDistance):
    """``update(generated=None, samples=None)`` takes IMAGES, turned into features exactly as ``FrechetInceptionDistance`` does (grey
    images tiled to three channels, ``to_255``, ``net``, flattened to ``[B, feature_size]``); everything else is ``KernelDistance``.
    ``net=None`` builds torchmetrics' Inception-v3 (``ImportError`` when that package is missing)."""

    def __init__(self, net: Optional[nn.Module] = None, feature_size: int = 2048, to_255: bool = False,
                 data_range: Tuple[float, float] = (0., 1.), **kernel_distance_kwargs):
        super().__init__(feature_size=feature_size, **kernel_distance_kwargs)
        self._init_features(net, feature_size, to_255, data_range)

    @torch.no_grad()
    def update(self, generated: Optional[Tensor] = None, samples: Optional[Tensor] = None) -> None:
        if generated is not None:
            self._append(self._extract_features(generated), "real")
        if samples is not None:
            self._append(self._extract_features(samples), "fake")
