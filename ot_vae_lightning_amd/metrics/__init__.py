"""Validation metrics on the device, with the interface the reference's model code uses and no ``torchmetrics`` dependency:
``MetricCollection({"psnr": PeakSignalNoiseRatio(), "fid": FrechetInceptionDistance(net=...)})`` goes into
``VAE(metrics=...)`` exactly as in the reference's ``configs/vae/defaults.yaml``.  The accumulation of every ``update`` is one
HIP entry of ``csrc/metrics.hip`` / ``csrc/ssim.hip`` / ``csrc/kid.hip`` (``torch.ops.otvae.sqerr_accum`` /
``moments_accum`` / ``ssim_accum`` / ``ms_ssim_accum`` / ``feature_append``); the Frechet distance's ``compute`` runs the fp64 eigensolver, the kernel distance's evaluates
all of its random subsets in one ``torch.ops.otvae.poly_mmd_subsets``, and precision / recall / density / coverage come from
``torch.ops.otvae.knn_sq_radii`` and ``manifold_counts`` (``csrc/knn_manifold.hip``)."""
from .base import Metric, MetricCollection
from .psnr import PeakSignalNoiseRatio
from .frechet import FrechetDistance, FrechetInceptionDistance, frechet_distance
from .ssim import StructuralSimilarityIndexMeasure, structural_similarity
from .ms_ssim import MultiScaleStructuralSimilarityIndexMeasure, multiscale_structural_similarity
from .kid import KernelDistance, KernelInceptionDistance, kernel_distance, poly_mmd2
from .prdc import InceptionPrecisionRecall, PrecisionRecall, knn_radii, precision_recall_density_coverage

__all__ = ["Metric", "MetricCollection", "PeakSignalNoiseRatio", "FrechetDistance", "FrechetInceptionDistance", "frechet_distance",
           "StructuralSimilarityIndexMeasure", "structural_similarity", "MultiScaleStructuralSimilarityIndexMeasure",
           "multiscale_structural_similarity", "KernelDistance", "KernelInceptionDistance", "kernel_distance",
           "poly_mmd2", "PrecisionRecall", "InceptionPrecisionRecall", "knn_radii", "precision_recall_density_coverage"]
