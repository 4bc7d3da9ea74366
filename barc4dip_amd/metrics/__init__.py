"""GPU drop-in for ``barc4dip.metrics`` (same public names as metrics/__init__.py:6-20) + temporal statistics, local contrast
and, in ``perceptual`` (a module the reference names and leaves empty), the scores of a frame against a reference frame: SSIM,
MS-SSIM, MSE / PSNR / NRMSE; frame and tile histograms."""
from __future__ import annotations

from . import kernels, multitau, sharpness, speckles, statistics, temporal, twotime
from .sharpness import sharpness_stack_stats, sharpness_stats
from .speckles import speckle_stack_stats, speckle_stats
from .statistics import distribution_moments
from . import sharded
from .temporal import temporal_stats
from .multitau import multi_tau_correlation
from . import order
from .order import temporal_median, temporal_percentile, temporal_robust_mean
from .twotime import correlation_decay, two_time_correlation
from . import contrast
from .contrast import local_contrast
from . import perceptual
from .perceptual import frame_errors, ms_ssim, mse, nrmse, psnr, ssim
from . import histogram
from .histogram import frame_histogram
from . import regions
from .regions import find_spots, region_properties

__all__ = ["order", "temporal_median", "temporal_percentile", "temporal_robust_mean","sharpness", "sharpness_stats", "sharpness_stack_stats", "statistics", "speckles", "speckle_stats",
           "speckle_stack_stats", "distribution_moments", "temporal", "temporal_stats", "sharded", "kernels", "twotime",
           "two_time_correlation", "correlation_decay", "multitau", "multi_tau_correlation", "contrast", "local_contrast",
           "perceptual", "ssim", "ms_ssim", "frame_errors", "mse", "psnr", "nrmse", "histogram", "frame_histogram", "regions", "region_properties", "find_spots"]
