"""GPU drop-in for ``barc4dip.preprocessing`` (deconvolve_psf, flat_field_correction), distortion correction and spatial
rank filters with outlier repair, linear separable filters and envelope removal, CLAHE and histogram equalisation."""
from __future__ import annotations

from . import distortion
from .distortion import correct_distortion, remove_distortion
from .filters import deconvolve_psf
from .normalize import flat_field_correction
from .rank import median_filter, percentile_filter, rank_filter, remove_outliers
from .combine import combine_frames, remove_zingers
from .smooth import gaussian_filter, remove_envelope, separable_filter, uniform_filter
from . import enhancement
from .enhancement import clahe, equalize_hist

__all__ = ["deconvolve_psf", "flat_field_correction", "distortion", "correct_distortion", "remove_distortion",
           "median_filter", "rank_filter", "percentile_filter", "remove_outliers", "combine_frames", "remove_zingers",
           "gaussian_filter", "uniform_filter", "separable_filter", "remove_envelope", "enhancement", "clahe", "equalize_hist"]
