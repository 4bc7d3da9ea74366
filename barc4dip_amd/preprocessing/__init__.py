"""GPU drop-in for ``barc4dip.preprocessing`` (deconvolve_psf, flat_field_correction) and distortion correction."""
from __future__ import annotations

from . import distortion
from .distortion import correct_distortion, remove_distortion
from .filters import deconvolve_psf
from .normalize import flat_field_correction

__all__ = ["deconvolve_psf", "flat_field_correction", "distortion", "correct_distortion", "remove_distortion"]
