"""GPU drop-in for ``barc4dip.signal`` (same public names as signal/__init__.py:6-26)."""
from __future__ import annotations

from . import corr, displacement, fft, focus, fringes, hartmann, modal, scanning, speckle, stepping, tracking, wavefront
from .corr import autocorr2d, autocorr2d_stack, psd_autocorr2d_stack, xcorr2d
from .displacement import displacement_grid, displacement_map
from .focus import beam_caustic, focal_spot, focus_geometry
from .fringes import (coarse_carriers, fringe_carriers, fringe_demodulate, fringe_displacement, fringe_grid, phase_unwrap)
from .hartmann import hartmann_cells, hartmann_displacement, hartmann_lattice, spot_centroids
from .modal import modal_eval, modal_fit, modal_table
from .scanning import speckle_scan
from .speckle import speckle_contrast, speckle_imaging
from .stepping import calibrate_steps, phase_stepping, stepping_displacement, stepping_fit
from .tracking import (phase_correlation, phase_correlation_batch, template_matching, template_matching_batch,
                       track_translation)
from .wavefront import integrate_gradient, wavefront_from_displacement
from .fft import fft1d, fft2d, fft2d_stack, freq_axes2d, freq_axis1d, psd1d, psd2d, psd2d_stack

__all__ = [
    "fft", "corr", "tracking", "phase_correlation", "template_matching", "track_translation",
    "phase_correlation_batch", "template_matching_batch",
    "freq_axis1d", "freq_axes2d", "fft1d", "fft2d", "psd1d", "psd2d", "xcorr2d", "autocorr2d",
    "fft2d_stack", "psd2d_stack", "autocorr2d_stack", "psd_autocorr2d_stack",
    "displacement", "displacement_map", "displacement_grid",
    "wavefront", "integrate_gradient", "wavefront_from_displacement",
    "modal", "modal_fit", "modal_eval", "modal_table",
    "focus", "focal_spot", "focus_geometry", "beam_caustic",
    "fringes", "fringe_grid", "fringe_demodulate", "phase_unwrap", "coarse_carriers", "fringe_carriers", "fringe_displacement",
    "speckle", "speckle_contrast", "speckle_imaging",
    "stepping", "stepping_fit", "phase_stepping", "calibrate_steps", "stepping_displacement",
    "scanning", "speckle_scan",
    "hartmann", "hartmann_cells", "spot_centroids", "hartmann_lattice", "hartmann_displacement",
]
