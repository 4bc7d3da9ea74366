"""Frame and tile histograms on the GPU (csrc/b4d_enhance.hip, b4d_tile_histogram): the counts behind
``preprocessing.clahe`` and ``preprocessing.equalize_hist``, with their quantiser and their tiles."""
from __future__ import annotations


def frame_histogram(images, levels=None, value_range=None, *, tile_grid_size=(1, 1)) -> dict:
    """Histograms of every frame ``(H, W)`` / ``(T, H, W)``, or of every tile of ``tile_grid_size`` (tiles along x, tiles along y;
    an axis its tile count does not divide is extended by reflected pixels, which are counted).

    ``uint8`` / ``uint16`` frames: one bin per value (256 / 65536 bins).  Every other dtype is taken as float32 and quantised to
    ``levels`` bins (default 65536) over ``value_range=(lo, hi)``, by default each frame's own minimum and maximum; pixels outside
    take the end bins, NaN pixels are not counted.

    Returns ``{"counts": (T, ty, tx, L) int64, "n_valid": (T, ty, tx) int64, "lo": (T,) float32, "hi": (T,) float32}``, without the
    leading axis for a single frame.  For integer frames and one tile ``counts`` is ``np.bincount(frame.ravel(), minlength=L)``."""
    from ..preprocessing import enhancement      # (preprocessing imports metrics.order: the import waits for the call)

    return enhancement.frame_histogram(images, levels, value_range, tile_grid_size=tile_grid_size)
