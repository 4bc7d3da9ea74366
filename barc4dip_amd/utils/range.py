"""GPU drop-in for ``barc4dip.utils.range`` (range.py:14-86): robust (vmin, vmax) bounds of an image or a stack.

The filtered bounds come from the range-only variant of the median filter (csrc/b4d_rankfilt.hip): the frames are read once, the
filtered copy is never written, and the NaN-aware minimum and maximum are reduced per frame with integer min / max on ordered
keys, so the result is deterministic and equal to ``nanmin`` / ``nanmax`` of ``scipy.ndimage.median_filter``'s output.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import MODES, frame_stack, window
from ..preprocessing import rank as R


def _ndim(image) -> int:
    nd = int(image.ndim) if hasattr(image, "ndim") else int(np.ndim(image))
    if nd not in (2, 3):
        raise ValueError(f"Expected 2D or 3D array, got ndim={nd}")
    return nd


def _frame_ranges(t, size):
    """(batch, 2) float32 device tensor {nanmin, nanmax} of every median-filtered frame of device tensor t."""
    sy, sx = window(size, R.MAX_SIZE)
    batch = int(t.shape[0]) if t.ndim == 3 else 1
    _, mm = R.run_rank_filter(t, batch, int(t.shape[-2]), int(t.shape[-1]), sy, sx, (sy * sx) // 2, MODES["reflect"], 0.0,
                              want_out=False, want_range=True)
    return mm


def _bounds(mm: np.ndarray) -> tuple[float, float]:
    lo, hi = mm[:, 0], mm[:, 1]
    ok = ~np.isnan(lo)          # a frame without a non-NaN filtered value reports NaN for both
    vmin = float(lo[ok].min()) if ok.any() else float("nan")
    vmax = float(hi[ok].max()) if ok.any() else float("nan")
    if not np.isfinite(vmin) or not np.isfinite(vmax) or vmax <= vmin:
        raise ValueError(f"Invalid range after filtering: vmin={vmin}, vmax={vmax}")
    return vmin, vmax


def filtered_minmax_range(image, size: int = 3) -> tuple[float, float]:
    """(vmin, vmax) of the ``size`` x ``size`` median-filtered image (H, W) or, frame by frame, stack (N, H, W): salt-and-pepper
    suppression before scaling.  One pass over the data.  ValueError when the range is empty or not finite."""
    _ndim(image)
    window(size, R.MAX_SIZE)
    t, _, _, _ = frame_stack(image)
    return _bounds(_frame_ranges(t, size).cpu().numpy())


def filtered_minmax_range_streaming(image, size: int = 3, *, chunk_frames: int = 16) -> tuple[float, float]:
    """filtered_minmax_range of a stack that need not be resident: ``image`` (e.g. a memory-mapped .npy) goes through
    ``ingest.iter_device_chunks`` ``chunk_frames`` frames at a time, in its native dtype, while the previous chunk is filtered."""
    if _ndim(image) == 2 or D.is_tensor(image):
        return filtered_minmax_range(image, size)
    window(size, R.MAX_SIZE)
    if int(np.prod(image.shape)) == 0:
        raise ValueError(f"images must not be empty; got shape {tuple(image.shape)}")
    from .. import ingest

    torch = _ffi.require_gpu()
    parts = [_frame_ranges(chunk, size) for chunk in ingest.iter_device_chunks(image, chunk_frames)]
    return _bounds(torch.cat(parts).cpu().numpy())


def percentile_minmax_range(image, p_low: float = 0.05, p_high: float = 99.95) -> tuple[float, float]:
    """(np.nanpercentile(image, p_low), np.nanpercentile(image, p_high)) over ALL pixels of an image or a stack: exact selection
    of the bracketing order statistics on the device (metrics.kernels.percentiles_batch), NumPy's linear interpolation."""
    from ..metrics import kernels as K

    flat = image.reshape(1, 1, -1) if D.is_tensor(image) else np.asarray(image).reshape(1, 1, -1)
    vmin, vmax = K.percentiles_batch(flat, [float(p_low), float(p_high)])[0]
    return float(vmin), float(vmax)
