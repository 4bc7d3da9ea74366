"""GPU drop-in for ``barc4dip.utils.dtype`` (dtype.py:15-74): conversion of images and stacks to uint16.

``to_uint16`` is what every TIFF write of the reference goes through; its cost there is the median filter behind
``filtered_minmax_range``.  Here the frames go to the device once: the mean comes from b4d_moments, the bounds from the range-only
median filter, and the scaling, clipping and truncation from b4d_scale_to_u16, element by element in the reference's float32
operation order.  Differences: the arithmetic runs on the float32 cast of the input (the reference clips float64 counts in
float64), the mean is accumulated in float64 over the finite values, and NaN becomes 0 (NumPy's cast of NaN is undefined).
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import frame_stack
from .range import filtered_minmax_range


def _scale_to_u16(t, vmin: float, inv: float, mul_f64: bool) -> np.ndarray:
    torch = _ffi.require_gpu()
    out = torch.empty(tuple(t.shape), dtype=torch.int16, device=t.device)     # uint16 words in int16 storage
    _ffi.check(_ffi.lib().b4d_scale_to_u16(D.ptr(t), int(t.numel()), float(vmin), float(inv), 1 if mul_f64 else 0, D.ptr(out),
                                           _ffi.stream_ptr()))
    return out.cpu().numpy().view(np.uint16)


def _nanmean(t) -> float:
    """Mean of the finite values of device tensor t, accumulated in float64 (b4d_moments); NaN when there is none."""
    torch = _ffi.require_gpu()
    flat = t.reshape(-1)
    if flat.numel() % 4:        # b4d_moments reads 16 bytes a lane: pad with NaN (skipped)
        flat = torch.cat([flat, torch.full((4 - flat.numel() % 4,), float("nan"), device=t.device)])
    out = torch.empty((1, 8), dtype=torch.float64, device=t.device)
    _ffi.check(_ffi.lib().b4d_moments(D.ptr(flat), 1, int(flat.numel()), 0.0, float("inf"), D.ptr(out), _ffi.stream_ptr()))
    n, mean = out.cpu().numpy()[0, :2]
    return float(mean) if n >= 1 else float("nan")


def to_uint16(data: np.ndarray, *, median_size: int = 3, counts_threshold: float = 10.0, scaling: float = 1 / np.sqrt(2)) -> np.ndarray:
    """Convert a 2D image (H, W) or a 3D stack (N, H, W) to uint16.

    Data whose mean exceeds ``counts_threshold`` are taken as counts: clipped to [0, 65535] and truncated.  Other data are
    stretched: with (vmin, vmax) = filtered_minmax_range(data, median_size) widened by 5 % each way, the output is
    ``(data - vmin) * (65535 * scaling / (vmax - vmin))`` clipped and truncated; ``scaling`` is the grey level, as a fraction of
    full scale, that vmax maps to."""
    if not isinstance(data, np.ndarray):
        raise TypeError("to_uint16 expects a numpy.ndarray")
    if data.dtype == np.uint16:
        return data
    if data.ndim not in (2, 3):
        raise ValueError(f"Expected 2D or 3D array, got ndim={data.ndim}")
    t, _, _, _ = frame_stack(data)
    if _nanmean(t) > counts_threshold:
        return _scale_to_u16(t, 0.0, 1.0, False)        # x - 0 and x * 1 are exact: clip and truncate
    vmin, vmax = filtered_minmax_range(t, size=median_size)
    vmin *= 0.95
    vmax /= 0.95
    inv = 65535 * scaling / (vmax - vmin)
    # NumPy multiplies a float32 array by a NumPy float64 scalar in float64 and rounds once into the float32 output; a Python
    # float is a weak scalar and the product is taken in float32 (for a float32 NumPy scalar the two coincide)
    return _scale_to_u16(t, vmin, float(inv), isinstance(inv, np.generic))


def round_uint16_bounds(vmin: float, vmax: float, k: float = 1000) -> tuple[int, int]:
    """Bounds widened to multiples of ``k`` (vmin down, vmax up) and clipped to [0, 65535]."""
    lo = int(np.floor(vmin / k) * k)
    hi = int(np.ceil(vmax / k) * k)
    return max(0, lo), min(65535, hi)
