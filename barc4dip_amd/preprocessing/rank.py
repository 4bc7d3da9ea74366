"""Spatial median / rank / percentile filters and outlier repair on the GPU (csrc/b4d_rankfilt.hip).

``median_filter``, ``rank_filter`` and ``percentile_filter`` are ``scipy.ndimage``'s functions of the same names for a frame
``(H, W)`` or, frame by frame (SciPy ``size=(1, s, s)``), a stack ``(T, H, W)``.  A rank filter is a selection: on finite
input the result equals SciPy's bit for bit.  Differences from SciPy: the output is always float32 (the reference casts to
float32 before it filters; SciPy keeps the input dtype), windows are rectangles of at most 15 x 15 without ``footprint`` or
``origin``, and NaN is defined: it sorts above +Inf (``np.sort``'s order), where SciPy leaves it unspecified.

``remove_outliers`` replaces hot / dead pixels and zingers by the window median in one pass over the frames.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import frame_stack, mode_code, window
from ..metrics.order import _robust_args      # the outlier rule's arguments: one check for the window and the stack form

MAX_SIZE = 15


def run_rank_filter(t, batch, ny, nx, sy, sx, rank, mode, cval, *, general=False, want_out=True, want_range=False):
    """b4d_rank_filter on a float32 device tensor: (filtered tensor or None, (batch, 2) float32 {nanmin, nanmax} tensor or None)."""
    torch = _ffi.require_gpu()
    out = torch.empty_like(t) if want_out else None
    mm = torch.empty((batch, 2), dtype=torch.float32, device=t.device) if want_range else None
    null = C.c_void_p(0)
    _ffi.check(_ffi.lib().b4d_rank_filter(D.ptr(t), batch, ny, nx, sy, sx, int(rank), int(mode), float(cval), 1 if general else 0,
                                          D.ptr(out) if want_out else null, D.ptr(mm) if want_range else null, _ffi.stream_ptr()))
    return out, mm


def _filter(images, rank_of, size, mode, cval, return_tensors, general):
    sy, sx = window(size, MAX_SIZE)      # argument errors come before the device is asked for
    m = mode_code(mode)
    rank = rank_of(sy * sx)
    t, batch, ny, nx = frame_stack(images)
    out, _ = run_rank_filter(t, batch, ny, nx, sy, sx, rank, m, cval, general=general)
    return out if return_tensors else D.to_host(out)


def median_filter(images, size=3, *, mode: str = "reflect", cval: float = 0.0, return_tensors: bool = False, _general: bool = False):
    """scipy.ndimage.median_filter(images.astype(float32), size) per frame: the element of rank ``n // 2`` of every window.
    Square windows of 3, 5 and 7 run as selection networks on registers, every other size by counting passes."""
    return _filter(images, lambda n: n // 2, size, mode, cval, return_tensors, _general)


def rank_filter(images, rank: int, size=3, *, mode: str = "reflect", cval: float = 0.0, return_tensors: bool = False,
                _general: bool = False):
    """scipy.ndimage.rank_filter per frame; negative ranks count from the top (-1 is the maximum)."""
    def rank_of(n):
        r = int(rank)
        if r != rank:
            raise ValueError(f"rank must be an integer; got {rank!r}")
        r = r + n if r < 0 else r
        if not 0 <= r < n:
            raise ValueError(f"rank {rank} not within the {n} elements of the window")
        return r

    return _filter(images, rank_of, size, mode, cval, return_tensors, _general)


def percentile_filter(images, percentile: float, size=3, *, mode: str = "reflect", cval: float = 0.0, return_tensors: bool = False,
                      _general: bool = False):
    """scipy.ndimage.percentile_filter per frame, with SciPy's rank: p < 0 -> p + 100; p == 100 -> n - 1; else int(n * p / 100)."""
    def rank_of(n):
        p = float(percentile)
        if p < 0.0:
            p += 100.0
        if not 0.0 <= p <= 100.0:
            raise ValueError(f"invalid percentile: {percentile!r}")
        return n - 1 if p == 100.0 else int(float(n) * p / 100.0)

    return _filter(images, rank_of, size, mode, cval, return_tensors, _general)


def remove_outliers(images, size: int = 3, *, threshold: float = 6.0, scale: str = "mad", polarity: str = "both", min_scale: float = 0.0,
                    mode: str = "reflect", cval: float = 0.0, return_mask: bool = False, return_tensors: bool = False):
    """Replace outlying pixels (hot and dead pixels, zingers) by the median of their ``size`` x ``size`` window (3, 5 or 7).

    With ``med`` the window median and ``d = x - med``, all in float32, a pixel is an outlier when
      ``scale="absolute"``: ``|d| > threshold``;
      ``scale="mad"``     : ``|d| > threshold * max(1.4826 * mad, min_scale)``, ``mad`` the median of ``|w - med|`` over the window;
      ``scale="poisson"`` : ``d * d > threshold**2 * max(med, min_scale)`` (counting noise: the variance is the level),
    restricted to ``d > 0`` by ``polarity="hot"`` and to ``d < 0`` by ``"dead"``; a non-finite pixel is always an outlier.
    Returns the repaired frames (float32), or with ``return_mask`` also ``{"mask": bool array of the frames' shape,
    "count": int64 (T,) replaced pixels per frame}``."""
    if np.ndim(size) != 0 or size not in (3, 5, 7):
        raise ValueError(f"size must be 3, 5 or 7; got {size!r}")
    kind, thr, floor_, pol = _robust_args(threshold, scale, polarity, min_scale)
    m = mode_code(mode)
    torch = _ffi.require_gpu()
    t, batch, ny, nx = frame_stack(images)
    out = torch.empty_like(t)
    mask = torch.empty(tuple(t.shape), dtype=torch.uint8, device=t.device) if return_mask else None
    count = torch.empty((batch,), dtype=torch.int64, device=t.device) if return_mask else None
    null = C.c_void_p(0)
    _ffi.check(_ffi.lib().b4d_despeckle(D.ptr(t), batch, ny, nx, int(size), kind, thr, floor_, pol, m, float(cval), D.ptr(out), D.ptr(mask) if return_mask else null,
                                        D.ptr(count) if return_mask else null, _ffi.stream_ptr()))
    frames = out if return_tensors else D.to_host(out)
    if not return_mask:
        return frames
    if return_tensors:
        return frames, {"mask": mask.to(torch.bool), "count": count}
    return frames, {"mask": mask.cpu().numpy().astype(bool), "count": count.cpu().numpy()}
