"""Linear separable filters on the GPU (csrc/b4d_smooth.hip): Gaussian and box filters, envelope removal.

``gaussian_filter`` and ``uniform_filter`` are ``scipy.ndimage``'s functions of the same names for a frame ``(H, W)`` or, frame by
frame (SciPy ``sigma=(0, sy, sx)``), a stack ``(T, H, W)``; ``separable_filter`` is the primitive below them: one 1-D tap array per
axis, applied as a correlation with SciPy's placement (``scipy.ndimage.correlate1d``, ``origin=0``) along x first, then along y.
``remove_envelope`` divides a frame by (or subtracts from it) its own Gaussian-smoothed copy in the filter's last pass.

Windows of half-width up to 4 take the fused route (one launch, both passes in LDS), longer ones the two-pass route; both give the
same bits.  ``_general=True`` takes the two-pass route everywhere and ``_fused=True`` the fused route up to 49 taps (for tests and
timing).

Differences from SciPy: the output is always float32 and the arithmetic is float32 FMA (error bound: DESIGN.md section 26.5),
windows have at most 511 taps per axis, there is no ``origin``.  SciPy filters y first and x second; with a linear filter the
order only shows under ``mode="constant"`` with ``cval != 0`` and taps that do not sum to one (derivative orders), where the
values within a half-width of the frame's border differ.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import frame_stack, mode_code, pair, window

MAX_TAPS = 511
MAX_HALF_WIDTH = 255
_EPILOGUES = {"none": 0, "subtract": 1, "divide": 2}


def gaussian_taps(sigma: float, order: int = 0, truncate: float = 4.0, radius=None, *, max_half_width: int = MAX_HALF_WIDTH) -> np.ndarray:
    """Correlation taps (float64) of scipy.ndimage.gaussian_filter1d: exp(-x^2 / 2 sigma^2) on x = -lw .. lw with
    lw = radius or int(truncate * sigma + 0.5), normalised to sum 1, times the derivative's polynomial (order 1: -x / sigma^2;
    order 2: x^2 / sigma^4 - 1 / sigma^2), and reversed.  sigma == 0 gives the identity {1}."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma < 0.0:
        raise ValueError(f"sigma must be finite and >= 0; got {sigma!r}")
    if order not in (0, 1, 2) or isinstance(order, bool):
        raise ValueError(f"order must be 0, 1 or 2; got {order!r}")
    if sigma == 0.0:
        return np.ones(1)
    if radius is None:
        if not np.isfinite(truncate) or truncate < 0.0:
            raise ValueError(f"truncate must be finite and >= 0; got {truncate!r}")
        lw = int(float(truncate) * sigma + 0.5)
    else:
        if int(radius) != radius or radius < 0:
            raise ValueError(f"radius must be a non-negative integer; got {radius!r}")
        lw = int(radius)
    if lw > max_half_width:
        raise ValueError(f"the Gaussian's half-width {lw} exceeds the limit of {max_half_width} (sigma {sigma}, truncate {truncate})")
    sigma2 = sigma * sigma
    x = np.arange(-lw, lw + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    phi = phi / phi.sum()
    if order == 1:
        phi = (x * (-1.0 / sigma2)) * phi
    elif order == 2:
        phi = (-1.0 / sigma2 + x ** 2 * (1.0 / (sigma2 * sigma2))) * phi
    return np.ascontiguousarray(phi[::-1])


def _weights(w, name) -> np.ndarray:
    """float64 taps of one axis; None is the identity."""
    if w is None:
        return np.ones(1)
    a = np.ascontiguousarray(w, dtype=np.float64)
    if a.ndim != 1 or not 1 <= a.size <= MAX_TAPS:
        raise ValueError(f"{name} must be a 1-D array of 1 .. {MAX_TAPS} taps; got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return a


def run_separable(t, batch, ny, nx, wy, wx, mode, cval, *, epilogue=0, eps=0.0, general=False, wide_fused=False):
    """b4d_separable_filter on a float32 device tensor with float64 host taps; returns the filtered tensor.  `general` takes the
    two-pass route everywhere, `wide_fused` the fused route up to 49 taps (tools/bench_smoothing.py times the boundary with them)."""
    torch = _ffi.require_gpu()
    out = torch.empty_like(t)
    _ffi.check(_ffi.lib().b4d_separable_filter(D.ptr(t), batch, ny, nx, wy.ctypes.data_as(C.c_void_p), int(wy.size), wx.ctypes.data_as(C.c_void_p),
                                               int(wx.size), int(mode), float(cval), int(epilogue), float(eps), (1 if general else 0) | (2 if wide_fused else 0), D.ptr(out),
                                               _ffi.stream_ptr()))
    return out


def _apply(images, wy, wx, mode, cval, return_tensors, general, fused, epilogue=0, eps=0.0):
    m = mode_code(mode)      # argument errors come before the device is asked for
    cval = float(cval)
    t, batch, ny, nx = frame_stack(images)
    out = run_separable(t, batch, ny, nx, wy, wx, m, cval, epilogue=epilogue, eps=eps, general=general, wide_fused=fused)
    return out if return_tensors else D.to_host(out)


def separable_filter(images, weights_y, weights_x, *, mode: str = "reflect", cval: float = 0.0, return_tensors: bool = False,
                     _general: bool = False, _fused: bool = False):
    """``correlate1d(correlate1d(images, weights_x, axis=-1), weights_y, axis=-2)`` per frame in float32; a weight array of
    ``None`` leaves its axis alone.  An even number of taps puts the longer side of the window on the left, as SciPy does."""
    return _apply(images, _weights(weights_y, "weights_y"), _weights(weights_x, "weights_x"), mode, cval, return_tensors, _general, _fused)


def gaussian_filter(images, sigma, *, order=0, mode: str = "reflect", cval: float = 0.0, truncate: float = 4.0, radius=None,
                    return_tensors: bool = False, _general: bool = False, _fused: bool = False):
    """scipy.ndimage.gaussian_filter per frame.  ``sigma``, ``order`` (0, 1 or 2) and ``radius`` are scalars or pairs ``(y, x)``;
    ``sigma == 0`` on an axis leaves that axis alone.  Half-widths up to 255."""
    sy, sx = pair(sigma, "sigma")
    oy, ox = pair(order, "order", int)
    ry, rx = (None, None) if radius is None else pair(radius, "radius", int)
    wy, wx = gaussian_taps(sy, oy, truncate, ry), gaussian_taps(sx, ox, truncate, rx)
    return _apply(images, wy, wx, mode, cval, return_tensors, _general, _fused)


def uniform_filter(images, size=3, *, mode: str = "reflect", cval: float = 0.0, return_tensors: bool = False, _general: bool = False, _fused: bool = False):
    """scipy.ndimage.uniform_filter per frame: the mean of a ``size_y`` x ``size_x`` window, each side in 1 .. 511."""
    sy, sx = window(size, MAX_TAPS)
    return _apply(images, np.full(sy, 1.0 / sy), np.full(sx, 1.0 / sx), mode, cval, return_tensors, _general, _fused)


def remove_envelope(images, sigma, *, method: str = "divide", eps=None, mode: str = "reflect", cval: float = 0.0, truncate: float = 4.0,
                    return_tensors: bool = False, _general: bool = False, _fused: bool = False):
    """Remove the slowly varying beam envelope ``g = gaussian_filter(x, sigma)`` from every frame: ``x / max(g, eps)`` for
    ``method="divide"`` (``eps=None``: the smallest normal float32), ``x - g`` for ``"subtract"``.  It costs no pass over
    memory beyond the filter's own: the quotient is formed where the filter's last pass has ``g`` in registers."""
    if method not in ("divide", "subtract"):
        raise ValueError(f"method must be 'divide' or 'subtract'; got {method!r}")
    eps = float(np.finfo(np.float32).tiny) if eps is None else float(eps)
    if not eps > 0.0:
        raise ValueError(f"eps must be > 0; got {eps!r}")
    sy, sx = pair(sigma, "sigma")
    wy, wx = gaussian_taps(sy, 0, truncate), gaussian_taps(sx, 0, truncate)
    return _apply(images, wy, wx, mode, cval, return_tensors, _general, _fused, epilogue=_EPILOGUES[method], eps=eps)
