"""Dense local speckle contrast on the GPU (csrc/b4d_smooth.hip, b4d_local_stats): per pixel the mean, the population variance
and the contrast sigma / mu of a sliding window, accumulated in float64 from one read of the frames."""
from __future__ import annotations

import ctypes as C

from .. import _device as D
from .. import _ffi
from .._frames import frame_stack, mode_code, pair, window as size_pair
from ..preprocessing.smooth import gaussian_taps

MAX_SIZE = 63
MAX_HALF_WIDTH = 31


def run_local_stats(t, batch, ny, nx, sy, sx, wy, wx, mode, cval, *, want=("mean", "variance", "contrast")):
    """b4d_local_stats on a float32 device tensor; wy = wx = None is the box window.  Returns {name: tensor} of `want`."""
    torch = _ffi.require_gpu()
    out = {k: torch.empty_like(t) for k in ("mean", "variance", "contrast") if k in want}
    null = C.c_void_p(0)
    p = lambda k: D.ptr(out[k]) if k in out else null  # noqa: E731
    _ffi.check(_ffi.lib().b4d_local_stats(D.ptr(t), batch, ny, nx, int(sy), int(sx), wy.ctypes.data_as(C.c_void_p) if wy is not None else null,
                                          wx.ctypes.data_as(C.c_void_p) if wx is not None else null, int(mode), float(cval), p("mean"),
                                          p("variance"), p("contrast"), _ffi.stream_ptr()))
    return out


def local_contrast(images, size=7, *, window: str = "box", sigma=None, truncate: float = 3.0, mode: str = "reflect", cval: float = 0.0,
                   return_tensors: bool = False):
    """Windowed statistics of every frame ``(H, W)`` or ``(T, H, W)``: ``{"mean", "variance", "contrast"}``, float32 arrays of the
    frames' shape, with ``variance = max(<x^2> - <x>^2, 0)`` (population, ddof 0) and ``contrast = sqrt(variance) / mean`` where
    the mean is positive, NaN elsewhere.

    ``window="box"``: a ``size`` (int or pair ``(y, x)``, 1 .. 63) window of equal weights, placed as SciPy places it.
    ``window="gaussian"``: weights of ``sigma`` (scalar or pair), half-width ``int(truncate * sigma + 0.5)`` <= 31; ``size`` is
    ignored.  A NaN poisons the outputs of every window that contains it."""
    if window not in ("box", "gaussian"):
        raise ValueError(f"window must be 'box' or 'gaussian'; got {window!r}")
    m = mode_code(mode)
    if window == "box":
        sy, sx = size_pair(size, MAX_SIZE)
        wy = wx = None
    else:
        if sigma is None:
            raise ValueError("window='gaussian' needs sigma")
        gy, gx = pair(sigma, "sigma")
        wy = gaussian_taps(gy, 0, truncate, max_half_width=MAX_HALF_WIDTH)
        wx = gaussian_taps(gx, 0, truncate, max_half_width=MAX_HALF_WIDTH)
        sy, sx = int(wy.size), int(wx.size)
    t, batch, ny, nx = frame_stack(images)
    out = run_local_stats(t, batch, ny, nx, sy, sx, wy, wx, m, cval)
    return out if return_tensors else {k: D.to_host(v) for k, v in out.items()}
