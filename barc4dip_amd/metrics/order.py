"""Per-pixel order statistics along the frame axis of a stack on the GPU (csrc/b4d_torder.hip).

``temporal_median``, ``temporal_percentile`` and ``temporal_robust_mean`` reduce a stack ``(T, H, W)`` to frames ``(H, W)``.

Semantics.  Per pixel the T samples (cast to float32) are sorted in ``np.sort``'s order (NaN above +Inf).  ``ignore_nan=False``
("propagate"): all T samples take part and a pixel with any NaN is NaN (``np.percentile``, ``np.median``); ``ignore_nan=True``
("omit"): the n non-NaN samples take part and n = 0 gives NaN (``np.nanpercentile``, ``np.nanmedian``).  With ``s[0..n)`` the
sorted samples taking part, ``q`` a fraction in [0, 1] and ``h = q (n - 1)`` in float64, the methods are NumPy's
  linear: ``i = floor(h)``, ``g = h - i``;  lower: ``i = floor(h)``, ``g = 0``;  higher: ``i = ceil(h)``, ``g = 0``;
  nearest: ``i = rint(h)`` (half to even), ``g = 0``;  midpoint: ``i = floor(h)``, ``g = 0.5`` if ``h > i``, else 0.
Where ``g == 0`` the result is ``s[i]`` itself; otherwise it is ``float32(a + (b - a) g)`` with ``a = float64(s[i])``,
``b = float64(s[i + 1])``, each operation rounded once in float64.  Selections are exact, so every quantile equals this model bit
for bit; the lower, higher and nearest methods and the median (``q = 0.5``, midpoint) of finite data equal NumPy's float32
results, linear and midpoint lie within 2 float32 ulps of NumPy's own float32 interpolation.

Robust mean.  A sample that is not finite takes no part and counts as rejected; n is the count of finite samples, ``med`` their
midpoint median, ``d = x - med`` in float32, ``mad`` the midpoint median of ``|d|``.  A sample is rejected when
  ``scale="absolute"``: ``|d| > threshold``;  ``scale="mad"``: ``|d| > threshold * max(1.4826 * mad, min_scale)``;
  ``scale="poisson"``: ``d * d > threshold**2 * max(med, min_scale)``,
restricted to ``d > 0`` by ``polarity="hot"`` and to ``d < 0`` by ``"dead"`` -- the rules of ``preprocessing.remove_outliers``
along T.  The mean of the kept samples is formed in float64 and rounded once to float32; no kept sample gives NaN.
MAD degeneracy: if more than half of a pixel's samples are equal, ``mad`` is 0, and with ``min_scale=0`` every sample that
differs from the median is rejected.  Give ``min_scale`` a floor (a read-noise level) for data with many ties.

Stacks of at most 1024 frames; T <= 64 is sorted in registers in one read of the stack.  A host source (NumPy array, memory map or
anything sliceable with a ``shape``) whose float32 image exceeds ``max_bytes`` is processed in bands of rows; the results are the
same bits as those of a resident call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi

MAX_T = 1024
MAX_Q = 8                      # quantiles per call of b4d_temporal_quantiles; longer lists go down in groups
DEFAULT_MAX_BYTES = 8 << 30
_METHODS = {"linear": 0, "lower": 1, "higher": 2, "nearest": 3, "midpoint": 4}
_SCALES = {"absolute": 0, "mad": 1, "poisson": 2}
_POLARITIES = {"both": 0, "hot": 1, "dead": 2}


# ------------------------------------------------------------------------------------------------ arguments and bands
def _source(stack):
    """`stack` as something with a shape and slicing, and its checked (T, H, W)."""
    if not hasattr(stack, "shape"):
        stack = np.asarray(stack)
    shape = tuple(int(v) for v in stack.shape)
    if len(shape) != 3:
        raise ValueError(f"stack must be (T, H, W); got shape {shape}")
    if min(shape) < 1:
        raise ValueError(f"stack must not be empty; got shape {shape}")
    if shape[0] > MAX_T:
        raise NotImplementedError(f"temporal order statistics take at most {MAX_T} frames; got {shape[0]}")
    return stack, shape


def row_bands(shape, max_bytes):
    """[(r0, r1), ..] covering the H rows of a (T, H, W) stack so that the float32 image of a band stays within max_bytes (a band
    has at least one row); one band if the whole stack does."""
    T, H, W = (int(v) for v in shape)
    max_bytes = int(max_bytes)
    if max_bytes < 1:
        raise ValueError("max_bytes must be positive")
    if 4 * T * H * W <= max_bytes:
        return [(0, H)]
    rows = max(1, max_bytes // (4 * T * W))
    return [(r0, min(H, r0 + rows)) for r0 in range(0, H, rows)]


def _fractions(q):
    """(float64 fractions, scalar?) of percentiles in [0, 100]."""
    scalar = np.ndim(q) == 0
    p = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if p.ndim != 1 or p.size < 1:
        raise ValueError("q must be a scalar or a non-empty sequence of percentiles")
    if not np.all((p >= 0.0) & (p <= 100.0)):      # NaN fails both
        raise ValueError("Percentiles must be in the range [0, 100]")
    return p / 100.0, scalar


def _robust_args(threshold, scale, polarity, min_scale):
    if scale not in _SCALES:
        raise ValueError(f"Invalid scale option: {scale!r} (expected one of {sorted(_SCALES)})")
    if polarity not in _POLARITIES:
        raise ValueError(f"Invalid polarity: {polarity!r} (expected one of {sorted(_POLARITIES)})")
    if not float(threshold) >= 0.0 or not float(min_scale) >= 0.0:
        raise ValueError("threshold and min_scale must be >= 0")
    return _SCALES[scale], float(threshold), float(min_scale), _POLARITIES[polarity]


def over_bands(stack, shape, max_bytes, fn, return_tensors):
    """fn(float32 device tensor (T, rows, W)) -> tuple of device tensors (.., rows, W) or None, for every band of rows; the
    results joined along the rows (as device tensors, or band by band on the host)."""
    torch = _ffi.require_gpu()
    resident = D.is_tensor(stack) or len(row_bands(shape, max_bytes)) == 1
    bands = [(0, shape[1])] if resident else row_bands(shape, max_bytes)
    parts = []
    for r0, r1 in bands:
        t, _, _ = D.to_device_f32(stack if resident else np.asarray(stack[:, r0:r1, :]), ndim=(3,))
        res = fn(t)
        parts.append(res if return_tensors else tuple(None if r is None else D.to_host(r) for r in res))
    if len(parts) == 1:
        return parts[0]
    join = (lambda xs: torch.cat(xs, dim=-2)) if return_tensors else (lambda xs: np.concatenate(xs, axis=-2))
    return tuple(None if parts[0][k] is None else join([p[k] for p in parts]) for k in range(len(parts[0])))


# ------------------------------------------------------------------------------------------------ the two entry points of the ABI
def run_quantiles(t, fractions, method: int, nan_policy: int, *, general: bool = False, want_count: bool = False):
    """b4d_temporal_quantiles on a float32 device tensor (T, h, w): ((Q, h, w) float32 tensor, (h, w) int16 count tensor or None)."""
    torch = _ffi.require_gpu()
    T, h, w = (int(v) for v in t.shape)
    fr = np.ascontiguousarray(fractions, dtype=np.float64)
    out = torch.empty((fr.size, h, w), dtype=torch.float32, device=t.device)
    nv = torch.empty((h, w), dtype=torch.int16, device=t.device) if want_count else None
    lib, null = _ffi.lib(), C.c_void_p(0)
    for k in range(0, fr.size, MAX_Q):
        part = np.ascontiguousarray(fr[k:k + MAX_Q])
        _ffi.check(lib.b4d_temporal_quantiles(D.ptr(t), T, h * w, h * w, part.ctypes.data_as(C.c_void_p), int(part.size), int(method),
                                              int(nan_policy), 1 if general else 0, D.ptr(out[k]),
                                              D.ptr(nv) if (want_count and k == 0) else null, _ffi.stream_ptr()))
    return out, nv


def run_robust_mean(t, scale_kind: int, threshold: float, min_scale: float, polarity: int, *, general: bool = False,
                    want_info: bool = False, want_mask: bool = False, want_cleaned: bool = False):
    """b4d_temporal_robust_mean on a float32 device tensor (T, h, w): (mean, median, scale, n_kept (int16), rejected (uint8),
    cleaned), None for what was not asked for."""
    torch = _ffi.require_gpu()
    T, h, w = (int(v) for v in t.shape)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=t.device)  # noqa: E731
    mean = new((h, w), torch.float32)
    med = new((h, w), torch.float32) if want_info else None
    sc = new((h, w), torch.float32) if want_info else None
    nk = new((h, w), torch.int16) if want_info else None
    rej = new((T, h, w), torch.uint8) if want_mask else None
    cl = new((T, h, w), torch.float32) if want_cleaned else None
    null = C.c_void_p(0)
    p = lambda x: D.ptr(x) if x is not None else null  # noqa: E731
    _ffi.check(_ffi.lib().b4d_temporal_robust_mean(D.ptr(t), T, h * w, h * w, int(scale_kind), float(threshold), float(min_scale),
                                                   int(polarity), 1 if general else 0, D.ptr(mean), p(med), p(sc), p(nk), p(rej), p(cl),
                                                   h * w, _ffi.stream_ptr()))
    return mean, med, sc, nk, rej, cl


# ------------------------------------------------------------------------------------------------ public functions
def temporal_percentile(stack, q, *, method: str = "linear", ignore_nan: bool = False, return_count: bool = False,
                        return_tensors: bool = False, max_bytes: int = DEFAULT_MAX_BYTES, _general: bool = False):
    """np.percentile(stack.astype(float32), q, axis=0, method=method) (``ignore_nan``: np.nanpercentile) as float32: ``(H, W)``
    for a scalar ``q`` in percent, ``(Q, H, W)`` for a sequence.  ``return_count`` adds the (H, W) count of non-NaN samples."""
    fractions, scalar = _fractions(q)      # argument errors come before the device is asked for
    if method not in _METHODS:
        raise ValueError(f"Invalid method: {method!r} (expected one of {sorted(_METHODS)})")
    stack, shape = _source(stack)
    row_bands(shape, max_bytes)

    def fn(t):
        return run_quantiles(t, fractions, _METHODS[method], 1 if ignore_nan else 0, general=_general, want_count=return_count)

    out, nv = over_bands(stack, shape, max_bytes, fn, return_tensors)
    res = out[0] if scalar else out
    if not return_count:
        return res
    return res, (nv.to(_ffi.require_gpu().int32) if return_tensors else nv.astype(np.int32))


def temporal_median(stack, *, ignore_nan: bool = False, return_tensors: bool = False, max_bytes: int = DEFAULT_MAX_BYTES,
                    _general: bool = False):
    """np.median(stack.astype(float32), axis=0) (``ignore_nan``: np.nanmedian): ``(H, W)`` float32."""
    return temporal_percentile(stack, 50.0, method="midpoint", ignore_nan=ignore_nan, return_tensors=return_tensors, max_bytes=max_bytes,
                               _general=_general)


def temporal_robust_mean(stack, *, threshold: float = 5.0, scale: str = "mad", polarity: str = "both", min_scale: float = 0.0,
                         return_info: bool = False, return_mask: bool = False, return_tensors: bool = False,
                         max_bytes: int = DEFAULT_MAX_BYTES, _general: bool = False):
    """Mean along T of the samples that lie within ``threshold`` scales of the per-pixel median (module docstring): ``(H, W)``
    float32.  ``return_info`` adds ``{"median", "scale", "n_kept"}`` -- the (H, W) median, the right-hand side of the test that
    was applied, and the count of kept samples; ``return_mask`` (which implies it) also ``"rejected"``, the (T, H, W) bool mask."""
    kind, thr, floor_, pol = _robust_args(threshold, scale, polarity, min_scale)
    stack, shape = _source(stack)
    row_bands(shape, max_bytes)
    info = return_info or return_mask

    def fn(t):
        return run_robust_mean(t, kind, thr, floor_, pol, general=_general, want_info=info, want_mask=return_mask)

    mean, med, sc, nk, rej, _ = over_bands(stack, shape, max_bytes, fn, return_tensors)
    if not info:
        return mean
    torch = _ffi.require_gpu()
    out = {"median": med, "scale": sc, "n_kept": nk.to(torch.int32) if return_tensors else nk.astype(np.int32)}
    if return_mask:
        out["rejected"] = rej.to(torch.bool) if return_tensors else rej.astype(bool)
    return mean, out
