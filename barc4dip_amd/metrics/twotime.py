"""Two-time correlation of a stack of speckle frames: how fast, where, and whether evenly in time a pattern decorrelates.

``two_time_correlation`` gives, per region of a label map, the T x T matrix C[t1, t2] of the frames' correlation over the
region's pixels, the per-frame mean, variance and contrast, and the lag curve g2(tau) read along the matrix's diagonals with its
standard error.  The definitions are those of ``include/b4d.h`` (b4d_two_time); the arithmetic runs on the float32 matrix cores
with centred data and float64 everywhere across chunks.  There is no CPU path.

``correlation_decay`` is host NumPy: the lag at which the normalised g2 falls below a level.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from ._regions import MAX_REGIONS, _host, region_map, stack_shape

NORMS = {"pearson": 0, "intensity": 1, "covariance": 2}
MAX_FRAMES = 2048
CHUNK = 2048            # pixels of a region per float32 accumulation (TT_KC, csrc/b4d_twotime.hip)


def _check(images, labels, mask, norm, max_lag):
    """Every argument error, before the GPU is touched.  Returns (T, H, W, host label map as int32 or None, R, norm code, L)."""
    if D.is_tensor(images):
        shape, cplx = tuple(int(s) for s in images.shape), bool(images.is_complex())
    else:
        images = np.asarray(images)
        shape, cplx = images.shape, np.iscomplexobj(images)
    T, H, W = stack_shape(shape, cplx, "two_time_correlation")
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
    if max_lag is None:
        L = T - 1
    else:
        if isinstance(max_lag, bool) or int(max_lag) != max_lag or not 0 <= int(max_lag) <= T - 1:
            raise ValueError(f"max_lag must be an integer in 0 .. T - 1 = {T - 1}, got {max_lag!r}")
        L = int(max_lag)
    lab, R = region_map(labels, mask, H, W)
    if T > MAX_FRAMES or R > MAX_REGIONS or H * W >= 2 ** 31:
        raise NotImplementedError(f"two_time_correlation: T <= {MAX_FRAMES}, at most {MAX_REGIONS} regions and fewer than 2^31 "
                                  f"pixels per frame (got T = {T}, R = {R}, {H} x {W})")
    return T, H, W, lab, R, NORMS[norm], L


def two_time_correlation(images, *, labels=None, mask=None, norm: str = "pearson", max_lag: int | None = None,
                         return_tensors: bool = False) -> dict:
    """Two-time correlation matrix, per-frame statistics and lag curve of a stack of frames.

    images: (T, H, W), NumPy of any real dtype or a ROCm tensor; 2 <= T <= 2048.
    labels: (H, W) integer map, 0 = pixel not used, 1 .. R = regions (R = its largest value, at most 64).
    mask:   (H, W) bool map of the one region; with neither, all pixels form it.  A pixel that is NaN or +-Inf in any frame
            takes no part.
    norm:   "pearson"    C_ij = cov_ij / sqrt(var_i var_j)
            "intensity"  C_ij = 1 + cov_ij / (m_i m_j) = <I_i I_j> / (<I_i><I_j>), the XPCS two-time function
            "covariance" C_ij = cov_ij
    max_lag: L in 0 .. T - 1 (default T - 1); entries with |i - j| > L are NaN and frame blocks wholly outside the band are
            not computed.

    Returns a dict of float64 arrays (device tensors with ``return_tensors=True``); with ``labels`` every array has a leading
    R axis, otherwise not: ``two_time`` (T, T), ``mean``, ``var``, ``contrast`` (T,), ``n_pixels`` int64, ``lags`` arange(L + 1),
    ``g2``, ``g2_err`` (L + 1,), and ``meta`` {norm, max_lag, n_regions}.  A quotient whose denominator is not above 0 is NaN
    (a constant frame under "pearson", a frame of mean 0 under "intensity"); a region without pixels is NaN with n_pixels 0.
    The matrix is exactly symmetric and the same bits from run to run.  Argument errors are raised before the GPU is touched."""
    T, H, W, lab, R, code, L = _check(images, labels, mask, norm, max_lag)
    torch = _ffi.require_gpu()
    x = D.to_device_f32(images, ndim=(3,))[0].reshape(T, H * W)
    dev = x.device
    lab_dev = torch.from_numpy(lab.reshape(-1)).to(dev) if lab is not None else None
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    nbytes = int(lib.b4d_two_time_workspace_bytes(T, H * W, R, L))
    if nbytes == 0:
        raise NotImplementedError(f"two_time_correlation: no native path for T = {T}, {H} x {W}, {R} regions")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    C2 = torch.empty((R, T, T), dtype=torch.float64, device=dev)
    mean = torch.empty((R, T), dtype=torch.float64, device=dev)
    var = torch.empty((R, T), dtype=torch.float64, device=dev)
    npx = torch.empty((R,), dtype=torch.int64, device=dev)
    g2 = torch.empty((R, L + 1), dtype=torch.float64, device=dev)
    g2e = torch.empty((R, L + 1), dtype=torch.float64, device=dev)
    _ffi.check(lib.b4d_two_time(D.ptr(x), T, H * W, D.ptr(lab_dev) if lab_dev is not None else None, R, code, L, D.ptr(ws),
                                D.ptr(C2), D.ptr(mean), D.ptr(var), D.ptr(npx), st))
    _ffi.check(lib.b4d_two_time_lags(D.ptr(C2), R, T, L, D.ptr(g2), D.ptr(g2e), st))
    nan = torch.full_like(var, float("nan"))
    contrast = torch.where((var > 0) & (mean > 0), torch.sqrt(torch.where(var > 0, var, nan)) / mean, nan)
    out = {"two_time": C2, "mean": mean, "var": var, "contrast": contrast, "n_pixels": npx,
           "lags": torch.arange(L + 1, device=dev), "g2": g2, "g2_err": g2e}
    if labels is None:
        out = {k: (v if k == "lags" else v[0]) for k, v in out.items()}
    if not return_tensors:
        out = {k: v.cpu().numpy() for k, v in out.items()}
    out["meta"] = {"norm": norm, "max_lag": L, "n_regions": R}
    return out


def correlation_decay(result_or_g2, *, level: float = 1.0 / np.e, baseline: float | None = None, lags=None) -> np.ndarray:
    """Lag at which the normalised lag curve g = (g2 - b) / (g2[0] - b) first falls below ``level``, per region.

    result_or_g2: the dict of ``two_time_correlation`` (then b defaults to 1 for norm "intensity" and to 0 otherwise), the dict of
    ``multi_tau_correlation`` (b defaults to 1), or a g2 array of shape (L + 1,) or (R, L + 1) (b defaults to 0).
    lags: the delays of the curve's entries, shape (L + 1,), increasing; default ``result["lags"]`` for a dict and 0, 1 .. L for
    an array.  The lag is interpolated linearly between the last lag at or above the level and the first below it; NaN where g
    never falls below the level.  Returns a float64 array of shape () or (R,)."""
    if isinstance(result_or_g2, dict):
        g2 = result_or_g2["g2"]
        meta = result_or_g2.get("meta", {})
        if baseline is None:
            baseline = 1.0 if meta.get("norm") == "intensity" or "lags_per_level" in meta else 0.0
        if lags is None:
            lags = result_or_g2.get("lags")
    else:
        g2 = result_or_g2
    b = 0.0 if baseline is None else float(baseline)
    g2 = np.asarray(_host(g2), dtype=np.float64)
    if g2.ndim not in (1, 2) or g2.shape[-1] < 1:
        raise ValueError(f"g2 must have shape (L + 1,) or (R, L + 1), got {g2.shape}")
    lag = np.arange(g2.shape[-1], dtype=np.float64) if lags is None else np.asarray(_host(lags), dtype=np.float64)
    if lag.shape != g2.shape[-1:]:
        raise ValueError(f"lags must have shape {g2.shape[-1:]}, got {lag.shape}")
    rows = np.atleast_2d(g2)
    out = np.full(rows.shape[0], np.nan)
    for r, row in enumerate(rows):
        with np.errstate(invalid="ignore", divide="ignore"):
            g = (row - b) / (row[0] - b)
        below = np.flatnonzero(g < level)
        if below.size == 0:
            continue
        k = int(below[0])
        out[r] = lag[0] if k == 0 else lag[k - 1] + (g[k - 1] - level) / (g[k - 1] - g[k]) * (lag[k] - lag[k - 1])
    return out.reshape(g2.shape[:-1])
