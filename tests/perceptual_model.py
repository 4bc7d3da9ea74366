"""float64 NumPy / SciPy models of csrc/b4d_perceptual.hip and the error bounds of DESIGN.md section 28.

SSIM: the five window sums are scipy.ndimage.correlate1d (along x, then along y, the same float64 taps) of the float64 cast of the
float32 frames, padded in two dimensions by the border index of tests/smoothing_model.py; the quantities then repeat include/b4d.h
operation by operation.  pool2 is restated in float32 (bit for bit), the error sums in NumPy.  Every bound is formed from the data;
no tolerance is picked by hand."""
from __future__ import annotations

import os
import sys

import numpy as np
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smoothing_model as SM  # noqa: E402

MODES = SM.MODES
EPS = 2.0 ** -53
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
ulp32 = SM.ulp32
gaussian_taps = SM.gaussian_taps


def ssim_taps(sigma: float = 1.5, truncate: float = 3.5) -> np.ndarray:
    """The default window: 11 taps."""
    return gaussian_taps(sigma, 0, truncate)


def pad2(x, sy: int, sx: int, mode: str, cval: float) -> np.ndarray:
    """x (.., ny, nx) float64 with the halo of an sy x sx window (SciPy's placement), padded in two dimensions."""
    x = np.asarray(x, dtype=np.float64)
    ny, nx = x.shape[-2:]
    iy = SM.border_index(np.arange(ny + sy - 1) - sy // 2, ny, mode)
    ix = SM.border_index(np.arange(nx + sx - 1) - sx // 2, nx, mode)
    p = SM._take(SM._take(x, iy, x.ndim - 2, cval), ix, x.ndim - 1, cval)
    if mode == "constant":      # a corner: outside on either axis is cval
        p = np.where((iy < 0)[:, None] | (ix < 0)[None, :], cval, p)
    return p


def window_sum(p, wy, wx, ny: int, nx: int) -> np.ndarray:
    """sum_j sum_k wy[j] wx[k] p[y + j, x + k] by correlate1d along x, then y (its output i + n // 2 is the sum that starts at i)."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = ndi.correlate1d(p, wx, axis=-1, mode="constant", cval=0.0)[..., wx.size // 2: wx.size // 2 + nx]
        return ndi.correlate1d(a, wy, axis=-2, mode="constant", cval=0.0)[..., wy.size // 2: wy.size // 2 + ny, :]


def window_weight(wy, wx) -> float:
    """W as the kernel sums it: the x taps in ascending order, then sum_j wy[j] * that."""
    sx = 0.0
    for w in wx:
        sx += float(w)
    W = 0.0
    for w in wy:
        W += float(w) * sx
    return W


def model_ssim(r, x, sy: int, sx: int, wy=None, wx=None, mode: str = "reflect", cval: float = 0.0, c1: float = 1.0, c2: float = 1.0,
               cov_norm: float = 1.0, crop=(0, 0)) -> dict:
    """ssim_map, cs_map (float64), their means over the cropped region per frame, and the bounds `tol_*` of the kernel's values
    against them.  r and x broadcast against each other (a shared reference frame)."""
    r = np.asarray(r, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    r, x = np.broadcast_arrays(r, x)
    ny, nx = x.shape[-2:]
    box = wy is None
    wy = np.ones(sy) if box else np.asarray(wy, dtype=np.float64)
    wx = np.ones(sx) if box else np.asarray(wx, dtype=np.float64)
    W = float(sy * sx) if box else window_weight(wy, wx)
    pr, px = pad2(r, sy, sx, mode, cval), pad2(x, sy, sx, mode, cval)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        S = lambda a: window_sum(a, wy, wx, ny, nx)  # noqa: E731
        iw = 1.0 / W
        mr, mx = S(pr) * iw, S(px) * iw
        qrr, qxx, qrx = S(pr * pr) * iw, S(px * px) * iw, S(pr * px) * iw
        vr = cov_norm * (qrr - mr * mr)
        vx = cov_norm * (qxx - mx * mx)
        vrx = cov_norm * (qrx - mr * mx)
        n2, d2 = 2.0 * vrx + c2, vr + vx + c2
        cs = n2 / d2
        n1, d1 = 2.0 * (mr * mx) + c1, mr * mr + mx * mx + c1
        lum = n1 / d1
        ssim = lum * cs
        # ---- bounds: g = 2 (K + 4) 2^-53 covers the kernel's and the model's own rounding of a K-term sum and of the few
        # operations behind it; magnitudes are the window sums of the absolute values
        aw_y, aw_x = np.abs(wy), np.abs(wx)
        A = lambda a: window_sum(np.abs(a), aw_y, aw_x, ny, nx) / abs(W)  # noqa: E731
        g = 2.0 * (sy * sx + 4) * EPS
        e_mr, e_mx = g * A(pr), g * A(px)
        amr, amx = np.abs(mr), np.abs(mx)
        e_vr = cov_norm * (g * (A(pr * pr) + mr * mr) + 2.0 * amr * e_mr)
        e_vx = cov_norm * (g * (A(px * px) + mx * mx) + 2.0 * amx * e_mx)
        e_vrx = cov_norm * (g * (A(pr * px) + amr * amx) + amr * e_mx + amx * e_mr)
        e_n2, e_d2 = 2.0 * e_vrx + 4.0 * EPS * np.abs(n2), e_vr + e_vx + 4.0 * EPS * np.abs(d2)
        e_cs = (e_n2 + np.abs(cs) * e_d2) / (d2 - e_d2) + 2.0 * EPS * np.abs(cs)
        e_n1 = 2.0 * (amr * e_mx + amx * e_mr) + 4.0 * EPS * np.abs(n1)
        e_d1 = 2.0 * (amr * e_mr + amx * e_mx) + 4.0 * EPS * np.abs(d1)
        e_lum = (e_n1 + np.abs(lum) * e_d1) / (d1 - e_d1) + 2.0 * EPS * np.abs(lum)
        e_ssim = np.abs(lum) * e_cs + np.abs(cs) * e_lum + e_lum * e_cs + 2.0 * EPS * np.abs(ssim)
        bad = ~((d2 > e_d2) & (d1 > e_d1))       # a denominator that rounding can take to zero: no bound
        e_cs = np.where(bad, np.inf, e_cs)
        e_ssim = np.where(bad, np.inf, e_ssim)
    cy, cx = crop
    reg = (slice(None),) * (x.ndim - 2) + (slice(cy, ny - cy), slice(cx, nx - cx))
    n = max(1, (ny - 2 * cy) * (nx - 2 * cx))
    out = {"ssim_map": ssim, "cs_map": cs, "tol_ssim_map": ulp32(ssim) + e_ssim, "tol_cs_map": ulp32(cs) + e_cs}
    with np.errstate(invalid="ignore"):
        for k, v, e in (("ssim", ssim, e_ssim), ("cs", cs, e_cs)):
            out[k] = v[reg].mean(axis=(-2, -1))
            out["tol_" + k] = e[reg].mean(axis=(-2, -1)) + n * EPS * np.abs(v[reg]).mean(axis=(-2, -1))   # + the summation term
    return out


def pool2(x) -> np.ndarray:
    """((a + b) + (c + d)) * 0.25 in float32 over 2 x 2 blocks; a trailing odd row or column is dropped."""
    x = np.asarray(x, dtype=np.float32)
    ny, nx = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    a, b = x[..., 0:ny:2, 0:nx:2], x[..., 0:ny:2, 1:nx:2]
    c, d = x[..., 1:ny:2, 0:nx:2], x[..., 1:ny:2, 1:nx:2]
    with np.errstate(invalid="ignore", over="ignore"):
        return (((a + b) + (c + d)) * np.float32(0.25)).astype(np.float32)


def ms_ssim_min_side(size: int, scales: int) -> int:
    """Smallest side that still holds a window of `size` after scales - 1 halvings (each drops an odd row): size * 2^(scales - 1)."""
    n = size
    for _ in range(scales - 1):
        n *= 2
    return n


def model_ms_ssim(r, x, weights=MS_SSIM_WEIGHTS, **kw) -> dict:
    """Per-scale mean ssim and cs ((T, S)), the score and its bound: relative errors of the factors weighted by the exponents."""
    r32, x32 = np.asarray(r, dtype=np.float32), np.asarray(x, dtype=np.float32)
    w = np.asarray(weights, dtype=np.float64)
    ss, cs, es, ec = [], [], [], []
    for s in range(w.size):
        m = model_ssim(r32, x32, **kw)
        ss.append(np.atleast_1d(m["ssim"]))
        cs.append(np.atleast_1d(m["cs"]))
        es.append(np.atleast_1d(m["tol_ssim"]))
        ec.append(np.atleast_1d(m["tol_cs"]))
        if s + 1 < w.size:
            r32, x32 = pool2(r32), pool2(x32)
    ss, cs, es, ec = (np.stack(a, axis=1) for a in (ss, cs, es, ec))
    f = np.maximum(np.concatenate([cs[:, :-1], ss[:, -1:]], axis=1), 0.0)
    e = np.concatenate([ec[:, :-1], es[:, -1:]], axis=1)
    score = np.prod(f ** w[None, :], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.sum(w[None, :] * e / (f - e), axis=1)
        tol = np.where(np.all(f > e, axis=1), score * (rel + 4.0 * (w.size + 1) * EPS), np.inf)   # pow and the product: a few roundings each
    return {"ms_ssim": score, "ssim": ss, "cs": cs, "tol_ms_ssim": tol, "tol_ssim": es, "tol_cs": ec}


def model_pair_errors(r, x) -> dict:
    """The eight columns of b4d_pair_errors per frame and the bound n 2^-53 sum |terms| of the five sums (extrema: exact, 0)."""
    r = np.asarray(r, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    r, x = np.broadcast_arrays(r, x)
    if x.ndim == 2:
        r, x = r[None], x[None]
    n = x.shape[-2] * x.shape[-1]
    d = x - r
    ax = (-2, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [np.sum(d * d, ax), np.sum(np.abs(d), ax), np.max(np.abs(d), ax), np.sum(r * r, ax), np.sum(r, ax), np.min(r, ax), np.max(r, ax),
                np.sum(x, ax)]
        mags = [np.sum(d * d, ax), np.sum(np.abs(d), ax), None, np.sum(r * r, ax), np.sum(np.abs(r), ax), None, None, np.sum(np.abs(x), ax)]
    tol = [np.zeros(x.shape[0]) if m is None else n * EPS * m for m in mags]
    return {"out": np.stack(cols, axis=1), "tol": np.stack(tol, axis=1), "npix": n}


def model_frame_errors(r, x, data_range=None) -> dict:
    """mse, rmse, mae, max_abs, psnr, nrmse (Euclidean) and first-order bounds from those of the sums."""
    m = model_pair_errors(r, x)
    e, t, n = m["out"], m["tol"], m["npix"]
    L = float(np.max(e[:, 6]) - np.min(e[:, 5])) if data_range is None else float(data_range)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = e[:, 0] / n
        t_mse = t[:, 0] / n + EPS * mse
        rmse = np.sqrt(mse)
        t_rmse = np.where(mse > 0, t_mse / (2.0 * rmse), 0.0) + EPS * rmse
        rr = np.sqrt(e[:, 3] / n)
        t_rr = np.where(rr > 0, (t[:, 3] / n) / (2.0 * rr), 0.0) + 2.0 * EPS * rr
        psnr = np.where(mse == 0.0, np.inf, 10.0 * np.log10(L * L / mse))
        t_psnr = np.where(mse == 0.0, 0.0, 10.0 / np.log(10.0) * t_mse / mse + 4.0 * EPS * np.abs(psnr))
        nrmse = rmse / rr
        t_nrmse = t_rmse / rr + nrmse * t_rr / rr + EPS * nrmse
    return {"mse": mse, "rmse": rmse, "mae": e[:, 1] / n, "max_abs": e[:, 2], "psnr": psnr, "nrmse": nrmse, "data_range": L,
            "tol": {"mse": t_mse, "rmse": t_rmse, "mae": t[:, 1] / n + EPS * e[:, 1] / n, "max_abs": np.zeros_like(mse), "psnr": t_psnr,
                    "nrmse": t_nrmse}}
