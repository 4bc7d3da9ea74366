"""The float64 model of speckle scanning (barc4dip_amd.signal.speckle_scan, b4d_speckle_scan): the definition of include/b4d.h,
written with NumPy and scipy.ndimage only.  The GPU tests compare the device against it on the same float32 input
(tests/test_gpu_scanning.py); tests/test_scanning_host.py checks the model itself.

The moments are sums of values from which the global mean of the scan was subtracted first, so that the model keeps its digits at
1 % contrast on 30 000 counts.  Besides the planes it returns, per pixel, the margin between the best and the second-best rho
and the two curvatures a - 2 b + c of the sub-pixel step, which the tests use to leave out pixels that rounding may decide."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

TINY = 1e-12


def hann(w: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(w) + 0.5) / w)


def _pair(v):
    return (int(v[0]), int(v[1])) if np.ndim(v) else (int(v), int(v))


def _window(plane, hy, hx):
    """sum_j sum_i hy[j] hx[i] plane[y - wy // 2 + j, x - wx // 2 + i]; zeros beyond the frame (those pixels are dropped later)."""
    t = ndimage.correlate1d(plane, hy, axis=0, mode="constant", cval=0.0)
    return ndimage.correlate1d(t, hx, axis=1, mode="constant", cval=0.0)


def _shifted(plane, uy, ux):
    """plane[p + u]; wraps at the frame border, which only pixels inside the margin see."""
    return np.roll(plane, (-uy, -ux), axis=(0, 1))


def scan_model(reference, sample, *, window=5, search=4, taper="hann", subpixel=True, weights=None, min_correlation=None) -> dict:
    """One scan: reference and sample (N, H, W), taken as the float32 frames that the device sees.  Returns the planes of
    ``speckle_scan`` (dy, dx, correlation, transmission, dark_field, valid, edge), the integer peak uy, ux (0 where the pixel has
    no result) and margin, curv_y, curv_x (float64 (H, W); a curvature is NaN where the peak lies on the border of that axis)."""
    R = np.asarray(reference).astype(np.float32).astype(np.float64)
    S = np.asarray(sample).astype(np.float32).astype(np.float64)
    N, H, W = R.shape
    assert S.shape == R.shape
    (wy, wx), (sy, sx) = _pair(window), _pair(search)
    g = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    use = np.flatnonzero(g > 0.0)
    gn = g / g.sum()
    hy = hann(wy) if taper == "hann" else np.ones(wy)
    hx = hann(wx) if taper == "hann" else np.ones(wx)
    hy, hx = hy / hy.sum(), hx / hx.sum()

    # values that are not finite: remembered, then 0 (every pixel that sees one is dropped below)
    badR = np.zeros((H, W))
    badS = np.zeros((H, W))
    for n in use:
        badR += ~np.isfinite(R[n])
        badS += ~np.isfinite(S[n])
    R = np.where(np.isfinite(R), R, 0.0)
    S = np.where(np.isfinite(S), S, 0.0)
    mu_r = float(np.mean(R[use]))
    mu_s = float(np.mean(S[use]))
    R, S = R - mu_r, S - mu_s

    def pooled(prod):
        acc = np.zeros((H, W))
        for n in use:
            acc += gn[n] * prod(n)
        return acc

    mR = _window(pooled(lambda n: R[n]), hy, hx)
    VR = _window(pooled(lambda n: R[n] * R[n]), hy, hx) - mR * mR
    mS = _window(pooled(lambda n: S[n]), hy, hx)
    VS = _window(pooled(lambda n: S[n] * S[n]), hy, hx) - mS * mS
    Rm = mR + mu_r

    ky, kx = 2 * sy + 1, 2 * sx + 1
    rho = np.full((ky, kx, H, W), np.nan)
    cov = np.empty((ky, kx, H, W))
    smean = np.empty((ky, kx, H, W))
    with np.errstate(all="ignore"):
        for iy in range(ky):
            for ix in range(kx):
                uy, ux = iy - sy, ix - sx
                X = _window(pooled(lambda n: R[n] * _shifted(S[n], uy, ux)), hy, hx)
                mSu, VSu = _shifted(mS, uy, ux), _shifted(VS, uy, ux)
                Smu = mSu + mu_s
                C = X - mR * mSu
                defined = (VR > TINY * Rm * Rm) & (VSu > TINY * Smu * Smu)
                rho[iy, ix] = np.where(defined, C / np.sqrt(np.where(defined, VR * VSu, 1.0)), np.nan)
                cov[iy, ix] = C
                smean[iy, ix] = Smu

    # pixels without a result
    my, mx = wy // 2 + sy, wx // 2 + sx
    ok = np.zeros((H, W), bool)
    ok[my:H - my, mx:W - mx] = True
    ok &= ndimage.maximum_filter(badR, size=(wy, wx), mode="constant", cval=0.0) == 0
    ok &= ndimage.maximum_filter(badS, size=(wy + 2 * sy, wx + 2 * sx), mode="constant", cval=0.0) == 0
    flat = np.where(np.isnan(rho), -np.inf, rho).reshape(ky * kx, H, W)
    ok &= np.isfinite(flat.max(axis=0))
    k = np.argmax(flat, axis=0)                       # the first among equals, row-major: uy ascending, then ux
    iy, ix = k // kx, k % kx
    yy, xx = np.mgrid[0:H, 0:W]
    best = rho[iy, ix, yy, xx]
    second = np.sort(flat, axis=0)[-2] if ky * kx > 1 else np.full((H, W), -np.inf)
    margin = best - second

    def neighbour(diy, dix):
        jy, jx = np.clip(iy + diy, 0, ky - 1), np.clip(ix + dix, 0, kx - 1)
        return rho[jy, jx, yy, xx]

    edge_y, edge_x = (iy == 0) | (iy == ky - 1), (ix == 0) | (ix == kx - 1)
    curv, delta = [], []
    with np.errstate(all="ignore"):
        for (diy, dix), on_edge in (((1, 0), edge_y), ((0, 1), edge_x)):
            a, c = neighbour(-diy, -dix), neighbour(diy, dix)
            den = a - 2.0 * best + c
            usable = ~on_edge & np.isfinite(den) & (den < 0.0)
            d = np.where(usable, np.clip(0.5 * (a - c) / np.where(usable, den, 1.0), -0.5, 0.5), 0.0)
            curv.append(np.where(on_edge, np.nan, den))
            delta.append(d if subpixel else np.zeros((H, W)))
        T = smean[iy, ix, yy, xx] / Rm
        dark = cov[iy, ix, yy, xx] / (VR * T)
    nan = np.where(ok, 0.0, np.nan)
    out = {"dy": (iy - sy) + delta[0] + nan, "dx": (ix - sx) + delta[1] + nan, "correlation": best + nan,
           "transmission": T + nan, "dark_field": dark + nan, "edge": ok & (edge_y | edge_x), "valid": ok.copy(),
           "uy": np.where(ok, iy - sy, 0), "ux": np.where(ok, ix - sx, 0), "margin": np.where(ok, margin, np.nan), "curv_y": np.where(ok, curv[0], np.nan), "curv_x": np.where(ok, curv[1], np.nan)}
    if min_correlation is not None:
        with np.errstate(invalid="ignore"):
            out["valid"] = ok & (out["correlation"] >= min_correlation)
    return out


def band_limited(shape, seed, sigma=1.0):
    """Seeded random frames, Gaussian-filtered with ``sigma`` px per frame, scaled to mean 100 and standard deviation 25."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    a = ndimage.gaussian_filter(a, sigma=(0,) * (a.ndim - 2) + (sigma, sigma), mode="wrap")
    return 100.0 + 25.0 * a / a.std()
