"""Oracle (test infrastructure, NOT product code): a float64 NumPy model of every reduction / selection entry
point of csrc/b4d_stats.hip, written from the kernel contracts in include/b4d.h.

Each function takes the float32 input the kernel takes and returns what the kernel writes, computed the plain way
(np.sort, np.sum, scipy.ndimage), so that a GPU test can compare raw outputs and not only finished metrics.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from . import metrics_np as M
from . import temporal_np as T


# --------------------------------------------------------------------------- percentiles
def virtual_index(n, q):
    """NumPy's virtual index for method="linear" (alpha = beta = 1), numpy.lib._function_base_impl
    _compute_virtual_index, in its operation order: n*qf + (1 + qf*(1 - 1 - 1)) - 1 with qf = q/100."""
    qf = np.true_divide(np.asarray(q, dtype=np.float64), 100)
    n = np.asarray(n, dtype=np.float64)
    return n * qf + (1.0 + qf * (1.0 - 1.0 - 1.0)) - 1.0


def select_rows(frames, q):
    """b4d_percentiles: (B, ...) frames, nq percentiles -> (B, nq, 4) float64 {x_lo, x_hi, fraction, n_valid} from
    np.sort of the non-NaN values of every frame.  A frame without one gives {NaN, NaN, 0, 0}."""
    f = np.asarray(frames)
    f = f.reshape(f.shape[0], -1)
    qs = np.asarray(q, dtype=np.float64).ravel()
    out = np.empty((f.shape[0], qs.size, 4), dtype=np.float64)
    for b in range(f.shape[0]):
        s = np.sort(f[b][~np.isnan(f[b])])
        n = int(s.size)
        if n == 0:
            out[b] = (np.nan, np.nan, 0.0, 0.0)
            continue
        vi = virtual_index(n, qs)
        fl = np.floor(vi)
        lo = np.clip(fl, 0, n - 1).astype(np.int64)
        hi = np.minimum(lo + 1, n - 1)
        out[b, :, 0] = s[lo]
        out[b, :, 1] = s[hi]
        out[b, :, 2] = vi - fl
        out[b, :, 3] = n
    return out


# --------------------------------------------------------------------------- moments
def moments_rows(frames, *, eps=1e-6, saturation=65535.0):
    """b4d_moments: (B, ...) -> (B, 8) {n_finite, mean, sum d^2, sum d^3, sum d^4, n_zero, n_sat, 0} over the finite
    pixels (d = x - mean); zeros where a frame has no finite pixel.  saturation None = +inf."""
    f = np.asarray(frames)
    f = f.reshape(f.shape[0], -1)
    sat = np.inf if saturation is None else float(saturation)
    out = np.zeros((f.shape[0], 8), dtype=np.float64)
    for b in range(f.shape[0]):
        v = f[b].astype(np.float64)
        v = v[np.isfinite(v)]
        if v.size == 0:
            continue
        mean = np.sum(v) / v.size
        d = v - mean
        d2 = d * d
        out[b] = (v.size, mean, np.sum(d2), np.sum(d2 * d), np.sum(d2 * d2), np.sum(np.abs(v) <= float(eps)),
                  np.sum(v >= sat), 0.0)
    return out


# --------------------------------------------------------------------------- Sobel / Laplace
def sobel_laplace_rows(frames):
    """b4d_sobel_laplace_stats: (B, ny, nx) -> (B, 4) {mean gx^2, mean gy^2, mean lap, mean lap^2} over the pixels
    whose own value is finite (scipy.ndimage sobel / laplace, mode="reflect", float64)."""
    f = np.asarray(frames)
    out = np.empty((f.shape[0], 4), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(f.shape[0]):
            v = f[b].astype(np.float64)
            fin = np.isfinite(v)
            gx = ndimage.sobel(v, axis=1, mode="reflect")
            gy = ndimage.sobel(v, axis=0, mode="reflect")
            lap = ndimage.laplace(v, mode="reflect")
            out[b] = (np.mean((gx * gx)[fin]), np.mean((gy * gy)[fin]), np.mean(lap[fin]), np.mean((lap * lap)[fin]))
    return out


# --------------------------------------------------------------------------- radial profile
def radial_profile(maps, *, r_max=None, nr=None, ntheta=None, fill_value=0.0):
    """b4d_radial_profile (plus the wrapper's fill value): (B, ny, nx) -> ((B, nr) float64, r)."""
    rows = [M.radial_mean_interpolated(np.asarray(m, dtype=np.float64), r_max=r_max, nr=nr, ntheta=ntheta,
                                       fill_value=fill_value) for m in np.asarray(maps)]
    return np.stack([p for p, _ in rows]), rows[0][1]


# --------------------------------------------------------------------------- PSD statistics
def psd_stats_rows(psd):
    """b4d_psd_stats: (B, ny, nx) shifted PSD maps -> (B, 8) {S_disc, sum FR^2 P, sum FX^2 P, sum FY^2 P, sum P^2
    (over the inscribed frequency disc FR <= min(max|fx|, max|fy|)), S_all, sum P ln P over P > 0 (all bins), f95}.
    Non-finite bins and the DC bin count as 0 (metrics_np.bandwidth, lines 234-249).  f95 is NaN for non-square maps
    and where the disc holds no power."""
    p = np.asarray(psd)
    out = np.empty((p.shape[0], 8), dtype=np.float64)
    ny, nx = p.shape[1:]
    fx = np.fft.fftshift(np.fft.fftfreq(nx, d=1.0))
    fy = np.fft.fftshift(np.fft.fftfreq(ny, d=1.0))
    FX, FY = np.meshgrid(fx, fy, indexing="xy")
    FR = np.sqrt(FX * FX + FY * FY)
    m = FR <= min(float(np.max(np.abs(fx))), float(np.max(np.abs(fy))))
    FXm, FYm, FRm = FX[m], FY[m], FR[m]
    order = np.argsort(FRm, kind="stable")
    for b in range(p.shape[0]):
        P = np.nan_to_num(p[b].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
        P[ny // 2, nx // 2] = 0.0
        Pm = P[m]
        tot = float(np.sum(Pm))
        pos = P[P > 0]
        f95 = np.nan
        if ny == nx and tot > 0.0:
            cdf = np.cumsum(Pm[order]) / tot
            k = min(int(np.searchsorted(cdf, 0.95, side="left")), FRm.size - 1)
            f95 = float(FRm[order][k])
        out[b] = (tot, np.sum(FRm * FRm * Pm), np.sum(FXm * FXm * Pm), np.sum(FYm * FYm * Pm), np.sum(Pm * Pm),
                  np.sum(P), np.sum(pos * np.log(pos)), f95)
    return out


def bandwidth_from_row(row):
    """feq, sig_fx, sig_fy, f95, spr of metrics_np.bandwidth from one psd_stats row."""
    s, sfr, sfx, sfy, sp2, _, _, f95 = (float(v) for v in row)
    return {"feq": float(np.sqrt(sfr / s)), "f95": f95, "sig_fx": float(np.sqrt(sfx / s)), "sig_fy": float(np.sqrt(sfy / s)),
            "spr": float(s * s / sp2)}


def entropy_from_row(row, size):
    """metrics_np.spectral_entropy (mean and DC removed) from one psd_stats row of a `size`-bin map."""
    s_all, splnp = float(row[5]), float(row[6])
    return float((np.log(s_all) - splnp / s_all) / np.log(float(size - 1)))


# --------------------------------------------------------------------------- temporal
def temporal_sums_range(stack, pix0, npix):
    """b4d_temporal_accumulate_range on zeroed accumulators: (sum x, sum x^2) of pixels [pix0, pix0 + npix) of every
    (flattened) frame."""
    s = np.asarray(stack)
    s64 = s.reshape(s.shape[0], -1)[:, pix0:pix0 + npix].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return s64.sum(axis=0), (s64 * s64).sum(axis=0)


def temporal_finalize(sum_x, sum_xx, count):
    """b4d_temporal_finalize: (mean, var, contrast) in float64; a negative variance is clamped to 0, NaN stays NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        return T.finalize_sums(np.asarray(sum_x, dtype=np.float64), np.asarray(sum_xx, dtype=np.float64), count)


# --------------------------------------------------------------------------- edge-value input families (tests)
SELECT_FAMILIES = ("squares", "normal", "three", "equal", "bin11", "low10", "zeros", "denormal", "fltmax", "inf",
                   "nan1", "nan50", "nan100", "one_valid")


def select_family(name, n, batch=3, seed=0):
    """(batch, n) float32 frames of one input family of the selection tests; every frame differs.
    squares: distinct shuffled squares; normal: signed; three: three distinct values; equal: one value; bin11: 1000 + U(0, 1)
    (one bin of the top 11 key bits); low10: values differing in their lowest 10 mantissa bits only; zeros: +-0.0 among
    +-1; denormal: signed float32 denormals; fltmax: +-FLT_MAX among small values; inf: +-inf mixed into normal data;
    nan1 / nan50 / nan100: that share of NaN; one_valid: a single non-NaN element."""
    rng = np.random.default_rng([seed, n, SELECT_FAMILIES.index(name)])
    out = np.empty((batch, n), dtype=np.float32)
    fmax = np.finfo(np.float32).max
    for b in range(batch):
        if name == "squares":
            x = (np.arange(n, dtype=np.float64) + b) ** 2
            rng.shuffle(x)
        elif name == "three":
            x = rng.choice(np.array([-2.5, 0.25, 7.0]), size=n)
        elif name == "equal":
            x = np.full(n, 3.25 + b)
        elif name == "bin11":
            x = 1000.0 + rng.random(n)
        elif name == "low10":
            x = (np.uint32(0x42F00000) | rng.integers(0, 1024, size=n).astype(np.uint32)).view(np.float32)
        elif name == "zeros":
            x = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0]), size=n)
        elif name == "denormal":
            x = rng.integers(-4000, 4001, size=n).astype(np.float64) * float(np.float32(1.4e-45))
        elif name == "fltmax":
            x = rng.choice(np.array([fmax, -fmax, 1.0, -1.0, 0.5, 3.0]), size=n)
        else:
            x = rng.standard_normal(n) * 100.0
        x = np.asarray(x).astype(np.float32)
        if name == "inf":
            u = rng.random(n)
            x[u < 0.02] = np.inf
            x[u > 0.98] = -np.inf
        elif name in ("nan1", "nan50"):
            x[rng.random(n) < (0.01 if name == "nan1" else 0.5)] = np.nan
        elif name == "nan100":
            x[:] = np.nan
        elif name == "one_valid":
            keep = int(rng.integers(0, n))
            v = x[keep]
            x[:] = np.nan
            x[keep] = v
        out[b] = x
    return out
