"""float64 NumPy models of the separable filters and the local statistics (csrc/b4d_smooth.hip), built on an explicit restatement
of the border index, and the error bounds of DESIGN.md section 26.5.  No SciPy here: tests/test_smoothing_host.py checks these
models against scipy.ndimage, and the GPU tests check the kernels against both."""
from __future__ import annotations

import numpy as np

from barc4dip_amd._frames import MODES as _CODES

MODES = {m: c for m, c in _CODES.items() if not m.startswith("grid-")}     # the five modes, without SciPy's two aliases
U = 2.0 ** -24


def border_index(i, n: int, mode: str) -> np.ndarray:
    """Source index of positions i on an axis of n samples under scipy.ndimage's border modes, any overhang; -1 = outside."""
    i = np.asarray(i, dtype=np.int64)
    inside = (i >= 0) & (i < n)
    if mode == "constant":
        return np.where(inside, i, -1)
    if mode == "nearest" or n == 1:
        return np.clip(i, 0, n - 1)
    if mode == "wrap":
        return np.mod(i, n)
    if mode == "reflect":          # d c b a | a b c d | d c b a
        p = np.mod(i, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p)
    if mode == "mirror":           # d c b | a b c d | c b a
        p = np.mod(i, 2 * n - 2)
        return np.where(p < n, p, 2 * n - 2 - p)
    raise ValueError(mode)


def _take(x: np.ndarray, idx: np.ndarray, axis: int, cval: float) -> np.ndarray:
    out = np.take(x, np.maximum(idx, 0), axis=axis)
    if np.any(idx < 0):
        shape = [1] * x.ndim
        shape[axis] = idx.size
        out = np.where((idx < 0).reshape(shape), cval, out)
    return out


def correlate_axis(x: np.ndarray, w, axis: int, mode: str, cval: float = 0.0) -> np.ndarray:
    """out[i] = sum_k w[k] x[i - n // 2 + k] along `axis`, in float64, k ascending; 0 * NaN = NaN as in IEEE arithmetic."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = x.shape[axis]
    pos = np.arange(n) - w.size // 2
    out = None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(w.size):
            term = w[k] * _take(x, border_index(pos + k, n, mode), axis, cval)
            out = term if out is None else out + term
    return out


def model_separable(x, wy, wx, mode: str = "reflect", cval: float = 0.0) -> np.ndarray:
    """The filter's definition: rows (x axis) first, columns second, the border rule applied to each pass's own input."""
    return correlate_axis(correlate_axis(x, wx, -1, mode, cval), wy, -2, mode, cval)


def gaussian_taps(sigma: float, order: int = 0, truncate: float = 4.0, radius=None) -> np.ndarray:
    """Correlation taps of scipy.ndimage.gaussian_filter1d, restated: normalised Gaussian on -lw .. lw times the derivative's
    polynomial, reversed."""
    if sigma == 0:
        return np.ones(1)
    lw = int(truncate * float(sigma) + 0.5) if radius is None else int(radius)
    x = np.arange(-lw, lw + 1)
    s2 = float(sigma) ** 2
    phi = np.exp(-0.5 / s2 * x ** 2)
    phi /= phi.sum()
    if order == 1:
        phi = -x / s2 * phi
    elif order == 2:
        phi = (x ** 2 / s2 ** 2 - 1.0 / s2) * phi
    elif order != 0:
        raise ValueError(order)
    return phi[::-1].copy()


def box_taps(size: int) -> np.ndarray:
    return np.full(int(size), 1.0 / int(size))


def model_local_stats(x, sy: int, sx: int, wy=None, wx=None, mode: str = "reflect", cval: float = 0.0) -> dict:
    """mean, variance, contrast (float64) and S2 / W of the sy x sx window of the frame padded in two dimensions; wy = wx = None
    is the box window (weights 1, W = sy sx)."""
    x = np.asarray(x, dtype=np.float64)
    ny, nx = x.shape[-2:]
    iy = border_index(np.arange(ny + sy - 1) - sy // 2, ny, mode)
    ix = border_index(np.arange(nx + sx - 1) - sx // 2, nx, mode)
    p = _take(_take(x, iy, x.ndim - 2, cval), ix, x.ndim - 1, cval)
    if mode == "constant":      # a corner: outside on either axis is cval
        p = np.where((iy < 0)[:, None] | (ix < 0)[None, :], cval, p)
    wy = np.ones(sy) if wy is None else np.asarray(wy, dtype=np.float64)
    wx = np.ones(sx) if wx is None else np.asarray(wx, dtype=np.float64)
    W = float(np.sum(wy) * np.sum(wx))

    def window_sum(a):
        r = sum(wx[k] * a[..., :, k:k + nx] for k in range(sx))
        return sum(wy[j] * r[..., j:j + ny, :] for j in range(sy))

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s1, s2 = window_sum(p), window_sum(p * p)
        mean = s1 / W
        var = s2 / W - mean * mean
        var = np.where(var < 0.0, 0.0, var)
        contrast = np.where(mean > 0.0, np.sqrt(var) / np.where(mean > 0.0, mean, 1.0), np.nan)
    return {"mean": mean, "variance": var, "contrast": contrast, "s2_over_w": s2 / W}


# ------------------------------------------------------------------------------------------------- bounds
def _frame_max(x) -> np.ndarray:
    """max |x| over the finite pixels of every frame, broadcastable against the frames."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    return a.max(axis=(-2, -1), keepdims=True)


def bound_separable(x, wy, wx) -> np.ndarray:
    """1.01 u M A_y A_x ((K_y + 4) + (K_x + 4)): gamma_K of a K-term float32 sum, one rounding per tap and of the intermediate."""
    wy32 = np.asarray(wy, dtype=np.float64).astype(np.float32).astype(np.float64)
    wx32 = np.asarray(wx, dtype=np.float64).astype(np.float32).astype(np.float64)
    ay, ax = np.abs(wy32).sum(), np.abs(wx32).sum()
    return 1.01 * U * _frame_max(x) * ay * ax * ((wy32.size + 4) + (wx32.size + 4))


def bound_subtract(e, out_ref) -> np.ndarray:
    return e + U * np.abs(out_ref)


def bound_divide(e, x, g_ref, out_ref) -> np.ndarray:
    return np.abs(x) * e / (g_ref * g_ref) + 2 * U * np.abs(out_ref)


def ulp32(v) -> np.ndarray:
    """One float32 unit in the last place at |v| (of the model value, in float64)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def tolerances_local_stats(model: dict, sy: int, sx: int) -> dict:
    """One float32 ulp of the model value, plus K_y K_x 2^-52 S2 / W in the variance (the cancellation in S2 / W - mean^2) and that
    term over 2 sqrt(var) mean in the contrast wherever var > 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = sy * sx * 2.0 ** -52 * np.abs(model["s2_over_w"])
        var, mean = model["variance"], model["mean"]
        tc = np.where(var > 0.0, c / (2.0 * np.sqrt(var) * np.abs(mean)), 0.0)
    return {"mean": ulp32(model["mean"]), "variance": ulp32(var) + c, "contrast": ulp32(model["contrast"]) + tc}
