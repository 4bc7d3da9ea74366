"""Float64 NumPy model of b4d_spot_centroids, written cell by cell from the rule in include/b4d.h -- not a
port of any implementation -- and the cases the host and GPU tiers share.

spot_model() returns the fourteen maps plus "cy_iw", "cx_iw" (the iteratively weighted centre of gravity), so that one evaluation
serves both methods.  Every sum goes through one function chosen by `order`: "fsum" (math.fsum, exactly rounded; the default and
the reference of the GPU tier), "forward" or "reverse" (one addition after the other): tests/test_hartmann_host.py compares the
three to show how little the centroids depend on the order.

Thresholds.  n_pixels counts the pixels above t = b + threshold (peak - b), so a pixel within rounding of t would make the count
depend on the last bit of t.  The model asserts that no pixel lies within 1e-6 (peak - b) of its cell's t.  A pixel exactly AT t is
harmless where t is exact in any evaluation -- threshold 0 with a background that is a pixel value or a constant, a constant cell,
or a whole-number t on whole-number frames (0.2 k for a multiple k of 5 rounds to the whole number both as a product and inside a
fused multiply-add) -- since its weight is 0 on either side; such ties pass, except under "border" with a threshold > 0, where t
comes out of a division.  All case frames hold whole numbers (detector counts), which keeps every other pixel at least 1 / (5 n)
away from t for a ring of n pixels.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

QUANTITIES = ("cy", "cx", "flux", "peak", "peak_y", "peak_x", "background", "noise", "var_y", "var_x", "cov_yx", "n_pixels",
              "n_saturated", "n_nan")
COUNTS = ("n_pixels", "n_saturated", "n_nan")
MARGIN = 1e-6

SUMS = {
    "fsum": lambda a: math.fsum(a.tolist()),
    "forward": lambda a: float(np.cumsum(a)[-1]) if a.size else 0.0,
    "reverse": lambda a: float(np.cumsum(a[::-1])[-1]) if a.size else 0.0,
}


def spot_cell(v32, y0: int, x0: int, *, background, threshold: float, sigma: float, iterations: int, saturation: float,
              order: str = "fsum", check_margin: bool = True) -> dict:
    """The quantities of one cell: v32 its float32 pixels, (y0, x0) its first pixel in the frame."""
    S = SUMS[order]
    nan = float("nan")
    v = np.asarray(v32, dtype=np.float32).astype(np.float64)
    h, w = v.shape
    ok = ~np.isnan(v)
    rr, cc = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    q = {"n_nan": int((~ok).sum()), "n_saturated": int((v[ok] >= saturation).sum())}
    if ok.any():
        k = int(np.argmax(np.where(ok, v, -np.inf)))       # first occurrence, row-major
        peak, q["peak_y"], q["peak_x"] = float(v.ravel()[k]), float(y0 + k // w), float(x0 + k % w)
        low = float(v[ok].min())
    else:
        peak = q["peak_y"] = q["peak_x"] = low = nan
    q["peak"] = peak
    edge = ok & ((rr == 0) | (rr == h - 1) | (cc == 0) | (cc == w - 1))
    n_ring = int(edge.sum())
    ring = S(v[edge]) / n_ring if n_ring else nan
    q["noise"] = math.sqrt(S((v[edge] - ring) ** 2) / n_ring) if n_ring >= 2 else 0.0
    b = {"none": 0.0, "min": low, "border": ring}[background] if isinstance(background, str) else float(background)
    q["background"] = b
    t = b + threshold * (peak - b)
    with np.errstate(invalid="ignore"):
        d = v - t
        lit = ok & (d > 0.0)
    if check_margin and ok.any() and peak - b > 0.0:
        gap = np.abs(d[ok])
        tie_ok = not (background == "border" and threshold > 0.0)
        near = (gap <= MARGIN * (peak - b)) & ~((gap == 0.0) & tie_ok)
        assert not near.any(), f"cell at ({y0}, {x0}): a pixel within {MARGIN} (peak - b) of the threshold {t!r} ({background}, {threshold})"
    wgt = d[lit]
    F = S(wgt)
    if not F > 0.0:
        q.update(cy=nan, cx=nan, flux=0.0, n_pixels=0, var_y=nan, var_x=nan, cov_yx=nan, cy_iw=nan, cx_iw=nan)
        return q
    yc, xc = 0.5 * (h - 1), 0.5 * (w - 1)
    ry, rx = rr[lit] - yc, cc[lit] - xc                      # about the cell's geometric centre
    cy = (y0 + yc) + S(wgt * ry) / F
    cx = (x0 + xc) + S(wgt * rx) / F
    fy, fx = (y0 + rr[lit]), (x0 + cc[lit])                  # frame coordinates
    q.update(cy=cy, cx=cx, flux=F, n_pixels=int(lit.sum()),
             var_y=S(wgt * (fy - cy) * (fy - cy)) / F, var_x=S(wgt * (fx - cx) * (fx - cx)) / F,
             cov_yx=S(wgt * (fy - cy) * (fx - cx)) / F)
    iy, ix = cy, cx
    for _ in range(iterations):
        g = wgt * np.exp(-((fy - iy) ** 2 + (fx - ix) ** 2) / (2.0 * sigma * sigma))
        G = S(g)
        with np.errstate(invalid="ignore", divide="ignore"):
            iy, ix = (y0 + yc) + np.float64(S(g * ry)) / np.float64(G), (x0 + xc) + np.float64(S(g * rx)) / np.float64(G)
    q.update(cy_iw=float(iy), cx_iw=float(ix))
    return q


def spot_model(frames, y_edges, x_edges, *, background="border", threshold=0.1, sigma=None, iterations=8, saturation=None,
               pitch=None, order="fsum", check_margin=True) -> dict:
    """Maps (T, gy, gx) of every quantity of QUANTITIES plus cy_iw, cx_iw for frames (T, H, W) or (H, W) (then (gy, gx))."""
    a = np.asarray(frames, dtype=np.float32)
    stack = a.reshape((-1,) + a.shape[-2:])
    gy, gx = len(y_edges) - 1, len(x_edges) - 1
    if sigma is None:
        sigma = 0.25 * min(pitch)
    sat = np.inf if saturation is None else float(saturation)
    names = QUANTITIES + ("cy_iw", "cx_iw")
    out = {k: np.zeros((stack.shape[0], gy, gx), dtype=np.int64 if k in COUNTS else np.float64) for k in names}
    for f, frame in enumerate(stack):
        for i in range(gy):
            for j in range(gx):
                y0, y1, x0, x1 = int(y_edges[i]), int(y_edges[i + 1]), int(x_edges[j]), int(x_edges[j + 1])
                q = spot_cell(frame[y0:y1, x0:x1], y0, x0, background=background, threshold=threshold, sigma=sigma,
                              iterations=iterations, saturation=sat, order=order, check_margin=check_margin)
                for k in names:
                    out[k][f, i, j] = q[k]
    if a.ndim == 2:
        out = {k: m[0] for k, m in out.items()}
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
BACKGROUNDS = ("none", "min", "border", 2.3)     # 2.3: t = 1.84 + 0.2 peak under threshold 0.2 is never a whole number
THRESHOLDS = (0.0, 0.2)
METHODS = ("cog", "iwcog")
OPTION_SETS = tuple((m, b, t) for m in METHODS for b in BACKGROUNDS for t in THRESHOLDS)
SATURATION = 4095.0


def sub_cells(cells: dict, gy: int, gx: int) -> dict:
    """The first gy x gx cells of a lattice."""
    out = dict(cells)
    out.update(y_edges=cells["y_edges"][:gy + 1].copy(), x_edges=cells["x_edges"][:gx + 1].copy(), y=cells["y"][:gy].copy(),
               x=cells["x"][:gx].copy(), shape=(gy, gx))
    return out


def _cells(shape, pitch, origin=(0.0, 0.0)):
    from barc4dip_amd.signal.hartmann import hartmann_cells

    return hartmann_cells(shape, pitch, origin)


def _spots(shape, pitch, origin, *, sigma, reach, seeds, background=3.0):
    """Frames of Poisson counts: spots shifted by up to +-reach px per cell, one frame per seed."""
    from barc4dip_amd import synth

    c = _cells(shape, pitch, origin)
    frames = []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        d = rng.uniform(-reach, reach, (2,) + c["shape"])
        frames.append(synth.hartmann_frame(shape, pitch, origin, (d[0], d[1]), sigma=sigma, background=background, seed=seed + 1000))
    return np.stack(frames).astype(np.float32)


def _ragged():
    return _spots((147, 203), (13.37, 17.5), (3.2, 5.7), sigma=1.6, reach=2.0, seeds=(11, 12, 13))


def _aligned():
    return _spots((128, 256), 32, (0, 0), sigma=2.0, reach=2.0, seeds=(21, 22))


def _largest():
    return _spots((130, 259), 128, (1, 2), sigma=20.0, reach=10.0, seeds=(31,))[0]


def _smallest():
    return _spots((9, 11), 2, (0, 0), sigma=0.6, reach=0.3, seeds=(41,), background=1.0)[0]


def _many():
    # rings of 16 pixels make t = (4 S + 16 peak) / 80 a whole number often; this seed is one whose frame keeps the margin
    return _spots((6, 4100), (6, 4), (0, 0), sigma=0.8, reach=0.5, seeds=(57,), background=2.0)[0]


EDGE_CELLS = {"constant": (0, 0), "all_nan": (0, 1), "nan_flank": (0, 2), "saturated": (0, 3), "negative": (1, 0),
              "corner": (2, 2), "two_maxima": (1, 3)}


def _edge():
    """96 x 120 at pitch 24 (4 x 5 cells of whole-number counts), one special cell each (EDGE_CELLS)."""
    from barc4dip_amd import synth

    d = np.zeros((2, 4, 5))
    d[:, 2, 2] = 12.0                                        # the spot of cell (2, 2) sits on its lower right corner
    f = np.round(synth.hartmann_frame((96, 120), 24, (0, 0), (d[0], d[1]), sigma=2.0, background=5.0))
    f += np.random.default_rng(61).integers(0, 3, f.shape)   # a little texture, so that rings are not constant

    def cell(name):
        i, j = EDGE_CELLS[name]
        return f[24 * i:24 * i + 24, 24 * j:24 * j + 24]

    cell("constant")[:] = 7.0
    cell("all_nan")[:] = np.nan
    cell("nan_flank")[9:14, 13:17] = np.nan                  # the spot is at (11.5, 11.5) of its cell
    cell("saturated")[11, 11:13] = SATURATION
    cell("saturated")[12, 11] = SATURATION
    cell("negative")[:] -= 2000.0
    top = cell("two_maxima").max() + 50.0
    cell("two_maxima")[14, 9] = top
    cell("two_maxima")[9, 15] = top                          # the first in row-major order
    return f.astype(np.float32)


# name -> (frame maker, cells maker, options beyond method / background / threshold)
CASES = {
    "ragged": (_ragged, lambda: sub_cells(_cells((147, 203), (13.37, 17.5), (3.2, 5.7)), 9, 10), {}),
    "aligned": (_aligned, lambda: _cells((128, 256), 32), {}),
    "largest": (_largest, lambda: _cells((130, 259), 128, (1, 2)), {}),
    "smallest": (_smallest, lambda: _cells((9, 11), 2), {}),
    "many": (_many, lambda: _cells((6, 4100), (6, 4)), {}),
    "edge": (_edge, lambda: _cells((96, 120), 24), {"saturation": SATURATION}),
}

_DATA = None


def case_data() -> dict:
    """name -> (frames float32, cells), built once."""
    global _DATA
    if _DATA is None:
        _DATA = {name: (make(), cells()) for name, (make, cells, _) in CASES.items()}
    return _DATA


_MODELS: dict = {}


def case_model(name: str, background, threshold: float, order: str = "fsum") -> dict:
    """spot_model of a case under (background, threshold), computed once; serves both methods."""
    key = (name, background, threshold, order)
    if key not in _MODELS:
        frames, cells = case_data()[name]
        _MODELS[key] = spot_model(frames, cells["y_edges"], cells["x_edges"], background=background, threshold=threshold,
                                  pitch=cells["pitch"], order=order, **CASES[name][2])
    return _MODELS[key]
