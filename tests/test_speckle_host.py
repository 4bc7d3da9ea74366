"""Speckle transmission and dark-field maps, host tier (no GPU): the float64 NumPy model of b4d_speckle_contrast that the GPU tests
compare against (tests/test_gpu_speckle.py), checked against closed forms, and the argument checks of
barc4dip_amd.signal.speckle, all of which are raised before a device is needed."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from barc4dip_amd import _ffi
from barc4dip_amd.signal import displacement as DM
from barc4dip_amd.signal import speckle as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("transmission", "dark_field", "dark_field_fit", "correlation", "visibility_ref", "visibility")


# ---- the model: the definitions of include/b4d.h in float64, two-pass moments (mean first, then centred sums)
def hann(w: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(w) + 0.5) / w)


def taps(d: float, order: int):
    """(integer tap t, weight of t, weight of t + 1); a tap of weight 0 is never read, a fraction that rounds to 1 moves the tap."""
    t = np.floor(d + 0.5) if order == 0 else np.floor(d)
    w1 = 0.0 if order == 0 else d - t
    w0 = 1.0 - w1
    if w0 == 0.0:
        t, w0, w1 = t + 1.0, 1.0, 0.0
    return t, w0, w1


def _ratio(num, den):
    return num / den if den > 0.0 else np.nan


def _sqrt(v):
    return np.sqrt(v) if v > 0.0 else np.nan


def window_model(ref, img, y0, x0, wy, wx, dy, dx, order=1, taper=0) -> np.ndarray:
    """The six planes of one window; ref, img float64 (H, W)."""
    H, W = img.shape
    if not (np.isfinite(dy) and np.isfinite(dx)):
        return np.full(6, np.nan)
    ty, wy0, wy1 = taps(float(dy), order)
    tx, wx0, wx1 = taps(float(dx), order)
    if (y0 + ty < 0 or y0 + wy - 1 + ty + (wy1 != 0.0) > H - 1 or x0 + tx < 0 or x0 + wx - 1 + tx + (wx1 != 0.0) > W - 1):
        return np.full(6, np.nan)
    iy, ix = int(ty), int(tx)
    r = ref[y0:y0 + wy, x0:x0 + wx]

    def cut(oy, ox):
        return img[y0 + iy + oy:y0 + iy + oy + wy, x0 + ix + ox:x0 + ix + ox + wx]

    def row(oy):
        v = wx0 * cut(oy, 0)
        return v + wx1 * cut(oy, 1) if wx1 != 0.0 else v

    s = wy0 * row(0)
    if wy1 != 0.0:
        s = s + wy1 * row(1)
    h = np.outer(hann(wy), hann(wx)) if taper else np.ones((wy, wx))
    h = h / h.sum()
    Rm, Sm = float(np.sum(h * r)), float(np.sum(h * s))
    VR, VS = float(np.sum(h * (r - Rm) ** 2)), float(np.sum(h * (s - Sm) ** 2))
    C = float(np.sum(h * (r - Rm) * (s - Sm)))
    T = _ratio(Sm, Rm)
    vr, vs = _ratio(_sqrt(VR), Rm), _ratio(_sqrt(VS), Sm)
    return np.array([T, _ratio(vs, vr), _ratio(C, VR * T), _ratio(C, _sqrt(VS * VR) if VS > 0.0 and VR > 0.0 else np.nan), vr, vs])


def model_map(ref, img, dy, dx, *, window, step=None, search=8, order=1, taper=0) -> np.ndarray:
    """(gy, gx, 6) float64 of one frame pair; ref and img are taken as the float32 frames that the device sees."""
    ref = np.asarray(ref).astype(np.float32).astype(np.float64)
    img = np.asarray(img).astype(np.float32).astype(np.float64)
    g = DM.displacement_grid(ref.shape, window=window, step=step, search=search)
    (wy, wx) = g["window"]
    out = np.empty(g["shape"] + (6,))
    for iy, ix in np.ndindex(*g["shape"]):
        out[iy, ix] = window_model(ref, img, int(g["y0"][iy]), int(g["x0"][ix]), wy, wx, dy[iy, ix], dx[iy, ix], order, taper)
    return out


def deviation(got: np.ndarray, want: np.ndarray) -> float:
    """Largest deviation of (..., 6) maps from the model, each plane against its own scale: transmission, dark_field and the two
    visibilities relative to their value; correlation against 1 (its range); dark_field_fit = correlation x dark_field against
    dark_field.  The NaN pattern must be the model's."""
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    scale = np.abs(want).copy()
    scale[..., 3] = 1.0
    scale[..., 2] = np.where(np.isnan(want[..., 1]), scale[..., 2], np.abs(want[..., 1]))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / scale[ok]))


def speckle(shape, seed, *, counts=None, contrast=None, dtype=np.float32):
    """Seeded positive frames with correlated grain; ``counts`` and ``contrast`` give detector words (mean, relative std)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    a = a + 0.5 * (np.roll(a, 1, -1) + np.roll(a, 1, -2))
    a = a / a.std()
    out = counts * (1.0 + contrast * a) if counts else 100.0 + 25.0 * a
    out = np.rint(out) if np.dtype(dtype).kind in "ui" else out
    out = out.astype(dtype)
    out.setflags(write=False)
    return out


# ---- the model against closed forms
@pytest.mark.parametrize("taper", [0, 1])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("pq", [(0, 0), (3, -2), (-4, 4), (4, -4), (1, 0)])
def test_model_affine_shifted_copy(pq, order, taper):
    """S = a shift(R, (p, q)) + b: transmission (a Rm + b) / Rm, dark_field = dark_field_fit = a / transmission, correlation 1."""
    a, b = 0.7, 12.5
    R = speckle((47, 52), 5).astype(np.float64)
    S = a * np.roll(R, pq, axis=(0, 1)) + b
    kw = dict(window=(9, 11), step=(5, 6), search=4)
    g = DM.displacement_grid(R.shape, **kw)
    dy, dx = np.full(g["shape"], float(pq[0])), np.full(g["shape"], float(pq[1]))
    h = np.outer(hann(9), hann(11)) if taper else np.ones((9, 11))
    h /= h.sum()
    for iy, ix in np.ndindex(*g["shape"]):
        y0, x0 = int(g["y0"][iy]), int(g["x0"][ix])
        m = window_model(R, S, y0, x0, 9, 11, dy[iy, ix], dx[iy, ix], order, taper)
        Rm = np.sum(h * R[y0:y0 + 9, x0:x0 + 11])
        T = (a * Rm + b) / Rm
        np.testing.assert_allclose(m[0], T, rtol=1e-12)
        np.testing.assert_allclose(m[2], a / T, rtol=1e-12)
        np.testing.assert_allclose(m[3], 1.0, rtol=1e-12)
        np.testing.assert_allclose(m[1], m[2], rtol=1e-12)
        np.testing.assert_allclose(m[5], m[4] * m[1], rtol=1e-12)


def test_model_single_pixel_window():
    R = speckle((20, 23), 6).astype(np.float64)
    S = 0.5 * R + 3.0
    for order in (0, 1):
        m = window_model(R, S, 8, 9, 1, 1, 0.25, -0.5, order, 0)
        assert np.isfinite(m[0]) and m[0] > 0.0
        assert np.all(np.isnan(m[1:]))


def test_model_bilinear_on_a_ramp():
    """A bilinear sample of a linear ramp is the ramp at the displaced position."""
    y, x = np.mgrid[0:40, 0:44].astype(np.float64)
    R = 50.0 + 0.0 * y
    S = 10.0 + 0.75 * y - 0.5 * x + 40.0
    for dy, dx in [(0.3, -1.6), (-2.0, 2.999), (2.5, 0.0), (-3.0 + 2.0 ** -20, 3.0 - 2.0 ** -20)]:
        m = window_model(R, S, 6, 7, 8, 5, dy, dx, 1, 0)
        np.testing.assert_allclose(m[0], (50.0 + 0.75 * (6 + 3.5 + dy) - 0.5 * (7 + 2.0 + dx)) / 50.0, rtol=1e-13)
        assert np.all(np.isnan(m[1:5])) and np.isfinite(m[5])      # a constant reference has a transmission and nothing else
    m0 = window_model(R, S, 6, 7, 8, 5, 0.5, -0.5, 0, 0)           # order 0: floor(d + 0.5) -> (1, 0)
    np.testing.assert_allclose(m0[0], (50.0 + 0.75 * (6 + 3.5 + 1) - 0.5 * (7 + 2.0)) / 50.0, rtol=1e-13)


def test_model_taps_and_exclusion():
    assert taps(2.0, 1) == (2.0, 1.0, 0.0) and taps(-2.0, 1) == (-2.0, 1.0, 0.0)
    assert taps(-1e-20, 1) == (0.0, 1.0, 0.0)                      # the fraction rounds to 1: the tap moves, nothing is read at -1
    assert taps(-0.5, 0)[0] == 0.0 and taps(0.5, 0)[0] == 1.0 and taps(-0.51, 0)[0] == -1.0
    t, w0, w1 = taps(2.25, 1)
    assert (t, w0, w1) == (2.0, 0.75, 0.25)
    R = speckle((30, 30), 7).astype(np.float64)
    # window (6, 6, 10 x 10): 6 px to the top and left edge, 14 to the bottom and right
    e = 2.0 ** -20
    # (displacement, inside at order 0, inside at order 1): order 0 rounds a hair beyond the edge back inside
    for d, in0, in1 in [(-6.0, True, True), (-6.0 - e, True, False), (-7.0, False, False), (14.0, True, True), (14.0 + e, True, False),
                        (15.0, False, False), (np.nan, False, False), (np.inf, False, False), (-np.inf, False, False),
                        (1e300, False, False), (-1e300, False, False)]:
        for order, want in ((0, in0), (1, in1)):
            assert np.all(np.isfinite(window_model(R, R, 6, 6, 10, 10, d, 0.0, order, 0))) == want, (d, order)
            assert np.all(np.isfinite(window_model(R, R, 6, 6, 10, 10, 0.0, d, order, 1))) == want, (d, order)


def test_model_noise_raises_dark_field_but_not_the_fit():
    rng = np.random.default_rng(8)
    R = speckle((64, 64), 9).astype(np.float64)
    S = 0.8 * R + 5.0 * rng.standard_normal(R.shape)
    m = window_model(R, S, 8, 8, 48, 48, 0.0, 0.0, 1, 0)
    assert m[1] > m[2] and abs(m[2] - 1.0) < 0.02 and 1.01 < m[1] < 1.1 and 0.9 < m[3] < 1.0


# ---- argument checks: host only
def _field(shape=(64, 64), T=None, **kw):
    kw = dict(dict(window=15, step=None, search=4), **kw)
    g = DM.displacement_grid(shape, **kw)
    mshape = (() if T is None else (T,)) + g["shape"]
    return {"dy": np.zeros(mshape), "dx": np.zeros(mshape), "y": g["y"], "x": g["x"],
            "meta": {"window": g["window"], "step": g["step"], "search": g["search"], "backend": "opencv"}}


def test_contrast_argument_errors_before_any_device_work():
    ref = np.zeros((64, 64), np.float32)
    f = _field()
    with pytest.raises(ValueError, match="window grid"):                      # field of another frame shape
        SP.speckle_contrast(np.zeros((80, 64)), np.zeros((80, 64)), f)
    with pytest.raises(ValueError, match="window grid"):                      # (gy, gx) field for a stack
        SP.speckle_contrast(ref, np.zeros((3, 64, 64)), f)
    with pytest.raises(ValueError, match="window grid"):
        SP.speckle_contrast(ref, ref, (np.zeros((5, 5)), np.zeros((5, 5))), window=15, search=4)
    with pytest.raises(ValueError, match="window grid"):                      # dx of another shape than dy
        SP.speckle_contrast(ref, ref, (f["dy"], f["dx"][:-1]), window=15, search=4)
    for order in (2, -1, 0.5, "linear", True, None):
        with pytest.raises(ValueError, match="order"):
            SP.speckle_contrast(ref, ref, f, order=order)
    for taper in ("hanning", "", 1, None):
        with pytest.raises(ValueError, match="taper"):
            SP.speckle_contrast(ref, ref, f, taper=taper)
    with pytest.raises(ValueError):                                           # unpaired (T, H, W) reference
        SP.speckle_contrast(np.zeros((3, 64, 64)), ref, f)
    with pytest.raises(ValueError):
        SP.speckle_contrast(np.zeros((3, 64, 64)), np.zeros((4, 64, 64)), _field(T=4))
    with pytest.raises(ValueError):
        SP.speckle_contrast(ref, np.zeros((64, 63), np.float32), f)
    with pytest.raises(ValueError):
        SP.speckle_contrast(ref, ref, {"dy": f["dy"], "dx": f["dx"]})         # no meta
    with pytest.raises(ValueError):
        SP.speckle_contrast(ref, ref, f, window=15)                           # geometry given twice
    with pytest.raises(ValueError):
        SP.speckle_contrast(ref, ref, f["dy"])                                # neither a dict nor a pair
    with pytest.raises(ValueError):
        SP.speckle_contrast(ref, ref, (f["dy"] + 0j, f["dx"]), window=15, search=4)
    big = np.zeros((400, 400), np.float32)
    with pytest.raises(NotImplementedError):
        SP.speckle_contrast(big, big, (np.zeros((1, 1)), np.zeros((1, 1))), window=129, search=8)
    with pytest.raises(NotImplementedError):
        SP.speckle_contrast(big, big, (np.zeros((1, 1)), np.zeros((1, 1))), window=31, search=33)
    bad = _field()
    bad["meta"] = dict(bad["meta"], window=(130, 15))
    with pytest.raises(NotImplementedError):
        SP.speckle_contrast(big, big, bad)
    with pytest.raises(ValueError):                                           # the window plus its margin does not fit
        SP.speckle_contrast(ref, ref, (np.zeros((1, 1)), np.zeros((1, 1))), window=60, search=4)


def test_imaging_argument_errors_before_any_device_work():
    ref = np.zeros((64, 64), np.float32)
    kw = dict(window=15, search=4)
    with pytest.raises(ValueError, match="order"):
        SP.speckle_imaging(ref, ref, order=3, **kw)
    with pytest.raises(ValueError, match="taper"):
        SP.speckle_imaging(ref, ref, taper="hamming", **kw)
    with pytest.raises(ValueError, match="backend"):
        SP.speckle_imaging(ref, ref, backend="internal", **kw)
    for mc in (1.5, -2, "0.5", True, np.nan, [0.5]):
        with pytest.raises(ValueError, match="min_correlation"):
            SP.speckle_imaging(ref, ref, min_correlation=mc, **kw)
    with pytest.raises(ValueError):
        SP.speckle_imaging(np.zeros((3, 64, 64)), ref, **kw)
    with pytest.raises(ValueError):
        SP.speckle_imaging(np.zeros((3, 64, 64)), np.zeros((2, 64, 64)), **kw)
    with pytest.raises(ValueError):
        SP.speckle_imaging(ref, np.zeros((64, 63)), **kw)
    with pytest.raises(ValueError):
        SP.speckle_imaging(ref, ref, window=60, search=4)
    with pytest.raises(ValueError):
        SP.speckle_imaging(ref, ref, window=15, step=0, search=4)
    with pytest.raises(NotImplementedError):
        SP.speckle_imaging(np.zeros((400, 400)), np.zeros((400, 400)), window=130, search=4)
    with pytest.raises(NotImplementedError):
        SP.speckle_imaging(np.zeros((400, 400)), np.zeros((400, 400)), window=15, search=40)


def test_symbol_declared_bound_and_exported():
    from barc4dip_amd import signal

    assert signal.speckle_contrast is SP.speckle_contrast and signal.speckle_imaging is SP.speckle_imaging
    assert {"speckle", "speckle_contrast", "speckle_imaging"} <= set(signal.__all__)
    assert SP.PLANES == PLANES
    hdr = open(os.path.join(ROOT, "include", "b4d.h")).read()
    assert re.search(r"\bint b4d_speckle_contrast\s*\(", hdr)
    res, args = _ffi.SIGNATURES["b4d_speckle_contrast"]
    assert len(args) == 22 and args[17] is _ffi.C.c_longlong
    if not os.path.exists(_ffi.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "barc4dip_amd", "csrc"), "libb4d.so"], check=True)
    lib = _ffi.load_library()
    assert "b4d_speckle_contrast" not in lib.b4d_missing_symbols and lib.b4d_speckle_contrast.argtypes == args
    assert "b4d_speckle.hip" in open(os.path.join(ROOT, "barc4dip_amd", "csrc", "Makefile")).read()
