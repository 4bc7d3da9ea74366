"""Displacement maps, host tier (no GPU): grid geometry and argument checks of barc4dip_amd.signal.displacement, and the
per-window oracle the GPU tests compare against (tests/test_gpu_displacement.py), checked against a brute-force NCC and a
piecewise integer shift field."""
from __future__ import annotations

import numpy as np
import pytest

from barc4dip_amd import synth
from barc4dip_amd.signal import displacement as DM
from oracle import ncc_np as N
from oracle import signal_np as S


# ---- per-window oracle: the definition of a displacement map in terms of the single-pair oracle
def oracle_map(ref, img, *, window=31, step=None, search=8, backend="opencv", subpixel=True, eps=1e-9, windows=None):
    """(dy, dx, peak, snr) float64 arrays of shape (gy, gx) from oracle.ncc_np.template_matching on cut boxes; `windows`
    (iterable of (iy, ix) grid indices) restricts the work to those windows (the others stay NaN)."""
    g = DM.displacement_grid(np.shape(ref), window=window, step=step, search=search)
    (wy, wx), (sy, sx) = g["window"], g["search"]
    out = np.full(g["shape"] + (4,), np.nan)
    if windows is None:
        windows = np.ndindex(*g["shape"])
    for iy, ix in windows:
        y0, x0 = int(g["y0"][iy]), int(g["x0"][ix])
        out[iy, ix] = N.template_matching(ref[y0:y0 + wy, x0:x0 + wx], img[y0 - sy:y0 + wy + sy, x0 - sx:x0 + wx + sx],
                                          slices_yx=(slice(sy, sy + wy), slice(sx, sx + wx)), backend=backend,
                                          subpixel=subpixel, eps=eps)
    return out[..., 0], out[..., 1], out[..., 2], out[..., 3]


def piecewise_field(n=192, block=64, seed=11):
    """Reference speckle frame and an image whose (block x block) tiles are the reference rolled by different integer
    shifts.  Returns (ref, img, shift_of(y, x) -> (sy, sx) of the tile holding pixel (y, x))."""
    rng = np.random.default_rng(seed)
    ref = rng.poisson(synth.speckle_intensity(n, seed, pupil_div=6)).astype(np.float32)
    shifts = {}
    img = np.empty_like(ref)
    for by in range(0, n, block):
        for bx in range(0, n, block):
            s = (int(rng.integers(-4, 5)), int(rng.integers(-4, 5)))
            shifts[(by // block, bx // block)] = s
            img[by:by + block, bx:bx + block] = np.roll(ref, s, axis=(0, 1))[by:by + block, bx:bx + block]
    img = img + rng.normal(size=img.shape).astype(np.float32) * 5
    return ref, img, lambda y, x: shifts[(y // block, x // block)]


def inside_one_tile(g, iy, ix, block):
    (wy, wx), (sy, sx) = g["window"], g["search"]
    y0, x0 = int(g["y0"][iy]), int(g["x0"][ix])
    ya, yb, xa, xb = y0 - sy, y0 + wy + sy - 1, x0 - sx, x0 + wx + sx - 1
    return ya // block == yb // block and xa // block == xb // block


# ---- grid geometry
def test_grid_origins_centres_counts():
    g = DM.displacement_grid((100, 120), window=21, step=10, search=5)
    assert g["window"] == (21, 21) and g["step"] == (10, 10) and g["search"] == (5, 5)
    np.testing.assert_array_equal(g["y0"], 5 + 10 * np.arange(7))      # last: 65 + 21 + 5 = 91 <= 100, next 101 > 100
    np.testing.assert_array_equal(g["x0"], 5 + 10 * np.arange(9))      # last: 85 + 26 = 111 <= 120
    assert g["shape"] == (7, 9)
    np.testing.assert_array_equal(g["y"], g["y0"] + 10.0)
    assert g["y"].dtype == np.float64 and g["y0"].dtype == np.int64
    for a, b in zip(g["y0"], g["y0"][1:]):
        assert b - a == 10
    assert g["y0"][-1] + 21 + 5 <= 100 < g["y0"][-1] + 10 + 21 + 5


def test_grid_exact_fit_and_single_window():
    g = DM.displacement_grid((31 + 16, 31 + 16), window=31, step=16, search=8)
    assert g["shape"] == (1, 1) and g["y0"][0] == 8 and g["y"][0] == 23.0


def test_grid_pairs_even_window_and_default_step():
    g = DM.displacement_grid((300, 517), window=(16, 31), step=None, search=(3, 8))
    assert g["step"] == (8, 15)
    np.testing.assert_array_equal(g["y"], g["y0"] + 7.5)                # even window: half-integer centres
    np.testing.assert_array_equal(g["x"], g["x0"] + 15.0)
    assert g["shape"] == ((300 - 16 - 6) // 8 + 1, (517 - 31 - 16) // 15 + 1)
    assert DM.displacement_grid((64, 64), window=(9, 9), step=(4, 4), search=(2, 2))["shape"] == \
        DM.displacement_grid((64, 64), window=9, step=4, search=2)["shape"]
    assert DM.displacement_grid((64, 64), window=1, step=None, search=1)["step"] == (1, 1)   # 1 // 2 -> at least 1
    assert DM.displacement_grid((64, 64), window=np.int64(9), search=[2, 3])["search"] == (2, 3)
    g = DM.displacement_grid((64, 64), window=np.array(9), step=np.array([4, 5]), search=np.array(2))   # 0-d arrays are scalars
    assert g["window"] == (9, 9) and g["step"] == (4, 5) and g["search"] == (2, 2)


@pytest.mark.parametrize("kw", [dict(window=0), dict(window=(5, 0)), dict(step=0), dict(step=(1, -1)), dict(search=0),
                                dict(search=(0, 3)), dict(window=(5, 5, 5)), dict(window=2.5), dict(search=True),
                                dict(window=np.array(0)), dict(window=np.array(2.5)), dict(step=np.ones((2, 2), int))])
def test_grid_value_errors(kw):
    with pytest.raises(ValueError):
        DM.displacement_grid((256, 256), **kw)


def test_grid_limits_and_fit():
    assert DM.displacement_grid((400, 400), window=128, search=32)["shape"] == (4, 4)      # the documented limits fit: (400 - 192) // 64 + 1
    with pytest.raises(NotImplementedError):
        DM.displacement_grid((400, 400), window=129, search=8)
    with pytest.raises(NotImplementedError):
        DM.displacement_grid((400, 400), window=(31, 200), search=8)
    with pytest.raises(NotImplementedError):
        DM.displacement_grid((400, 400), window=31, search=33)
    with pytest.raises(ValueError):                         # 31 + 2 * 8 = 47 > 46: no grid point
        DM.displacement_grid((46, 100), window=31, search=8)
    with pytest.raises(ValueError):
        DM.displacement_grid((100, 46), window=31, search=8)


def test_map_argument_errors_before_any_device_work():
    """Every ValueError / NotImplementedError of displacement_map that depends only on shapes and arguments is raised on the
    host, before the GPU is touched."""
    ref = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError):
        DM.displacement_map(ref, ref, window=15, search=4, backend="internal")
    with pytest.raises(ValueError):
        DM.displacement_map(ref, np.zeros((64, 63), np.float32), window=15, search=4)
    with pytest.raises(ValueError):
        DM.displacement_map(np.zeros((3, 64, 64)), np.zeros((4, 64, 64)), window=15, search=4)
    with pytest.raises(ValueError):
        DM.displacement_map(np.zeros((3, 64, 64)), ref, window=15, search=4)
    with pytest.raises(ValueError):
        DM.displacement_map(np.zeros(64), ref, window=15, search=4)
    with pytest.raises(ValueError):
        DM.displacement_map(ref, ref, window=60, search=4)
    with pytest.raises(ValueError):
        DM.displacement_map(ref, ref, window=15, search=0)
    with pytest.raises(ValueError):
        DM.displacement_map(ref, ref, window=15, step=0, search=4)
    with pytest.raises(NotImplementedError):
        DM.displacement_map(np.zeros((400, 400)), np.zeros((400, 400)), window=130, search=4)
    with pytest.raises(NotImplementedError):
        DM.displacement_map(np.zeros((400, 400)), np.zeros((400, 400)), window=15, search=40)


def test_public_export():
    from barc4dip_amd import signal

    assert signal.displacement_map is DM.displacement_map and "displacement_map" in signal.__all__


# ---- the oracle itself
def test_oracle_equals_bruteforce_ncc_on_tiny_case():
    rng = np.random.default_rng(3)
    ref = rng.random((26, 29)).astype(np.float32)
    img = np.roll(ref, (1, -2), axis=(0, 1)) + rng.normal(size=ref.shape).astype(np.float32) * 0.05
    win, step, srch = (7, 6), (5, 4), (2, 3)
    for backend in ("opencv", "skimage"):
        dy, dx, peak, snr = oracle_map(ref, img, window=win, step=step, search=srch, backend=backend, subpixel=False)
        g = DM.displacement_grid(ref.shape, window=win, step=step, search=srch)
        for iy, ix in np.ndindex(*g["shape"]):
            y0, x0 = int(g["y0"][iy]), int(g["x0"][ix])
            box = img[y0 - 2:y0 + 7 + 2, x0 - 3:x0 + 6 + 3]
            box = S.zscore2d(box, 1e-9).astype(np.float32) if backend == "opencv" else box
            m = N.match_template_bruteforce(box, S.zscore2d(ref[y0:y0 + 7, x0:x0 + 6], 1e-9).astype(np.float32))
            assert m.shape == (5, 7)
            mi, mj = np.unravel_index(int(np.argmax(m)), m.shape)
            assert (dy[iy, ix], dx[iy, ix]) == (mi - 2, mj - 3)
            assert abs(peak[iy, ix] - m[mi, mj]) < 1e-6
            assert abs(snr[iy, ix] - abs(m[mi, mj]) / (np.median(np.abs(m)) + 1e-9)) < 1e-5 * snr[iy, ix]
        assert np.all((dy == 1) & (dx == -2))


def test_oracle_recovers_piecewise_integer_shift_field():
    ref, img, shift_of = piecewise_field()
    kw = dict(window=15, step=8, search=4)
    g = DM.displacement_grid(ref.shape, **kw)
    sel = [(iy, ix) for iy, ix in np.ndindex(*g["shape"]) if inside_one_tile(g, iy, ix, 64)]
    assert len(sel) > 40
    dy, dx, peak, _ = oracle_map(ref, img, subpixel=False, windows=sel, **kw)
    for iy, ix in sel:
        assert (dy[iy, ix], dx[iy, ix]) == shift_of(int(g["y0"][iy]), int(g["x0"][ix]))
        assert peak[iy, ix] > 0.9
