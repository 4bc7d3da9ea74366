"""Host tier of the separable filters and local statistics: the float64 models of tests/smoothing_model.py against scipy.ndimage,
the tap builders against SciPy's impulse response, argument errors without a device, and the wiring.  No GPU needed."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smoothing_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = sorted(M.MODES)
RNG = np.random.default_rng(2611)
FRAME = RNG.poisson(40.0, (2, 9, 13)).astype(np.float64) + RNG.random((2, 9, 13))


def rel(got, ref, x=FRAME):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(x)))


def scipy_separable(x, wy, wx, mode, cval):
    """correlate1d along x, then along y, per frame."""
    return ndi.correlate1d(ndi.correlate1d(x, wx, axis=-1, mode=mode, cval=cval), wy, axis=-2, mode=mode, cval=cval)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 25, 41])
def test_model_matches_correlate1d(mode, n):
    """Every mode and tap count, the overhang longer than the 9 x 13 frame, cval != 0: pins the border index, the even-size
    placement (the window one sample longer on the left) and the tap order."""
    wy, wx = RNG.standard_normal(n), RNG.standard_normal(max(1, n - 1))
    got = M.model_separable(FRAME, wy, wx, mode, 2.5)
    assert rel(got, scipy_separable(FRAME, wy, wx, mode, 2.5)) <= 1e-12 * np.abs(wy).sum() * np.abs(wx).sum()
    for axis, w in ((-1, wx), (-2, wy)):
        assert rel(M.correlate_axis(FRAME, w, axis, mode, 2.5), ndi.correlate1d(FRAME, w, axis=axis, mode=mode, cval=2.5)) <= 1e-12 * np.abs(w).sum()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sigma,order,kw", [(1.0, 0, {}), (3.0, 0, {}), ((1.5, 6.0), 0, {}), (2.0, (1, 0), {}), (2.0, (0, 2), {}),
                                            (1.2, (2, 1), {}), ((0.0, 2.0), 0, {}), ((2.0, 0.0), (1, 0), {}), (2.0, 0, {"truncate": 2.5}),
                                            (2.0, 0, {"radius": 3}), (1.0, 0, {"radius": (2, 5)})])
def test_model_matches_gaussian_filter(mode, sigma, order, kw):
    """Orders 0 / 1 / 2 per axis, anisotropic sigma, sigma = 0 on one axis, truncate and radius.  cval = 0 with derivative orders:
    SciPy filters y first, and under "constant" with cval != 0 and taps that do not sum to one the pass order shows in the border."""
    sy, sx = (sigma, sigma) if np.ndim(sigma) == 0 else sigma
    oy, ox = (order, order) if np.ndim(order) == 0 else order
    radius = kw.get("radius")
    ry, rx = (radius, radius) if radius is None or np.ndim(radius) == 0 else radius
    wy = M.gaussian_taps(sy, oy, kw.get("truncate", 4.0), ry)
    wx = M.gaussian_taps(sx, ox, kw.get("truncate", 4.0), rx)
    cval = 1.75 if (oy, ox) == (0, 0) else 0.0
    ref = ndi.gaussian_filter(FRAME, sigma=(0, sy, sx), order=(0, oy, ox), mode=mode, cval=cval,
                              **({"radius": (0, ry, rx)} if radius is not None else {"truncate": kw.get("truncate", 4.0)}))
    assert rel(M.model_separable(FRAME, wy, wx, mode, cval), ref) <= 1e-12 * max(1.0, np.abs(wy).sum() * np.abs(wx).sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [1, 2, 3, 4, 7, (2, 5), (25, 4), 41])
def test_model_matches_uniform_filter(mode, size):
    sy, sx = (size, size) if np.ndim(size) == 0 else size
    ref = ndi.uniform_filter(FRAME, size=(1, sy, sx), mode=mode, cval=2.5)
    assert rel(M.model_separable(FRAME, M.box_taps(sy), M.box_taps(sx), mode, 2.5), ref) <= 1e-12


@pytest.mark.parametrize("sigma", [0.8, 2.0, 4.25, 30.0])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_tap_builders_are_scipys_impulse_response(sigma, order):
    """The package's builder and the model's equal the response of gaussian_filter1d to an impulse, reversed (a correlation with
    taps w answers an impulse with w reversed), to 1e-15 of the largest tap."""
    from barc4dip_amd.preprocessing.smooth import gaussian_taps

    lw = int(4.0 * sigma + 0.5)
    imp = np.zeros(2 * lw + 1)
    imp[lw] = 1.0
    resp = ndi.gaussian_filter1d(imp, sigma, order=order, mode="constant")
    for taps in (gaussian_taps(sigma, order), M.gaussian_taps(sigma, order)):
        assert taps.size == 2 * lw + 1
        assert np.max(np.abs(taps - resp[::-1])) <= 1e-15 * np.max(np.abs(resp))
    assert np.array_equal(gaussian_taps(0.0, 0), [1.0]) and np.array_equal(gaussian_taps(2.0, 0, radius=0), [1.0])
    assert gaussian_taps(1.0, 0, truncate=2.4).size == 5 and gaussian_taps(1.0, 0, radius=7).size == 15


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [1, 2, 3, (3, 9), 7, (25, 4)])
def test_local_stats_model_matches_uniform_filter(mode, size):
    sy, sx = (size, size) if np.ndim(size) == 0 else size
    m = M.model_local_stats(FRAME, sy, sx, mode=mode, cval=2.5)
    mean = ndi.uniform_filter(FRAME, size=(1, sy, sx), mode=mode, cval=2.5)
    # (SciPy pads the frame with cval and squares afterwards only if the square is taken of the padded frame: cval^2 outside)
    sq = ndi.uniform_filter(FRAME ** 2, size=(1, sy, sx), mode=mode, cval=2.5 ** 2)
    assert rel(m["mean"], mean) <= 1e-12
    assert float(np.max(np.abs(m["s2_over_w"] - sq)) / np.max(FRAME ** 2)) <= 1e-12
    assert float(np.max(np.abs(m["variance"] - np.maximum(sq - mean * mean, 0.0))) / np.max(FRAME ** 2)) <= 1e-12
    g = M.gaussian_taps(1.0, 0, 3.0)
    mg = M.model_local_stats(FRAME, g.size, g.size, g, g, mode=mode, cval=2.5)
    assert rel(mg["mean"], ndi.gaussian_filter(FRAME, (0, 1.0, 1.0), mode=mode, cval=2.5, truncate=3.0)) <= 1e-12


def test_local_stats_model_edge_values():
    c = np.full((5, 6), 7.0)
    m = M.model_local_stats(c, 3, 3)
    assert np.all(m["variance"] == 0.0) and np.all(m["contrast"] == 0.0) and np.all(m["mean"] == 7.0)
    assert np.all(np.isnan(M.model_local_stats(np.zeros((4, 4)), 3, 3)["contrast"]))
    x = FRAME[0].copy()
    x[4, 6] = np.nan
    m = M.model_local_stats(x, 3, 5)
    foot = np.zeros_like(x, dtype=bool)
    foot[3:6, 4:9] = True
    for k in ("mean", "variance", "contrast"):
        assert np.array_equal(np.isnan(m[k]), foot)


def test_nan_poisons_exactly_the_footprint_in_the_model():
    x = FRAME[0].copy()
    x[4, 6] = np.nan
    w = np.array([0.0, 0.5, 0.0, 0.25])          # zero taps poison too; even size: offsets -2 .. 1
    got = np.isnan(M.model_separable(x, w, [1.0], "reflect"))
    foot = np.zeros_like(got)
    foot[3:7, 6] = True                            # outputs i with i - 2 + k = 4: i = 6 - k, k = 0 .. 3
    assert np.array_equal(got, foot)


def test_bounds_are_formed_from_the_data():
    wy, wx = M.gaussian_taps(30.0), M.gaussian_taps(30.0)
    x = np.full((1, 4, 4), 68.0)                   # a typical maximum of a Poisson(40) frame: 1.01 u 68 (245 + 245) = 2.0e-3
    b = M.bound_separable(x, wy, wx)
    assert b.shape == (1, 1, 1) and 1.9e-3 < float(b.squeeze()) < 2.1e-3
    assert np.allclose(M.bound_subtract(1e-3, -2.0), 1e-3 + 2.0 * M.U)
    assert np.allclose(M.bound_divide(1e-3, 4.0, 2.0, 2.0), 1e-3 + 4.0 * M.U)


def test_argument_errors_without_a_device(monkeypatch):
    from barc4dip_amd import _ffi
    from barc4dip_amd.metrics import local_contrast
    from barc4dip_amd.preprocessing import gaussian_filter, remove_envelope, separable_filter, uniform_filter

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the arguments were checked")

    monkeypatch.setattr(_ffi, "require_gpu", no_device)
    img = np.ones((8, 8), dtype=np.float32)
    bad = [
        lambda: gaussian_filter(img, -1.0), lambda: gaussian_filter(img, float("nan")), lambda: gaussian_filter(img, (1.0, 2.0, 3.0)),
        lambda: gaussian_filter(img, 1.0, order=3), lambda: gaussian_filter(img, 1.0, order=(0, -1)), lambda: gaussian_filter(img, 1.0, mode="edge"),
        lambda: gaussian_filter(img, 64.0), lambda: gaussian_filter(img, 1.0, radius=256), lambda: gaussian_filter(img, 1.0, radius=-1),
        lambda: uniform_filter(img, 0), lambda: uniform_filter(img, 512), lambda: uniform_filter(img, 2.5), lambda: uniform_filter(img, 3, mode="x"),
        lambda: separable_filter(img, np.ones(512), None), lambda: separable_filter(img, None, np.ones((2, 2))),
        lambda: separable_filter(img, [], None), lambda: separable_filter(img, [np.inf], None),
        lambda: remove_envelope(img, 2.0, method="ratio"), lambda: remove_envelope(img, 2.0, eps=0.0), lambda: remove_envelope(img, 64.0),
        lambda: local_contrast(img, 0), lambda: local_contrast(img, 64), lambda: local_contrast(img, (3, 64)), lambda: local_contrast(img, 3, window="hann"),
        lambda: local_contrast(img, window="gaussian"), lambda: local_contrast(img, window="gaussian", sigma=11.0),
        lambda: local_contrast(img, window="gaussian", sigma=-1.0), lambda: local_contrast(img, 3, mode="edge"),
        lambda: gaussian_filter(np.ones((0, 8), dtype=np.float32), 1.0), lambda: uniform_filter(np.ones((2, 8, 0)), 3),
        lambda: separable_filter(np.ones(8), None, None), lambda: remove_envelope(np.ones((1, 2, 0, 8)), 2.0),
        lambda: local_contrast(np.ones((0, 8, 8)), 3),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} raised nothing")
    with pytest.raises(ValueError, match="255"):
        gaussian_filter(img, 64.0)
    with pytest.raises(ValueError, match="31"):
        local_contrast(img, window="gaussian", sigma=11.0)


def test_wiring():
    import barc4dip_amd.metrics as metrics
    import barc4dip_amd.preprocessing as prep
    from barc4dip_amd import _ffi

    for name in ("gaussian_filter", "uniform_filter", "separable_filter", "remove_envelope"):
        assert name in prep.__all__ and callable(getattr(prep, name))
    assert "local_contrast" in metrics.__all__ and callable(metrics.local_contrast)
    assert "b4d_separable_filter" in _ffi.SIGNATURES and "b4d_local_stats" in _ffi.SIGNATURES
    mk = open(os.path.join(ROOT, "barc4dip_amd", "csrc", "Makefile")).read()
    src = next(line for line in mk.splitlines() if line.startswith("SRC"))
    assert "b4d_smooth.hip" in src.split()
