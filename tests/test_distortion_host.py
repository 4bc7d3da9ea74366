"""Distortion correction, host tier (no GPU): the float64 oracle that tests/test_gpu_distortion.py compares against -- scipy's
map_coordinates for the warp, the grid-expansion rule, and a NumPy restatement of the kernel algorithm (truncated FIR
prefilter per mode, explicit taps) checked against scipy -- and the argument checks of barc4dip_amd.preprocessing.distortion,
which all run before the GPU is touched."""
from __future__ import annotations

import numpy as np
import pytest
from scipy import ndimage as ndi

from barc4dip_amd.preprocessing import distortion as DI
from barc4dip_amd.signal import displacement as DM

MODES = ("nearest", "reflect", "mirror", "constant")

# ---- oracle -----------------------------------------------------------------------------------------------------------------
FIR = np.sqrt(3.0) * (np.sqrt(3.0) - 2.0) ** np.abs(np.arange(-14, 15))    # truncated cubic B-spline prefilter, |k| <= 14


def expand_grid(g, y, x, shape):
    """Per-pixel field of grid values g (gy, gx) on the regular window-centre axes y, x: bilinear between the centres, held
    constant beyond the outermost ones."""
    H, W = shape
    sy = (y[-1] - y[0]) / (len(y) - 1) if len(y) > 1 else 1.0
    sx = (x[-1] - x[0]) / (len(x) - 1) if len(x) > 1 else 1.0
    u, v = np.meshgrid((np.arange(H) - y[0]) / sy, (np.arange(W) - x[0]) / sx, indexing="ij")
    return ndi.map_coordinates(np.asarray(g, np.float64), [u, v], order=1, mode="nearest")


def dense_field(field, shape, t=None):
    """(dyp, dxp) per-pixel float64 field of frame t from a grid dict or a dense pair (as correct_distortion reads it)."""
    if isinstance(field, dict):
        dy, dx = np.asarray(field["dy"], np.float64), np.asarray(field["dx"], np.float64)
        if dy.ndim == 3:
            dy, dx = dy[t], dx[t]
        return expand_grid(dy, field["y"], field["x"], shape), expand_grid(dx, field["y"], field["x"], shape)
    dy, dx = (np.asarray(a, np.float64) for a in field)
    if dy.ndim == 3:
        dy, dx = dy[t], dx[t]
    return dy, dx


def warp_scipy(images, field, *, order=3, mode="nearest", cval=0.0):
    """The definition: map_coordinates of every float64 frame at (y + dyp, x + dxp)."""
    im = np.asarray(images, np.float64)
    frames = im.reshape((-1,) + im.shape[-2:])
    H, W = frames.shape[1:]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty_like(frames)
    for t in range(frames.shape[0]):
        dy, dx = dense_field(field, (H, W), t)
        out[t] = ndi.map_coordinates(frames[t], [yy + dy, xx + dx], order=order, mode=mode, cval=cval)
    return out.reshape(im.shape)


def fold(i, n, mode):
    """Index i of an n-sample signal folded into [0, n): edge clamp / half-sample (reflect) / whole-sample (mirror)."""
    i = np.asarray(i, np.int64)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "reflect":
        i = np.mod(i, 2 * n)
        return np.where(i >= n, 2 * n - 1 - i, i)
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * (n - 1))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def prefilter(frame, mode):
    """Cubic B-spline coefficients as the kernels compute them: "nearest" pads 12 px with edge values and filters with mirror
    extension, "reflect" filters with reflect extension, "mirror" and "constant" with mirror extension.  Returns (coef, pad)."""
    c = np.asarray(frame, np.float64)
    pad = 12 if mode == "nearest" else 0
    if pad:
        c = np.pad(c, pad, mode="edge")
    fm = "reflect" if mode == "reflect" else "mirror"
    for ax in (0, 1):
        n = c.shape[ax]
        idx = fold(np.arange(n)[None, :] + np.arange(-14, 15)[:, None], n, fm)     # (29, n)
        c = np.moveaxis(np.einsum("k,kn...->n...", FIR, np.moveaxis(c, ax, 0)[idx]), 0, ax)
    return c, pad


def _cubic_weights(t):
    return [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]


def warp_restated(frame, dy, dx, *, order=3, mode="nearest", cval=0.0):
    """NumPy restatement of the warp kernel for one frame: taps from floor(displacement), weights from its fraction."""
    H, W = frame.shape
    c, pad = prefilter(frame, mode) if order == 3 else (np.asarray(frame, np.float64), 0)
    ch, cw = c.shape
    tm = "mirror" if mode == "constant" else mode
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fy, fx = np.floor(dy), np.floor(dx)
    ty, tx = dy - fy, dx - fx
    iy, ix = yy + pad + fy.astype(np.int64), xx + pad + fx.astype(np.int64)
    if order == 0:                                      # floor(c + 0.5): half-integers round up
        out = c[fold(iy + (ty >= 0.5), ch, tm), fold(ix + (tx >= 0.5), cw, tm)]
    else:
        wy, wx = ([1 - ty, ty], [1 - tx, tx]) if order == 1 else (_cubic_weights(ty), _cubic_weights(tx))
        o = 0 if order == 1 else 1
        out = 0.0
        for a in range(order + 1):
            for b in range(order + 1):
                out = out + wy[a] * wx[b] * c[fold(iy - o + a, ch, tm), fold(ix - o + b, cw, tm)]
    if mode == "constant":
        out = np.where((dy < -yy) | (dy > H - 1 - yy) | (dx < -xx) | (dx > W - 1 - xx), cval, out)
    return out


def smooth_field(shape, amp, seed, *, knots=4):
    """Smooth random per-pixel field (dy, dx) of amplitude up to `amp` px (cubic zoom of a few random knots)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    out = []
    for _ in range(2):
        k = rng.uniform(-amp, amp, (knots, knots))
        u, v = np.meshgrid(np.linspace(0, knots - 1, H), np.linspace(0, knots - 1, W), indexing="ij")
        out.append(np.clip(ndi.map_coordinates(k, [u, v], order=3, mode="nearest"), -amp, amp))
    return out[0], out[1]


# ---- the restatement against scipy -------------------------------------------------------------------------------------------
SHAPES = [(37, 53), (128, 96), (64, 64), (9, 300), (1, 7)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_matches_scipy(shape, order, mode):
    rng = np.random.default_rng(sum(shape) + 10 * order)
    frame = rng.random(shape)
    dy, dx = smooth_field(shape, 12.0, seed=order + 3)
    dy, dx = dy + rng.uniform(-1, 1, shape), dx + rng.uniform(-1, 1, shape)     # rough on top of smooth: every fraction
    want = warp_scipy(frame, (dy, dx), order=order, mode=mode, cval=0.375)
    got = warp_restated(frame, dy, dx, order=order, mode=mode, cval=0.375)
    if order == 0:
        np.testing.assert_array_equal(got, want)
    else:
        assert np.max(np.abs(got - want)) <= 1e-7 * np.ptp(frame)


def test_restatement_reflect_startup_of_short_frames():
    """scipy's reflect prefilter starts up differently on frames shorter than ~8 px: the FIR route differs there, which is
    why the order-3 reflect parity keeps to larger frames."""
    frame = np.random.default_rng(0).random((2, 9))
    dy, dx = smooth_field((2, 9), 3.0, seed=1)
    d = np.abs(warp_restated(frame, dy, dx, mode="reflect") - warp_scipy(frame, (dy, dx), mode="reflect"))
    assert 1e-7 < d.max() < 1e-2


def test_fir_taps_sum_to_one_and_decay():
    assert abs(FIR.sum() - 1.0) < 1e-8
    assert abs(FIR[0]) < 3e-8 and FIR[14] == pytest.approx(np.sqrt(3.0))


def test_grid_expansion_rule():
    """Bilinear between the window centres, constant beyond the outermost ones; a plane is reproduced inside."""
    y, x = 15.0 + 16.0 * np.arange(5), 15.0 + 16.0 * np.arange(7)
    g = 0.25 * y[:, None] - 0.5 * x[None, :]
    f = expand_grid(g, y, x, (120, 140))
    yy, xx = np.meshgrid(np.arange(120.0), np.arange(140.0), indexing="ij")
    inside = (yy >= y[0]) & (yy <= y[-1]) & (xx >= x[0]) & (xx <= x[-1])
    np.testing.assert_allclose(f[inside], (0.25 * yy - 0.5 * xx)[inside], atol=1e-12)
    assert np.all(f[:15, 30] == f[15, 30]) and np.all(f[100:, 30] == f[79, 30])
    assert np.all(expand_grid(np.array([[2.5]]), [40.0], [7.0], (8, 9)) == 2.5)     # one window: a constant field


def test_oracle_sign_convention():
    """out(p) = img(p + d): a frame shifted by +3 rows is brought back by dy = +3."""
    ref = np.random.default_rng(1).random((40, 50))
    img = np.roll(ref, 3, axis=0)
    out = warp_scipy(img, (np.full((40, 50), 3.0), np.zeros((40, 50))), order=1)
    np.testing.assert_array_equal(out[:37], ref[:37])


# ---- argument checks (no GPU needed: they come before the device is touched) ------------------------------------------------
def _grid_field(shape=(64, 64), T=None, **kw):
    g = DM.displacement_grid(shape, window=15, step=8, search=4)
    s = g["shape"] if T is None else (T,) + g["shape"]
    return dict({"dy": np.zeros(s), "dx": np.zeros(s), "y": g["y"], "x": g["x"]}, **kw)


@pytest.mark.parametrize("kw", [dict(order=2), dict(order=5), dict(order=1.0), dict(order=True), dict(order="1"),
                                dict(mode="wrap"), dict(mode="grid-constant"), dict(mode="NEAREST"), dict(mode=None)])
def test_bad_order_or_mode(kw):
    img = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError):
        DI.correct_distortion(img, _grid_field(), **kw)
    with pytest.raises(ValueError):
        DI.remove_distortion(img, img, window=15, step=8, search=4, **kw)


def test_field_errors():
    img = np.zeros((64, 64), np.float32)
    stack = np.zeros((3, 64, 64), np.float32)
    z = np.zeros((64, 64))
    bad = [
        (img, (z, np.zeros((64, 63)))),                         # dy and dx differ
        (img, (np.zeros((64, 65)), np.zeros((64, 65)))),        # dense field and frame shapes differ
        (img, (np.zeros((3, 64, 64)),) * 2),                    # per-frame field for a single frame
        (stack, (np.zeros((2, 64, 64)),) * 2),                  # T mismatch
        (stack, _grid_field(T=4)),                              # T mismatch, grid
        (img, (z,)),                                            # not a pair
        (img, z),                                               # not a field
        (img, {"dy": z, "dx": z}),                              # grid without axes
        (img, (np.zeros(64), np.zeros(64))),                    # 1-D field
        (img, (np.zeros((0, 64)), np.zeros((0, 64)))),          # empty dense field
        (img, {"dy": np.zeros((0, 3)), "dx": np.zeros((0, 3)), "y": np.zeros(0), "x": np.arange(3.0)}),   # empty grid
        (img, _grid_field(y=np.array([7.0, 15.0, 24.0, 31.0, 39.0, 47.0]))),    # irregular y axis
        (img, _grid_field(x=np.array([7.0, 15.0, 23.0, 31.0, 39.0, 39.0]))),    # irregular x axis (repeated point)
        (img, _grid_field(x=np.full(6, 7.0))),                  # zero step
        (img, _grid_field(y=np.arange(5.0))),                   # axis length differs from the grid
        (img, _grid_field(y=np.array([7.0, np.nan, 23.0, 31.0, 39.0, 47.0]))),  # non-finite axis
        (np.zeros((0, 64)), (np.zeros((0, 64)),) * 2),          # empty images
        (np.zeros((2, 2, 64, 64)), _grid_field()),              # 4-D images
    ]
    for images, field in bad:
        with pytest.raises(ValueError):
            DI.correct_distortion(images, field)


def test_remove_distortion_checks_before_device():
    ref = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError):                             # displacement_map's own checks
        DI.remove_distortion(ref, np.zeros((64, 63), np.float32), window=15, search=4)
    with pytest.raises(ValueError):
        DI.remove_distortion(ref, ref, window=15, search=4, backend="internal")
    with pytest.raises(ValueError):
        DI.remove_distortion(np.zeros((2, 64, 64)), ref, window=15, search=4)


def test_grid_axes_accept_displacement_grid_and_single_points():
    g = DM.displacement_grid((300, 517), window=(16, 31), step=(8, 15), search=(3, 8))
    assert DI._regular_axis(g["y"], g["shape"][0], "y") == (g["y"][0], 8.0)
    assert DI._regular_axis(g["x"], g["shape"][1], "x") == (g["x"][0], 15.0)
    assert DI._regular_axis([42.5], 1, "y") == (42.5, 1.0)
    assert DI._regular_axis([10.0, 7.0, 4.0], 3, "y") == (10.0, -3.0)     # a decreasing axis is regular too


def test_newton_subpixel_argument():
    ref = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError):
        DM.displacement_map(ref, ref, window=15, search=4, subpixel="taylor")
    assert DM._subpixel_code("newton") == 2 and DM._subpixel_code(True) == 1 and DM._subpixel_code(False) == 0
