"""Distortion correction on the MI355X (b4d_spline_prefilter / b4d_warp_dense / b4d_warp_grid,
barc4dip_amd/preprocessing/distortion.py) against the float64 scipy oracle of tests/test_distortion_host.py, exact cases, input
kinds, the Newton sub-pixel step of displacement maps and a full round trip.  Bars: 2 x the observed maximum (DESIGN.md
section 5), relative to the data range."""
from __future__ import annotations

import numpy as np
import pytest
from scipy import ndimage as ndi

from barc4dip_amd import synth
from test_displacement_host import oracle_map
from test_distortion_host import dense_field, smooth_field, warp_scipy

pytestmark = pytest.mark.gpu

BARS = {    # 2 x the observed maximum on MI355X; newton/subpx_mae is the issue's 0.1 px
    "warp/o1_dense": 2.1e-7, "warp/o1_grid": 6e-6, "warp/o3_dense": 1.3e-6, "warp/o3_grid": 7.5e-6, "warp/o0_grid_ties": 2e-3,
    "warp/o3_integer": 1.1e-6, "warp/uint16": 1e-6, "warp/2160x2560": 6e-7,
    "newton/subpx_mae": 0.1, "newton/sub_px": 7e-7,
    "roundtrip/field_mae": 0.08, "roundtrip/residual_mae": 0.04,
}
MODES = ("nearest", "reflect", "mirror", "constant")


@pytest.fixture(scope="module")
def di():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.preprocessing import distortion

    return distortion


def _frames(shape, T, seed):
    return np.random.default_rng(seed).random((T,) + shape).astype(np.float32)


def _grid(shape, T, amp, seed, gy=7, gx=9):
    """Grid field dict on regular centres that lie inside the frame, values up to +-amp px, (T, gy, gx) or (gy, gx)."""
    H, W = shape
    rng = np.random.default_rng(seed)
    y = 0.15 * H + (0.7 * H / (gy - 1)) * np.arange(gy)
    x = 0.1 * W + (0.8 * W / (gx - 1)) * np.arange(gx)
    s = (gy, gx) if T is None else (T, gy, gx)
    return {"dy": rng.uniform(-amp, amp, s), "dx": rng.uniform(-amp, amp, s), "y": y, "x": x}


def _f32_field(field):
    """The field as the kernels receive it (float32 values), for the oracle."""
    if isinstance(field, dict):
        return dict(field, dy=np.asarray(field["dy"], np.float32), dx=np.asarray(field["dx"], np.float32))
    return tuple(np.asarray(a, np.float32) for a in field)


def _keep_mask(field, shape, T, order, mode, near):
    """Pixels away from the discontinuities of the definition, where a float32 field may fall on the other side: the frame
    border in "constant" mode and the rounding ties of order 0 (grid fields: the field is interpolated in float32)."""
    H, W = shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    keep = np.ones((T, H, W), bool)
    for t in range(T):
        dy, dx = dense_field(field, shape, t)
        for c, n in ((yy + dy, H), (xx + dx, W)):
            if mode == "constant":
                keep[t] &= (np.abs(c) > near) & (np.abs(c - (n - 1)) > near)
            if order == 0:
                keep[t] &= np.abs(np.abs(c - np.floor(c)) - 0.5) > near
    return keep


def _compare(got, want, keep, frames, order, observe, key):
    got, want = got[keep], want[keep]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    if order == 0:
        np.testing.assert_array_equal(got[fin], want[fin])
        return
    observe(key, np.max(np.abs(got[fin] - want[fin]), initial=0.0) / np.ptp(frames), BARS[key])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("shape", [(64, 64), (37, 53), (300, 517)])
def test_parity_dense_per_frame(di, shape, order, mode, observe):
    T = 3
    frames = _frames(shape, T, seed=order + 7)
    fl = [smooth_field(shape, 20.0, seed=t + 11) for t in range(T)]
    field = (np.stack([f[0] for f in fl]), np.stack([f[1] for f in fl]))
    for cval in ((np.nan, 2.5) if mode == "constant" else (0.0,)):
        got = di.correct_distortion(frames, field, order=order, mode=mode, cval=cval)
        assert got.dtype == np.float32 and got.shape == frames.shape
        want = warp_scipy(frames, _f32_field(field), order=order, mode=mode, cval=cval)
        keep = _keep_mask(_f32_field(field), shape, T, order, mode, 0.0)
        _compare(got, want, keep, frames, order, observe, f"warp/o{order}_dense" if order else "")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("shape,per_frame", [((64, 64), True), ((37, 53), False), ((300, 517), True), ((300, 517), False)])
def test_parity_grid(di, shape, per_frame, order, mode, observe):
    T = 3
    frames = _frames(shape, T, seed=order + 17)
    field = _grid(shape, T if per_frame else None, 20.0, seed=5)
    for cval in ((np.nan, -1.0) if mode == "constant" else (0.0,)):
        got = di.correct_distortion(frames, field, order=order, mode=mode, cval=cval)
        want = warp_scipy(frames, _f32_field(field), order=order, mode=mode, cval=cval)
        keep = _keep_mask(_f32_field(field), shape, T, order, mode, 1e-4)
        if order == 0:      # a tie moved by the float32 field rounds the other way: count how many pixels were set aside
            observe("warp/o0_grid_ties", 1.0 - keep.mean(), BARS["warp/o0_grid_ties"])
        _compare(got, want, keep, frames, order, observe, f"warp/o{order}_grid" if order else "")


@pytest.mark.parametrize("order,mode", [(1, "nearest"), (3, "nearest"), (3, "constant"), (0, "mirror")])
def test_parity_2048_shared_grid(di, order, mode, observe):
    shape = (2048, 2048)
    frames = _frames(shape, 1, seed=3)[0]
    g = _grid(shape, None, 20.0, seed=8, gy=15, gx=13)
    got = di.correct_distortion(frames, g, order=order, mode=mode, cval=np.nan)
    want = warp_scipy(frames, _f32_field(g), order=order, mode=mode, cval=np.nan)
    keep = _keep_mask(_f32_field(g), shape, 1, order, mode, 1e-4)[0]
    _compare(got, want, keep, frames, order, observe, f"warp/o{order}_grid" if order else "")


# ---- exact cases
@pytest.mark.parametrize("mode", MODES)
def test_zero_field_is_identity(di, mode):
    frames = _frames((37, 53), 2, seed=1)
    z = np.zeros((37, 53))
    g = _grid((37, 53), None, 0.0, seed=1)
    for order in (0, 1):
        for field in ((z, z), g):
            got = di.correct_distortion(frames, field, order=order, mode=mode)
            assert np.array_equal(got.view(np.uint32), frames.view(np.uint32))


def test_integer_field_nearest_is_clamped_slicing(di):
    H, W = 64, 80
    frames = _frames((H, W), 2, seed=2)
    rng = np.random.default_rng(3)
    dy = rng.integers(-30, 31, (H, W)).astype(np.float64)
    dx = rng.integers(-30, 31, (H, W)).astype(np.float64)
    got = di.correct_distortion(frames, (dy, dx), order=1, mode="nearest")
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    iy, ix = np.clip(yy + dy.astype(int), 0, H - 1), np.clip(xx + dx.astype(int), 0, W - 1)
    np.testing.assert_array_equal(got, frames[:, iy, ix])


@pytest.mark.parametrize("mode", MODES)
def test_order3_at_integer_positions(di, mode, observe):
    frames = _frames((300, 517), 1, seed=4)
    rng = np.random.default_rng(5)
    dy = rng.integers(-5, 6, (300, 517)).astype(np.float64)
    dx = rng.integers(-5, 6, (300, 517)).astype(np.float64)
    got = di.correct_distortion(frames, (dy, dx), order=3, mode=mode, cval=0.0)
    want = warp_scipy(frames, (dy, dx), order=0, mode=mode, cval=0.0)     # at integer positions the spline is the sample
    observe("warp/o3_integer", np.max(np.abs(got - want)), BARS["warp/o3_integer"])


# ---- inputs
def test_uint16_stack(di, observe):
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 65535, (3, 128, 96)).astype(np.uint16)
    field = smooth_field((128, 96), 6.0, seed=9)
    got = di.correct_distortion(frames, field, order=3, mode="reflect")
    assert got.dtype == np.float32 and got.shape == frames.shape
    want = warp_scipy(frames.astype(np.float64), _f32_field(field), order=3, mode="reflect")
    observe("warp/uint16", np.max(np.abs(got - want)) / 65535.0, BARS["warp/uint16"])
    assert np.any(got != np.round(got))     # float32 output: not rounded back to the input's integers


def test_tensor_stack_return_tensors(di):
    import torch

    frames = _frames((64, 96), 4, seed=7)
    g = _grid((64, 96), 4, 3.0, seed=2)
    t = torch.from_numpy(frames).cuda()
    gt = dict(g, dy=torch.from_numpy(g["dy"]).cuda(), dx=torch.from_numpy(g["dx"]).cuda())
    out = di.correct_distortion(t, gt, order=1, mode="mirror", return_tensors=True)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (4, 64, 96)
    np.testing.assert_array_equal(out.cpu().numpy(), di.correct_distortion(frames, g, order=1, mode="mirror"))


def test_detector_frame_2160x2560(di, observe):
    shape = (2160, 2560)
    frame = synth.speckle_frame(2560, 12)[:2160]
    g = _grid(shape, None, 8.0, seed=4, gy=12, gx=15)
    got = di.correct_distortion(frame, g, order=3)
    want = warp_scipy(frame, _f32_field(g), order=3)
    observe("warp/2160x2560", np.max(np.abs(got - want)) / np.ptp(frame), BARS["warp/2160x2560"])


# ---- Newton sub-pixel step of displacement maps
def test_newton_fourier_shift(observe):
    """The Fourier-shifted pair of tests/test_gpu_displacement.py: "newton" returns (0.3, -0.45) on the right axes."""
    from barc4dip_amd.signal import displacement_map

    n = 512
    i0 = synth.speckle_intensity(n, 5, pupil_div=4)
    ky, kx = np.fft.fftfreq(n)[:, None], np.fft.fftfreq(n)[None, :]
    sy, sx = 0.3, -0.45
    sh = np.real(np.fft.ifft2(np.fft.fft2(i0) * np.exp(-2j * np.pi * (ky * sy + kx * sx))))
    rng = np.random.default_rng(9)
    f0 = rng.poisson(i0).astype(np.float32)
    fr = rng.poisson(np.maximum(sh, 0)).astype(np.float32)
    r = displacement_map(f0, fr, window=31, step=16, search=4, subpixel="newton")
    mae = 0.5 * (np.mean(np.abs(r["dy"] - sy)) + np.mean(np.abs(r["dx"] - sx)))
    observe("newton/subpx_mae", mae, BARS["newton/subpx_mae"])


@pytest.mark.parametrize("backend", ["opencv", "skimage"])
def test_newton_parity_with_oracle(backend, observe):
    """The oracle map with the unswapped step: integer arg-max plus the y correction on dy and the x correction on dx."""
    from barc4dip_amd.signal import displacement_map

    f0 = synth.speckle_frame(256, 21)
    rng = np.random.default_rng(22)
    fr = (np.roll(f0, (3, -5), axis=(0, 1)) + rng.normal(size=f0.shape) * 20.0).astype(np.float32)
    kw = dict(window=31, step=16, search=8, backend=backend)
    got = displacement_map(f0, fr, subpixel="newton", **kw)
    wi, ws = oracle_map(f0, fr, subpixel=False, **kw), oracle_map(f0, fr, **kw)
    want_dy, want_dx = wi[0] + (ws[1] - wi[1]), wi[1] + (ws[0] - wi[0])     # swap the reference's two corrections back
    err = max(np.max(np.abs(got["dy"] - want_dy)), np.max(np.abs(got["dx"] - want_dx)))
    observe("newton/sub_px", err, BARS["newton/sub_px"])
    np.testing.assert_array_equal(got["peak"], displacement_map(f0, fr, **kw)["peak"])


# ---- round trip
def _ncc(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float(np.sum(a * b) / np.sqrt(np.sum(a * a) * np.sum(b * b)))


def test_round_trip_remove_distortion(di, observe):
    from barc4dip_amd.signal import displacement_map

    n = 512
    ref = synth.speckle_frame(n, 31, pupil_div=4).astype(np.float64)
    ty, tx = smooth_field((n, n), 2.5, seed=33, knots=4)             # D(p) = R(p + t(p))
    yy, xx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    dist = ndi.map_coordinates(ref, [yy + ty, xx + tx], order=3, mode="nearest").astype(np.float32)
    out, f = di.remove_distortion(ref.astype(np.float32), dist, window=31, step=16, search=6, return_field=True)
    # true field: d(p) = -t(p + d(p)), by fixed-point iteration at the window centres
    gy, gx = np.meshgrid(f["y"], f["x"], indexing="ij")
    dy, dx = np.zeros_like(gy), np.zeros_like(gx)
    for _ in range(30):
        c = [gy + dy, gx + dx]
        dy, dx = -ndi.map_coordinates(ty, c, order=1), -ndi.map_coordinates(tx, c, order=1)
    inner = (slice(1, -1), slice(1, -1))
    mae = 0.5 * (np.mean(np.abs(f["dy"][inner] - dy[inner])) + np.mean(np.abs(f["dx"][inner] - dx[inner])))
    observe("roundtrip/field_mae", mae, BARS["roundtrip/field_mae"])
    r2 = displacement_map(ref.astype(np.float32), out, window=31, step=16, search=6, subpixel="newton")
    res = 0.5 * (np.mean(np.abs(r2["dy"][inner])) + np.mean(np.abs(r2["dx"][inner])))
    observe("roundtrip/residual_mae", res, BARS["roundtrip/residual_mae"])
    m = slice(48, n - 48)
    assert _ncc(out[m, m], ref[m, m]) > _ncc(dist[m, m], ref[m, m]) + 0.05
