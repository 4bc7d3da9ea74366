"""Wavefront reconstruction on the MI355X (b4d_integrate_gradient / b4d_poly2_fit, barc4dip_amd/signal/wavefront.py) against the
float64 oracle of tests/test_wavefront_host.py.  Errors are max|got - ref| / ptp(ref) per map.

Bars: 2 x the maximum observed on an MI355X.  Next to its bar every parity case is held against
what the same four products give in float32 NumPy (integrate_mm32) on the same input: more than 4 x that is a bug, not a
tolerance.  The error follows the conditioning of the grid: (130, 2048) with the larger spacing along the long axis is
1.8e-4 in float32 NumPy as well."""
from __future__ import annotations

import numpy as np
import pytest

from barc4dip_amd import synth
from test_wavefront_host import (MONOMIALS, integrate_mm32, integrate_np, smooth_slopes, wavefront_np, white_slopes)

pytestmark = pytest.mark.gpu

HY, HX = 0.7, 1.9
SHAPES = [(1, 5), (5, 1), (2, 2), (2, 3), (7, 9), (33, 65), (64, 64), (37, 53), (126, 126), (300, 517), (2048, 130), (130, 2048)]
BARS = {    # 2 x the observed maximum on MI355X
    "wavefront/smooth_1x5": 1.8e-07, "wavefront/white_1x5": 2.6e-07,
    "wavefront/smooth_5x1": 1.3e-07, "wavefront/white_5x1": 5.2e-08,
    "wavefront/smooth_2x2": 4.6e-07, "wavefront/white_2x2": 2.2e-07,
    "wavefront/smooth_2x3": 3.1e-07, "wavefront/white_2x3": 8.8e-08,
    "wavefront/smooth_7x9": 9.1e-07, "wavefront/white_7x9": 5.9e-07,
    "wavefront/smooth_33x65": 1.1e-06, "wavefront/white_33x65": 1.5e-06,
    "wavefront/smooth_64x64": 5.5e-07, "wavefront/white_64x64": 1.1e-06,
    "wavefront/smooth_37x53": 2.1e-06, "wavefront/white_37x53": 3.2e-06,
    "wavefront/smooth_126x126": 1.6e-06, "wavefront/white_126x126": 1.8e-06,
    "wavefront/smooth_300x517": 4.3e-06, "wavefront/white_300x517": 1.4e-05,
    "wavefront/smooth_2048x130": 4.3e-06, "wavefront/white_2048x130": 2.2e-05,
    "wavefront/smooth_130x2048": 0.00011, "wavefront/white_130x2048": 0.00041,
    "wavefront/mean": 4.9e-08, "wavefront/transposed": 1.5e-06, "wavefront/spacing_2.5_0.4": 6.3e-07,
    "wavefront/fit_coefficients": 1.4e-07, "wavefront/fit_radius": 3.9e-07, "wavefront/fit_rms": 5.6e-07, "wavefront/fit_map": 6.9e-06,
    "wavefront/fit_phase": 6.9e-06,
    # condition on every parity bar: error <= 4 x integrate_mm32's on the same input (floor: 4 float32 roundings
    # of the range, 4 x 2^-24, where the yardstick happens to be exact)
    "wavefront/vs_mm32": 4.0,
}
MM32_FLOOR = 4.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def wf():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import wavefront

    return wavefront


def _err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.ptp(ref))


def _slopes(kind, shape, seed):
    gy, gx = smooth_slopes(shape, HY, HX, seed) if kind == "smooth" else white_slopes(shape, seed)
    return gy.astype(np.float32), gx.astype(np.float32)      # what the device receives


# ---- parity
@pytest.mark.parametrize("kind", ["smooth", "white"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_with_oracle(wf, shape, kind, observe):
    T = 3 if shape == (7, 9) else 1       # (7, 9): different data per map, so that a wrong batch stride shows
    maps = [_slopes(kind, shape, seed=11 + t) for t in range(T)]
    gy, gx = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    got = wf.integrate_gradient(gy, gx, dy=HY, dx=HX)
    assert got.dtype == np.float64 and got.shape == (T,) + shape
    key = f"wavefront/{kind}_{shape[0]}x{shape[1]}"
    for t in range(T):
        ref = integrate_np(gy[t], gx[t], HY, HX)
        e, e32 = _err(got[t], ref), _err(integrate_mm32(gy[t], gx[t], HY, HX), ref)
        print(f"{key}[{t}]: error {e:.3e}, integrate_mm32 {e32:.3e}, |mean| {abs(got[t].mean()) / np.ptp(ref):.3e}")
        observe("wavefront/vs_mm32", e / max(e32, MM32_FLOOR), BARS["wavefront/vs_mm32"])
        observe(key, e, BARS[key])
        observe("wavefront/mean", abs(got[t].mean()) / np.ptp(ref), BARS["wavefront/mean"])


def test_unequal_spacings_transpose(wf, observe):
    """Swapping the axes together with their slopes and spacings transposes the result."""
    gy, gx = _slopes("smooth", (37, 53), seed=5)
    a = wf.integrate_gradient(gy, gx, dy=2.5, dx=0.4)
    b = wf.integrate_gradient(gx.T, gy.T, dy=0.4, dx=2.5)
    ref = integrate_np(gy, gx, 2.5, 0.4)
    print(f"wavefront/transposed: {_err(b.T, a):.3e}; against the oracle {_err(a, ref):.3e}")
    observe("wavefront/transposed", _err(b.T, a), BARS["wavefront/transposed"])
    observe("wavefront/spacing_2.5_0.4", _err(a, ref), BARS["wavefront/spacing_2.5_0.4"])
    c = wf.integrate_gradient(gy, gx, dy=0.4, dx=2.5)       # the spacings matter: the other assignment is another surface
    assert _err(c, ref) > 1e-2


# ---- exact and structural properties
def test_batch_single_and_2d_calls_agree_bitwise(wf):
    maps = [_slopes("white", (33, 65), seed=21 + t) for t in range(3)]
    gy, gx = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    full = wf.integrate_gradient(gy, gx, dy=HY, dx=HX)
    for t in range(3):
        one = wf.integrate_gradient(gy[t:t + 1], gx[t:t + 1], dy=HY, dx=HX)
        two = wf.integrate_gradient(gy[t], gx[t], dy=HY, dx=HX)
        assert one.shape == (1, 33, 65) and two.shape == (33, 65)
        np.testing.assert_array_equal(one[0], full[t])
        np.testing.assert_array_equal(two, full[t])
    assert not np.array_equal(full[0], full[1])


def test_input_dtypes_agree(wf):
    rng = np.random.default_rng(31)
    gy, gx = rng.integers(0, 65536, (2, 37, 53)).astype(np.uint16), rng.integers(0, 65536, (2, 37, 53)).astype(np.uint16)
    want = wf.integrate_gradient(gy, gx, dy=HY, dx=HX)
    assert np.all(np.isfinite(want)) and np.ptp(want) > 0
    for dt in (np.float32, np.float64, np.int32):
        np.testing.assert_array_equal(wf.integrate_gradient(gy.astype(dt), gx.astype(dt), dy=HY, dx=HX), want)


def test_input_layouts_agree(wf):
    import torch

    rng = np.random.default_rng(32)
    big = rng.normal(size=(2, 4, 74, 159)).astype(np.float32)
    gy, gx = big[0, ::2, ::2, ::3], big[1, ::2, ::2, ::3]            # strided views, (2, 37, 53)
    assert not gy.flags.c_contiguous
    want = wf.integrate_gradient(np.ascontiguousarray(gy), np.ascontiguousarray(gx), dy=HY, dx=HX)
    np.testing.assert_array_equal(wf.integrate_gradient(gy, gx, dy=HY, dx=HX), want)
    swapped = (gy.astype(gy.dtype.newbyteorder()), gx.astype(gx.dtype.newbyteorder()))
    assert not swapped[0].dtype.isnative
    np.testing.assert_array_equal(wf.integrate_gradient(*swapped, dy=HY, dx=HX), want)
    np.testing.assert_array_equal(wf.integrate_gradient(np.asfortranarray(gy), np.asfortranarray(gx), dy=HY, dx=HX), want)
    ty, tx = torch.from_numpy(big[0]).cuda()[::2, ::2, ::3], torch.from_numpy(big[1]).cuda()[::2, ::2, ::3]
    out = wf.integrate_gradient(ty, tx, dy=HY, dx=HX, return_tensors=True)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (2, 37, 53)
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), want)


def test_non_finite_input_propagates(wf):
    gy, gx = _slopes("smooth", (7, 9), seed=3)
    gy = np.stack([gy, gy])
    gx = np.stack([gx, gx])
    gy[1, 3, 4] = np.nan
    out = wf.integrate_gradient(gy, gx)
    assert np.all(np.isfinite(out[0])) and np.any(np.isnan(out[1]))


# ---- wavefront_from_displacement against the oracle chain
def _grid_field(T, seed):
    """Shift maps (px) on (29, 31) window centres, step 16: defocus + astigmatism + a bump + noise, (T, 29, 31) or (29, 31)."""
    rng = np.random.default_rng(seed)
    y, x = 23.0 + 16.0 * np.arange(29), 23.0 + 16.0 * np.arange(31)
    yy, xx = np.meshgrid(y - y.mean(), x - x.mean(), indexing="ij")
    dys, dxs = [], []
    for _ in range(T or 1):
        a, b, c = rng.uniform(4e-3, 8e-3), rng.uniform(-3e-3, 3e-3), rng.uniform(-2e-3, 2e-3)
        ty, tx = rng.uniform(-0.5, 0.5, 2)
        bump = 40.0 * np.exp(-((yy - 30) ** 2 + (xx + 50) ** 2) / (2 * 90.0 ** 2))
        dys.append((a + b) * yy + c * xx + ty - bump * (yy - 30) / 90.0 ** 2 + 0.02 * rng.normal(size=yy.shape))
        dxs.append((a - b) * xx + c * yy + tx - bump * (xx + 50) / 90.0 ** 2 + 0.02 * rng.normal(size=yy.shape))
    dy, dx = np.array(dys, np.float32), np.array(dxs, np.float32)
    if T is None:
        dy, dx = dy[0], dx[0]
    return {"dy": dy, "dx": dx, "y": y, "x": x}


@pytest.fixture(scope="module")
def fit_cases():
    """(field, oracle with remove=None) for a shared 2-D field and a per-frame T = 2 field; the oracle is computed once."""
    kw = dict(pixel_size=6.5e-6, distance=0.75, wavelength=1.24e-10)
    out = []
    for T, seed in ((None, 41), (2, 42)):
        f = _grid_field(T, seed)
        dy, dx = (f["dy"][None], f["dx"][None]) if T is None else (f["dy"], f["dx"])
        out.append((f, dy, dx, kw, {r: wavefront_np(dy, dx, f["y"], f["x"], remove=r, **kw) for r in (None, "tilt", "quadratic")}))
    return out


@pytest.mark.parametrize("remove", [None, "tilt", "quadratic"])
def test_wavefront_from_displacement_parity(wf, fit_cases, remove, observe):
    for f, dy, dx, kw, oracles in fit_cases:
        ref, full = oracles[remove], oracles[None]
        got = wf.wavefront_from_displacement(f, remove=remove, **kw)
        T = dy.shape[0]
        assert got["wavefront"].shape == f["dy"].shape and got["wavefront"].dtype == np.float64
        assert got["coefficients"].shape == (T, 6) and got["rms"].shape == (T,) and got["radius_x"].shape == (T,)
        np.testing.assert_array_equal(got["y"], f["y"])
        np.testing.assert_array_equal(got["x"], f["x"])
        w, ph = got["wavefront"].reshape(dy.shape), got["phase"].reshape(dy.shape)
        ax, ay = 0.5 * np.ptp(f["x"]) * kw["pixel_size"], 0.5 * np.ptp(f["y"]) * kw["pixel_size"]
        height = np.array([ax ** pu * ay ** pv for pu, pv in MONOMIALS])      # a coefficient as a height at the aperture edge
        for t in range(T):
            span = np.ptp(full["wavefront"][t])
            figs = {
                "fit_coefficients": np.max(np.abs(got["coefficients"][t] - ref["coefficients"][t]) * height) / span,
                "fit_radius": max(abs(got["radius_x"][t] / ref["radius_x"][t] - 1.0), abs(got["radius_y"][t] / ref["radius_y"][t] - 1.0)),
                "fit_rms": abs(got["rms"][t] / ref["rms"][t] - 1.0),
                "fit_map": _err(w[t], ref["wavefront"][t]),
                "fit_phase": _err(ph[t], ref["phase"][t]),
            }
            print(f"remove={remove} T={T} t={t}: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
            for k, v in figs.items():
                observe("wavefront/" + k, v, BARS["wavefront/" + k])
            assert abs(np.std(w[t]) / got["rms"][t] - 1.0) < 1e-6        # rms is the ddof-0 deviation of what is returned


def test_wavefront_tensors_and_dense_pair(wf, fit_cases):
    import torch

    f, dy, dx, kw, _ = fit_cases[1]
    want = wf.wavefront_from_displacement(f, remove="tilt", **kw)
    ft = dict(f, dy=torch.from_numpy(f["dy"]).cuda(), dx=torch.from_numpy(f["dx"]).cuda())
    got = wf.wavefront_from_displacement(ft, remove="tilt", return_tensors=True, **kw)
    for k in ("wavefront", "phase"):
        assert isinstance(got[k], torch.Tensor) and got[k].is_cuda and got[k].dtype == torch.float32
        np.testing.assert_array_equal(got[k].cpu().numpy().astype(np.float64), want[k])
    np.testing.assert_array_equal(got["coefficients"], want["coefficients"])
    # a dense pair is the same grid with a step of one pixel and no wavelength: no phase
    dense = wf.wavefront_from_displacement((f["dy"], f["dx"]), pixel_size=kw["pixel_size"], distance=kw["distance"], remove="tilt")
    assert "phase" not in dense
    np.testing.assert_array_equal(dense["y"], np.arange(29.0))
    unit = wf.wavefront_from_displacement(dict(f, y=np.arange(29.0), x=np.arange(31.0)), remove="tilt", **kw)
    np.testing.assert_array_equal(dense["wavefront"], unit["wavefront"])
    np.testing.assert_array_equal(dense["coefficients"], unit["coefficients"])


# ---- end to end
def test_end_to_end_curvature_512(wf, observe):
    """A speckle frame warped by an analytic defocus + astigmatism field of +-3 px, measured by displacement_map and integrated:
    the curvature terms are no further from the truth than the float64 oracle chain on the same measured map, plus the parity bar."""
    from barc4dip_amd.preprocessing import correct_distortion
    from barc4dip_amd.signal import displacement_map

    n, p, L = 512, 6.5e-6, 0.75
    ref = synth.speckle_frame(n, 51, pupil_div=4)
    a, b, c = 6e-3, 3e-3, 2e-3
    A = np.array([[a + b, c], [c, a - b]])                       # t(q) = A q, q = (y, x) - centre
    q = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    ty = A[0, 0] * q[:, None] + A[0, 1] * q[None, :]
    tx = A[1, 0] * q[:, None] + A[1, 1] * q[None, :]
    assert 2.5 < max(np.max(np.abs(ty)), np.max(np.abs(tx))) <= 3.0
    dist = correct_distortion(ref, (ty, tx), order=3)            # dist(p) = ref(p + t(p))
    m = displacement_map(ref, dist, window=31, step=16, search=8, subpixel="newton")
    # the measured shift solves d = -t(p + d): d = B q with B = -(I + A)^-1 A, and W = q_m^T B q_m / (2 L)
    B = -np.linalg.solve(np.eye(2) + A, A)
    truth = np.array([B[1, 1] / (2 * L), B[0, 1] / L, B[0, 0] / (2 * L)])      # c3 (u^2), c4 (uv), c5 (v^2)
    # (the fit is taken about the grid centre, half a pixel from the frame centre: second-order coefficients do not depend on it)
    got = wf.wavefront_from_displacement(m, pixel_size=p, distance=L, remove=None)
    orc = wavefront_np(m["dy"].astype(np.float32)[None], m["dx"].astype(np.float32)[None], m["y"], m["x"], pixel_size=p,
                       distance=L, remove=None)
    scale = np.max(np.abs(truth))
    e_gpu = np.abs(got["coefficients"][0, 3:] - truth) / scale
    e_orc = np.abs(orc["coefficients"][0, 3:] - truth) / scale
    ax, ay = 0.5 * np.ptp(m["x"]) * p, 0.5 * np.ptp(m["y"]) * p
    height = np.array([ax * ax, ax * ay, ay * ay])
    parity = BARS["wavefront/fit_coefficients"] * np.ptp(orc["wavefront"][0]) / (height * scale)
    print(f"end to end: truth error of the oracle chain {e_orc}, of the device {e_gpu}, parity allowance {parity}; "
          f"radius_x {got['radius_x'][0]:.6g} m against {1 / (2 * truth[0]):.6g}")
    assert np.all(e_gpu <= e_orc + parity), (e_gpu, e_orc, parity)
