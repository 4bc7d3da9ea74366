"""CPU tier of the focal-spot prediction (barc4dip_amd/signal/focus.py): the float64 NumPy oracle that tests/test_gpu_focus.py
compares the device with, its self-checks, and the host side of the product (canvas choice, plane axes, the sampling check, every
argument error -- none of which touches the GPU).

The oracle follows the definition literally: the pupil A exp(i phi) of the valid nodes with phi in float64 from the issue's
formula, np.fft.fft2(U, s=(Py, Px)), fftshift, |.|^2 / (sum A)^2, then the statistics and the marginals by plain NumPy sums."""
from __future__ import annotations

import numpy as np
import pytest

# physical parameters shared with the GPU tests
LAM = 1.24e-10
H = 1.04e-4
RX, RY = 0.75002, 0.74998
Z0 = -0.75
COEFF = np.array([0.0, 1e-7, -2e-7, 1.0 / (2.0 * RX), 2e-6, 1.0 / (2.0 * RY)])


# ---- oracle
def node_axes(ny, nx, hy, hx):
    """(v (ny,), u (nx,)): metres from the grid centre, v along y and u along x."""
    return (np.arange(ny) - 0.5 * (ny - 1)) * hy, (np.arange(nx) - 0.5 * (nx - 1)) * hx


def analytic_phase(ny, nx, hy, hx, lam, z, c):
    """Polynomial plus chirp, float64 radians, (ny, nx)."""
    v, u = node_axes(ny, nx, hy, hx)
    u, v = u[None, :], v[:, None]
    return (2.0 * np.pi / lam) * (c[0] + c[1] * u + c[2] * v + c[3] * u * u + c[4] * u * v + c[5] * v * v) + (np.pi / (lam * z)) * (u * u + v * v)


def pupil(e, amp, c, hy, hx, lam, z, mask=None):
    """(U complex128 (ny, nx), A float64 with 0 outside the aperture)."""
    e = np.asarray(e, np.float64)
    ny, nx = e.shape
    A = np.ones((ny, nx)) if amp is None else np.asarray(amp, np.float64)
    valid = np.isfinite(e) & np.isfinite(A) & (A > 0)
    if mask is not None:
        valid &= np.asarray(mask) != 0
    A = np.where(valid, A, 0.0)
    phi = (2.0 * np.pi / lam) * np.where(valid, e, 0.0) + analytic_phase(ny, nx, hy, hx, lam, z, c)
    return A * np.exp(1j * phi), A


def plane(e, amp, c, hy, hx, lam, z, canvas, mask=None) -> dict:
    """Everything b4d_focal_spot returns for one (map, plane) pair, in float64."""
    Py, Px = canvas
    U, A = pupil(e, amp, c, hy, hx, lam, z, mask)
    sa, sa2 = float(A.sum()), float((A * A).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        I = np.abs(np.fft.fftshift(np.fft.fft2(U, s=(Py, Px)))) ** 2 / (sa * sa if sa > 0 else np.nan)
    p, q = (np.arange(Py) - Py // 2)[:, None], (np.arange(Px) - Px // 2)[None, :]
    out = {"I": I, "sum_a": sa, "sum_a2": sa2, "total": float(I.sum()), "marg_x": I.sum(axis=0), "marg_y": I.sum(axis=1),
           "moments": np.array([(I * p).sum(), (I * q).sum(), (I * p * p).sum(), (I * q * q).sum(), (I * p * q).sum()])}
    if sa > 0:
        k = int(np.argmax(I))                    # first index in row-major shifted order
        out["peak"], out["peak_index"] = float(I.flat[k]), (k // Px, k % Px)
    else:
        out["peak"], out["peak_index"] = np.nan, (-1, -1)
    return out


def centroid_sigma(total, m):
    """(cy, cx, sy, sx) in bins from the total and the five moments."""
    cy, cx = m[0] / total, m[1] / total
    return cy, cx, np.sqrt(max(m[2] / total - cy * cy, 0.0)), np.sqrt(max(m[3] / total - cx * cx, 0.0))


def smooth_error(shape, rms, seed):
    """A smooth map of the given rms (population, over the rectangle) with zero mean and no tilt."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    y, x = np.linspace(-1, 1, ny)[:, None], np.linspace(-1, 1, nx)[None, :]
    e = np.zeros(shape)
    for _ in range(6):
        fy, fx, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * np.pi)
        e += rng.normal() * np.cos(np.pi * (fy * y + fx * x) + ph)
    B = np.stack([np.ones(shape), np.broadcast_to(y, shape), np.broadcast_to(x, shape)], axis=-1).reshape(-1, 3)
    e = e - (B @ np.linalg.lstsq(B, e.reshape(-1), rcond=None)[0]).reshape(shape)
    return e * (rms / np.sqrt(np.mean(e * e)))


def disc_mask(shape, frac=0.95):
    ny, nx = shape
    y, x = np.linspace(-1, 1, ny)[:, None], np.linspace(-1, 1, nx)[None, :]
    return (y * y + x * x) <= frac * frac


def gaussian_amp(shape, width=0.8):
    ny, nx = shape
    y, x = np.linspace(-1, 1, ny)[:, None], np.linspace(-1, 1, nx)[None, :]
    return np.exp(-(y * y + x * x) / (2.0 * width * width)).astype(np.float32)


def case_maps(shape, T, seed=0):
    """(T, ny, nx) float32 figure errors of 0.05 lambda rms."""
    return np.stack([smooth_error(shape, 0.05 * LAM, seed + 17 * t) for t in range(T)]).astype(np.float32)


# ---- oracle self-checks
@pytest.mark.parametrize("shape,canvas", [((7, 5), (64, 64)), ((33, 47), (128, 128)), ((20, 30), (96, 160))])
def test_parseval(shape, canvas):
    e = case_maps(shape, 1)[0]
    amp = gaussian_amp(shape)
    for a in (None, amp):
        o = plane(e, a, COEFF, H, H, LAM, Z0 + 2e-5, canvas)
        want = canvas[0] * canvas[1] * o["sum_a2"] / o["sum_a"] ** 2
        assert abs(o["total"] - want) <= 1e-12 * want
        assert abs(o["marg_x"].sum() - want) <= 1e-12 * want and abs(o["marg_y"].sum() - want) <= 1e-12 * want


def test_in_focus_flat_pupil_has_unit_dc():
    R = 0.75
    c = np.array([0.0, 0.0, 0.0, 1.0 / (2 * R), 0.0, 1.0 / (2 * R)])
    for amp in (None, gaussian_amp((24, 31))):
        o = plane(np.zeros((24, 31)), amp, c, H, 1.3 * H, LAM, -R, (128, 128))
        assert abs(o["I"][64, 64] - 1.0) <= 1e-12
        assert o["peak_index"] == (64, 64) and abs(o["peak"] - 1.0) <= 1e-12


@pytest.mark.parametrize("m", [3, -5])
def test_tilt_moves_the_peak_by_whole_bins(m):
    """A tilt c1 = m lambda / (Px hx) moves the peak by exactly m bins TOWARDS GROWING COLUMN INDEX for m > 0 (c2 likewise along
    the rows): the phase 2 pi m j / Px meets exp(-2 pi i j k / Px) at k = +m.  With z < 0 the x axis descends, so a positive
    tilt coefficient lands at a negative plane coordinate."""
    R, Py, Px = 0.75, 96, 128
    c = np.array([0.0, m * LAM / (Px * H), -2 * m * LAM / (Py * H), 1.0 / (2 * R), 0.0, 1.0 / (2 * R)])
    o = plane(np.zeros((20, 26)), None, c, H, H, LAM, -R, (Py, Px))
    assert o["peak_index"] == (Py // 2 - 2 * m, Px // 2 + m)
    assert abs(o["peak"] - 1.0) <= 1e-9
    cy, cx, _, _ = centroid_sigma(o["total"], o["moments"])
    assert np.sign(cx) == np.sign(m) and np.sign(cy) == -np.sign(m)


def test_strehl_of_a_small_error_follows_marechal():
    R, sig = 0.75, 0.1
    c = np.array([0.0, 0.0, 0.0, 1.0 / (2 * R), 0.0, 1.0 / (2 * R)])
    for seed in range(4):
        e = smooth_error((40, 36), sig * LAM / (2 * np.pi), seed)
        o = plane(e, None, c, H, H, LAM, -R, (256, 256))
        assert abs(o["peak"] - np.exp(-sig * sig)) <= 2e-3


def test_pupil_position_and_mask():
    e = case_maps((12, 9), 1)[0]
    m = disc_mask((12, 9))
    e_nan = np.where(m, e, np.nan)
    a = plane(e_nan, None, COEFF, H, H, LAM, Z0, (64, 64))
    b = plane(e, None, COEFF, H, H, LAM, Z0, (64, 64), mask=m)
    assert np.array_equal(a["I"], b["I"]) and a["sum_a"] == float(m.sum())
    empty = plane(np.full((12, 9), np.nan), None, COEFF, H, H, LAM, Z0, (64, 64))
    assert np.isnan(empty["total"]) and np.isnan(empty["peak"]) and np.all(np.isnan(empty["I"]))


# ---- the product's host side
@pytest.fixture(scope="module")
def focus():
    from barc4dip_amd.signal import focus

    return focus


def test_exports():
    from barc4dip_amd import signal as gs

    for name in ("focal_spot", "focus_geometry", "beam_caustic"):
        assert name in gs.__all__ and callable(getattr(gs, name))


@pytest.mark.parametrize("shape,kw,want", [((7, 5), {}, (64, 64)), ((33, 47), {}, (256, 256)), ((48, 40), {}, (256, 256)),
                                           ((128, 128), {}, (512, 512)), ((128, 128), {"pad": 8}, (1024, 1024)),
                                           ((100, 300), {"pad": 2}, (256, 1024)), ((2000, 1500), {}, (4096, 4096)),
                                           ((20, 30), {"canvas": (96, 160)}, (96, 160)), ((33, 47), {"canvas": 128}, (128, 128))])
def test_canvas_choice(focus, shape, kw, want):
    g = focus.focus_geometry(shape, spacing=(H, H), wavelength=LAM, planes=Z0, coefficients=COEFF, **kw)
    assert g["canvas"] == want
    assert g["y"].shape == (1, want[0]) and g["x"].shape == (1, want[1]) and g["phase_step"].shape == (1, 1, 2)


def test_axes_and_sign_flip(focus):
    z = np.array([-0.75, 0.4])
    g = focus.focus_geometry((20, 30), spacing=(H, 2 * H), wavelength=LAM, planes=z, coefficients=COEFF, canvas=(96, 160))
    for k in range(2):
        dy, dx = LAM * z[k] / (96 * H), LAM * z[k] / (160 * 2 * H)
        np.testing.assert_allclose(g["y"][k], (np.arange(96) - 48) * dy, rtol=1e-15, atol=0)
        np.testing.assert_allclose(g["x"][k], (np.arange(160) - 80) * dx, rtol=1e-15, atol=0)
        np.testing.assert_allclose(g["pixel_size"][k], [abs(dy), abs(dx)], rtol=1e-15)
        assert g["y"][k][48] == 0.0 and g["x"][k][80] == 0.0
    assert np.all(np.diff(g["x"][0]) < 0) and np.all(np.diff(g["y"][0]) < 0)      # z < 0: the axes descend
    assert np.all(np.diff(g["x"][1]) > 0) and np.all(np.diff(g["y"][1]) > 0)
    np.testing.assert_array_equal(g["planes"], z)


@pytest.mark.parametrize("shape", [(7, 5), (33, 47), (48, 40), (1, 9), (6, 1)])
def test_phase_step_against_brute_force(focus, shape):
    ny, nx = shape
    rng = np.random.default_rng(3)
    cs = np.stack([COEFF, COEFF * np.array([1, -3, 2, 1.0001, -40, 0.9998]), rng.normal(size=6) * np.array([1e-9, 1e-7, 1e-7, 0.6, 1e-5, 0.7])])
    z = np.array([Z0, Z0 + 5e-5, 0.9, -2.0])
    g = focus.focus_geometry(shape, spacing=(H, 1.5 * H), wavelength=LAM, planes=z, coefficients=cs)
    for t in range(3):
        for k in range(4):
            phi = analytic_phase(ny, nx, H, 1.5 * H, LAM, z[k], cs[t])
            by = np.max(np.abs(np.diff(phi, axis=0))) if ny > 1 else 0.0
            bx = np.max(np.abs(np.diff(phi, axis=1))) if nx > 1 else 0.0
            # the brute-force differences of phases of 1e6 rad carry their own rounding: 1e-9 rad absolute
            assert abs(g["phase_step"][t, k, 0] - by) <= 1e-9 + 1e-9 * by
            assert abs(g["phase_step"][t, k, 1] - bx) <= 1e-9 + 1e-9 * bx


def test_the_gpu_cases_are_sampled(focus):
    """The physical parameters of tests/test_gpu_focus.py keep the analytic phase below pi per node at the planes they use."""
    for shape, deltas in (((7, 5), [0.0, 5e-5]), ((33, 47), [-2e-5, 2e-5]), ((48, 40), np.linspace(-5e-5, 5e-5, 5)), ((128, 128), [0.0]),
                          ((20, 30), [3e-5])):
        g = focus.focus_geometry(shape, spacing=(H, H), wavelength=LAM, planes=Z0 + np.asarray(deltas), coefficients=COEFF)
        assert np.max(g["phase_step"]) < np.pi
    g = focus.focus_geometry((128, 128), spacing=(H, H), wavelength=LAM, planes=Z0 + 1e-4, coefficients=COEFF)
    assert np.max(g["phase_step"]) > np.pi


def test_default_plane_is_the_mean_focus(focus):
    g = focus.focus_geometry((8, 8), spacing=(H, H), wavelength=LAM, planes=None, coefficients=COEFF)
    assert g["planes"].shape == (1,) and abs(g["planes"][0] + 0.5 * (RX + RY)) <= 1e-15
    flat = COEFF.copy()
    flat[3] = 0.0
    with pytest.raises(ValueError, match="not finite"):
        focus.focus_geometry((8, 8), spacing=(H, H), wavelength=LAM, planes=None, coefficients=flat)


GEO = dict(spacing=(H, H), wavelength=LAM, planes=Z0, coefficients=COEFF)


@pytest.mark.parametrize("kw", [{"planes": 0.0}, {"planes": [Z0, 0.0]}, {"planes": np.nan}, {"planes": [np.inf]}, {"planes": []},
                                {"planes": [[Z0]]}, {"planes": "far"}, {"wavelength": 0.0}, {"wavelength": -1e-10},
                                {"wavelength": np.nan}, {"spacing": (H, 0.0)}, {"spacing": H}, {"spacing": (H, np.inf)},
                                {"coefficients": np.zeros(5)}, {"coefficients": np.zeros((2, 3, 6))}, {"coefficients": [np.nan] * 6},
                                {"pad": 0}, {"pad": 2.5}, {"canvas": 128.0}, {"canvas": (128, 128, 128)}])
def test_geometry_value_errors(focus, kw):
    with pytest.raises(ValueError):
        focus.focus_geometry((33, 47), **{**GEO, **kw})


@pytest.mark.parametrize("shape", [(0, 5), (5,), "ab"])
def test_geometry_bad_shape(focus, shape):
    with pytest.raises(ValueError):
        focus.focus_geometry(shape, **GEO)


@pytest.mark.parametrize("shape,kw", [((33, 47), {"canvas": 32}), ((33, 47), {"canvas": (64, 40)}), ((33, 47), {"canvas": 8192}),
                                      ((5000, 40), {}), ((100, 100), {"canvas": (64, 128)})])
def test_geometry_size_errors(focus, shape, kw):
    from barc4dip_amd._ffi import B4DSizeError

    with pytest.raises(B4DSizeError):
        focus.focus_geometry(shape, **{**GEO, **kw})


def _dict_input(shape=(12, 9), remove="quadratic"):
    d = {"wavefront": case_maps(shape, 1)[0], "coefficients": COEFF[None], "y": 16.0 * np.arange(shape[0]), "x": 16.0 * np.arange(shape[1])}
    if remove is not None:
        d["remove"] = remove
    return d


def test_focal_spot_argument_errors_need_no_gpu(focus):
    e = case_maps((12, 9), 1)[0]
    kw = dict(wavelength=LAM, spacing=(H, H), coefficients=COEFF, planes=Z0)
    with pytest.raises(ValueError, match="spacing"):
        focus.focal_spot(e, wavelength=LAM, coefficients=COEFF, planes=Z0)
    with pytest.raises(ValueError, match="coefficients"):
        focus.focal_spot(e, wavelength=LAM, spacing=(H, H), planes=Z0)
    with pytest.raises(ValueError, match="ny, nx"):
        focus.focal_spot(e[0], **kw)
    with pytest.raises(ValueError, match="coefficient sets"):
        focus.focal_spot(np.stack([e, e, e]), **{**kw, "coefficients": np.stack([COEFF, COEFF])})
    with pytest.raises(ValueError, match="crop"):
        focus.focal_spot(e, crop=(65, 8), **kw)
    with pytest.raises(ValueError, match="crop"):
        focus.focal_spot(e, crop=0, **kw)
    with pytest.raises(ValueError, match="chunk"):
        focus.focal_spot(e, chunk=0, **kw)
    with pytest.raises(ValueError, match="non-zero"):
        focus.focal_spot(e, **{**kw, "planes": [Z0, 0.0]})
    with pytest.raises(ValueError, match="must have the shape"):
        focus.focal_spot(e, amplitude=np.ones((3, 3)), **kw)
    # a dict that does not say remove="quadratic" cannot be used without explicit coefficients
    for d in (_dict_input(remove="tilt"), _dict_input(remove=None)):
        with pytest.raises(ValueError, match="quadratic"):
            focus.focal_spot(d, wavelength=LAM, pixel_size=6.5e-6, planes=Z0)
    with pytest.raises(ValueError, match="pixel_size"):
        focus.focal_spot(_dict_input(), wavelength=LAM, planes=Z0)
    with pytest.raises(ValueError, match="wavefront"):
        focus.focal_spot({"coefficients": COEFF}, wavelength=LAM, pixel_size=6.5e-6, planes=Z0)


def test_undersampled_planes_are_refused_before_the_gpu(focus):
    e = case_maps((128, 128), 1)[0]
    with pytest.raises(ValueError, match="undersampled"):
        focus.focal_spot(e, wavelength=LAM, spacing=(H, H), coefficients=COEFF, planes=Z0 + 1e-4)
    with pytest.raises(ValueError, match="undersampled"):
        focus.beam_caustic(e, span=1e-3, n_planes=5, wavelength=LAM, spacing=(H, H), coefficients=COEFF)


def test_without_a_gpu_there_is_no_fallback(focus):
    import torch

    from barc4dip_amd._ffi import B4DUnavailable

    if torch.cuda.is_available():
        return      # the GPU tier covers the device
    with pytest.raises(B4DUnavailable):
        focus.focal_spot(case_maps((12, 9), 1)[0], wavelength=LAM, spacing=(H, H), coefficients=COEFF, planes=Z0)


@pytest.mark.parametrize("kw", [{"span": -1.0}, {"span": np.nan}, {"n_planes": 0}, {"n_planes": 2.0}, {"planes": [Z0]},
                                {"z_focus": np.inf}])
def test_caustic_argument_errors(focus, kw):
    args = dict(span=1e-4, n_planes=3, wavelength=LAM, spacing=(H, H), coefficients=COEFF)
    with pytest.raises(ValueError):
        focus.beam_caustic(case_maps((12, 9), 1)[0], **{**args, **kw})


def test_header_and_bindings_agree():
    import os

    from barc4dip_amd import _ffi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "b4d.h")).read()
    for name in ("b4d_focal_spot", "b4d_focal_spot_workspace_bytes"):
        assert name + "(" in text and name in _ffi.SIGNATURES
    assert len(_ffi.SIGNATURES["b4d_focal_spot"][1]) == 21
