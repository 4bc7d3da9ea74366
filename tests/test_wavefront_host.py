"""CPU tier of the wavefront reconstruction (barc4dip_amd/signal/wavefront.py): the float64 oracle that the GPU tests compare
against, checked here against a dense least-squares solution of the edge equations and against analytic cases, and the argument
checks of the public functions, which are raised before any device is needed."""
from __future__ import annotations

import numpy as np
import pytest
from scipy import fft as sfft

MONOMIALS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))      # powers (of u along x, of v along y) of (1, u, v, u^2, uv, v^2)
REMOVE = {None: (), "tilt": (0, 1, 2), "quadratic": (0, 1, 2, 3, 4, 5)}


# ---- oracle
def edge_means(gy, gx):
    """Southwell edge slopes: the mean of the two node slopes, (ny-1, nx) along y and (ny, nx-1) along x."""
    return 0.5 * (gy[:-1, :] + gy[1:, :]), 0.5 * (gx[:, :-1] + gx[:, 1:])


def rhs_np(gy, gx, hy, hx):
    ey, ex = edge_means(np.asarray(gy, np.float64), np.asarray(gx, np.float64))
    r = np.zeros(np.shape(gy), np.float64)
    r[1:, :] += ey / hy
    r[:-1, :] -= ey / hy
    r[:, 1:] += ex / hx
    r[:, :-1] -= ex / hx
    return r


def eigenvalues_np(ny, nx, hy, hx):
    ly = 4.0 * np.sin(np.pi * np.arange(ny) / (2.0 * ny)) ** 2 / hy ** 2
    lx = 4.0 * np.sin(np.pi * np.arange(nx) / (2.0 * nx)) ** 2 / hx ** 2
    return ly[:, None] + lx[None, :]


def integrate_np(gy, gx, hy=1.0, hx=1.0):
    """float64 least-squares integral of one (ny, nx) slope pair: zero-mean minimiser of the squared edge residuals."""
    r = rhs_np(gy, gx, hy, hx)
    lam = eigenvalues_np(*r.shape, hy, hx)
    lam[0, 0] = 1.0
    p = sfft.dctn(r, type=2, norm="ortho") / lam
    p[0, 0] = 0.0
    return sfft.idctn(p, type=2, norm="ortho")


def dct_basis(n):
    """Orthonormal DCT-II matrix C[k, j] = s_k sqrt(2/n) cos(pi (2j+1) k / 2n), float64."""
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    c = np.sqrt(2.0 / n) * np.cos(np.pi * (2 * j + 1) * k / (2.0 * n))
    c[0] /= np.sqrt(2.0)
    return c


def integrate_mm32(gy, gx, hy=1.0, hx=1.0):
    """The same solution as four float32 matrix products (basis and eigenvalues rounded from float64): the yardstick for what
    float32 arithmetic can deliver."""
    r = rhs_np(gy, gx, hy, hx).astype(np.float32)
    ny, nx = r.shape
    cy, cx = dct_basis(ny).astype(np.float32), dct_basis(nx).astype(np.float32)
    lam = eigenvalues_np(ny, nx, hy, hx)
    lam[0, 0] = 1.0
    p = (cy @ (r @ cx.T)) / lam.astype(np.float32)
    p[0, 0] = 0.0
    return (cy.T @ (p @ cx)).astype(np.float64)


def integrate_lstsq(gy, gx, hy, hx):
    """Dense solution of the edge equations with one zero-mean row."""
    ny, nx = gy.shape
    ey, ex = edge_means(np.asarray(gy, np.float64), np.asarray(gx, np.float64))
    idx = np.arange(ny * nx).reshape(ny, nx)
    rows, rhs = [], []
    for i in range(ny - 1):
        for j in range(nx):
            a = np.zeros(ny * nx)
            a[idx[i + 1, j]], a[idx[i, j]] = 1.0 / hy, -1.0 / hy
            rows.append(a)
            rhs.append(ey[i, j])
    for i in range(ny):
        for j in range(nx - 1):
            a = np.zeros(ny * nx)
            a[idx[i, j + 1]], a[idx[i, j]] = 1.0 / hx, -1.0 / hx
            rows.append(a)
            rhs.append(ex[i, j])
    rows.append(np.ones(ny * nx))
    rhs.append(0.0)
    sol = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
    return sol.reshape(ny, nx)


def poly2_fit_np(w, y_m, x_m):
    """Least-squares coefficients of (1, u, v, u^2, uv, v^2) on one map w (ny, nx); u = x_m - mean(x_m), v = y_m - mean(y_m).
    Returns (coefficients (6,), design matrix (ny nx, 6))."""
    u, v = np.meshgrid(x_m - np.mean(x_m), y_m - np.mean(y_m))
    a = np.stack([(u ** pu * v ** pv).ravel() for pu, pv in MONOMIALS], axis=1)
    norm = np.sqrt(np.sum(a * a, axis=0))      # column scaling: metres, metres^2 ... differ by many orders of magnitude
    c = np.linalg.lstsq(a / norm, np.ravel(w), rcond=None)[0] / norm
    return c, a


def wavefront_np(dy, dx, y, x, *, pixel_size, distance, wavelength=None, remove="tilt"):
    """Oracle chain of wavefront_from_displacement for (T, ny, nx) shift maps (pixels) on the axes y, x (pixels)."""
    dy, dx = np.asarray(dy, np.float64), np.asarray(dx, np.float64)
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    sy = (y[-1] - y[0]) / (len(y) - 1) if len(y) > 1 else 1.0
    sx = (x[-1] - x[0]) / (len(x) - 1) if len(x) > 1 else 1.0
    out = {"wavefront": [], "coefficients": [], "rms": []}
    for t in range(dy.shape[0]):
        w = integrate_np(dy[t] * pixel_size / distance, dx[t] * pixel_size / distance, sy * pixel_size, sx * pixel_size)
        c, a = poly2_fit_np(w, y * pixel_size, x * pixel_size)
        sel = list(REMOVE[remove])
        w = w - (a[:, sel] @ c[sel]).reshape(w.shape)
        out["wavefront"].append(w)
        out["coefficients"].append(c)
        out["rms"].append(np.std(w))
    out = {k: np.array(v) for k, v in out.items()}
    c = out["coefficients"]
    with np.errstate(divide="ignore"):
        out["radius_x"], out["radius_y"] = 1.0 / (2.0 * c[:, 3]), 1.0 / (2.0 * c[:, 5])
    if wavelength is not None:
        out["phase"] = 2.0 * np.pi * out["wavefront"] / wavelength
    return out


# ---- inputs shared with the GPU tests
def smooth_slopes(shape, hy, hx, seed, noise=0.025):
    """Analytic gradient of a smooth field (a few waves and a bowl) on the nodes, plus `noise` (fraction of the slope rms) of
    white noise.  Returns (gy, gx) float64."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(ny) * hy, np.arange(nx) * hx, indexing="ij")
    ly, lx = max(ny - 1, 1) * hy, max(nx - 1, 1) * hx
    gy, gx = 0.8 * (y / ly - 0.4) / ly, -0.5 * (x / lx - 0.55) / lx
    for _ in range(4):
        ky, kx, ph, am = rng.uniform(0.5, 3.0) * np.pi / ly, rng.uniform(0.5, 3.0) * np.pi / lx, rng.uniform(0, 6.28), rng.uniform(0.2, 1)
        gy = gy + am * ky * np.cos(ky * y + kx * x + ph)
        gx = gx + am * kx * np.cos(ky * y + kx * x + ph)
    s = np.sqrt(0.5 * (np.mean(gy ** 2) + np.mean(gx ** 2)))
    return gy + noise * s * rng.normal(size=shape), gx + noise * s * rng.normal(size=shape)


def white_slopes(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=shape), rng.normal(size=shape)


# ---- the oracle against independent statements
@pytest.mark.parametrize("shape", [(2, 2), (2, 9), (7, 9), (12, 5), (1, 5), (5, 1)])
def test_oracle_equals_dense_least_squares(shape):
    hy, hx = 0.7, 1.9
    for gy, gx in (white_slopes(shape, 3), smooth_slopes(shape, hy, hx, 4)):
        want = integrate_lstsq(gy, gx, hy, hx)
        got = integrate_np(gy, gx, hy, hx)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.ptp(want)
        assert abs(got.mean()) <= 1e-12 * np.ptp(want)


@pytest.mark.parametrize("shape", [(7, 9), (37, 53), (126, 126)])
def test_oracle_is_exact_on_a_quadratic(shape):
    hy, hx = 1.3, 0.6
    y, x = np.meshgrid(np.arange(shape[0]) * hy, np.arange(shape[1]) * hx, indexing="ij")
    a, b, c, d, e = 0.3, -0.2, 0.15, 1.1, -0.7
    phi = a * x * x + b * y * y + c * x * y + d * x + e * y
    got = integrate_np(2 * b * y + c * x + e, 2 * a * x + c * y + d, hy, hx)     # the edge mean is exact for linear slopes
    assert np.max(np.abs(got - (phi - phi.mean()))) <= 1e-12 * np.ptp(phi)


def test_oracle_constant_slopes_give_a_plane():
    ny, nx, hy, hx = 6, 11, 2.0, 0.5
    got = integrate_np(np.full((ny, nx), 0.25), np.full((ny, nx), -1.5), hy, hx)
    np.testing.assert_allclose(np.diff(got, axis=0), 0.25 * hy, rtol=0, atol=1e-13)
    np.testing.assert_allclose(np.diff(got, axis=1), -1.5 * hx, rtol=0, atol=1e-13)


def test_float32_yardstick_tracks_the_oracle():
    """integrate_mm32 at (37, 53) deviates by a few 1e-7 (smooth) to 1.4e-6 (white noise) of the range."""
    for (gy, gx), bar in ((smooth_slopes((37, 53), 0.7, 1.9, 1), 1e-6), (white_slopes((37, 53), 2), 3e-6)):
        ref = integrate_np(gy, gx, 0.7, 1.9)
        assert np.max(np.abs(integrate_mm32(gy, gx, 0.7, 1.9) - ref)) <= bar * np.ptp(ref)


def test_oracle_physical_scaling_and_radius():
    """A pure defocus d = kappa (x - x0) px is the wavefront x_m^2 kappa / (2 distance): radius = distance / kappa."""
    p, L, kappa, ky = 6.5e-6, 0.8, 2e-3, -5e-4
    y, x = 20.0 + 16.0 * np.arange(29), 24.0 + 16.0 * np.arange(31)
    dy = np.broadcast_to((ky * (y - y.mean()))[:, None], (29, 31))[None]
    dx = np.broadcast_to((kappa * (x - x.mean()))[None, :], (29, 31))[None]
    o = wavefront_np(dy, dx, y, x, pixel_size=p, distance=L, wavelength=1e-10, remove=None)
    assert abs(o["radius_x"][0] - L / kappa) <= 1e-9 * L / kappa
    assert abs(o["radius_y"][0] - L / ky) <= 1e-9 * abs(L / ky)
    xm = (x - x.mean()) * p
    np.testing.assert_allclose(np.gradient(o["wavefront"][0], xm, axis=1)[:, 1:-1], dx[0][:, 1:-1] * p / L, rtol=1e-9,
                               atol=1e-12 * np.max(np.abs(dx)) * p / L)
    np.testing.assert_allclose(o["phase"], 2 * np.pi * o["wavefront"] / 1e-10)
    q = wavefront_np(dy, dx, y, x, pixel_size=p, distance=L, remove="quadratic")
    assert q["rms"][0] <= 1e-12 * np.ptp(o["wavefront"]) and "phase" not in q


# ---- argument checks of the product, raised on the host
@pytest.fixture(scope="module")
def wf():
    from barc4dip_amd import signal
    from barc4dip_amd.signal import wavefront

    assert signal.integrate_gradient is wavefront.integrate_gradient
    assert signal.wavefront_from_displacement is wavefront.wavefront_from_displacement
    return wavefront


def test_integrate_gradient_argument_errors(wf):
    z = np.zeros((4, 5))
    bad = [
        lambda: wf.integrate_gradient(z, np.zeros((5, 4))),
        lambda: wf.integrate_gradient(z[0], z[0]),
        lambda: wf.integrate_gradient(z[None, None], z[None, None]),
        lambda: wf.integrate_gradient(np.zeros((0, 5)), np.zeros((0, 5))),
        lambda: wf.integrate_gradient(z, z, dy=0.0),
        lambda: wf.integrate_gradient(z, z, dx=-1.0),
        lambda: wf.integrate_gradient(z, z, dy=np.nan),
        lambda: wf.integrate_gradient(z, z, dx=np.inf),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_side_limit_is_raised_on_the_host(wf):
    from barc4dip_amd import _ffi

    for shape in ((2049, 3), (2, 3, 2049)):
        with pytest.raises(NotImplementedError) as e:
            wf.integrate_gradient(np.zeros(shape), np.zeros(shape))
        assert isinstance(e.value, _ffi.B4DSizeError)
    with pytest.raises(NotImplementedError):
        wf.wavefront_from_displacement((np.zeros((3, 2049)), np.zeros((3, 2049))), pixel_size=1e-6, distance=1.0)


def test_wavefront_from_displacement_argument_errors(wf):
    z = np.zeros((4, 5))
    y, x = np.arange(4.0), np.arange(5.0)
    kw = dict(pixel_size=1e-6, distance=1.0)
    bad = [
        lambda: wf.wavefront_from_displacement({"dy": z, "dx": z, "y": np.array([0.0, 1.0, 2.0, 4.0]), "x": x}, **kw),
        lambda: wf.wavefront_from_displacement({"dy": z, "dx": z, "y": y, "x": x[:4]}, **kw),
        lambda: wf.wavefront_from_displacement({"dy": z, "dx": z, "y": y}, **kw),
        lambda: wf.wavefront_from_displacement({"dy": z, "dx": z, "y": y, "x": x}, remove="defocus", **kw),
        lambda: wf.wavefront_from_displacement({"dy": z, "dx": z[:, :4], "y": y, "x": x}, **kw),
        lambda: wf.wavefront_from_displacement((z, z, z), **kw),
        lambda: wf.wavefront_from_displacement((z, z), pixel_size=0.0, distance=1.0),
        lambda: wf.wavefront_from_displacement((z, z), pixel_size=1e-6, distance=np.inf),
        lambda: wf.wavefront_from_displacement((z, z), wavelength=-1.0, **kw),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
