"""CPU tier of the weighted / masked wavefront integration: the float64 oracles that the GPU tests compare
against, checked here against a dense construction of the defined solution, and the argument checks of the public functions,
which are raised before any device is needed.

Definition.  Node weights w >= 0 (0 where the weight is not finite and positive or a slope is not finite), edge weights the
harmonic mean of the two node weights, phi a minimiser of the weighted squared edge residuals.  Of all minimisers (every connected
piece of the valid region has a free piston, every weight-0 node is free) the one with the smallest unweighted Laplacian energy
phi^T L phi and zero mean over the grid is meant: it is what conjugate gradients from 0 with the DCT solve L^+ as preconditioner
converge to."""
from __future__ import annotations

import numpy as np
import pytest
from scipy import fft as sfft
from scipy import ndimage

from test_wavefront_host import MONOMIALS, REMOVE, dct_basis, edge_means, eigenvalues_np, integrate_np, smooth_slopes

HY, HX = 0.7, 1.9
PATTERNS = ("disc", "disc_holes", "gap", "gap_graded", "disc_graded")


# ---- inputs shared with the GPU tests
def weight_pattern(name, shape, seed=0):
    """Node weights (ny, nx) float64: a disc r^2 <= 0.9 in coordinates that run over [-1, 1] per side, the disc with 10 % random
    holes, a 2-column gap that cuts the grid into two pieces, the gap times U[0.05, 1], the disc times U clipped to [0.05, 1]."""
    ny, nx = shape
    rng = np.random.default_rng(1000 + seed)
    v = (np.arange(ny) - 0.5 * (ny - 1)) / max(0.5 * (ny - 1), 1.0)
    u = (np.arange(nx) - 0.5 * (nx - 1)) / max(0.5 * (nx - 1), 1.0)
    disc = ((v[:, None] ** 2 + u[None, :] ** 2) <= 0.9).astype(np.float64)
    gap = np.ones(shape)
    gap[:, nx // 2 - 1:nx // 2 + 1] = 0.0
    if name == "disc":
        return disc
    if name == "disc_holes":
        return disc * (rng.random(shape) >= 0.1)
    if name == "gap":
        return gap
    if name == "gap_graded":
        return gap * rng.uniform(0.05, 1.0, shape)
    if name == "disc_graded":
        return disc * np.clip(rng.random(shape), 0.05, 1.0)
    raise ValueError(name)


# ---- oracles
def effective_weights(w, gy, gx):
    w = np.asarray(w, np.float64)
    ok = np.isfinite(w) & (w > 0) & np.isfinite(gy) & np.isfinite(gx)
    return np.where(ok, w, 0.0)


def hmean(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((a > 0) & (b > 0), 2.0 * a * b / (a + b), 0.0)


def weighted_system(gy, gx, w, hy, hx):
    """(effective weights, wy / hy^2 (ny-1, nx), wx / hx^2 (ny, nx-1), b (ny, nx)) of the weighted normal equations, float64."""
    gy, gx = np.asarray(gy, np.float64), np.asarray(gx, np.float64)
    w = effective_weights(w, gy, gx)
    g0y, g0x = np.where(w > 0, gy, 0.0), np.where(w > 0, gx, 0.0)       # slopes of weight-0 nodes never enter
    wy, wx = hmean(w[:-1, :], w[1:, :]), hmean(w[:, :-1], w[:, 1:])
    ey, ex = edge_means(g0y, g0x)
    b = np.zeros(gy.shape)
    b[1:, :] += wy * ey / hy
    b[:-1, :] -= wy * ey / hy
    b[:, 1:] += wx * ex / hx
    b[:, :-1] -= wx * ex / hx
    return w, wy / hy ** 2, wx / hx ** 2, b


def apply_weighted(p, cy, cx):
    q = np.zeros_like(p)
    d = cy * (p[1:, :] - p[:-1, :])
    q[1:, :] += d
    q[:-1, :] -= d
    d = cx * (p[:, 1:] - p[:, :-1])
    q[:, 1:] += d
    q[:, :-1] -= d
    return q


def _pcg(b, apply, precond, dtype, rtol, max_iter):
    """The iteration of the device: vectors in `dtype`, dot products, alpha and beta in float64; a map stops when |r| <= rtol |b|,
    when b = 0 or when p.Ap is not finite and positive.  Returns (x, iterations, |r| / |b|)."""
    x, r = np.zeros_like(b), b.copy()
    dot = lambda a, c: float(np.sum(a.astype(np.float64) * c.astype(np.float64)))
    bb = dot(b, b)
    if not (bb > 0 and np.isfinite(bb)):
        return x, 0, 0.0
    z = precond(r)
    p, rz, rr, it = z.copy(), dot(r, z), bb, 0
    while it < max_iter:
        q = apply(p)
        pq = dot(p, q)
        if not (pq > 0 and np.isfinite(pq)):
            break
        alpha = dtype(rz / pq)
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * q).astype(dtype)
        rr, it = dot(r, r), it + 1
        if rr <= rtol * rtol * bb or not np.isfinite(rr):
            break
        z = precond(r)
        rz_new = dot(r, z)
        p = (z + dtype(rz_new / rz if rz > 0 else 0.0) * p).astype(dtype)
        rz = rz_new
    return x, it, float(np.sqrt(rr / bb))


def integrate_weighted_np(gy, gx, w, hy=1.0, hx=1.0, rtol=1e-6, max_iter=500, return_info=False):
    """float64 PCG with the DCT Poisson solve (scipy.fft.dctn) as preconditioner, harmonic fill."""
    _, cy, cx, b = weighted_system(gy, gx, w, hy, hx)
    lam = eigenvalues_np(*b.shape, hy, hx)
    lam[0, 0] = 1.0

    def precond(r):
        p = sfft.dctn(r, type=2, norm="ortho") / lam
        p[0, 0] = 0.0
        return sfft.idctn(p, type=2, norm="ortho")

    x, it, res = _pcg(b, lambda p: apply_weighted(p, cy, cx), precond, np.float64, rtol, max_iter)
    return (x, it, res) if return_info else x


def integrate_weighted_pcg32(gy, gx, w, hy=1.0, hx=1.0, rtol=1e-6, max_iter=500):
    """The same iteration with float32 vectors and the preconditioner as four float32 matrix products (basis and eigenvalues
    rounded from float64, as integrate_mm32): the yardstick for what float32 arithmetic can deliver."""
    _, cy, cx, b = weighted_system(np.asarray(gy, np.float32), np.asarray(gx, np.float32), np.asarray(w, np.float32), hy, hx)
    cy, cx, b = cy.astype(np.float32), cx.astype(np.float32), b.astype(np.float32)
    ny, nx = b.shape
    by, bx = dct_basis(ny).astype(np.float32), dct_basis(nx).astype(np.float32)
    lam = eigenvalues_np(ny, nx, hy, hx)
    lam[0, 0] = 1.0
    lam = lam.astype(np.float32)

    def precond(r):
        p = (by @ (r @ bx.T)) / lam
        p[0, 0] = 0.0
        return by.T @ (p @ bx)

    return _pcg(b, lambda p: apply_weighted(p, cy, cx), precond, np.float32, rtol, max_iter)[0].astype(np.float64)


def _dense_operator(cy, cx):
    """Dense matrix of apply_weighted for edge coefficients cy (ny-1, nx), cx (ny, nx-1)."""
    ny, nx = cx.shape[0], cy.shape[1]
    idx = np.arange(ny * nx).reshape(ny, nx)
    a = np.zeros((ny * nx, ny * nx))
    for (p, q, c) in ((idx[:-1, :], idx[1:, :], cy), (idx[:, :-1], idx[:, 1:], cx)):
        p, q, c = p.ravel(), q.ravel(), c.ravel()
        np.add.at(a, (p, p), c)
        np.add.at(a, (q, q), c)
        np.add.at(a, (p, q), -c)
        np.add.at(a, (q, p), -c)
    return a


def null_space(w):
    """Columns: the indicator of every connected piece of w > 0 (4-neighbourhood) and the unit vector of every weight-0 node."""
    lab, n = ndimage.label(w > 0)
    cols = [(lab == k).ravel().astype(np.float64) for k in range(1, n + 1)]
    for e in np.flatnonzero(w.ravel() == 0):
        c = np.zeros(w.size)
        c[e] = 1.0
        cols.append(c)
    return np.array(cols).T, lab


def integrate_weighted_dense(gy, gx, w, hy=1.0, hx=1.0):
    """The defined solution by dense linear algebra: the minimum-norm lstsq solution of A phi = b, plus the null-space
    combination that minimises phi^T L phi, minus the mean."""
    w, cy, cx, b = weighted_system(gy, gx, w, hy, hx)
    ny, nx = b.shape
    a = _dense_operator(cy, cx)
    lap = _dense_operator(np.full((ny - 1, nx), 1.0 / hy ** 2), np.full((ny, nx - 1), 1.0 / hx ** 2))
    phi = np.linalg.lstsq(a, b.ravel(), rcond=None)[0]
    z, _ = null_space(w)
    c = np.linalg.lstsq(z.T @ lap @ z, -z.T @ (lap @ phi), rcond=None)[0]
    phi = phi + z @ c
    return (phi - phi.mean()).reshape(ny, nx)


def piece_lstsq(gy, gx, w, lab, k, hy, hx):
    """Plain weighted least squares of the edge equations inside piece k; returns (node index arrays, solution with zero mean)."""
    w = effective_weights(w, gy, gx)
    ii, jj = np.nonzero(lab == k)
    num = -np.ones(w.shape, int)
    num[ii, jj] = np.arange(ii.size)
    ey, ex = edge_means(np.where(w > 0, gy, 0.0), np.where(w > 0, gx, 0.0))
    wy, wx = hmean(w[:-1, :], w[1:, :]), hmean(w[:, :-1], w[:, 1:])
    rows, rhs = [], []
    for i, j in zip(ii, jj):
        if i + 1 < w.shape[0] and num[i + 1, j] >= 0:
            a = np.zeros(ii.size)
            s = np.sqrt(wy[i, j])
            a[num[i + 1, j]], a[num[i, j]] = s / hy, -s / hy
            rows.append(a)
            rhs.append(s * ey[i, j])
        if j + 1 < w.shape[1] and num[i, j + 1] >= 0:
            a = np.zeros(ii.size)
            s = np.sqrt(wx[i, j])
            a[num[i, j + 1]], a[num[i, j]] = s / hx, -s / hx
            rows.append(a)
            rhs.append(s * ex[i, j])
    rows.append(np.ones(ii.size))
    rhs.append(0.0)
    return ii, jj, np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]


def poly2_weighted_np(w_map, weights, y_m, x_m):
    """Weighted least-squares coefficients of (1, u, v, u^2, uv, v^2) on one map: lstsq on the sqrt(w)-scaled rows of the valid
    nodes, u = x_m - mean(x_m), v = y_m - mean(y_m) over the full grid.  Monomials are taken in order; one that the valid nodes
    cannot tell from the kept ones before it (squared remainder below 1e-12 of its own squared norm) is left out and gets 0.
    Returns (coefficients (6,), design matrix (ny nx, 6))."""
    u, v = np.meshgrid(x_m - np.mean(x_m), y_m - np.mean(y_m))
    a = np.stack([(u ** pu * v ** pv).ravel() for pu, pv in MONOMIALS], axis=1)
    w = np.asarray(weights, np.float64).ravel()
    ok = np.isfinite(w) & (w > 0)
    s = np.sqrt(w[ok])
    rows, rhs = a[ok] * s[:, None], np.ravel(w_map)[ok] * s
    kept = []
    for k in range(6):
        col = rows[:, k]
        n2 = float(col @ col)
        if not n2 > 0:
            continue
        if kept:
            q = rows[:, kept] / np.sqrt(np.sum(rows[:, kept] ** 2, axis=0))
            col = col - q @ np.linalg.lstsq(q, col, rcond=None)[0]
        if float(col @ col) > 1e-12 * n2:
            kept.append(k)
    c = np.zeros(6)
    if kept:
        norm = np.sqrt(np.sum(rows[:, kept] ** 2, axis=0))
        c[kept] = np.linalg.lstsq(rows[:, kept] / norm, rhs, rcond=None)[0] / norm
    return c, a


def wavefront_weighted_np(dy, dx, w, y, x, *, pixel_size, distance, remove="tilt", rtol=1e-6):
    """Oracle chain of wavefront_from_displacement with weights for (T, ny, nx) shift maps (pixels) on the axes y, x (pixels):
    harmonic fill, weighted fit, rms the weighted population standard deviation over the valid nodes."""
    dy, dx = np.asarray(dy, np.float64), np.asarray(dx, np.float64)
    w = np.broadcast_to(np.asarray(w, np.float64), dy.shape)
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    sy = (y[-1] - y[0]) / (len(y) - 1) if len(y) > 1 else 1.0
    sx = (x[-1] - x[0]) / (len(x) - 1) if len(x) > 1 else 1.0
    out = {"wavefront": [], "coefficients": [], "rms": []}
    for t in range(dy.shape[0]):
        we = effective_weights(w[t], dy[t], dx[t])
        phi = integrate_weighted_np(dy[t] * pixel_size / distance, dx[t] * pixel_size / distance, we, sy * pixel_size,
                                    sx * pixel_size, rtol=rtol)
        c, a = poly2_weighted_np(phi, we, y * pixel_size, x * pixel_size)
        sel = list(REMOVE[remove])
        phi = phi - (a[:, sel] @ c[sel]).reshape(phi.shape)
        m = np.sum(we * phi) / np.sum(we)
        out["wavefront"].append(phi)
        out["coefficients"].append(c)
        out["rms"].append(np.sqrt(max(0.0, np.sum(we * phi ** 2) / np.sum(we) - m * m)))
    return {k: np.array(v) for k, v in out.items()}


# ---- the oracle against independent statements
def _case(shape, pattern, seed=7):
    gy, gx = smooth_slopes(shape, HY, HX, seed)
    return gy, gx, weight_pattern(pattern, shape, seed)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [(7, 9), (23, 31)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pcg_equals_the_dense_construction(shape, pattern):
    gy, gx, w = _case(shape, pattern)
    want = integrate_weighted_dense(gy, gx, w, HY, HX)
    got, it, res = integrate_weighted_np(gy, gx, w, HY, HX, rtol=1e-13, return_info=True)
    assert it < 500 and res <= 1e-13
    assert np.max(np.abs(got - want)) <= 1e-8 * np.ptp(want)          # over the whole grid: the fill and the levelling too
    assert abs(got.mean()) <= 1e-10 * np.ptp(want)


@pytest.mark.parametrize("shape,hole", [((1, 5), (0, 2)), ((5, 1), (2, 0)), ((2, 2), (0, 1)), ((2, 3), None)])
def test_pcg_equals_the_dense_construction_on_degenerate_grids(shape, hole):
    gy, gx = smooth_slopes(shape, HY, HX, 5)
    w = np.ones(shape)
    if hole is not None:
        w[hole] = 0.0
    want = integrate_weighted_dense(gy, gx, w, HY, HX)
    got = integrate_weighted_np(gy, gx, w, HY, HX, rtol=1e-13)
    assert np.max(np.abs(got - want)) <= 1e-8 * np.ptp(want)


@pytest.mark.parametrize("shape", [(7, 9), (23, 31), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_ones_is_the_unweighted_solution_in_one_iteration(shape):
    gy, gx = smooth_slopes(shape, HY, HX, 3)
    got, it, _ = integrate_weighted_np(gy, gx, np.ones(shape), HY, HX, rtol=1e-10, return_info=True)
    want = integrate_np(gy, gx, HY, HX)
    assert it == 1
    assert np.max(np.abs(got - want)) <= 1e-12 * np.ptp(want)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_piece_is_its_own_least_squares_solution(pattern):
    shape = (23, 31)
    gy, gx, w = _case(shape, pattern)
    got = integrate_weighted_np(gy, gx, w, HY, HX, rtol=1e-13)
    lab, n = ndimage.label(w > 0)
    assert n >= (2 if pattern.startswith("gap") else 1)
    for k in range(1, n + 1):
        ii, jj, sol = piece_lstsq(gy, gx, w, lab, k, HY, HX)
        part = got[ii, jj] - got[ii, jj].mean()
        assert np.max(np.abs(part - (sol - sol.mean()))) <= 1e-8 * np.ptp(got)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_result_does_not_depend_on_the_scale_of_the_weights(pattern):
    gy, gx, w = _case((23, 31), pattern)
    a = integrate_weighted_np(gy, gx, w, HY, HX, rtol=1e-13)
    b = integrate_weighted_np(gy, gx, 1000.0 * w, HY, HX, rtol=1e-13)
    assert np.max(np.abs(a - b)) <= 1e-10 * np.ptp(a)


def test_non_finite_slopes_and_weights_count_as_weight_zero():
    gy, gx, w = _case((23, 31), "disc")
    want = integrate_weighted_np(gy, gx, w, HY, HX, rtol=1e-13)
    gy2, gx2, w2 = gy.copy(), gx.copy(), w.copy()
    gy2[w == 0] = np.nan
    gx2[0, 0] = np.inf
    w2[0, 1], w2[1, 0], w2[0, 2] = np.nan, -3.0, np.inf
    assert w[0, 0] == 0 and w[0, 1] == 0 and w[1, 0] == 0 and w[0, 2] == 0
    np.testing.assert_array_equal(integrate_weighted_np(gy2, gx2, w2, HY, HX, rtol=1e-13), want)
    # NaN slopes under all-ones weights mask themselves
    gy3, w3 = gy.copy(), np.ones(gy.shape)
    gy3[5, 7] = np.nan
    w3[5, 7] = 0.0
    np.testing.assert_array_equal(integrate_weighted_np(gy3, gx, np.ones(gy.shape), HY, HX), integrate_weighted_np(gy, gx, w3, HY, HX))


@pytest.mark.parametrize("shape", [(23, 31), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern", PATTERNS)
def test_float32_yardstick_tracks_the_oracle(shape, pattern):
    """integrate_weighted_pcg32 at rtol = 1e-6 stays within 3e-5 of the range of the float64 iteration on every pattern (binary
    masks a few 1e-7, graded weights up to several 1e-6), in fewer than 500 iterations."""
    gy, gx, w = _case(shape, pattern)
    ref, it, _ = integrate_weighted_np(gy, gx, w, HY, HX, return_info=True)
    assert it < 500
    assert np.max(np.abs(integrate_weighted_pcg32(gy, gx, w, HY, HX) - ref)) <= 3e-5 * np.ptp(ref)


def test_weighted_fit_oracle():
    ny, nx = 23, 31
    y, x = np.arange(ny) * 0.7, np.arange(nx) * 1.9
    u, v = np.meshgrid(x - x.mean(), y - y.mean())
    c = np.array([0.3, -0.2, 0.15, 1.1e-2, -0.7e-2, 0.4e-2])
    phi = sum(ck * u ** pu * v ** pv for ck, (pu, pv) in zip(c, MONOMIALS))
    w = weight_pattern("disc_graded", (ny, nx))
    got, _ = poly2_weighted_np(np.where(w > 0, phi, np.nan), w, y, x)        # a quadratic is returned exactly, NaN outside is unread
    np.testing.assert_allclose(got, c, rtol=1e-9, atol=1e-12)
    row = np.zeros((ny, nx))
    row[11, :] = 1.0                                                          # a single valid row: v is constant on it
    got, _ = poly2_weighted_np(phi, row, y, x)
    assert np.all(got[[2, 4, 5]] == 0.0) and np.all(got[[0, 1, 3]] != 0.0)
    few = np.zeros((ny, nx))
    few[[2, 5, 9, 17, 20], [3, 25, 14, 7, 28]] = 1.0                          # five nodes: the sixth monomial is dropped
    got, a = poly2_weighted_np(phi, few, y, x)
    assert got[5] == 0.0 and np.max(np.abs((a @ got).reshape(ny, nx)[few > 0] - phi[few > 0])) <= 1e-9 * np.ptp(phi)


# ---- argument checks of the product, raised on the host
@pytest.fixture(scope="module")
def wf():
    from barc4dip_amd.signal import wavefront

    return wavefront


def test_integrate_gradient_weight_argument_errors(wf):
    z = np.zeros((3, 4, 5))
    bad = [
        lambda: wf.integrate_gradient(z, z, weights=np.ones((5, 4))),
        lambda: wf.integrate_gradient(z, z, mask=np.ones((2, 4, 5), bool)),
        lambda: wf.integrate_gradient(z, z, weights=np.ones((1, 4, 5))),
        lambda: wf.integrate_gradient(z[0], z[0], weights=np.ones((3, 4, 5))),
        lambda: wf.integrate_gradient(z, z, weights=np.ones((4, 5), complex)),
        lambda: wf.integrate_gradient(z, z, weights="peak"),
        lambda: wf.integrate_gradient(z, z, mask=np.ones((4, 5), bool), fill="zero"),
        lambda: wf.integrate_gradient(z, z, fill=None),
        lambda: wf.integrate_gradient(z, z, mask=np.ones((4, 5), bool), rtol=-1.0),
        lambda: wf.integrate_gradient(z, z, mask=np.ones((4, 5), bool), rtol=np.nan),
        lambda: wf.integrate_gradient(z, z, mask=np.ones((4, 5), bool), max_iter=0),
        lambda: wf.integrate_gradient(z, z, mask=np.ones((4, 5), bool), max_iter=2.5),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_wavefront_from_displacement_weight_argument_errors(wf):
    z = np.zeros((4, 5))
    y, x = np.arange(4.0), np.arange(5.0)
    kw = dict(pixel_size=1e-6, distance=1.0)
    field = {"dy": z, "dx": z, "y": y, "x": x, "peak": np.ones((4, 5))}
    bad = [
        lambda: wf.wavefront_from_displacement(field, weights="snr", **kw),                  # no such key
        lambda: wf.wavefront_from_displacement((z, z), weights="peak", **kw),                # a plain pair has no maps
        lambda: wf.wavefront_from_displacement(field, weights="ncc", **kw),
        lambda: wf.wavefront_from_displacement(field, weights=np.ones((5, 4)), **kw),
        lambda: wf.wavefront_from_displacement(field, mask=np.ones((4, 4), bool), **kw),
        lambda: wf.wavefront_from_displacement(field, weights="peak", fill="linear", **kw),
        lambda: wf.wavefront_from_displacement(dict(field, peak=np.ones((3, 5))), weights="peak", **kw),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
