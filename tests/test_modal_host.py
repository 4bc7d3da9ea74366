"""CPU tier of the modal fits (barc4dip_amd/signal/modal.py): the float64 oracle that tests/test_gpu_modal.py compares the device
with, its self-checks, and the host side of the product (mode tables, argument errors, no host fallback).

The oracle is written independently of the device algorithm: Zernike modes from the explicit factorial formula (exact integer
radial coefficients) with arctan2, cos and sin in np.longdouble, rounded to float64; Legendre modes from
numpy.polynomial.legendre; the solve by np.linalg.lstsq on sqrt(w) A where every mode is kept, by the sequential drop-rule
Cholesky (in np.longdouble) where the case is rank-deficient."""
from __future__ import annotations

from math import factorial

import numpy as np
import pytest
from numpy.polynomial import legendre as npleg

from test_wavefront_weighted_host import weight_pattern

LD = np.longdouble
NOLL_15 = [(0, 0), (1, 1), (1, -1), (2, 0), (2, -2), (2, 2), (3, -1), (3, 1), (3, -3), (3, 3), (4, 0), (4, 2), (4, -2), (4, 4),
           (4, -4)]


# ---- mode tables
def noll_table(J):
    """(n, m) of Noll's modes 1 .. J, m > 0 the cosine: orders n ascending, |m| ascending within n, even j the cosine."""
    out, j, n = [], 1, 0
    while len(out) < J:
        for am in range(n % 2, n + 1, 2):
            for _ in range(1 if am == 0 else 2):
                out.append((n, 0 if am == 0 else (am if j % 2 == 0 else -am)))
                j += 1
        n += 1
    return np.array(out[:J], dtype=np.int64)


def legendre_table(J):
    """(a, b), the degrees in u and v: by total degree, within a degree by growing power of v."""
    out, d = [], 0
    while len(out) < J:
        out += [(d - b, b) for b in range(d + 1)]
        d += 1
    return np.array(out[:J], dtype=np.int64)


# ---- modes
def radial_coefficients(n, m):
    """Exact integer coefficients of rho^(n - 2s), s = 0 .. (n - m) / 2, of R_n^m."""
    return [(-1) ** s * factorial(n - s) // (factorial(s) * factorial((n + m) // 2 - s) * factorial((n - m) // 2 - s))
            for s in range((n - m) // 2 + 1)]


def zernike_modes(J, u, v):
    """(.., J) float64: Noll modes at the normalised coordinates u (along x), v (along y), evaluated in np.longdouble.
    The extended-precision pi puts cos and sin of a node on a nodal line (u = 0, v = 0, the diagonals) at 1e-19 instead of 0,
    which would make an identically vanishing mode pass the drop rule with a coefficient of 1e19; the absolute error of the
    evaluation is below 1e-18 for modes of size 1, so values below 1e-17 are the zeros they stand for."""
    u, v = np.asarray(u, LD), np.asarray(v, LD)
    rho, th = np.sqrt(u * u + v * v), np.arctan2(v, u)
    table = noll_table(J)
    top = int(table[-1, 0])
    power = [np.ones_like(rho)]
    for _ in range(top):
        power.append(power[-1] * rho)
    cos, sin = [np.cos(m * th) for m in range(top + 1)], [np.sin(m * th) for m in range(top + 1)]
    out = np.empty(u.shape + (J,), np.float64)
    for k, (n, m) in enumerate(table):
        n, am = int(n), abs(int(m))
        R = sum(LD(c) * power[n - 2 * s] for s, c in enumerate(radial_coefficients(n, am)))
        if m == 0:
            z = np.sqrt(LD(n + 1)) * R
        else:
            z = np.sqrt(LD(2 * (n + 1))) * R * (cos[am] if m > 0 else sin[am])
        z = z.astype(np.float64)
        z[np.abs(z) < 1e-17] = 0.0
        out[..., k] = z
    return out


def legendre_modes(J, u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    out = np.empty(u.shape + (J,), np.float64)
    for k, (a, b) in enumerate(legendre_table(J)):
        ca, cb = np.zeros(a + 1), np.zeros(b + 1)
        ca[a], cb[b] = 1.0, 1.0
        out[..., k] = np.sqrt(2.0 * a + 1.0) * np.sqrt(2.0 * b + 1.0) * npleg.legval(u, ca) * npleg.legval(v, cb)
    return out


def geometry(shape, basis, dy=1.0, dx=1.0, center=None, radius=None):
    """(u, v) normalised node coordinates (ny, nx) and the radius (None for Legendre), as modal_fit defines them."""
    ny, nx = shape
    cy, cx = (0.5 * (ny - 1), 0.5 * (nx - 1)) if center is None else center
    if basis == "legendre":
        sy, sx, radius = 1.0 / max(cy, 1.0), 1.0 / max(cx, 1.0), None
    else:
        radius = min(cy * dy, cx * dx) if radius is None else radius
        sy, sx = dy / radius, dx / radius
    v = (np.arange(ny, dtype=np.float64) - cy) * sy
    u = (np.arange(nx, dtype=np.float64) - cx) * sx
    return np.broadcast_to(u[None, :], shape), np.broadcast_to(v[:, None], shape), radius


def design(shape, basis, J, **geo):
    """A (ny, nx, J) float64 and the aperture (ny, nx) bool (all True for Legendre)."""
    u, v, _ = geometry(shape, basis, **geo)
    if basis == "legendre":
        return legendre_modes(J, u, v), np.ones(shape, bool)
    return zernike_modes(J, u, v), (u * u + v * v) <= 1.0 + 1e-9


# ---- solve
def effective_weights(phi, w, aperture):
    w = np.ones(phi.shape) if w is None else np.broadcast_to(np.asarray(w, np.float64), phi.shape)
    ok = np.isfinite(w) & (w > 0) & np.isfinite(phi) & aperture
    return np.where(ok, w, 0.0)


def drop_rule_cholesky(G, rhs):
    """Sequential Cholesky without pivoting, modes in order, in the precision of G: (coefficients, kept, remainder / diagonal)."""
    J = len(rhs)
    L = np.zeros((J, J), G.dtype)
    y, x = np.zeros(J, G.dtype), np.zeros(J, G.dtype)
    kept, rel = np.zeros(J, bool), np.zeros(J)
    for a in range(J):
        d = G[a, a]
        for b in range(a):
            if kept[b]:
                L[a, b] = (G[a, b] - L[a, :b] @ L[b, :b]) / L[b, b]
                d = d - L[a, b] * L[a, b]
        rel[a] = float(d / G[a, a]) if G[a, a] > 0 else 0.0
        kept[a] = bool(d > 1e-12 * G[a, a] and G[a, a] > 0)
        if kept[a]:
            L[a, a] = np.sqrt(d)
            y[a] = (rhs[a] - L[a, :a] @ y[:a]) / L[a, a]
    for a in range(J - 1, -1, -1):
        if kept[a]:
            x[a] = (y[a] - L[a + 1:, a] @ x[a + 1:]) / L[a, a]
    return x, kept, rel


def fit_oracle(phi, w, A, aperture, remove="all", fill="nan"):
    """One map phi (ny, nx) (float32 values), weights w or None -> dict as modal_fit returns, plus the diagnostics "rel"
    (remainder / diagonal of every mode) and "cond" (condition number of the normalised Gram matrix of the kept modes)."""
    J = A.shape[-1]
    phi64 = np.asarray(phi, np.float64)
    we = effective_weights(phi64, w, aperture)
    sel = we > 0
    sw = np.sqrt(we[sel])
    Aw, bw = A[sel] * sw[:, None], np.where(sel, phi64, 0.0)[sel] * sw
    AwL = Aw.astype(LD if Aw.shape[0] <= 4096 else np.float64)      # the Gram matrix only decides `kept` where nothing is dropped
    G, rhs = AwL.T @ AwL, AwL.T @ bw.astype(LD)
    c, kept, rel = drop_rule_cholesky(G, rhs)
    c = c.astype(np.float64)
    if kept.all() and sel.any():
        c = np.linalg.lstsq(Aw, bw, rcond=None)[0]
    cond = np.nan
    if kept.any():
        d = np.sqrt(np.diag(G)[kept].astype(np.float64))
        cond = float(np.linalg.cond(G[np.ix_(kept, kept)].astype(np.float64) / np.outer(d, d)))
    flags = np.ones(J, bool) if isinstance(remove, str) else np.isin(np.arange(1, J + 1), [] if remove is None else list(remove))
    with np.errstate(invalid="ignore"):
        r = (phi64 - A[..., flags] @ c[flags]).astype(np.float32)
    if sel.any():
        r64 = r[sel].astype(np.float64)
        mean = np.sum(we[sel] * r64) / np.sum(we[sel])
        rms = float(np.sqrt(max(0.0, np.sum(we[sel] * r64 * r64) / np.sum(we[sel]) - mean * mean)))
    else:
        rms = np.nan
    if fill == "nan":
        r = np.where(sel, r, np.float32(np.nan))
    return {"coefficients": c, "kept": kept, "residual": r, "rms": rms, "valid": sel, "rel": rel, "cond": cond}


def smooth_map(shape, seed, amplitude=1.0):
    """A float32 test wavefront: low-order surface of order 1 plus 1 % noise, offset and tilt included."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    v = np.linspace(-1.0, 1.0, ny)[:, None] if ny > 1 else np.zeros((1, 1))
    u = np.linspace(-1.0, 1.0, nx)[None, :] if nx > 1 else np.zeros((1, 1))
    c = rng.normal(size=8)
    phi = (c[0] + c[1] * u + c[2] * v + c[3] * u * u + c[4] * u * v + c[5] * v * v + c[6] * np.cos(3.0 * u + 2.0 * v)
           + c[7] * np.sin(4.0 * u * v + 1.0) + 0.01 * rng.normal(size=shape))
    return (amplitude * phi).astype(np.float32)


# the degenerate parity cases of the device test: (basis, grid, J, radius)
DEGENERATE = [("zernike", (1, 9), 10, 4.0), ("zernike", (9, 1), 10, 4.0), ("zernike", (2, 2), 6, 1.0), ("zernike", (3, 3), 10, 1.5),
              ("zernike", (5, 5), 15, 2.0), ("legendre", (1, 9), 10, None), ("legendre", (2, 2), 6, None),
              ("legendre", (3, 3), 10, None), ("legendre", (2, 7), 15, None)]


def degenerate_case(basis, shape, J, radius):
    geo = {} if basis == "legendre" else {"radius": radius}
    A, ap = design(shape, basis, J, **geo)
    return smooth_map(shape, 11), A, ap, geo


# ---- self-checks of the oracle
def test_longdouble_is_extended_precision():
    assert np.finfo(LD).eps < 1e-18


def test_noll_indices_equal_the_literature_table():
    assert [tuple(r) for r in noll_table(15)] == NOLL_15
    t = noll_table(66)
    assert t[-1, 0] == 10 and np.all((t[:, 0] - np.abs(t[:, 1])) % 2 == 0) and len({tuple(r) for r in t}) == 66


def test_zernike_modes_are_orthonormal_over_the_unit_disc():
    x, wx = np.polynomial.legendre.leggauss(16)           # exact for polynomials of degree 31 >= 2 * 10 + 1 in rho
    rho, wr = 0.5 * (x + 1.0), 0.5 * wx
    nth = 32                                              # uniform rule, exact for |m| + |m'| <= 20 < 32
    th = 2.0 * np.pi * np.arange(nth) / nth
    R, T = np.meshgrid(rho, th, indexing="ij")
    Z = zernike_modes(66, R * np.cos(T), R * np.sin(T))
    W = (wr * rho)[:, None] * np.full(nth, 2.0 / nth)[None, :]     # area element / pi
    G = np.einsum("rtk,rt,rtl->kl", Z, W, Z)
    assert np.max(np.abs(G - np.eye(66))) <= 1e-12


def test_legendre_modes_are_orthonormal_over_the_square():
    x, wx = np.polynomial.legendre.leggauss(12)
    U, V = np.meshgrid(x, x, indexing="xy")
    P = legendre_modes(66, U, V)
    G = np.einsum("ijk,ij,ijl->kl", P, np.outer(wx, wx) / 4.0, P)
    assert np.max(np.abs(G - np.eye(66))) <= 1e-12
    # the first six span the six monomials (1, u, v, u^2, u v, v^2) in the same order
    assert [tuple(r) for r in legendre_table(6)] == [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]


@pytest.mark.parametrize("basis,pattern", [("zernike", "disc_holes"), ("legendre", "gap_graded")])
def test_lstsq_and_drop_rule_cholesky_agree_where_nothing_is_dropped(basis, pattern):
    shape, J = (23, 31), 36
    A, ap = design(shape, basis, J)
    phi, w = smooth_map(shape, 3), weight_pattern(pattern, shape)
    ref = fit_oracle(phi, w, A, ap)
    assert ref["kept"].all() and ref["cond"] < 1e2
    we = effective_weights(phi.astype(np.float64), w, ap)
    Aw = (A * np.sqrt(we)[..., None]).reshape(-1, J).astype(LD)
    c, kept, _ = drop_rule_cholesky(Aw.T @ Aw, Aw.T @ (np.sqrt(we) * phi).reshape(-1).astype(LD))
    assert kept.all()
    assert np.max(np.abs(c.astype(np.float64) - ref["coefficients"])) <= 1e-13 * np.max(np.abs(ref["coefficients"]))


@pytest.mark.parametrize("basis,shape,J,radius", DEGENERATE)
def test_degenerate_cases_are_no_close_call_for_the_drop_rule(basis, shape, J, radius):
    """Kept remainders are far above, dropped ones far below the 1e-12 of the rule, so the device must agree on `kept`."""
    phi, A, ap, _ = degenerate_case(basis, shape, J, radius)
    ref = fit_oracle(phi, None, A, ap)
    assert not ref["kept"].all()
    assert np.all(ref["rel"][ref["kept"]] >= 1e-6) and np.all(np.abs(ref["rel"][~ref["kept"]]) <= 1e-14)


# ---- host side of the product
@pytest.fixture(scope="module")
def modal():
    from barc4dip_amd.signal import modal

    return modal


def test_modal_table_equals_the_oracle_tables(modal):
    from barc4dip_amd import signal

    assert signal.modal_table is modal.modal_table and signal.modal_fit is modal.modal_fit and signal.modal_eval is modal.modal_eval
    for J in (1, 2, 15, 66):
        assert np.array_equal(modal.modal_table("zernike", J), noll_table(J))
        assert np.array_equal(modal.modal_table("legendre", J), legendre_table(J))
    assert modal.modal_table("zernike", 15).shape == (15, 2)


def test_argument_errors_raise_before_the_gpu_is_touched(modal, monkeypatch):
    from barc4dip_amd import _ffi

    def no_gpu():
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_ffi, "require_gpu", no_gpu)
    z = np.zeros((8, 9), np.float32)
    bad = [
        (ValueError, dict(basis="chebyshev")), (ValueError, dict(basis=0)), (ValueError, dict(n_modes=0)),
        (ValueError, dict(n_modes=2.5)), (ValueError, dict(n_modes=True)), (NotImplementedError, dict(n_modes=67)),
        (ValueError, dict(n_modes=6, remove=(1, 7))), (ValueError, dict(n_modes=6, remove=(0,))), (ValueError, dict(remove="tilt")),
        (ValueError, dict(remove=3)), (ValueError, dict(fill="harmonic")), (ValueError, dict(weights=np.ones((9, 8)))),
        (ValueError, dict(mask=np.ones((2, 8, 9), bool))), (ValueError, dict(weights="peak")), (ValueError, dict(dy=0.0)),
        (ValueError, dict(dx=np.nan)), (ValueError, dict(radius=-1.0)), (ValueError, dict(center=(1.0,))),
        (ValueError, dict(center=(np.inf, 0.0))), (ValueError, dict(basis="legendre", center=(3.5, 4.0))),
    ]
    for exc, kw in bad:
        with pytest.raises(exc):
            modal.modal_fit(z, **kw)
    with pytest.raises(_ffi.B4DSizeError):
        modal.modal_fit(np.zeros((1, 2049), np.float32))
    with pytest.raises(NotImplementedError):            # B4DSizeError is one
        modal.modal_fit(np.zeros((2049, 1), np.float32), radius=1.0)
    for shape in ((1, 9), (9, 1), (1, 1)):              # the inscribed circle of a side of 1 has no radius
        with pytest.raises(ValueError, match="radius"):
            modal.modal_fit(np.zeros(shape, np.float32))
    for arr in (np.zeros(5, np.float32), np.zeros((2, 2, 3, 3), np.float32), np.zeros((0, 4), np.float32)):
        with pytest.raises(ValueError):
            modal.modal_fit(arr)
    with pytest.raises(ValueError, match="wavefront"):
        modal.modal_fit({"y": np.arange(8.0), "x": np.arange(9.0)})
    for exc, args, kw in [(ValueError, (np.zeros(6), (8, 9)), dict(basis="fourier")), (NotImplementedError, (np.zeros(67), (8, 9)), {}),
                          (ValueError, (np.zeros((2, 2, 6)), (8, 9)), {}), (ValueError, (np.zeros(6), (8,)), {}),
                          (ValueError, (np.zeros(6), (0, 9)), {}), (_ffi.B4DSizeError, (np.zeros(6), (8, 4096)), {}),
                          (ValueError, (np.zeros(6), (1, 9)), {}), (ValueError, (np.zeros(6), (8, 9)), dict(basis="legendre", center=(1, 1)))]:
        with pytest.raises(exc):
            modal.modal_eval(*args, **kw)
    for exc, args in [(ValueError, ("noll", 3)), (ValueError, ("zernike", 0)), (NotImplementedError, ("legendre", 67))]:
        with pytest.raises(exc):
            modal.modal_table(*args)


def test_no_host_fallback(modal):
    import torch

    from barc4dip_amd import _ffi

    z = np.zeros((8, 9), np.float32)
    if torch.cuda.is_available():       # with a GPU the same calls compute (tests/test_gpu_modal.py)
        return
    for call in (lambda: modal.modal_fit(z), lambda: modal.modal_fit(z, basis="legendre", n_modes=6, mask=z == 0),
                 lambda: modal.modal_eval(np.ones(6), (8, 9)), lambda: modal.modal_eval(np.ones((2, 6)), (8, 9), basis="legendre")):
        with pytest.raises(_ffi.B4DUnavailable):
            call()
