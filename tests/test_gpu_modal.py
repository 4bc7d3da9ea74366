"""Modal fits on the MI355X (b4d_modal_fit, b4d_modal_residual, b4d_modal_eval, barc4dip_amd/signal/modal.py) against the float64
oracle of tests/test_modal_host.py.  Maps are float32; the error of a coefficient vector is max|c - c_ref| / max|c_ref|.

Bars.  Coefficients: 1e-12, the project's bar for a float64 fit against a float64 oracle on the same float32 map; every parity
case asserts that the normalised Gram matrix of the oracle has a condition number below 1e2, so that 2^-53 times the condition is
four orders below the bar.  Residual map against the oracle's float64 residual rounded to float32: 2^-23 max|ref residual| +
1e-13 max|phi| (one float32 rounding each way plus the float64 error of the synthesis).  rms: 2^-23 relative wherever the
oracle's rms is above 1e-10 max|phi|; below that as many modes are kept as there are valid nodes, the residual is rounding noise
of 1e-16 max|phi|, a relative bar would measure nothing, and the rms is held to the 1e-13 max|phi| that the residual values it is
taken from are allowed.  `kept`, `valid` and the
NaN positions are equal exactly.  Observed maxima on an MI355X are listed in DESIGN.md section 15."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from test_modal_host import DEGENERATE, degenerate_case, design, fit_oracle, geometry, smooth_map
from test_wavefront_weighted_host import PATTERNS, weight_pattern

pytestmark = pytest.mark.gpu

COEFF_BAR = 1e-12
EPS32 = 2.0 ** -23
DISC_PATTERNS = tuple(p for p in PATTERNS if p.startswith("disc"))
GAP_PATTERNS = tuple(p for p in PATTERNS if p.startswith("gap"))
assert len(DISC_PATTERNS) == 3 and len(GAP_PATTERNS) == 2


@pytest.fixture(scope="module")
def modal():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import modal

    return modal


@functools.lru_cache(maxsize=None)
def _design66(shape, basis, geo):
    """All 66 modes of a geometry, computed once: the modes do not depend on how many are fitted."""
    A, ap = design(shape, basis, 66, **dict(geo))
    A.setflags(write=False)
    ap.setflags(write=False)
    return A, ap


def _design(shape, basis, J, geo=None):
    A, ap = _design66(tuple(shape), basis, tuple(sorted((geo or {}).items())))
    return A[..., :J], ap


def _weights(pattern, shape, seed=0):
    return weight_pattern(pattern, shape, seed).astype(np.float32)


def _compare(observe, name, got, t, phi, w, A, ap, remove="all", fill="nan"):
    """Map t of the result `got` against the oracle for the single map phi with weights w."""
    ref = fit_oracle(phi, w, A, ap, remove, fill)
    if ref["kept"].any():
        assert ref["cond"] < 1e2, f"{name}: condition {ref['cond']:.3g} of the oracle's normalised Gram matrix"
    np.testing.assert_array_equal(got["kept"][t], ref["kept"], err_msg=name)
    np.testing.assert_array_equal(got["valid"].reshape((-1,) + phi.shape)[t], ref["valid"], err_msg=name)
    c, cref = got["coefficients"][t], ref["coefficients"]
    assert np.all(c[~ref["kept"]] == 0.0)
    scale = np.max(np.abs(cref))
    err = float(np.max(np.abs(c - cref)) / scale) if scale > 0 else float(np.max(np.abs(c)))
    print(f"{name}: coefficients {err:.3e}")
    observe("modal/coefficients", err, COEFF_BAR)
    r, rref = got["residual"].reshape((-1,) + phi.shape)[t], ref["residual"].astype(np.float64)
    np.testing.assert_array_equal(np.isnan(r), np.isnan(rref), err_msg=name)
    fin = np.isfinite(rref)
    if fin.any():
        bar = EPS32 * np.max(np.abs(rref[fin])) + 1e-13 * np.max(np.abs(phi[np.isfinite(phi)]))
        d = float(np.max(np.abs(r[fin] - rref[fin])))
        print(f"{name}: residual {d:.3e} of bar {bar:.3e}")
        observe("modal/residual_over_bar", d / bar, 1.0)
    if np.isnan(ref["rms"]):
        assert np.isnan(got["rms"][t])
    else:
        e, top = abs(got["rms"][t] - ref["rms"]), np.max(np.abs(phi[np.isfinite(phi)]))
        if ref["rms"] > 1e-10 * top:
            print(f"{name}: rms {e / ref['rms']:.3e} relative")
            observe("modal/rms", e / ref["rms"], EPS32)
        else:       # an interpolating fit: the residual is rounding noise, held to the absolute term of the residual bar
            print(f"{name}: rms {e:.3e} absolute (rms {ref['rms']:.3e})")
            observe("modal/rms_of_noise_over_bar", e / (1e-13 * top), 1.0)
    return ref


def _fit_and_compare(observe, modal, name, phi, w, basis, J, geo=None, **kw):
    geo = geo or {}
    A, ap = _design(phi.shape[-2:], basis, J, geo)
    got = modal.modal_fit(phi, basis=basis, n_modes=J, weights=w, **geo, **kw)
    maps = phi.reshape((-1,) + phi.shape[-2:])
    assert got["coefficients"].shape == (len(maps), J) and got["coefficients"].dtype == np.float64
    assert got["kept"].dtype == bool and got["rms"].shape == (len(maps),) and got["residual"].shape == phi.shape
    assert got["valid"].shape == phi.shape and got["valid"].dtype == bool and got["residual"].dtype == np.float64
    for t, m in enumerate(maps):
        wt = None if w is None else (w if np.ndim(w) == 2 else w[t])
        _compare(observe, f"{name}[{t}]", got, t, m, wt, A, ap, kw.get("remove", "all"), kw.get("fill", "nan"))
    return got


# ---- parity
@pytest.mark.parametrize("basis,shape,J,radius", DEGENERATE)
def test_parity_degenerate(observe, modal, basis, shape, J, radius):
    phi, A, ap, geo = degenerate_case(basis, shape, J, radius)
    got = modal.modal_fit(phi, basis=basis, n_modes=J, **geo)
    # singular by construction: the condition bound holds on the kept modes, and the gap of the drop rule is asserted in
    # tests/test_modal_host.py
    ref = _compare(observe, f"degenerate/{basis}/{shape}", got, 0, phi, None, A, ap)
    assert not ref["kept"].all()
    if (basis, shape) == ("zernike", (5, 5)):
        assert int(ref["valid"].sum()) == 13


@pytest.mark.parametrize("basis", ["zernike", "legendre"])
def test_parity_batch(observe, modal, basis):
    shape, T, J = (7, 9), 3, 10
    rng = np.random.default_rng(5)
    phi = np.stack([smooth_map(shape, 20 + t) for t in range(T)])
    w = rng.uniform(0.2, 1.0, (T,) + shape).astype(np.float32)
    w[0, 2, 3] = w[1, 0, 0] = w[2, 6, 8] = 0.0
    _fit_and_compare(observe, modal, f"batch/{basis}/per_map", phi, w, basis, J)
    _fit_and_compare(observe, modal, f"batch/{basis}/shared", phi, w[1], basis, J)


@pytest.mark.parametrize("shape,J", [((23, 31), 36), ((37, 53), 66)])
@pytest.mark.parametrize("basis,pattern", [("zernike", p) for p in DISC_PATTERNS] + [("legendre", p) for p in GAP_PATTERNS])
def test_parity_patterns(observe, modal, basis, pattern, shape, J):
    _fit_and_compare(observe, modal, f"patterns/{basis}/{shape}/{pattern}", smooth_map(shape, 31), _weights(pattern, shape), basis, J)


@pytest.mark.parametrize("J", [1, 2, 15, 16, 17, 32, 33, 48, 49, 65, 66])
@pytest.mark.parametrize("basis,pattern", [("zernike", "disc_holes"), ("legendre", "gap_graded")])
def test_parity_tile_boundaries(observe, modal, basis, pattern, J):
    shape = (23, 31)
    _fit_and_compare(observe, modal, f"tiles/{basis}/J{J}", smooth_map(shape, 41), _weights(pattern, shape), basis, J)


@pytest.mark.parametrize("shape,J", [((130, 141), 66), ((300, 517), 17), ((300, 517), 66)])
def test_parity_chunk_boundaries(observe, modal, shape, J):
    """Several chunks, node counts that are no multiple of any tile."""
    _fit_and_compare(observe, modal, f"chunks/{shape}/J{J}", smooth_map(shape, 51), _weights("disc_holes", shape), "zernike", J)


GEO = dict(dy=0.7, dx=1.9, center=(17.3, 25.6), radius=14.0)


def test_geometry(observe, modal):
    shape = (37, 53)
    u, v, _ = geometry(shape, "zernike", **GEO)
    rho2 = u * u + v * v
    close = np.abs(rho2 - (1.0 + 1e-9)) < 1e-6
    assert not np.any(close & (rho2 != 1.0)), "a node of the test grid sits on the edge rule"
    assert 0.2 < np.mean(rho2 <= 1.0) < 0.9 and rho2[0, 0] > 1.0       # the radius cuts the grid
    got = _fit_and_compare(observe, modal, "geometry", smooth_map(shape, 61), None, "zernike", 21, GEO)
    assert got["center"] == GEO["center"] and got["radius"] == GEO["radius"] and got["basis"] == "zernike"


# ---- semantics
def test_non_finite_values_are_excluded_and_never_read(observe, modal):
    shape, J = (23, 31), 15
    phi, w = smooth_map(shape, 71), _weights("disc_graded", shape)
    inside = np.argwhere(w > 0)
    bad = phi.copy()
    for k, val in enumerate((np.nan, np.inf, -np.inf)):
        bad[tuple(inside[7 + 13 * k])] = val
    got = _fit_and_compare(observe, modal, "semantics/non_finite", bad, w, "zernike", J)
    assert not got["valid"][tuple(inside[7])] and np.isnan(got["residual"][tuple(inside[7])])
    # NaN at weight-0 nodes: the same bits as the map with those nodes zeroed
    poisoned, zeroed = phi.copy(), phi.copy()
    poisoned[w == 0], zeroed[w == 0] = np.nan, 0.0
    a = modal.modal_fit(poisoned, n_modes=J, weights=w)
    b = modal.modal_fit(zeroed, n_modes=J, weights=w)
    for k in ("coefficients", "kept", "rms", "valid", "residual"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # a fill="nan" wavefront needs no mask: the NaN nodes are the mask
    c = modal.modal_fit(np.where(w > 0, phi, np.nan).astype(np.float32), n_modes=J)
    d = modal.modal_fit(phi, n_modes=J, mask=w > 0)
    for k in ("coefficients", "kept", "rms", "valid", "residual"):
        np.testing.assert_array_equal(c[k], d[k], err_msg=k)


def test_remove_and_fill(observe, modal):
    shape, J = (23, 31), 15
    phi, w = smooth_map(shape, 81), _weights("disc_holes", shape)
    A, ap = _design(shape, "zernike", J)
    none = _fit_and_compare(observe, modal, "semantics/remove_none", phi, w, "zernike", J, remove=None)
    v = none["valid"]
    np.testing.assert_array_equal(none["residual"][v], phi[v].astype(np.float64))
    part = _fit_and_compare(observe, modal, "semantics/remove_123", phi, w, "zernike", J, remove=(1, 2, 3))
    full = modal.modal_fit(phi, n_modes=J, weights=w)
    np.testing.assert_array_equal(part["coefficients"], full["coefficients"])
    rest = full["coefficients"][0].copy()
    rest[:3] = 0.0
    synth = modal.modal_eval(rest, shape)
    d = np.max(np.abs((part["residual"] - full["residual"])[v] - synth[v]))
    observe("modal/remove_subset", d / np.max(np.abs(phi)), EPS32)
    # outside the disc and at the holes: NaN, or the extension
    assert np.all(np.isnan(full["residual"][~v])) and not np.any(np.isnan(full["residual"][v])) and not ap.all()
    ext = _fit_and_compare(observe, modal, "semantics/extend", phi, w, "zernike", J, fill="extend")
    assert np.all(np.isfinite(ext["residual"])) and np.array_equal(ext["valid"], v)
    np.testing.assert_array_equal(ext["residual"][v], full["residual"][v])
    np.testing.assert_array_equal(ext["coefficients"], full["coefficients"])


def test_zero_and_scaled_weights(observe, modal):
    shape, J = (23, 31), 15
    phi = smooth_map(shape, 91)
    # each basis on the apertures it is conditioned for: Legendre products on a disc reach a condition number of 1e6
    for basis, pattern in (("zernike", "disc_graded"), ("legendre", "gap_graded")):
        w = (np.round(_weights(pattern, shape) * 1024.0) / 1024.0).astype(np.float32)    # 10 bits: 1000 w is exact in float32
        assert np.array_equal((1000.0 * w).astype(np.float32).astype(np.float64), 1000.0 * w.astype(np.float64))
        z = modal.modal_fit(phi, basis=basis, n_modes=J, weights=np.zeros(shape, np.float32))
        assert np.all(z["coefficients"] == 0.0) and not z["kept"].any() and np.isnan(z["rms"][0]) and not z["valid"].any()
        assert np.all(np.isnan(z["residual"]))
        a = modal.modal_fit(phi, basis=basis, n_modes=J, weights=w)
        b = modal.modal_fit(phi, basis=basis, n_modes=J, weights=1000.0 * w)
        scale = np.max(np.abs(a["coefficients"]))
        observe("modal/weights_x1000", np.max(np.abs(a["coefficients"] - b["coefficients"])) / scale, COEFF_BAR)


# ---- synthesis and round trip
def test_round_trip(observe, modal):
    shape, J = (64, 64), 36
    c = np.random.default_rng(101).normal(size=J)
    A, ap = _design(shape, "zernike", J)
    m = modal.modal_eval(c, shape)
    assert m.shape == shape and m.dtype == np.float64
    want = A @ c
    top = np.max(np.abs(want[ap]))
    observe("modal/eval", np.max(np.abs(m - want)[ap]) / top, EPS32)
    m32 = m.astype(np.float32)                  # exact: the device stored float32
    bar = 4.0 * 2.0 ** -24 * np.max(np.abs(m32[ap]))
    ref = fit_oracle(m32, None, A, ap)
    assert np.max(np.abs(ref["coefficients"] - c)) <= bar, "the oracle alone leaves the round-trip bar"
    got = modal.modal_fit(m32, n_modes=J)
    assert got["kept"].all()
    observe("modal/round_trip_over_bar", np.max(np.abs(got["coefficients"][0] - c)) / bar, 1.0)
    # a batch of coefficient vectors, Legendre, device tensors
    import torch

    cs = np.random.default_rng(102).normal(size=(3, 10))
    AL, _ = _design((19, 33), "legendre", 10)
    mt = modal.modal_eval(torch.from_numpy(cs).cuda(), (19, 33), basis="legendre", return_tensors=True)
    assert mt.is_cuda and mt.dtype == torch.float32 and tuple(mt.shape) == (3, 19, 33)
    wantL = AL @ cs.T
    observe("modal/eval", np.max(np.abs(np.moveaxis(mt.cpu().numpy(), 0, -1) - wantL)) / np.max(np.abs(wantL)), EPS32)


# ---- agreement with the 6-term quadratic fit
def test_legendre_six_is_the_quadratic_fit(observe, modal):
    from barc4dip_amd.signal import wavefront as wf
    from test_wavefront_host import smooth_slopes

    shape = (37, 53)
    gy, gx = smooth_slopes(shape, 16.0, 16.0, 3)
    field = {"dy": gy.astype(np.float32), "dx": gx.astype(np.float32), "y": 23.0 + 16.0 * np.arange(shape[0]),
             "x": 23.0 + 16.0 * np.arange(shape[1])}
    M = weight_pattern("disc_holes", shape) > 0
    kw = dict(pixel_size=6.5e-6, distance=0.75, mask=M)
    w0 = wf.wavefront_from_displacement(field, remove=None, **kw)
    wq = wf.wavefront_from_displacement(field, remove="quadratic", **kw)
    got = modal.modal_fit(w0, basis="legendre", n_modes=6)
    np.testing.assert_array_equal(got["valid"], M)
    top = np.max(np.abs(w0["wavefront"][M]))
    observe("modal/vs_quadratic", np.max(np.abs(got["residual"] - wq["wavefront"])[M]) / top, 2.0 ** -22)
    assert got["radius"] is None and got["kept"].all()


# ---- determinism
def test_determinism_and_input_forms(modal):
    import torch

    shape, T, J = (130, 141), 5, 36
    phi = np.stack([smooth_map(shape, 200 + t) for t in range(T)])
    w = np.stack([_weights("disc_graded", shape, t) for t in range(T)])
    keys = ("coefficients", "kept", "rms", "valid", "residual")
    a = modal.modal_fit(phi, n_modes=J, weights=w)
    b = modal.modal_fit(phi, n_modes=J, weights=w)
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for t in (0, 3):
        one = modal.modal_fit(phi[t], n_modes=J, weights=w[t])
        for k in keys:
            np.testing.assert_array_equal(one[k].reshape(a[k][t].shape), a[k][t], err_msg=f"map {t} alone: {k}")
    shared = modal.modal_fit(phi, n_modes=J, weights=w[2])
    one = modal.modal_fit(phi[4], n_modes=J, weights=w[2])
    np.testing.assert_array_equal(one["coefficients"][0], shared["coefficients"][4])
    np.testing.assert_array_equal(one["residual"], shared["residual"][4])
    # float64, non-contiguous and device inputs give what their float32 contiguous copy gives
    big = np.zeros((T, shape[0], 2 * shape[1]))
    big[:, :, ::2] = phi
    for form in (phi.astype(np.float64), big[:, :, ::2], np.asfortranarray(phi), torch.from_numpy(phi).cuda()):
        c = modal.modal_fit(form, n_modes=J, weights=w)
        for k in keys:
            np.testing.assert_array_equal(c[k], a[k], err_msg=k)
    t = modal.modal_fit(torch.from_numpy(phi).cuda(), n_modes=J, weights=torch.from_numpy(w).cuda(), return_tensors=True)
    assert t["residual"].is_cuda and t["residual"].dtype == torch.float32 and t["valid"].dtype == torch.bool
    np.testing.assert_array_equal(t["residual"].cpu().numpy().astype(np.float64), a["residual"])
    np.testing.assert_array_equal(t["valid"].cpu().numpy(), a["valid"])
