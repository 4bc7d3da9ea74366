"""Weighted / masked wavefront integration on the MI355X (b4d_integrate_gradient_weighted, b4d_poly2_fit_weighted,
barc4dip_amd/signal/wavefront.py) against the float64 oracles of tests/test_wavefront_weighted_host.py.
Errors are max|got - ref| / ptp(ref) per map, the reference integrate_weighted_np at the same rtol = 1e-6.

Bars: 2 x the maximum observed on an MI355X.  Next to its bar every parity case is held against what the
same iteration gives with float32 vectors in NumPy (integrate_weighted_pcg32) on the same input: more than 4 x that (floor
4 x 2^-24) is a bug, not a tolerance.  The direct fit test compares two float64 computations on the same float32 map, so its
observations sit at rounding level (coefficients 4e-15, residual map 1.6e-8, rms 2.5e-9) where twice the observation would
measure the LAPACK of the test machine; those three bars are held at the rounding of what is compared instead: 1e-12 for the
coefficients (2^-53 times the condition of the 6 x 6 normal equations, below 1e4 on these node sets), 2^-24 for the float32
residual map and for the rms taken from it."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

from barc4dip_amd import synth
from test_wavefront_host import MONOMIALS, integrate_np, smooth_slopes
from test_wavefront_weighted_host import (PATTERNS, effective_weights, integrate_weighted_np, integrate_weighted_pcg32,
                                          poly2_weighted_np, wavefront_weighted_np, weight_pattern)

pytestmark = pytest.mark.gpu

HY, HX = 0.7, 1.9
BARS = {    # 2 x the observed maximum on MI355X (fit_*: the rounding floors of the module docstring)
    "wwf/1x5": 5.9e-08, "wwf/5x1": 7.0e-08, "wwf/2x2": 9.8e-08, "wwf/2x3": 9.3e-08, "wwf/7x9_per_map": 3.2e-06, "wwf/7x9_shared": 4.0e-06,
    "wwf/23x31_disc": 4.2e-07, "wwf/23x31_disc_holes": 5.3e-07, "wwf/23x31_gap": 3.8e-07, "wwf/23x31_gap_graded": 1.2e-06,
    "wwf/23x31_disc_graded": 6.7e-07,
    "wwf/37x53_disc": 4.3e-07, "wwf/37x53_disc_holes": 9.6e-07, "wwf/37x53_gap": 3.5e-07, "wwf/37x53_gap_graded": 1.1e-06,
    "wwf/37x53_disc_graded": 7.7e-07,
    "wwf/130x141_disc_holes": 1.5e-06, "wwf/300x517_disc_holes": 2.1e-06,
    "wwf/mean": 2.9e-08, "wwf/all_ones_vs_unweighted": 1.3e-06, "wwf/weights_x1000": 1.1e-06,
    "wwf/fit_coefficients": 1.0e-12, "wwf/fit_rms": 6.0e-08, "wwf/fit_map": 6.0e-08,
    "wwf/chain_coefficients": 1.1e-07, "wwf/chain_rms": 3.2e-07, "wwf/chain_map": 5.3e-06,
    # condition on every parity bar: error <= 4 x integrate_weighted_pcg32's on the same input (floor 4 x 2^-24)
    "wwf/vs_pcg32": 4.0,
}
PCG32_FLOOR = 4.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def wf():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import wavefront

    return wavefront


def _err(got, ref, sel=None):
    d = np.abs(got - ref)
    return float(np.max(d if sel is None else d[sel]) / np.ptp(ref))


def _slopes(shape, seed):
    gy, gx = smooth_slopes(shape, HY, HX, seed)
    return gy.astype(np.float32), gx.astype(np.float32)      # what the device receives


def _weights(pattern, shape, seed=0):
    return weight_pattern(pattern, shape, seed).astype(np.float32)


def _small_mask(shape):
    m = np.ones(shape, bool)
    m[{(1, 5): (0, 2), (5, 1): (2, 0), (2, 2): (0, 1), (2, 3): (0, 1)}[shape]] = False
    return m


def _check_parity(wf, observe, key, gy, gx, w, **kw):
    """gy, gx (T, ny, nx) float32; w (ny, nx) shared or (T, ny, nx); both fills against the float64 iteration."""
    T = gy.shape[0]
    wt = np.broadcast_to(w, gy.shape) if w.ndim == 2 else w
    full, info = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, fill="harmonic", return_info=True, **kw)
    holes = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, **kw)                       # fill="nan" is the default
    assert full.dtype == np.float64 and full.shape == gy.shape and holes.shape == gy.shape
    assert info["iterations"].shape == (T,) and info["residual"].shape == (T,) and np.all(info["converged"])
    for t in range(T):
        we = effective_weights(wt[t], gy[t], gx[t])
        ref, it, res = integrate_weighted_np(gy[t], gx[t], we, HY, HX, return_info=True)
        assert it < 500 and res <= 1e-6
        e32 = _err(integrate_weighted_pcg32(gy[t], gx[t], we, HY, HX), ref)
        e = _err(full[t], ref)
        np.testing.assert_array_equal(np.isnan(holes[t]), we == 0)                   # NaN exactly at the weight-0 nodes
        ev = _err(holes[t], ref, we > 0)
        print(f"{key}[{t}]: whole grid {e:.3e}, valid nodes {ev:.3e}, pcg32 {e32:.3e}, iterations {info['iterations'][t]} "
              f"(float64 {it}), residual {info['residual'][t]:.2e}, |mean| {abs(full[t].mean()) / np.ptp(ref):.2e}")
        observe("wwf/vs_pcg32", e / max(e32, PCG32_FLOOR), BARS["wwf/vs_pcg32"])
        observe(key, e, BARS[key])
        observe(key, ev, BARS[key])
        observe("wwf/mean", abs(full[t].mean()) / np.ptp(ref), BARS["wwf/mean"])


# ---- parity
@pytest.mark.parametrize("shape", [(1, 5), (5, 1), (2, 2), (2, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_degenerate_grids(wf, shape, observe):
    """One node masked: on (1, 5) and (5, 1) that leaves two pieces on a side of one node."""
    gy, gx = _slopes(shape, 5)
    m = _small_mask(shape)
    _check_parity(wf, observe, f"wwf/{shape[0]}x{shape[1]}", gy[None], gx[None], m.astype(np.float32), mask=m)


@pytest.mark.parametrize("shared", [False, True], ids=["per_map", "shared"])
def test_parity_batch_7x9(wf, shared, observe):
    """T = 3 with different data per map; different weights per map (a wrong weight stride shows), then one shared map (stride 0)."""
    maps = [_slopes((7, 9), 11 + t) for t in range(3)]
    gy, gx = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    w = _weights("disc_holes", (7, 9)) if shared else np.stack([_weights(p, (7, 9), t) for t, p in
                                                               enumerate(("disc_holes", "gap_graded", "disc_graded"))])
    _check_parity(wf, observe, "wwf/7x9_shared" if shared else "wwf/7x9_per_map", gy, gx, w, weights=w)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [(23, 31), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_patterns(wf, shape, pattern, observe):
    gy, gx = _slopes(shape, 7)
    w = _weights(pattern, shape, 7)
    _check_parity(wf, observe, f"wwf/{shape[0]}x{shape[1]}_{pattern}", gy[None], gx[None], w, weights=w)


@pytest.mark.parametrize("shape", [(130, 141), (300, 517)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_across_tiles(wf, shape, observe):
    """Sides beyond the 128-node product tiles and several workgroups' partial sums per map."""
    gy, gx = _slopes(shape, 9)
    w = _weights("disc_holes", shape, 9)
    _check_parity(wf, observe, f"wwf/{shape[0]}x{shape[1]}_disc_holes", gy[None], gx[None], w, weights=w)


# ---- behaviour
def test_all_ones_is_the_unweighted_route(wf, observe):
    """Exact arithmetic needs one iteration (the preconditioner is the inverse).  At (7, 9) float32 does too; from (23, 31) on
    the float32 rounding of the first residual lies above rtol = 1e-6 (1.5e-6 ... 5e-6 of |b| in the NumPy emulation), so a second
    iteration runs there, as it does in integrate_weighted_pcg32."""
    for shape, most in (((7, 9), 1), ((37, 53), 2)):
        gy, gx = _slopes(shape, 3)
        got, info = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=np.ones(shape), return_info=True)
        plain = wf.integrate_gradient(gy, gx, dy=HY, dx=HX)
        print(f"all ones {shape}: iterations {info['iterations'][0]}, against the unweighted route {_err(got, plain):.3e}")
        assert info["iterations"][0] <= most and info["iterations"][0] >= 1 and info["converged"][0]
        if most == 1:
            assert info["iterations"][0] == 1
        observe("wwf/all_ones_vs_unweighted", _err(got, plain), BARS["wwf/all_ones_vs_unweighted"])


def test_nan_slopes_under_the_mask_do_not_leak(wf):
    gy, gx = _slopes((23, 31), 7)
    m = _weights("disc_holes", (23, 31), 7) > 0
    want = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, mask=m, fill="harmonic")
    gy2, gx2 = gy.copy(), gx.copy()
    gy2[~m], gx2[~m] = np.nan, np.inf
    got = wf.integrate_gradient(gy2, gx2, dy=HY, dx=HX, mask=m, fill="harmonic")
    assert np.all(np.isfinite(got))
    np.testing.assert_array_equal(got, want)


def test_nan_slopes_mask_themselves(wf):
    gy, gx = _slopes((23, 31), 7)
    m = _weights("disc_holes", (23, 31), 7) > 0
    gy2, gx2 = gy.copy(), gx.copy()
    gy2[~m] = np.nan
    gx2[~m & (np.arange(31)[None, :] % 2 == 0)] = -np.inf
    for fill in ("nan", "harmonic"):
        want = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=np.ones((23, 31)), mask=m, fill=fill)
        got = wf.integrate_gradient(gy2, gx2, dy=HY, dx=HX, weights=np.ones((23, 31)), fill=fill)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(np.isnan(got), ~m if fill == "nan" else np.zeros_like(m))


@pytest.fixture(scope="module")
def batch():
    """Three (23, 31) maps with weights of their own, and what the device returns for them as one batch."""
    maps = [_slopes((23, 31), 21 + t) for t in range(3)]
    gy, gx = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    w = np.stack([_weights(p, (23, 31), t) for t, p in enumerate(("disc_holes", "gap_graded", "disc_graded"))])
    return gy, gx, w


def test_alone_in_a_batch_and_repeated_calls_agree_bitwise(wf, batch):
    gy, gx, w = batch
    full, info = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w, fill="harmonic", return_info=True)
    again, info2 = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w, fill="harmonic", return_info=True)
    np.testing.assert_array_equal(again, full)
    np.testing.assert_array_equal(info2["iterations"], info["iterations"])
    np.testing.assert_array_equal(info2["residual"], info["residual"])
    assert len(set(info["iterations"].tolist())) > 1, "the maps should stop at different iterations for this test to bite"
    for t in range(3):
        one, i1 = wf.integrate_gradient(gy[t:t + 1], gx[t:t + 1], dy=HY, dx=HX, weights=w[t:t + 1], fill="harmonic", return_info=True)
        two = wf.integrate_gradient(gy[t], gx[t], dy=HY, dx=HX, weights=w[t], fill="harmonic")
        assert one.shape == (1, 23, 31) and two.shape == (23, 31)
        np.testing.assert_array_equal(one[0], full[t])
        np.testing.assert_array_equal(two, full[t])
        assert i1["iterations"][0] == info["iterations"][t] and i1["residual"][0] == info["residual"][t]


def test_zero_weight_and_zero_slope_maps_in_a_batch(wf, batch):
    gy, gx, w = batch
    gy, gx, w = gy.copy(), gx.copy(), w.copy()
    w[0] = 0.0                    # nothing valid
    gy[1], gx[1] = 0.0, 0.0       # nothing to integrate
    alone = wf.integrate_gradient(gy[2], gx[2], dy=HY, dx=HX, weights=w[2])
    got, info = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w, return_info=True)
    assert np.all(np.isnan(got[0])) and info["iterations"][0] == 0 and info["converged"][0] and info["residual"][0] == 0.0
    assert np.all(got[1][w[1] > 0] == 0.0) and np.all(np.isnan(got[1][w[1] == 0])) and info["iterations"][1] == 0
    np.testing.assert_array_equal(got[2], alone)
    filled = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w, fill="harmonic")
    assert np.all(filled[0] == 0.0) and np.all(filled[1] == 0.0)


def test_scale_of_the_weights(wf, observe):
    gy, gx = _slopes((37, 53), 7)
    w = _weights("disc_graded", (37, 53), 7)
    a = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w, fill="harmonic")
    b = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=1000.0 * w.astype(np.float64), fill="harmonic")
    print(f"weights x 1000: {_err(b, a):.3e}")
    observe("wwf/weights_x1000", _err(b, a), BARS["wwf/weights_x1000"])


def test_max_iter_reached_warns_and_returns(wf):
    gy, gx = _slopes((37, 53), 7)
    w = _weights("disc_graded", (37, 53), 7)
    with pytest.warns(RuntimeWarning, match="did not reach rtol"):
        got, info = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w, max_iter=3, return_info=True)
    assert not info["converged"][0] and info["iterations"][0] == 3 and info["residual"][0] > 1e-6
    assert np.all(np.isfinite(got[w > 0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w)          # the default max_iter converges silently


def test_weight_dtypes_and_layouts_agree(wf):
    import torch

    gy, gx = _slopes((23, 31), 7)
    rng = np.random.default_rng(5)
    wi = rng.integers(0, 4, (23, 31))                                    # small integers: exact in every dtype below
    want = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=wi.astype(np.float32))
    assert np.any(np.isnan(want)) and np.any(np.isfinite(want))
    big = np.zeros((46, 93))
    big[::2, ::3] = wi
    forms = [wi.astype(np.float64), wi.astype(np.int64), wi.astype(np.uint8), big[::2, ::3], np.asfortranarray(wi.astype(np.float64)),
             torch.from_numpy(wi.astype(np.float64)).cuda(), torch.from_numpy(wi).cuda()]
    assert not forms[3].flags.c_contiguous
    for w in forms:
        np.testing.assert_array_equal(wf.integrate_gradient(gy, gx, dy=HY, dx=HX, weights=w), want)
    mb = wi > 0
    wantm = wf.integrate_gradient(gy, gx, dy=HY, dx=HX, mask=mb)
    for m in (mb.astype(np.float64), mb.astype(np.int32), np.asfortranarray(mb), torch.from_numpy(mb).cuda(), wi):
        np.testing.assert_array_equal(wf.integrate_gradient(gy, gx, dy=HY, dx=HX, mask=m), wantm)
    ty, tx = torch.from_numpy(gy).cuda(), torch.from_numpy(gx).cuda()
    out = wf.integrate_gradient(ty, tx, dy=HY, dx=HX, mask=torch.from_numpy(mb).cuda(), return_tensors=True)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (23, 31)
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), wantm)


# ---- b4d_poly2_fit_weighted against poly2_weighted_np (error measures of the unweighted fit tests)
def _fit_device(phi, w, remove_mask=0b111111, scale=1.0, nan_invalid=1):
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi

    n, ny, nx = phi.shape
    tp, tw = torch.from_numpy(phi.astype(np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()
    coeff = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    rms = torch.empty((n,), dtype=torch.float64, device="cuda")
    res = torch.empty_like(tp)
    stride = ny * nx if w.ndim == 3 else 0
    _ffi.check(_ffi.lib().b4d_poly2_fit_weighted(D.ptr(tp), D.ptr(tw), stride, n, ny, nx, remove_mask, scale, nan_invalid, D.ptr(coeff),
                                                 D.ptr(res), D.ptr(rms), _ffi.stream_ptr()))
    return coeff.cpu().numpy(), res.cpu().numpy().astype(np.float64), rms.cpu().numpy()


def _fit_weights(kind, shape):
    w = np.zeros(shape, np.float32)
    if kind == "disc":
        return _weights("disc", shape)
    if kind == "graded":
        return _weights("disc_graded", shape, 3)
    if kind == "single_row":
        w[5, :] = 1.0                   # v is constant and not 0 on it: the v terms repeat 1, u and u^2
    elif kind == "five_nodes":
        w[[2, 5, 9, 17, 20], [3, 25, 14, 7, 28]] = [1.0, 0.5, 2.0, 1.0, 0.25]
    elif kind == "three_nodes":
        w[[4, 12, 19], [6, 22, 11]] = 1.0
    return w


@pytest.mark.parametrize("kind", ["disc", "graded", "single_row", "five_nodes", "three_nodes"])
def test_weighted_fit_against_the_oracle(kind, observe):
    shape = (23, 31)
    gy, gx = _slopes(shape, 13)
    phi = integrate_np(gy, gx, HY, HX).astype(np.float32)
    w = _fit_weights(kind, shape)
    stack = np.stack([phi, 0.5 * phi[::-1, ::-1] + 0.1])                # two maps, shared weights (stride 0)
    u, v = np.linspace(-1.0, 1.0, shape[1]), np.linspace(-1.0, 1.0, shape[0])      # the C ABI's normalised coordinates
    coeff, res, rms = _fit_device(np.where(w > 0, stack, np.nan), w)
    coeff_p, res_p, rms_p = _fit_device(stack, np.stack([w, w]), nan_invalid=0)   # per-map weights, no NaN: same fit
    np.testing.assert_array_equal(coeff_p, coeff)
    for t in range(2):
        c, a = poly2_weighted_np(stack[t].astype(np.float64), w, v, u)
        want = stack[t].astype(np.float64) - (a @ c).reshape(shape)
        ww = w.astype(np.float64)
        m = np.sum(ww * want) / np.sum(ww)
        want_rms = np.sqrt(max(0.0, np.sum(ww * want ** 2) / np.sum(ww) - m * m))
        span = np.ptp(stack[t][w > 0])
        np.testing.assert_array_equal(np.isnan(res[t]), w == 0)
        assert np.all(np.isfinite(res_p[t]))
        np.testing.assert_array_equal(res_p[t][w > 0], res[t][w > 0])
        if kind in ("single_row", "five_nodes", "three_nodes"):
            dropped = {"single_row": [2, 4, 5], "five_nodes": [5], "three_nodes": [3, 4, 5]}[kind]
            assert np.all(coeff[t][dropped] == 0.0) and np.all(c[dropped] == 0.0), (coeff[t], c)
        figs = {"fit_coefficients": np.max(np.abs(coeff[t] - c)) / span,          # |u|, |v| <= 1: a coefficient is a height at the edge
                "fit_map": float(np.max(np.abs(res[t] - want)[w > 0]) / span)}
        if want_rms > 1e-6 * span:                                                 # an interpolating fit leaves rounding only
            figs["fit_rms"] = abs(rms[t] / want_rms - 1.0)
        else:
            assert rms[t] <= 1e-5 * span
        print(f"weighted fit {kind}[{t}]: " + ", ".join(f"{k} {x:.3e}" for k, x in figs.items()))
        for k, x in figs.items():
            observe("wwf/" + k, x, BARS["wwf/" + k])


def test_weighted_fit_of_an_empty_map():
    phi = np.ones((1, 7, 9), np.float32)
    coeff, res, rms = _fit_device(phi, np.zeros((7, 9), np.float32))
    assert np.all(coeff == 0.0) and np.all(np.isnan(res)) and np.isnan(rms[0])


# ---- wavefront_from_displacement with weights against the oracle chain
def test_wavefront_chain_with_weights(wf, observe):
    from test_gpu_wavefront import _grid_field

    import torch

    kw = dict(pixel_size=6.5e-6, distance=0.75)
    f = _grid_field(2, 42)
    shape = f["dy"].shape[-2:]
    w = _weights("disc_graded", shape, 4)
    assert w[14, 15] > 0
    f["dy"][1, 14, 15] = np.nan                                          # a failed window in map 1 only
    f["snr"] = np.broadcast_to(w, f["dy"].shape).copy()
    for remove in (None, "quadratic"):
        ref = wavefront_weighted_np(f["dy"], f["dx"], w, f["y"], f["x"], remove=remove, **kw)
        full = wavefront_weighted_np(f["dy"], f["dx"], w, f["y"], f["x"], remove=None, **kw)
        got = wf.wavefront_from_displacement(f, weights="snr", remove=remove, wavelength=1.24e-10, **kw)
        assert got["valid"].dtype == bool and got["valid"].shape == f["dy"].shape
        np.testing.assert_array_equal(got["valid"][0], w > 0)
        want_valid = w > 0
        want_valid[14, 15] = False
        np.testing.assert_array_equal(got["valid"][1], want_valid)
        assert got["iterations"].shape == (2,) and np.all(got["converged"]) and np.all(got["residual"] <= 1e-6 * (1 + 1e-12))
        ax, ay = 0.5 * np.ptp(f["x"]) * kw["pixel_size"], 0.5 * np.ptp(f["y"]) * kw["pixel_size"]
        height = np.array([ax ** pu * ay ** pv for pu, pv in MONOMIALS])
        for t in range(2):
            v = got["valid"][t]
            np.testing.assert_array_equal(np.isnan(got["wavefront"][t]), ~v)
            np.testing.assert_array_equal(np.isnan(got["phase"][t]), ~v)
            span = np.ptp(full["wavefront"][t][v])
            figs = {"chain_coefficients": np.max(np.abs(got["coefficients"][t] - ref["coefficients"][t]) * height) / span,
                    "chain_rms": abs(got["rms"][t] / ref["rms"][t] - 1.0),
                    "chain_map": float(np.max(np.abs(got["wavefront"][t] - ref["wavefront"][t])[v]) / np.ptp(ref["wavefront"][t][v]))}
            print(f"weighted chain remove={remove} t={t}: " + ", ".join(f"{k} {x:.3e}" for k, x in figs.items()))
            for k, x in figs.items():
                observe("wwf/" + k, x, BARS["wwf/" + k])
            np.testing.assert_allclose(got["phase"][t][v], 2 * np.pi * got["wavefront"][t][v] / 1.24e-10, rtol=1e-5)
    # harmonic fill and device tensors: the same numbers at the valid nodes, finite everywhere
    ft = dict(f, dy=torch.from_numpy(f["dy"]).cuda(), dx=torch.from_numpy(f["dx"]).cuda())
    filled = wf.wavefront_from_displacement(ft, weights=torch.from_numpy(w).cuda(), remove="quadratic", fill="harmonic",
                                            return_tensors=True, **kw)
    assert filled["wavefront"].is_cuda and filled["valid"].is_cuda and filled["valid"].dtype == torch.bool
    fw = filled["wavefront"].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(fw))
    np.testing.assert_array_equal(fw[got["valid"]], got["wavefront"][got["valid"]])
    np.testing.assert_array_equal(filled["coefficients"], got["coefficients"])


# ---- end to end
def test_end_to_end_masked_curvature_512(wf, observe):
    """The 512^2 speckle pair of the unweighted end-to-end test (+-3 px of defocus + astigmatism); outside a disc of 0.8 of the
    half side the second frame is fresh, independent Poisson speckle.  The peak map of displacement_map falls into two
    populations; the mask is peak > the midpoint of their medians.  The masked curvature terms are no further from the analytic
    truth than the float64 oracle chain on the same map and mask, plus the coefficient bar; the unmasked call is worse."""
    from barc4dip_amd.preprocessing import correct_distortion
    from barc4dip_amd.signal import displacement_map

    n, p, L = 512, 6.5e-6, 0.75
    ref = synth.speckle_frame(n, 51, pupil_div=4)
    a, b, c = 6e-3, 3e-3, 2e-3
    A = np.array([[a + b, c], [c, a - b]])
    q = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    ty = A[0, 0] * q[:, None] + A[0, 1] * q[None, :]
    tx = A[1, 0] * q[:, None] + A[1, 1] * q[None, :]
    dist = np.asarray(correct_distortion(ref, (ty, tx), order=3))
    outside = (q[:, None] ** 2 + q[None, :] ** 2) > (0.8 * 0.5 * n) ** 2
    dist = np.where(outside, synth.speckle_frame(n, 77, pupil_div=4), dist).astype(np.float32)
    m = displacement_map(ref, dist, window=31, step=16, search=8, subpixel="newton")
    # the two populations by geometry: windows that lie wholly inside the disc, and wholly outside it
    rc = np.hypot(m["y"][:, None] - 0.5 * (n - 1), m["x"][None, :] - 0.5 * (n - 1))
    inside, outer = rc < 0.8 * 0.5 * n - 24.0, rc > 0.8 * 0.5 * n + 24.0
    med_in, med_out = float(np.median(m["peak"][inside])), float(np.median(m["peak"][outer]))
    print(f"end to end: median peak inside the disc {med_in:.3f} ({inside.sum()} windows), outside {med_out:.3f} ({outer.sum()})")
    assert med_in > med_out
    mask = m["peak"] > 0.5 * (med_in + med_out)
    print(f"end to end: {mask[inside].mean():.3f} of the inside windows and {mask[outer].mean():.3f} of the outside ones pass the mask")
    B = -np.linalg.solve(np.eye(2) + A, A)
    truth = np.array([B[1, 1] / (2 * L), B[0, 1] / L, B[0, 0] / (2 * L)])      # c3 (u^2), c4 (uv), c5 (v^2)
    got = wf.wavefront_from_displacement(m, pixel_size=p, distance=L, remove=None, mask=mask)
    plain = wf.wavefront_from_displacement(m, pixel_size=p, distance=L, remove=None)
    dy32, dx32 = m["dy"].astype(np.float32)[None], m["dx"].astype(np.float32)[None]
    orc = wavefront_weighted_np(dy32, dx32, mask.astype(np.float64), m["y"], m["x"], pixel_size=p, distance=L, remove=None)
    np.testing.assert_array_equal(got["valid"], mask & np.isfinite(m["dy"]) & np.isfinite(m["dx"]))
    scale = np.max(np.abs(truth))
    e_gpu = np.abs(got["coefficients"][0, 3:] - truth) / scale
    e_orc = np.abs(orc["coefficients"][0, 3:] - truth) / scale
    e_plain = np.abs(plain["coefficients"][0, 3:] - truth) / scale
    ax, ay = 0.5 * np.ptp(m["x"]) * p, 0.5 * np.ptp(m["y"]) * p
    height = np.array([ax * ax, ax * ay, ay * ay])
    parity = BARS["wwf/chain_coefficients"] * np.ptp(orc["wavefront"][0][mask]) / (height * scale)
    print(f"end to end: truth error of the oracle chain {e_orc}, of the device {e_gpu}, parity allowance {parity}, "
          f"unmasked {e_plain}; iterations {got['iterations'][0]}, radius_x {got['radius_x'][0]:.6g} m against {1 / (2 * truth[0]):.6g}")
    assert np.all(e_gpu <= e_orc + parity), (e_gpu, e_orc, parity)
    assert np.max(e_plain) > np.max(e_gpu), (e_plain, e_gpu)
