"""GPU tier: tracker peaks on map borders, across the cyclic seams of the map-free route, and degenerate maps.

`b4d_phase_correlation` / `b4d_template_match` against the float64 oracle (oracle/signal_np.py, oracle/ncc_np.py) on inputs whose
peak lies where the index arithmetic lives: the first / last row and column of the shifted map (no Taylor step), shifts of -1 and
0 (the row-pair seam ny/2-1 | 0 of the rows recomputed around the peak and the column seam of `c = (x + NX/2) & (NX-1)`), maps
that are equal everywhere (first occurrence must win in every arg-max stage), all-NaN maps (the arg-max sentinel survives: the
answer is NumPy's, index 0 and NaN), a delta-like map and a map without a dominant peak (both leave the expected-median-bin
route), and NCC match maps of 1 ... 9 elements.  The inputs come from barc4dip_amd/synth.py (white speckle);
tests/test_tracking_edges_host.py asserts, without a GPU, that the oracle itself is unambiguous on every one of them.

NaN frames are OUT OF SCOPE for template matching: parity with cv2 / scikit-image is unpinned, and the oracle's summed-area tables
spread a NaN over the windows below and to the right of it while the device's FFT product spreads it over the whole map.

Bars.  On these inputs the device is at float32 rounding level from the float64 oracle (sub-pixel part 5e-8 px, peak 4e-7, snr
5e-6), three orders below the bars of tests/test_gpu_tracking.py, so the file holds keys of its own, `edges/*`, at 2 x the maxima
observed on MI355X (comments of BARS); NCC keeps `ncc_256/*`.  That closeness is the result of a fix this file led to: the z-scored
operands have zero mean, so the DC bin of their cross-power spectrum is a rounded zero.  In the float64 protocol |prod| there is far
below eps = 1e-9 and the whitened bin is 0; in float32 it is of the order of eps and the bin kept a modulus s anywhere in [0, 1]: a
constant s / N on the real map.  Before the fix this sweep measured exactly that constant (128 x 512: peak deviation 9.75e-5 x peak
0.157 = 1.00 / N; 64^2: 1.9e-4 px, snr 6.5e-3, the same figures as the oracle's own float32 path against its float64 path) and the snr of
the delta-like map, which is nothing but that bin, was 1.0e8 against 5.2e4 at 228^2.  The trackers now zero the bin on every route."""
import functools
import warnings

import numpy as np
import pytest

from barc4dip_amd import synth

pytestmark = pytest.mark.gpu

CASES = synth.TRACKING_EDGE_CASES
DEGENERATE = [c for c in CASES if c[0] in ((64, 64), (100, 37), (228, 228))]
_ids = lambda cs: [f"{c[0][0]}x{c[0][1]}" for c in cs]  # noqa: E731

# <key>: bar   # largest deviation from the float64 oracle observed on MI355X in this file; bar = 2 x that
BARS = {
    "edges/sub_px": 1e-7,              # 4.60e-8 px  (64 x 128)
    "edges/peak_rel": 9e-7,            # 4.28e-7     (100 x 37)
    "edges/snr_rel": 1.1e-5,           # 5.37e-6     (128 x 512)
    "edges/delta_snr_rel": 2.3e-6,     # 1.14e-6     (228^2; 64^2 1.8e-7, 100 x 37 1.1e-7); per pair also <= 4 x the oracle's own spread
    "ncc_256/peak_abs": 2e-6, "ncc_256/sub_px": 2e-6, "ncc_256/snr_rel": 2e-6,   # 1.8e-7, 2.8e-9 px, 7.0e-7 (bars of test_gpu_tracking.py)
}


def _sl(roi):
    return slice(roi[0], roi[1]), slice(roi[2], roi[3])


def _rel(got, want):
    return abs(got - want) / abs(want)


@pytest.fixture(scope="module")
def gs():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd import signal

    return signal


def _modes(route):
    """track_predict_bin settings that are distinct routes: the DFT-matrix path always runs the full select on the full map."""
    return (1,) if route == "dft" else (1, 0, 2)


def _in_every_mode(route, fn):
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    out = {}
    try:
        for mode in _modes(route):
            assert lib.b4d_set_option(b"track_predict_bin", mode) == 0
            out[mode] = fn()
    finally:
        lib.b4d_set_option(b"track_predict_bin", 1)
    return out


def _oracle_row(tpl, img, sl):
    """(peak_ij, integer row, sub-pixel row) of the float64 oracle from ONE evaluation of the map (the statements of
    oracle.signal_np.phase_correlation after the map)."""
    from oracle import signal_np as S

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mag = S.phase_correlation_map(tpl.astype(np.float64), img.astype(np.float64), slices_yx=sl)
    H, W = mag.shape
    mi, mj = np.unravel_index(np.argmax(mag), mag.shape)
    peak, snr = S.corr_peak_quality(mag, (mi, mj), 1e-9)
    di, dj = S.peak_subpixel_taylor(mag, (mi, mj))
    dy, dx = float(mi - H // 2), float(mj - W // 2)
    return (int(mi), int(mj)), (dy, dx, peak, snr), (dy + di, dx + dj, peak, snr)


@functools.lru_cache(maxsize=None)
def _sweep(shape, tpl_hw):
    H, W = shape
    shifts = synth.edge_shift_sweep(H, W)
    base, stack = synth.white_speckle_pairs(shape, shifts, seed=1000 * H + W)
    roi = synth.edge_roi(shape, tpl_hw)
    ref = [_oracle_row(base[_sl(roi)], stack[i], _sl(roi)) for i in range(len(shifts))]
    return shifts, base, stack, roi, ref


@pytest.mark.parametrize("shape,tpl_hw,route", CASES, ids=_ids(CASES))
def test_phase_correlation_edge_shift_sweep(gs, shape, tpl_hw, route, observe):
    """54 shifts per shape in one batched call: peaks on all four borders and corners of the shifted map, next to them, and on
    both sides of the zero-shift seams; every median route; against the float64 oracle pair by pair."""
    H, W = shape
    shifts, base, stack, roi, ref = _sweep(shape, tpl_hw)
    n = len(shifts)
    assert n == 54

    def run():
        return tuple(gs.phase_correlation_batch(stack, base[None], [0], [roi], list(range(n)), [0] * n, subpixel=sub, return_peak_ij=True)
                     for sub in (True, False))

    out = _in_every_mode(route, run)
    for m in _modes(route)[1:]:                              # the median expectation is only a route: bit-identical rows
        for (ra, pa), (rb, pb) in zip(out[m], out[1]):
            assert np.array_equal(ra, rb) and np.array_equal(pa, pb), (shape, m)
    (rs, ps), (ri, pi) = out[1]
    assert np.array_equal(ps, pi) and np.array_equal(rs[:, 2:], ri[:, 2:])      # peak and snr do not depend on the Taylor step
    worst = {"sub_px": 0.0, "peak_rel": 0.0, "snr_rel": 0.0}
    borders = 0
    for i, (dy, dx) in enumerate(shifts):
        (mi, mj), wi, ws = ref[i]
        assert (int(ps[i, 0]), int(ps[i, 1])) == (mi, mj) == (dy + H // 2, dx + W // 2), (shape, dy, dx, ps[i])
        assert (ri[i, 0], ri[i, 1]) == (wi[0], wi[1]) == (dy, dx), (shape, dy, dx, ri[i])
        assert (round(rs[i, 0]), round(rs[i, 1])) == (dy, dx), (shape, dy, dx, rs[i])
        if mi in (0, H - 1) or mj in (0, W - 1):            # border row / column: no Taylor step, exactly the integer result
            borders += 1
            assert (rs[i, 0], rs[i, 1]) == (ri[i, 0], ri[i, 1]) == (ws[0], ws[1]), (shape, dy, dx, rs[i])
        worst["sub_px"] = max(worst["sub_px"], abs(rs[i, 0] - ws[0]), abs(rs[i, 1] - ws[1]))
        worst["peak_rel"] = max(worst["peak_rel"], _rel(rs[i, 2], ws[2]))
        worst["snr_rel"] = max(worst["snr_rel"], _rel(rs[i, 3], ws[3]))
    assert borders == 26
    print(f"edge sweep {shape} {route}: observed maxima", {k: f"{v:.2e}" for k, v in worst.items()})
    for q, v in worst.items():
        observe(f"edges/{q}", v, BARS[f"edges/{q}"])


@pytest.mark.parametrize("shape,tpl_hw,route", DEGENERATE, ids=_ids(DEGENERATE))
def test_degenerate_maps(gs, shape, tpl_hw, route, observe):
    """All-zero, all-NaN, delta-like and peak-less maps, eight pairs in ONE call (a NaN pair next to finite ones), every route.

    All-zero maps (constant image, constant template, 1 x 1 template) are the tie test of every arg-max stage: index (0, 0).
    All-NaN maps (one NaN / Inf pixel) must come back as NumPy reports them: index (0, 0), peak and snr NaN.
    One-row template: parity of the arg-max and the integer shift with the oracle (which does not recover the shift itself; its
    runner-up is >= 1 % below the maximum, tests/test_tracking_edges_host.py).  Delta-like map: integer parts here, peak and snr in
    test_delta_like_map."""
    H, W = shape
    cases = synth.degenerate_tracking_inputs(shape, tpl_hw, seed=7000 + H + W)
    names = list(cases)
    srcs = np.stack([cases[k][0] for k in names])
    imgs = np.stack([cases[k][1] for k in names])
    rois = [cases[k][2] for k in names]
    idx = list(range(len(names)))

    def run():
        return tuple(gs.phase_correlation_batch(imgs, srcs, idx, rois, idx, idx, subpixel=sub, return_peak_ij=True) for sub in (True, False))

    out = _in_every_mode(route, run)
    for m in _modes(route)[1:]:
        for (ra, pa), (rb, pb) in zip(out[m], out[1]):
            assert np.array_equal(ra, rb, equal_nan=True) and np.array_equal(pa, pb), (shape, m, ra, rb)
    (rs, ps), (ri, pi) = out[1]
    assert np.array_equal(ps, pi)
    origin = (float(-(H // 2)), float(-(W // 2)))
    for i, name in enumerate(names):
        src, img, roi = cases[name]
        pij, wi, ws = _oracle_row(src[_sl(roi)], img, _sl(roi))
        assert (int(ps[i, 0]), int(ps[i, 1])) == pij, (shape, name, ps[i], pij)
        assert (ri[i, 0], ri[i, 1]) == (wi[0], wi[1]), (shape, name, ri[i], wi)
        if name in ("const_image", "const_template", "tpl_1x1"):
            assert pij == (0, 0) and wi == origin + (0.0, 0.0)
            assert tuple(rs[i]) == tuple(ri[i]) == wi, (shape, name, rs[i], ri[i])
        elif name in ("nan_image", "nan_template", "inf_image"):
            assert pij == (0, 0) and wi[:2] == origin and np.isnan(wi[2]) and np.isnan(wi[3])
            for r in (rs[i], ri[i]):
                assert (r[0], r[1]) == origin and np.isnan(r[2]) and np.isnan(r[3]), (shape, name, r)
        elif name == "whole_frame":
            assert (ri[i, 0], ri[i, 1]) == (3.0, -2.0) and (round(rs[i, 0]), round(rs[i, 1])) == (3, -2)
        else:
            assert name == "one_row" and (round(rs[i, 0]), round(rs[i, 1])) == (wi[0], wi[1])


@pytest.mark.parametrize("shape,tpl_hw,route", DEGENERATE, ids=_ids(DEGENERATE))
def test_delta_like_map(gs, shape, tpl_hw, route, observe):
    """Template = the whole frame, image = the frame rolled by (3, -2): the map is a delta, far from the expected median bin.  All
    routes agree bit for bit; peak within `edges/peak_rel`; snr against the float64 oracle under a key of its own.

    Every bin of the whitened spectrum has unit modulus except the DC bin, which is 0 (z-scored operands): every element off the peak
    is 1 / N, peak = 1 - 1 / N, snr = N - 1.  The oracle's float32 path keeps a rounded DC bin instead (snr 8.8e4 for N = 4096, N / 2 at
    228^2): the device must be within 4 x that spread of the float64 value, and within the bar.  Observed on MI355X, snr device /
    oracle float64:  64^2 4094.98396 / 4094.98323,  100 x 37 3698.98671 / 3698.98631,  228^2 51980.237 / 51980.297."""
    from oracle import signal_np as S

    H, W = shape
    src, img, roi = synth.degenerate_tracking_inputs(shape, tpl_hw, seed=7000 + H + W)["whole_frame"]

    def run():
        return gs.phase_correlation_batch(img[None], src[None], [0], [roi], [0], [0], return_peak_ij=True)

    out = _in_every_mode(route, run)
    for m in _modes(route)[1:]:
        assert np.array_equal(out[m][0], out[1][0]) and np.array_equal(out[m][1], out[1][1]), (shape, m, out[m], out[1])
    r = out[1][0][0]
    pij, wi, ws = _oracle_row(src[_sl(roi)], img, _sl(roi))
    w32 = S.phase_correlation(src[_sl(roi)], img, slices_yx=_sl(roi))                  # the oracle's float32 path on the same pair
    print(f"delta-like map {shape}: peak {r[2]!r} snr {r[3]!r}; oracle float64 {ws[2:]!r} float32 {w32[2:]!r}")
    assert tuple(int(v) for v in out[1][1][0]) == pij == (3 + H // 2, -2 + W // 2)
    assert (round(r[0]), round(r[1])) == (3, -2)
    observe("edges/peak_rel", _rel(r[2], ws[2]), BARS["edges/peak_rel"])
    assert abs(r[3] - ws[3]) <= 4 * abs(w32[3] - ws[3]), (shape, r[3], ws[3], w32[3])
    observe("edges/delta_snr_rel", _rel(r[3], ws[3]), BARS["edges/delta_snr_rel"])


NCC_POSITIONS = [(0, 0), (0, 16), (59, 0), (59, 16), (0, 7), (30, 0), (59, 5), (20, 16), (30, 8)]   # corners, edges, interior


def _ncc_inputs():
    base, stack = synth.white_speckle_pairs((100, 37), [(0, 0)], seed=100037, noise=5.0)
    return base, stack[0]          # image, template source = image + N(0, 5)


@pytest.mark.parametrize("backend", ["opencv", "skimage"])
def test_template_matching_peak_on_map_borders(gs, backend, observe):
    """(100, 37) frame on its 128 x 64 canvas, (41, 21) templates cut at the four corners, the four edges and the interior of the
    60 x 17 match map: exact arg-max, no Taylor step on the border, peak / snr / sub-pixel part at float32 rounding level."""
    from oracle import ncc_np as N

    img, noisy = _ncc_inputs()
    h, w = 41, 21
    rois = [(py, py + h, px, px + w) for py, px in NCC_POSITIONS]
    idx = list(range(len(rois)))
    (rs, ps), (ri, pi) = (gs.template_matching_batch(img[None], noisy[None], [0] * len(rois), rois, [0] * len(rois), idx,
                                                      backend=backend, subpixel=sub, return_peak_ij=True) for sub in (True, False))
    assert np.array_equal(ps, pi)
    for i, (py, px) in enumerate(NCC_POSITIONS):
        sl = _sl(rois[i])
        want = N.template_matching(noisy[sl], img, slices_yx=sl, backend=backend)
        wint = N.template_matching(noisy[sl], img, slices_yx=sl, backend=backend, subpixel=False)
        assert (int(ps[i, 0]), int(ps[i, 1])) == (py, px)
        assert (ri[i, 0], ri[i, 1]) == (wint[0], wint[1]) == (0.0, 0.0)
        one = gs.template_matching(noisy[sl], img, slices_yx=sl, backend=backend)        # the single-pair entry point
        assert (one[2], one[3]) == (rs[i, 2], rs[i, 3]), (backend, py, px, one, rs[i])
        assert abs(one[0] - rs[i, 0]) <= 1e-12 and abs(one[1] - rs[i, 1]) <= 1e-12       # (it adds and subtracts the ROI centre)
        if (py, px) != (30, 8):
            assert (rs[i, 0], rs[i, 1]) == (ri[i, 0], ri[i, 1]) == (want[0], want[1]), (backend, py, px, rs[i])
        observe("ncc_256/sub_px", max(abs(rs[i, 0] - want[0]), abs(rs[i, 1] - want[1])), BARS["ncc_256/sub_px"])
        observe("ncc_256/peak_abs", abs(rs[i, 2] - want[2]), BARS["ncc_256/peak_abs"])
        observe("ncc_256/snr_rel", _rel(rs[i, 3], want[3]), BARS["ncc_256/snr_rel"])


@pytest.mark.parametrize("backend", ["opencv", "skimage"])
def test_template_matching_tiny_and_constant_maps(gs, backend, observe):
    """Match maps of 1, 2, 2, 4 and 9 elements (median ranks n/2 = 0, even counts of two, a one-element sampler) and maps that are 0
    everywhere (constant image, constant template: first occurrence across the map's workgroups), both median routes."""
    from barc4dip_amd import _ffi
    from oracle import ncc_np as N

    img, noisy = _ncc_inputs()
    H, W = img.shape
    lib = _ffi.lib()
    got = {}
    try:
        for mode in (1, 0):
            assert lib.b4d_set_option(b"track_predict_bin", mode) == 0
            rows = []
            for ch, cw in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 2)):
                sl = (slice(0, H - ch), slice(0, W - cw))
                rows.append(gs.template_matching(img[sl], img, slices_yx=sl, backend=backend))
            got[mode] = rows
    finally:
        lib.b4d_set_option(b"track_predict_bin", 1)
    assert got[1] == got[0]
    for (ch, cw), r in zip(((0, 0), (0, 1), (1, 0), (1, 1), (2, 2)), got[1]):
        sl = (slice(0, H - ch), slice(0, W - cw))
        want = N.template_matching(img[sl], img, slices_yx=sl, backend=backend)
        assert (want[0], want[1]) == (0.0, 0.0) and (r[0], r[1]) == (0.0, 0.0), (ch, cw, r, want)    # every element is on the border
        observe("ncc_256/peak_abs", abs(r[2] - want[2]), BARS["ncc_256/peak_abs"])
        observe("ncc_256/snr_rel", _rel(r[3], want[3]), BARS["ncc_256/snr_rel"])
    y0, x0, h, w = 30, 8, 41, 21
    roi = (y0, y0 + h, x0, x0 + w)
    flat_img = np.full((H, W), 7.0, np.float32)
    flat_tpl = noisy.copy()
    flat_tpl[_sl(roi)] = 7.0
    imgs, srcs = np.stack([flat_img, img]), np.stack([noisy, flat_tpl])
    for sub in (True, False):
        res, pij = gs.template_matching_batch(imgs, srcs, [0, 1], [roi, roi], [0, 1], [0, 1], backend=backend, subpixel=sub,
                                              return_peak_ij=True)
        assert np.array_equal(pij, np.zeros((2, 2), np.int32)), pij
        assert np.array_equal(res, np.array([[-y0, -x0, 0.0, 0.0]] * 2)), res
    assert N.template_matching(noisy[_sl(roi)], flat_img, slices_yx=_sl(roi), backend=backend) == (-y0, -x0, 0.0, 0.0)
    assert gs.template_matching(noisy[_sl(roi)], flat_img, slices_yx=_sl(roi), backend=backend) == (-y0, -x0, 0.0, 0.0)
