"""Host tier: the inputs of tests/test_gpu_tracking_edges.py are unambiguous in the float64 oracle itself.

The GPU file asserts exact arg-max parity with the oracle on peaks that lie on map borders, next to them and on both sides of the
cyclic seams.  That only means something where the reference's own answer is well separated, so the same inputs (built by the
same helpers of barc4dip_amd/synth.py) are checked here without a GPU: every imposed shift is recovered, the highest map value
is at least twice the second highest, border peaks get no Taylor step, and the degenerate maps (all-zero, all-NaN, delta-like,
tiny NCC maps) give the values the GPU file expects."""
import warnings

import numpy as np
import pytest

from barc4dip_amd import synth
from oracle import ncc_np as N
from oracle import signal_np as S

CASES = synth.TRACKING_EDGE_CASES
DEGENERATE_SHAPES = [c for c in CASES if c[0] in ((64, 64), (100, 37), (228, 228))]


def _sl(roi):
    return slice(roi[0], roi[1]), slice(roi[2], roi[3])


def _oracle(tpl, img, sl, subpixel=True):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # NaN / Inf inputs: NumPy warns, the result is what counts
        return S.phase_correlation(tpl.astype(np.float64), img.astype(np.float64), slices_yx=sl, subpixel=subpixel)


@pytest.mark.parametrize("shape,tpl_hw,route", CASES, ids=[f"{c[0][0]}x{c[0][1]}" for c in CASES])
def test_oracle_recovers_every_edge_shift_with_a_dominant_peak(shape, tpl_hw, route):
    H, W = shape
    shifts = synth.edge_shift_sweep(H, W)
    assert len(shifts) == len(set(shifts)) == 54
    base, stack = synth.white_speckle_pairs(shape, shifts, seed=1000 * H + W)
    sl = _sl(synth.edge_roi(shape, tpl_hw))
    borders = 0
    for i, (dy, dx) in enumerate(shifts):
        mag = S.phase_correlation_map(base[sl].astype(np.float64), stack[i].astype(np.float64), slices_yx=sl)
        k = int(np.argmax(mag))
        mi, mj = divmod(k, W)
        assert (mi - H // 2, mj - W // 2) == (dy, dx), (shape, dy, dx)
        top = float(mag.flat[k])
        mag.flat[k] = 0.0
        assert top >= 2.0 * float(mag.max()), (shape, dy, dx, top, float(mag.max()))
        mag.flat[k] = top
        if mi in (0, H - 1) or mj in (0, W - 1):
            borders += 1
            assert S.peak_subpixel_taylor(mag, (mi, mj)) == (0.0, 0.0)
            full = _oracle(base[sl], stack[i], sl)
            assert (full[0], full[1]) == (float(dy), float(dx))       # border peak: the sub-pixel result is the integer one
    assert borders == 26


@pytest.mark.parametrize("shape,tpl_hw,route", DEGENERATE_SHAPES, ids=[f"{c[0][0]}x{c[0][1]}" for c in DEGENERATE_SHAPES])
def test_oracle_values_of_degenerate_maps(shape, tpl_hw, route):
    H, W = shape
    cases = synth.degenerate_tracking_inputs(shape, tpl_hw, seed=7000 + H + W)
    origin = (float(-(H // 2)), float(-(W // 2)))
    for name in ("const_image", "const_template", "tpl_1x1"):           # all-zero map: first element, peak 0, snr 0
        src, img, roi = cases[name]
        assert _oracle(src[_sl(roi)], img, _sl(roi)) == origin + (0.0, 0.0), name
    for name in ("nan_image", "nan_template", "inf_image"):             # all-NaN map: np.argmax names the first element
        src, img, roi = cases[name]
        got = _oracle(src[_sl(roi)], img, _sl(roi))
        assert got[:2] == origin and np.isnan(got[2]) and np.isnan(got[3]), (name, got)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mag = S.phase_correlation_map(src[_sl(roi)].astype(np.float64), img.astype(np.float64), slices_yx=_sl(roi))
        assert np.isnan(mag).all() and int(np.argmax(mag)) == 0
    src, img, roi = cases["whole_frame"]                                 # delta-like map: the median is rounding noise
    got = _oracle(src[_sl(roi)], img, _sl(roi), subpixel=False)
    assert got[:2] == (3.0, -2.0) and got[2] > 0.999 and got[3] > 1e3, got
    # one-row template: the oracle does not recover the shift, but its arg-max is separated from the runner-up by far more than
    # float32 rounding of the map (the all_routes / general_sizes peak bars are ~1e-3 relative), so exact parity can be asked for
    src, img, roi = cases["one_row"]
    mag = S.phase_correlation_map(src[_sl(roi)].astype(np.float64), img.astype(np.float64), slices_yx=_sl(roi))
    k = int(np.argmax(mag))
    top = float(mag.flat[k])
    mag.flat[k] = 0.0
    assert top >= 1.01 * float(mag.max()), (top, float(mag.max()))


def _ncc_inputs():
    base, stack = synth.white_speckle_pairs((100, 37), [(0, 0)], seed=100037, noise=5.0)
    return base, stack[0]          # image, template source = image + N(0, 5)


NCC_POSITIONS = [(0, 0), (0, 16), (59, 0), (59, 16), (0, 7), (30, 0), (59, 5), (20, 16), (30, 8)]


@pytest.mark.parametrize("backend", ["opencv", "skimage"])
def test_ncc_oracle_edge_positions_and_tiny_maps(backend):
    img, noisy = _ncc_inputs()
    H, W, h, w = 100, 37, 41, 21
    for (py, px) in NCC_POSITIONS:
        sl = (slice(py, py + h), slice(px, px + w))
        tz = S.zscore2d(noisy[sl], 1e-9).astype(np.float32)
        corr = N.match_template_ncc(S.zscore2d(img, 1e-9).astype(np.float32) if backend == "opencv" else img, tz)
        assert corr.shape == (60, 17)
        assert np.unravel_index(int(np.argmax(corr)), corr.shape) == (py, px)
        srt = np.sort(corr.ravel())
        assert srt[-1] > 0.99 and srt[-1] >= 2.0 * srt[-2]
        r = N.template_matching(noisy[sl], img, slices_yx=sl, backend=backend)
        ri = N.template_matching(noisy[sl], img, slices_yx=sl, backend=backend, subpixel=False)
        assert (ri[0], ri[1]) == (0.0, 0.0)
        if (py, px) != (30, 8):
            assert r == ri                                              # border of the match map: no Taylor step
        else:
            assert r[:2] != ri[:2] and abs(r[0]) < 0.5 and abs(r[1]) < 0.5
    # tiny match maps: 1x1, 1x2, 2x1, 2x2, 3x3 elements (even template sizes need explicit slices)
    for (ch, cw), n in (((0, 0), 1), ((0, 1), 2), ((1, 0), 2), ((1, 1), 4), ((2, 2), 9)):
        sl = (slice(0, H - ch), slice(0, W - cw))
        r = N.template_matching(img[sl], img, slices_yx=sl, backend=backend)
        assert (r[0], r[1]) == (0.0, 0.0) and abs(r[2] - 1.0) < 1e-6, (ch, cw, r)
        if n == 1:
            assert abs(r[3] - 1.0) < 1e-6                               # the median of a one-element map is the peak itself
        else:
            assert r[3] > 1.5                                           # (seed-dependent: 2 ... 60 on white speckle)
    # constant image / constant template: the response is 0 everywhere, np.argmax names the first element
    y0, x0 = 30, 8
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    assert N.template_matching(noisy[sl], np.full((H, W), 7.0, np.float32), slices_yx=sl, backend=backend) == (-y0, -x0, 0.0, 0.0)
    assert N.template_matching(np.full((h, w), 7.0, np.float32), img, slices_yx=sl, backend=backend) == (-y0, -x0, 0.0, 0.0)
