"""Displacement maps on the MI355X (b4d_displacement_map, barc4dip_amd/signal/displacement.py) against the per-window float64
oracle of tests/test_displacement_host.py, against ground truth, and against the existing GPU tracker on the same windows.
Bars: float32 rounding level, held like the NCC bars of tests/test_gpu_tracking.py."""
from __future__ import annotations

import numpy as np
import pytest

from barc4dip_amd import synth
from test_displacement_host import inside_one_tile, oracle_map, piecewise_field

pytestmark = pytest.mark.gpu

BARS = {
    "disp/peak_abs": 2e-6, "disp/sub_px": 2e-6, "disp/snr_rel": 2e-6,
    "disp_batch/peak_abs": 2e-6, "disp_batch/snr_rel": 2e-6,
    "disp_offset/peak_abs": 2e-6, "disp_offset/sub_px": 2e-6, "disp_offset/snr_rel": 2e-6,
    "disp_subpx/mae": 0.15,
}


@pytest.fixture(scope="module")
def dm():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import displacement

    return displacement.displacement_map


def _frames(shape, shift, seed=21, noise=20.0):
    n = max(shape)
    f0 = synth.speckle_frame(n, seed)[:shape[0], :shape[1]]
    rng = np.random.default_rng(seed + 1)
    fr = np.roll(f0, shift, axis=(0, 1)) + rng.normal(size=shape).astype(np.float32) * noise
    return f0, fr.astype(np.float32)


def _check_vs_oracle(got, want, observe, key, mask=None):
    """got: dict from displacement_map; want: oracle tuple; integer parts compared by the caller."""
    gy, gx = got["dy"].shape
    for iy, ix in np.ndindex(gy, gx):
        if mask is not None and not mask[iy, ix]:
            continue
        wdy, wdx, wpk, wsnr = (w[iy, ix] for w in want)
        observe(f"{key}/peak_abs", abs(got["peak"][iy, ix] - wpk), BARS[f"{key}/peak_abs"])
        observe(f"{key}/sub_px", max(abs(got["dy"][iy, ix] - wdy), abs(got["dx"][iy, ix] - wdx)), BARS[f"{key}/sub_px"])
        observe(f"{key}/snr_rel", abs(got["snr"][iy, ix] - wsnr) / abs(wsnr), BARS[f"{key}/snr_rel"])


CASES = [   # (frame shape, window, step, search, shift)
    ((256, 256), 31, 16, 8, (3, -5)),
    ((256, 256), (21, 33), (10, 12), (5, 7), (-2, 4)),     # non-square window, step and search
    ((256, 256), 16, 9, 3, (1, 2)),                         # even window: half-integer centres
    ((256, 256), 15, 20, 1, (1, -1)),                       # search 1: 3 x 3 map, peak often on the border
    ((256, 256), 24, 40, 32, (-20, 27)),                    # search 32
    ((300, 517), 31, 16, 8, (4, 6)),                        # frame that is not a power of two
    ((256, 320), (40, 80), (30, 50), (6, 4), (2, -3)),      # window wider than 64 px: the second template register
    ((300, 300), 63, 48, 32, (-9, 12)),                     # box over the 64 KiB target: three bands of output rows
    ((200, 200), 128, 64, 32, (5, -7)),                     # the documented limits: one window, two bands near 160 KiB
]


@pytest.mark.parametrize("backend", ["opencv", "skimage"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_parity_with_oracle(dm, backend, case, observe):
    shape, win, step, srch, shift = CASES[case]
    f0, fr = _frames(shape, shift)
    kw = dict(window=win, step=step, search=srch, backend=backend)
    gi = dm(f0, fr, subpixel=False, **kw)
    wi = oracle_map(f0, fr, subpixel=False, **kw)
    np.testing.assert_array_equal(gi["dy"], wi[0])
    np.testing.assert_array_equal(gi["dx"], wi[1])
    got = dm(f0, fr, **kw)
    want = oracle_map(f0, fr, **kw)
    _check_vs_oracle(got, want, observe, "disp")
    from barc4dip_amd.signal.displacement import displacement_grid

    g = displacement_grid(shape, window=win, step=step, search=srch)
    np.testing.assert_array_equal(got["y"], g["y"])
    np.testing.assert_array_equal(got["x"], g["x"])
    assert got["meta"]["backend"] == backend and got["dy"].dtype == np.float64


def test_ground_truth_uniform_and_piecewise(dm):
    f0, fr = _frames((256, 256), (3, -5), noise=5.0)
    for backend in ("opencv", "skimage"):
        r = dm(f0, fr, window=31, step=16, search=8, backend=backend, subpixel=False)
        assert np.all(r["dy"] == 3) and np.all(r["dx"] == -5)
        assert np.all(r["peak"] > 0.95)
    ref, img, shift_of = piecewise_field()
    r = dm(ref, img, window=15, step=8, search=4, subpixel=False)
    from barc4dip_amd.signal.displacement import displacement_grid

    g = displacement_grid(ref.shape, window=15, step=8, search=4)
    n = 0
    for iy, ix in np.ndindex(*g["shape"]):
        if inside_one_tile(g, iy, ix, 64):
            assert (r["dy"][iy, ix], r["dx"][iy, ix]) == shift_of(int(g["y0"][iy]), int(g["x0"][ix]))
            n += 1
    assert n > 40


def test_ground_truth_subpixel_fourier_shift(dm, observe):
    """A Fourier shift of (0.3, -0.45) px.  The reference's Taylor step swaps its two corrections (tracking.py:372-373,
    kept on purpose), so the y output carries the x fraction and vice versa: the expectation is (-0.45, 0.3)."""
    n = 512
    i0 = synth.speckle_intensity(n, 5, pupil_div=4)
    ky = np.fft.fftfreq(n)[:, None]
    kx = np.fft.fftfreq(n)[None, :]
    sy, sx = 0.3, -0.45
    sh = np.real(np.fft.ifft2(np.fft.fft2(i0) * np.exp(-2j * np.pi * (ky * sy + kx * sx))))
    rng = np.random.default_rng(9)
    f0 = rng.poisson(i0).astype(np.float32)
    fr = rng.poisson(np.maximum(sh, 0)).astype(np.float32)
    r = dm(f0, fr, window=31, step=16, search=4)
    mae = 0.5 * (np.mean(np.abs(r["dy"] - sx)) + np.mean(np.abs(r["dx"] - sy)))
    observe("disp_subpx/mae", mae, BARS["disp_subpx/mae"])


def test_same_answer_as_template_matching_batch(dm, observe):
    """The cut boxes through the existing GPU tracker (FFT route): same integer arg-max, peak and snr within the bars."""
    import torch

    from barc4dip_amd.signal import template_matching_batch
    from barc4dip_amd.signal.displacement import displacement_grid

    f0, fr = _frames((256, 256), (-3, 2))
    win, step, srch = 25, 20, 6
    g = displacement_grid(f0.shape, window=win, step=step, search=srch)
    tr = torch.from_numpy(fr).cuda()
    t0 = torch.from_numpy(f0).cuda()
    bh, bw = win + 2 * srch, win + 2 * srch
    boxes, tboxes = [], []
    for iy, ix in np.ndindex(*g["shape"]):
        y0, x0 = int(g["y0"][iy]), int(g["x0"][ix])
        boxes.append(tr[y0 - srch:y0 + win + srch, x0 - srch:x0 + win + srch])
        tboxes.append(t0[y0 - srch:y0 + win + srch, x0 - srch:x0 + win + srch])
    boxes, tboxes = torch.stack(boxes), torch.stack(tboxes)
    k = boxes.shape[0]
    assert (bh, bw) == tuple(boxes.shape[1:])
    for backend in ("opencv", "skimage"):
        ref_rows = template_matching_batch(boxes, tboxes, np.arange(k), [[srch, srch + win, srch, srch + win]] * k,
                                           np.arange(k), np.arange(k), backend=backend, subpixel=False)
        got = dm(f0, fr, window=win, step=step, search=srch, backend=backend, subpixel=False)
        np.testing.assert_array_equal(got["dy"].ravel(), ref_rows[:, 0])
        np.testing.assert_array_equal(got["dx"].ravel(), ref_rows[:, 1])
        for i in range(k):
            observe("disp_batch/peak_abs", abs(got["peak"].ravel()[i] - ref_rows[i, 2]), BARS["disp_batch/peak_abs"])
            observe("disp_batch/snr_rel", abs(got["snr"].ravel()[i] - ref_rows[i, 3]) / ref_rows[i, 3], BARS["disp_batch/snr_rel"])


def test_large_offset_low_contrast_uint16(dm, observe):
    """Mean 30 000 counts, 1 % speckle contrast, uint16 words: catches float32 cancellation in the denominator."""
    n = 256
    i0 = synth.speckle_intensity(n, 17)
    base = 30000.0 * (1.0 + 0.01 * (i0 / i0.mean() - 1.0))
    rng = np.random.default_rng(4)
    f0 = np.rint(base + rng.normal(size=base.shape) * 5).astype(np.uint16)
    fr = np.rint(np.roll(base, (2, -3), axis=(0, 1)) + rng.normal(size=base.shape) * 5).astype(np.uint16)
    for backend in ("opencv", "skimage"):
        kw = dict(window=31, step=24, search=6, backend=backend)
        gi = dm(f0, fr, subpixel=False, **kw)
        wi = oracle_map(f0, fr, subpixel=False, **kw)
        np.testing.assert_array_equal(gi["dy"], wi[0])
        np.testing.assert_array_equal(gi["dx"], wi[1])
        assert np.all(gi["dy"] == 2) and np.all(gi["dx"] == -3)
        _check_vs_oracle(dm(f0, fr, **kw), oracle_map(f0, fr, **kw), observe, "disp_offset")


def test_stacks_pairs_and_tensors(dm):
    import torch

    stack, _ = synth.shifted_stack(5, 256, seed=31, max_shift=6)
    kw = dict(window=(31, 25), step=(20, 18), search=(8, 7))
    full = dm(stack[0], stack, **kw)
    assert full["dy"].shape == (5,) + dm(stack[0], stack[1], **kw)["dy"].shape
    for t in range(5):
        one = dm(stack[0], stack[t], **kw)
        for key in ("dy", "dx", "peak", "snr"):
            np.testing.assert_array_equal(full[key][t], one[key])
    inc = dm(stack[:-1], stack[1:], **kw)
    for t in range(4):
        one = dm(stack[t], stack[t + 1], **kw)
        for key in ("dy", "dx", "peak", "snr"):
            np.testing.assert_array_equal(inc[key][t], one[key])
    ts = torch.from_numpy(stack).cuda()
    rt = dm(ts[:-1], ts[1:], return_tensors=True, **kw)
    assert isinstance(rt["dy"], torch.Tensor) and rt["dy"].is_cuda and rt["dy"].dtype == torch.float64
    for key in ("dy", "dx", "peak", "snr"):
        np.testing.assert_array_equal(rt[key].cpu().numpy(), inc[key])
    with pytest.raises(NotImplementedError):
        dm(stack[0].astype(np.complex64), stack[1], **kw)


def test_full_size_2048(dm, observe):
    n = 2048
    f0, fr = _frames((n, n), (-4, 7), seed=3, noise=10.0)
    kw = dict(window=31, step=16, search=8)
    gi = dm(f0, fr, subpixel=False, **kw)
    assert gi["dy"].shape == ((n - 47) // 16 + 1,) * 2
    assert np.all(gi["dy"] == -4) and np.all(gi["dx"] == 7)
    got = dm(f0, fr, **kw)
    rng = np.random.default_rng(0)
    sel = [(int(rng.integers(0, gi["dy"].shape[0])), int(rng.integers(0, gi["dy"].shape[1]))) for _ in range(64)]
    want = oracle_map(f0, fr, windows=sel, **kw)
    mask = np.zeros(gi["dy"].shape, bool)
    for iy, ix in sel:
        mask[iy, ix] = True
    _check_vs_oracle(got, want, observe, "disp", mask=mask)


def test_zero_variance_template_gives_zero_response(dm):
    """A flat patch in the reference: every template cut from it has zero variance, so the whole map is the oracle's masked
    response 0; arg-max is the first index (dy, dx) = (-Sy, -Sx), peak 0, snr 0 -- for every window inside the patch."""
    f0, fr = _frames((256, 256), (2, 3))
    f0 = f0.copy()
    f0[40:140, 60:180] = 1000.0
    from barc4dip_amd.signal.displacement import displacement_grid

    for backend in ("opencv", "skimage"):
        kw = dict(window=21, step=12, search=5, backend=backend)
        got = dm(f0, fr, **kw)
        want = oracle_map(f0, fr, **kw)
        g = displacement_grid(f0.shape, window=21, step=12, search=5)
        flat = (g["y0"][:, None] >= 40) & (g["y0"][:, None] + 21 <= 140) & (g["x0"][None, :] >= 60) & (g["x0"][None, :] + 21 <= 180)
        assert flat.sum() >= 20
        for key, w in zip(("dy", "dx", "peak", "snr"), want):
            np.testing.assert_array_equal(got[key][flat], w[flat])
        assert np.all(got["dy"][flat] == -5) and np.all(got["dx"][flat] == -5)
        assert np.all(got["peak"][flat] == 0) and np.all(got["snr"][flat] == 0)
        assert np.all(np.rint(got["dy"][~flat & (g["y0"][:, None] > 150)]) == 2)   # textured windows below the patch still track
