"""Host tier of SSIM, MS-SSIM and the frame errors: the float64 models of tests/perceptual_model.py against a brute-force double
loop over windows and against scikit-image's formula written out from its source (scipy.ndimage filters of the frames and their
products), the pool2 model, argument errors without a device, and the wiring.  No GPU needed."""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceptual_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = sorted(M.MODES)
RNG = np.random.default_rng(2811)
REF = RNG.poisson(40.0, (9, 13)).astype(np.float32)
IMG = (REF + RNG.normal(0.0, 3.0, REF.shape)).astype(np.float32)
C1, C2 = (0.01 * 50.0) ** 2, (0.03 * 50.0) ** 2


def brute_force(r, x, wy, wx, mode, cval, c1, c2, cov_norm):
    """The definition, pixel by pixel: the window of the padded frames, weights wy[j] wx[k], sums in plain Python order."""
    sy, sx = wy.size, wx.size
    pr, px = M.pad2(r, sy, sx, mode, cval), M.pad2(x, sy, sx, mode, cval)
    ny, nx = r.shape
    w2 = wy[:, None] * wx[None, :]
    W = w2.sum()
    ssim, cs = np.empty((ny, nx)), np.empty((ny, nx))
    for i in range(ny):
        for j in range(nx):
            a, b = pr[i:i + sy, j:j + sx], px[i:i + sy, j:j + sx]
            mr, mx = (w2 * a).sum() / W, (w2 * b).sum() / W
            vr = cov_norm * ((w2 * a * a).sum() / W - mr * mr)
            vx = cov_norm * ((w2 * b * b).sum() / W - mx * mx)
            vrx = cov_norm * ((w2 * a * b).sum() / W - mr * mx)
            cs[i, j] = (2 * vrx + c2) / (vr + vx + c2)
            ssim[i, j] = (2 * mr * mx + c1) / (mr * mr + mx * mx + c1) * cs[i, j]
    return ssim, cs


def float64_bound(m, k):
    """The model's own bound without the float32 ulp of the maps: what two float64 evaluations of the formula may differ by."""
    return m["tol_" + k] - M.ulp32(m[k])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("window", ["box", "gaussian", "box3x9"])
def test_model_matches_the_double_loop(mode, window):
    """9 x 13 frames, shorter than the 11-tap window, every border mode with cval != 0, odd, even and anisotropic boxes."""
    if window == "gaussian":
        wy = wx = M.ssim_taps()
        kw = dict(sy=11, sx=11, wy=wy, wx=wx)
    else:
        sy, sx = (7, 6) if window == "box" else (3, 9)
        wy, wx = np.ones(sy), np.ones(sx)
        kw = dict(sy=sy, sx=sx)
    cov = 42.0 / 41.0 if window == "box" else 1.0
    m = M.model_ssim(REF, IMG, mode=mode, cval=2.5, c1=C1, c2=C2, cov_norm=cov, **kw)
    ssim, cs = brute_force(REF.astype(np.float64), IMG.astype(np.float64), wy, wx, mode, 2.5, C1, C2, cov)
    for k, ref in (("ssim_map", ssim), ("cs_map", cs)):
        frac = float(np.max(np.abs(m[k] - ref) / float64_bound(m, k)))
        print(f"{k} {window} {mode}: {frac:.3f} of the bound")
        assert frac <= 1.0
    assert 0.0 < m["ssim"] < 1.0 and np.isclose(m["ssim"], ssim.mean(), rtol=1e-12)


@pytest.mark.parametrize("mode", MODES)
def test_model_of_identical_frames_is_exactly_one(mode):
    big = RNG.poisson(40000.0, (2, 20, 31)).astype(np.float32)
    for kw in (dict(sy=11, sx=11, wy=M.ssim_taps(), wx=M.ssim_taps()), dict(sy=7, sx=7, cov_norm=49.0 / 48.0), dict(sy=3, sx=9)):
        for frames in (REF, big):
            m = M.model_ssim(frames, frames.copy(), mode=mode, cval=1.0, c1=C1, c2=C2, **kw)
            assert np.all(m["ssim_map"] == 1.0) and np.all(m["cs_map"] == 1.0)
            assert np.all(m["ssim"] == 1.0) and np.all(m["cs"] == 1.0)


def skimage_formula(r, x, data_range, gaussian, win_size=7, sample_covariance=True, K1=0.01, K2=0.03):
    """skimage.metrics.structural_similarity (_structural_similarity.py), written out: filters of the frames and their products."""
    if gaussian:
        sigma, truncate = 1.5, 3.5
        win_size = 2 * int(truncate * sigma + 0.5) + 1
        filt = lambda a: ndi.gaussian_filter(a, sigma=sigma, truncate=truncate, mode="reflect")  # noqa: E731
    else:
        filt = lambda a: ndi.uniform_filter(a, size=win_size, mode="reflect")  # noqa: E731
    NP = win_size ** 2
    cov_norm = NP / (NP - 1) if sample_covariance else 1.0
    ux, uy = filt(r), filt(x)
    uxx, uyy, uxy = filt(r * r), filt(x * x), filt(r * x)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    a1, a2, b1, b2 = 2 * ux * uy + c1, 2 * vxy + c2, ux ** 2 + uy ** 2 + c1, vx + vy + c2
    S = (a1 * a2) / (b1 * b2)
    pad = (win_size - 1) // 2
    return S, S[pad:-pad, pad:-pad].mean(), win_size


@pytest.mark.parametrize("gaussian,sample", [(True, False), (False, True), (False, False)])
def test_model_matches_the_scikit_image_formula(gaussian, sample):
    r = RNG.poisson(40.0, (40, 53)).astype(np.float32)
    x = (r + RNG.normal(0.0, 4.0, r.shape)).astype(np.float32)
    L = 64.0
    S, mssim, n = skimage_formula(r.astype(np.float64), x.astype(np.float64), L, gaussian, sample_covariance=sample)
    taps = M.ssim_taps() if gaussian else None
    cov = n * n / (n * n - 1.0) if sample else 1.0
    crop = (n - 1) // 2
    m = M.model_ssim(r, x, n, n, taps, taps, "reflect", 0.0, (0.01 * L) ** 2, (0.03 * L) ** 2, cov, crop=(crop, crop))
    frac = float(np.max(np.abs(m["ssim_map"] - S) / float64_bound(m, "ssim_map")))
    fmean = float(abs(m["ssim"] - mssim) / m["tol_ssim"])
    print(f"gaussian={gaussian} sample={sample}: map {frac:.3f}, mean {fmean:.3f} of the bound")
    assert frac <= 1.0 and fmean <= 1.0
    assert 0.3 < mssim < 0.99


def test_pool2_model_on_odd_shapes():
    for shape in ((2, 7, 9), (1, 8, 5), (3, 2, 2), (5, 6)):
        x = RNG.standard_normal(shape).astype(np.float32)
        got = M.pool2(x)
        assert got.dtype == np.float32 and got.shape == shape[:-2] + (shape[-2] // 2, shape[-1] // 2)
        for idx in np.ndindex(got.shape):
            y, c = idx[-2], idx[-1]
            blk = x[idx[:-2] + (slice(2 * y, 2 * y + 2), slice(2 * c, 2 * c + 2))]
            want = np.float32(np.float32(np.float32(blk[0, 0] + blk[0, 1]) + np.float32(blk[1, 0] + blk[1, 1])) * np.float32(0.25))
            assert got[idx] == want
    assert np.array_equal(M.pool2(np.full((4, 6), 3.0, dtype=np.float32)), np.full((2, 3), 3.0, dtype=np.float32))


def test_ms_ssim_smallest_admissible_side():
    from barc4dip_amd.metrics import perceptual as P

    assert M.ms_ssim_min_side(11, 5) == 176 == P.ms_ssim_min_side(11, 5)
    assert M.ms_ssim_min_side(7, 3) == 28 == P.ms_ssim_min_side(7, 3) and M.ms_ssim_min_side(11, 1) == 11
    for size, scales in ((11, 5), (7, 3), (3, 4)):
        need = M.ms_ssim_min_side(size, scales)
        for n, ok in ((need, True), (need - 1, False)):
            side = n
            for _ in range(scales - 1):
                side //= 2          # what pool2 leaves
            assert (side >= size) == ok
    m = M.model_ms_ssim(RNG.poisson(40.0, (1, 44, 47)).astype(np.float32), RNG.poisson(40.0, (1, 44, 47)).astype(np.float32),
                        weights=(0.3, 0.7), sy=11, sx=11, wy=M.ssim_taps(), wx=M.ssim_taps(), c1=C1, c2=C2, crop=(5, 5))
    assert m["ssim"].shape == (1, 2) and np.isclose(m["ms_ssim"][0], max(m["cs"][0, 0], 0) ** 0.3 * max(m["ssim"][0, 1], 0) ** 0.7, rtol=1e-14)


def test_error_model():
    r = RNG.poisson(40.0, (2, 9, 13)).astype(np.float32)
    x = r.copy()
    x[1, 3, 4] += 3.0
    m = M.model_frame_errors(r, x)
    assert m["mse"][0] == 0.0 and m["psnr"][0] == np.inf and m["max_abs"][1] == 3.0 and m["mse"][1] == 9.0 / 117.0
    assert m["data_range"] == float(r.max() - r.min())
    assert np.isclose(m["psnr"][1], 10 * np.log10(m["data_range"] ** 2 / m["mse"][1]))
    assert np.isclose(m["nrmse"][1], np.sqrt(m["mse"][1]) / np.sqrt(np.mean(r[1].astype(np.float64) ** 2)))


def test_argument_errors_without_a_device(monkeypatch):
    from barc4dip_amd import _ffi
    from barc4dip_amd.metrics import frame_errors, ms_ssim, mse, nrmse, psnr, ssim

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the arguments were checked")

    monkeypatch.setattr(_ffi, "require_gpu", no_device)
    img = np.ones((32, 32), dtype=np.float32)
    stack = np.ones((3, 32, 32), dtype=np.float32)
    big = np.ones((176, 200), dtype=np.float32)
    bad = [
        lambda: ssim(img, np.ones((32, 31))), lambda: ssim(stack, img), lambda: ssim(stack, np.ones((2, 32, 32))), lambda: ssim(np.ones(32), img),
        lambda: ssim(img, np.ones((1, 3, 32, 32))), lambda: ssim(np.ones((0, 32)), np.ones((0, 32))), lambda: ssim(img, np.ones((0, 32, 32))),
        lambda: ssim(img, img, window="hann", data_range=1.0), lambda: ssim(img, img, window="gaussian", sample_covariance=True, data_range=1.0),
        lambda: ssim(img, img, window="box", size=1, sample_covariance=True, data_range=1.0),
        lambda: ssim(img, img, data_range=0.0), lambda: ssim(img, img, data_range=-2.0), lambda: ssim(img, img, data_range=float("nan")),
        lambda: ssim(img, img, window="box", size=0, data_range=1.0), lambda: ssim(img, img, window="box", size=64, data_range=1.0),
        lambda: ssim(img, img, window="box", size=(63, 26), data_range=1.0), lambda: ssim(img, img, sigma=10.0, data_range=1.0),
        lambda: ssim(img, img, sigma=-1.0, data_range=1.0), lambda: ssim(img, img, mode="edge", data_range=1.0),
        lambda: ssim(img, img, K1=0.0, data_range=1.0), lambda: ssim(img, img, K2=-1.0, data_range=1.0),
        lambda: ssim(np.ones((9, 13)), np.ones((9, 13)), data_range=1.0),                  # the crop leaves nothing
        lambda: ms_ssim(img, img, data_range=1.0), lambda: ms_ssim(np.ones((175, 200)), np.ones((175, 200)), data_range=1.0),
        lambda: ms_ssim(np.ones((176, 175)), np.ones((176, 175)), data_range=1.0), lambda: ms_ssim(big, big, weights=(), data_range=1.0),
        lambda: ms_ssim(big, big, weights=(0.5, -0.5), data_range=1.0), lambda: ms_ssim(big, big, window="tri", data_range=1.0),
        lambda: ms_ssim(big, np.ones((2, 176, 201)), data_range=1.0), lambda: ms_ssim(big, big, data_range=0.0),
        lambda: frame_errors(img, stack[:, :31]), lambda: frame_errors(img, img, data_range=0.0), lambda: mse(stack, img),
        lambda: psnr(img, img, data_range=-1.0), lambda: psnr(img, np.ones((31, 32))), lambda: nrmse(img, img, normalization="max"),
        lambda: nrmse(img, np.ones((2, 2))),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} raised nothing")
    with pytest.raises(ValueError, match="176"):
        ms_ssim(img, img, data_range=1.0)
    with pytest.raises(ValueError, match="31"):
        ssim(img, img, sigma=10.0, data_range=1.0)


def test_lds_formula_and_window_limit():
    from barc4dip_amd.metrics import perceptual as P

    assert P.lds_bytes(11, 11) == 68672 and P.lds_bytes(33, 33) == 114816
    assert all(P.lds_bytes(sy, sx) <= P.LDS_LIMIT for sy in range(1, 53) for sx in range(1, 53))
    assert P.lds_bytes(53, 53) > P.LDS_LIMIT and P.lds_bytes(63, 25) <= P.LDS_LIMIT < P.lds_bytes(63, 26)
    assert P.lds_bytes(48, 63) <= P.LDS_LIMIT < P.lds_bytes(49, 63)
    # that the kernel's layout and constants are these: tests/test_window_core_host.py, which runs csrc/b4d_window.hpp


def test_wiring():
    import barc4dip_amd.metrics as metrics
    from barc4dip_amd import _ffi

    for name in ("ssim", "ms_ssim", "frame_errors", "mse", "psnr", "nrmse", "perceptual"):
        assert hasattr(metrics, name) and name in metrics.__all__
    header = open(os.path.join(ROOT, "include", "b4d.h")).read()
    makefile = open(os.path.join(ROOT, "barc4dip_amd", "csrc", "Makefile")).read()
    for sym in ("b4d_ssim", "b4d_pair_errors", "b4d_pool2"):
        assert re.search(r"\bint " + sym + r"\(", header) and sym in _ffi.SIGNATURES
    src = re.search(r"^SRC = (.*)$", makefile, re.M).group(1).split()
    assert "b4d_perceptual.hip" in src
    assert len(_ffi.SIGNATURES["b4d_ssim"][1]) == 21 and len(_ffi.SIGNATURES["b4d_pair_errors"][1]) == 8
