"""Focal-spot prediction on the MI355X (b4d_focal_spot, barc4dip_amd/signal/focus.py) against the float64 oracle of
tests/test_focus_host.py.  The device works on float32 figure errors and amplitudes; the oracle reads the same float32 values.

Physical parameters of every case (test_focus_host.py): lambda = 1.24e-10 m, node spacing 1.04e-4 m, R = (0.75002, 0.74998) m,
tilt coefficients 1e-7 and -2e-7, c4 = 2e-6, a smooth figure error of 0.05 lambda rms, planes -0.75 + delta with
|delta| <= 5e-5 m.  Every case asserts phase_step < pi from focus_geometry: an undersampled input cannot pass as a numerical error.

Bars.  Intensity and Strehl: 2e-5 of the plane's largest reference value, the project's 1e-5 amplitude bar of the c2c engine
doubled for the square -- a cap, not a measurement.  Total: 2e-6 relative against the Parseval value.  Marginals: 2e-5 of their
own maximum.  Centroid and sigma, in bins: CENTROID_BAR, twice the largest value observed on the device over cases 1-5 (the
moments weight the far wings by p^2), capped at 0.05 bin.  peak_index: equal to the oracle's; every case asserts that the
oracle's two largest values differ by more than the intensity bar.  fwhm: 1e-3 bin against width_at_fraction of the oracle's
marginals.  Observed maxima on an MI355X are listed in DESIGN.md section 16."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from test_focus_host import (COEFF, H, LAM, Z0, case_maps, centroid_sigma, disc_mask, gaussian_amp, plane)

pytestmark = pytest.mark.gpu

INT_BAR = 2e-5
TOTAL_BAR = 2e-6
MARG_BAR = 2e-5
CENTROID_BAR = 3.7e-6   # bins: 2 x 1.83e-6, the largest value observed over cases 1-5 (case 4, centroid); the cap is 0.05
FWHM_BAR = 1e-3         # bins


@pytest.fixture(scope="module")
def focus():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import focus

    return focus


def _amp(kind, shape, T):
    if kind == "none":
        return None
    if kind == "shared":
        return gaussian_amp(shape)
    return np.stack([gaussian_amp(shape, 0.8 - 0.2 * t) for t in range(T)])


@functools.lru_cache(maxsize=None)
def _oracle(shape, canvas, deltas, T, disc, amp_kind):
    """Inputs and the oracle's planes of a case, computed once and shared."""
    e = case_maps(shape, T, seed=shape[0])
    mask = None
    if disc:     # map 0 carries the aperture as NaN, the others through the mask
        m = disc_mask(shape)
        e[0] = np.where(m, e[0], np.nan)
        mask = np.stack([np.ones(shape, bool)] + [m] * (T - 1))
    amp = _amp(amp_kind, shape, T)
    z = Z0 + np.asarray(deltas)
    ref = [[plane(e[t], None if amp is None else (amp if amp.ndim == 2 else amp[t]), COEFF, H, H, LAM, zk, canvas,
                  mask=None if mask is None else mask[t]) for zk in z] for t in range(T)]
    for a in (e,) + (() if mask is None else (mask,)) + (() if amp is None else (amp,)):
        a.setflags(write=False)
    return e, mask, amp, z, ref


def _run(focus, e, mask, amp, z, canvas, **kw):
    return focus.focal_spot(e, wavelength=LAM, spacing=(H, H), planes=z, amplitude=amp, mask=mask, coefficients=COEFF, canvas=canvas, **kw)


def _compare(observe, name, res, ref, canvas):
    from barc4dip_amd.maths.stats import width_at_fraction

    Py, Px = canvas
    assert np.max(res["phase_step"]) < np.pi
    T, Z = res["strehl"].shape
    assert res["intensity"].shape == (T, Z, Py, Px) and res["intensity"].dtype == np.float32
    for t in range(T):
        for k in range(Z):
            o = ref[t][k]
            top2 = np.partition(o["I"].ravel(), -2)[-2:]
            assert top2[1] - top2[0] > INT_BAR * top2[1], "the oracle's peak is not unique enough for an index comparison"
            observe(f"focus.{name}.intensity", np.max(np.abs(res["intensity"][t, k] - o["I"])) / o["peak"], INT_BAR)
            observe(f"focus.{name}.strehl", abs(res["strehl"][t, k] - o["peak"]) / o["peak"], INT_BAR)
            want = Py * Px * o["sum_a2"] / o["sum_a"] ** 2
            observe(f"focus.{name}.total", abs(res["total"][t, k] - want) / want, TOTAL_BAR)
            observe(f"focus.{name}.marg_x", np.max(np.abs(res["profile_x"][t, k] - o["marg_x"])) / np.max(o["marg_x"]), MARG_BAR)
            observe(f"focus.{name}.marg_y", np.max(np.abs(res["profile_y"][t, k] - o["marg_y"])) / np.max(o["marg_y"]), MARG_BAR)
            assert tuple(res["peak_index"][t, k]) == o["peak_index"]
            cy, cx, sy, sx = centroid_sigma(o["total"], o["moments"])
            dy, dx = res["pixel_size"][k]
            sgn = np.sign(res["planes"][k])
            got = (sgn * res["centroid_y"][t, k] / dy, sgn * res["centroid_x"][t, k] / dx, res["sigma_y"][t, k] / dy, res["sigma_x"][t, k] / dx)
            for lab, g, w in zip(("centroid_y", "centroid_x", "sigma_y", "sigma_x"), got, (cy, cx, sy, sx)):
                print(f"focus.{name}[{t},{k}].{lab}: {abs(g - w):.3e} bin")
                observe(f"focus.{name}.{lab[:-2]}", abs(g - w), CENTROID_BAR)
            observe(f"focus.{name}.fwhm", abs(res["fwhm_y"][t, k] / dy - width_at_fraction(o["marg_y"], fraction=0.5)[0]), FWHM_BAR)
            observe(f"focus.{name}.fwhm", abs(res["fwhm_x"][t, k] / dx - width_at_fraction(o["marg_x"], fraction=0.5)[0]), FWHM_BAR)
    np.testing.assert_allclose(res["sum_amplitude"], [r[0]["sum_a"] for r in ref], rtol=1e-13, atol=0)


CASES = {
    "c1_7x5_64": ((7, 5), (64, 64), (0.0, 5e-5), 1, False, "none"),                 # DFT-matrix engine, pupil far smaller than a tile
    "c2_33x47_128": ((33, 47), (128, 128), (-2e-5, 2e-5), 1, False, "none"),        # odd sides, nx > ny
    "c4_128_1024": ((128, 128), (1024, 1024), (0.0,), 1, False, "none"),            # the transform route above 512
    "c5_20x30_96x160": ((20, 30), (96, 160), (3e-5,), 1, False, "shared"),          # Py != Px, no power of two
}
C3_DELTAS = tuple(np.linspace(-5e-5, 5e-5, 5))


@pytest.mark.parametrize("name", list(CASES))
def test_planes_match_the_oracle(focus, observe, name):
    shape, canvas, deltas, T, disc, amp_kind = CASES[name]
    e, mask, amp, z, ref = _oracle(*CASES[name])
    _compare(observe, name, _run(focus, e[0] if T == 1 else e, mask, amp, z, canvas), ref, canvas)


@pytest.mark.parametrize("amp_kind", ["none", "shared", "per_map"])
def test_batch_of_masked_maps(focus, observe, amp_kind):
    """Case 3: two (48, 40) maps on canvas 256 in 5 planes: a disc aperture as NaN (map 0) and through the mask (map 1), without
    an amplitude, with one shared by both maps (stride 0) and with one per map; 10 (map, plane) pairs in one pass of the plan."""
    args = ((48, 40), (256, 256), C3_DELTAS, 2, True, amp_kind)
    e, mask, amp, z, ref = _oracle(*args)
    _compare(observe, "c3_" + amp_kind, _run(focus, e, mask, amp, z, (256, 256)), ref, (256, 256))


KEYS = ("intensity", "strehl", "peak_index", "total", "centroid_y", "centroid_x", "sigma_y", "sigma_x", "fwhm_y", "fwhm_x", "profile_y",
        "profile_x", "moments", "sum_amplitude")


def _assert_same(a, b, keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_results_do_not_depend_on_the_chunk_or_the_run(focus):
    """Cases 3 (chunk boundary) and 8: a plan chunk of 3 cuts the 10 pairs into 3 + 3 + 3 + 1, across maps and planes; every output
    carries the same bits as the call in one pass, and as a second run."""
    e, mask, amp, z, _ = _oracle((48, 40), (256, 256), C3_DELTAS, 2, True, "per_map")
    one = _run(focus, e, mask, amp, z, (256, 256))
    again = _run(focus, e, mask, amp, z, (256, 256))
    cut = _run(focus, e, mask, amp, z, (256, 256), chunk=3)
    _assert_same(one, again)
    _assert_same(one, cut)


@pytest.mark.parametrize("crop", [(31, 17), (32, 64), (128, 128)])
def test_crop_is_a_slice_of_the_canvas(focus, crop):
    e, mask, amp, z, _ = _oracle(*CASES["c2_33x47_128"])
    full = _run(focus, e[0], mask, amp, z, (128, 128))
    win = _run(focus, e[0], mask, amp, z, (128, 128), crop=crop)
    cy, cx = crop
    y0, x0 = 64 - cy // 2, 64 - cx // 2
    assert win["intensity"].shape == (1, 2, cy, cx)
    np.testing.assert_array_equal(win["intensity"], full["intensity"][:, :, y0:y0 + cy, x0:x0 + cx])
    _assert_same(full, win, keys=KEYS[1:])
    none = _run(focus, e[0], mask, amp, z, (128, 128), crop=False)
    assert "intensity" not in none
    _assert_same(full, none, keys=KEYS[1:])


def test_empty_map_next_to_a_valid_one(focus):
    e, _, _, z, _ = _oracle(*CASES["c2_33x47_128"])
    both = np.stack([np.full_like(e[0], np.nan), e[0]])
    res = _run(focus, both, None, None, z, (128, 128), crop=(16, 16))
    alone = _run(focus, e[0], None, None, z, (128, 128), crop=(16, 16))
    for k in ("strehl", "total", "centroid_y", "centroid_x", "sigma_y", "sigma_x", "fwhm_y", "fwhm_x", "profile_y", "profile_x", "intensity"):
        assert np.all(np.isnan(res[k][0])), k
        np.testing.assert_array_equal(res[k][1], alone[k][0], err_msg=k)
    assert np.all(res["peak_index"][0] == -1) and res["sum_amplitude"][0] == 0.0
    np.testing.assert_array_equal(res["peak_index"][1], alone["peak_index"][0])


def test_dict_input_tensors_and_caustic(focus):
    import torch

    shape = (33, 47)
    e, _, _, z, _ = _oracle(*CASES["c2_33x47_128"])
    plain = _run(focus, e[0], None, None, z, (128, 128))
    step, pix = 16.0, H / 16.0
    d = {"wavefront": e[0].astype(np.float64), "coefficients": COEFF[None], "remove": "quadratic", "y": 40 + step * np.arange(shape[0]),
         "x": 8 + step * np.arange(shape[1]), "valid": np.ones(shape, bool)}
    via = focus.focal_spot(d, wavelength=LAM, pixel_size=pix, planes=z, canvas=128, return_tensors=True)
    assert torch.is_tensor(via["intensity"]) and via["intensity"].is_cuda
    # the spacing 16 * (H / 16) is H to an ulp: same geometry to rounding, not to the bit
    np.testing.assert_allclose(via["intensity"].cpu().numpy(), plain["intensity"], rtol=0, atol=1e-6 * float(plain["strehl"].max()))
    np.testing.assert_allclose(via["strehl"], plain["strehl"], rtol=1e-6)
    cau = focus.beam_caustic(e[0], span=4e-5, n_planes=3, z_focus=Z0, wavelength=LAM, spacing=(H, H), coefficients=COEFF, canvas=128)
    assert "intensity" not in cau and cau["profile_x"].shape == (1, 3, 128) and cau["profile_y"].shape == (1, 3, 128)
    np.testing.assert_allclose(cau["z"], Z0 + np.array([-2e-5, 0.0, 2e-5]), rtol=1e-15)
    assert cau["best_focus"][0] == cau["z"][int(np.argmax(cau["strehl"][0]))]
    np.testing.assert_array_equal(cau["strehl"][0, [0, 2]], plain["strehl"][0])


def test_c_abi_argument_errors(focus):
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    gen, pow2 = _ffi.get_plan(64, 96, 4, general=True), _ffi.get_plan(64, 64, 4)
    e = torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda")
    c = torch.from_numpy(COEFF[None].copy()).cuda()
    stats = torch.zeros((1, 2, 10), dtype=torch.float64, device="cuda")
    inten = torch.zeros((1, 2, 64, 96), dtype=torch.float32, device="cuda")
    ws = torch.zeros(max(1, int(lib.b4d_focal_spot_workspace_bytes(gen.handle, 1, 2))), dtype=torch.uint8, device="cuda")
    assert int(lib.b4d_focal_spot_workspace_bytes(pow2.handle, 1, 2)) == 0 and int(lib.b4d_focal_spot_workspace_bytes(gen.handle, 1, 0)) == 0

    def call(plan=gen, ny=8, nx=8, z=(Z0, Z0 + 1e-5), nz=None, cy=0, cx=0, out=None, lam=LAM):
        zb = (C.c_double * max(len(z), 1))(*z)
        return lib.b4d_focal_spot(plan.handle, D.ptr(e), None, 0, 1, ny, nx, D.ptr(c), H, H, lam, C.cast(zb, C.c_void_p),
                                  len(z) if nz is None else nz, cy, cx, None if out is None else D.ptr(out), D.ptr(stats), None, None,
                                  D.ptr(ws), _ffi.stream_ptr())

    assert call() == 0
    assert call(cy=64, cx=96, out=inten) == 0
    torch.cuda.synchronize()
    for bad, word in ((dict(plan=pow2), "general"), (dict(ny=65), "fit"), (dict(nx=97), "fit"), (dict(cy=65, cx=96, out=inten), "crop"),
                      (dict(cy=64, cx=97, out=inten), "crop"), (dict(nz=0), "nz"), (dict(z=(Z0, 0.0)), "plane"),
                      (dict(z=(float("nan"),)), "plane"), (dict(z=(float("inf"),)), "plane"), (dict(lam=float("nan")), "wavelength"),
                      (dict(lam=float("inf")), "wavelength")):
        assert call(**bad) == -1, bad
        assert word in lib.b4d_last_error().decode(), (bad, lib.b4d_last_error())
