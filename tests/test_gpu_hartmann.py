"""GPU tier of the Hartmann analysis (csrc/b4d_hartmann.hip, barc4dip_amd.signal.hartmann) against the float64 model of
tests/hartmann_model.py, whose own checks are in tests/test_hartmann_host.py.

Bars (a mismatch beyond them is a bug in the kernel, not a tolerance to widen):
  exact     peak, peak_y, peak_x, the three counts, the background for none / min / a number, and the NaN pattern of every map;
  1e-9 px   cy, cx: at most 16 384 non-negative terms summed in float64 in another order, a relative n 2^-53 on sums taken about
            the cell centre, times a lever of at most 128 px: 5e-10;
  1e-8 px   the iteratively weighted centre: each round adds an error of that size plus a few ulp of exp, and the iteration
            contracts (by sigma_s^2 / (sigma_s^2 + sigma_w^2) for a Gaussian spot), so errors do not grow with the count;
  1e-10     relative, for flux, the ring mean (the background under "border"), the noise and the variances: sums of non-negative
            terms (on these frames), with room for the square root.  Two floors, from what the quantities are made of: the
            variances are taken about a centre that may itself differ by the 1e-9 px above, which moves them by up to
            (1e-9 px)^2 = 1e-18 px^2 (all there is in a cell with one pixel above the threshold); cov_yx is a sum of terms of
            either sign of size sqrt(var_y var_x), so that is the scale its 1e-10 refers to.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hartmann_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

DATA = M.case_data()
EXACT = ("peak", "peak_y", "peak_x") + M.COUNTS


def hm():
    import barc4dip_amd.signal.hartmann as h

    return h


def run(name, method, background, threshold, frames=None, **kw):
    frames0, cells = DATA[name]
    return hm().spot_centroids(frames0 if frames is None else frames, cells, method=method, background=background,
                               threshold=threshold, **M.CASES[name][2], **kw)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    g, w = (np.ascontiguousarray(a).ravel().view(f"u{a.itemsize}") for a in (got, want))
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{bad.size} of {got.size} values differ; first at {np.unravel_index(bad[:3], got.shape)}"


def worst(got, want, scale=None):
    """Largest |got - want| (over `scale` where given) on the cells that are not NaN in the model."""
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    d = np.abs(got[ok] - want[ok])
    return float((d / scale[ok] if scale is not None else d).max())


@pytest.mark.parametrize("method,background,threshold", M.OPTION_SETS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_spot_centroids_match_the_model(name, method, background, threshold, observe):
    got = run(name, method, background, threshold)
    m = M.case_model(name, background, threshold)
    frames, cells = DATA[name]
    assert got["cy"].shape == frames.shape[:-2] + cells["shape"]
    for k in EXACT:
        assert got[k].dtype == (np.int64 if k in M.COUNTS else np.float64), k
        assert np.array_equal(got[k], m[k], equal_nan=True), k
    if background != "border":
        assert np.array_equal(got["background"], m["background"], equal_nan=True)
    want = dict(m)
    if method == "iwcog":
        want["cy"], want["cx"] = m["cy_iw"], m["cx_iw"]
    for k in M.QUANTITIES:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"NaN pattern of {k}"
    tag = "iwcog" if method == "iwcog" else "cog"
    bar = 1e-8 if method == "iwcog" else 1e-9
    observe(f"hartmann_{tag}_px", max(worst(got["cy"], want["cy"]), worst(got["cx"], want["cx"])), bar)
    for k in ("flux", "background", "noise"):
        observe(f"hartmann_{k}_rel", worst(got[k], want[k], np.maximum(np.abs(want[k]), 1e-300)), 1e-10)
    for k in ("var_y", "var_x"):
        observe("hartmann_var_rel", worst(got[k], want[k], np.abs(want[k]) + 1e-8), 1e-10)      # 1e-10 (|var| + 1e-8) = .. + 1e-18
    with np.errstate(invalid="ignore"):
        observe("hartmann_cov_rel", worst(got["cov_yx"], want["cov_yx"], np.sqrt(want["var_y"] * want["var_x"]) + 1e-8), 1e-10)
    assert np.array_equal(got["y"], cells["y"]) and np.array_equal(got["x"], cells["x"])
    assert got["meta"]["method"] == method and got["meta"]["pitch"] == cells["pitch"]


def test_a_frame_alone_gives_the_bits_of_the_batch_and_of_a_second_call():
    for method in M.METHODS:
        batch = run("ragged", method, "border", 0.2)
        again = run("ragged", method, "border", 0.2)
        for k in M.QUANTITIES:
            same_bits(again[k], batch[k])
        for f in range(3):
            alone = run("ragged", method, "border", 0.2, frames=DATA["ragged"][0][f])
            for k in M.QUANTITIES:
                same_bits(alone[k], batch[k][f])
    both = run("aligned", "iwcog", "min", 0.0)
    alone = run("aligned", "iwcog", "min", 0.0, frames=DATA["aligned"][0][1])       # the second frame: another 16-byte phase is not possible
    for k in M.QUANTITIES:
        same_bits(alone[k], both[k][1])


def test_tensors_in_and_out_and_host_layouts():
    import torch

    frames, cells = DATA["ragged"]
    plain = run("ragged", "cog", "border", 0.1)
    t = run("ragged", "cog", "border", 0.1, frames=torch.from_numpy(frames).cuda(), return_tensors=True)
    for k in M.QUANTITIES:
        assert isinstance(t[k], torch.Tensor) and t[k].is_cuda and t[k].dtype == torch.float64, k
        same_bits(t[k].cpu().numpy().astype(plain[k].dtype), plain[k])
    big = np.zeros(frames.shape[:-1] + (2 * frames.shape[-1],), dtype=np.float32)
    big[..., ::2] = frames
    layouts = {"big_endian": frames.astype(">f4"), "strided": big[..., ::2], "float64": frames.astype(np.float64),
               "uint16": frames.astype(np.uint16), "cuda_strided": torch.from_numpy(big).cuda()[..., ::2]}
    for name, a in layouts.items():
        got = run("ragged", "cog", "border", 0.1, frames=a)
        for k in M.QUANTITIES:
            same_bits(got[k], plain[k])
    # an unaligned device view of 16-byte-friendly frames takes the scalar loads and gives the same bits
    al, cells_al = DATA["aligned"]
    pad = torch.zeros(al.size + 1, dtype=torch.float32, device="cuda")
    pad[1:] = torch.from_numpy(al).cuda().reshape(-1)
    assert pad[1:].data_ptr() % 16 == 4
    a = run("aligned", "iwcog", "border", 0.2)
    b = hm().spot_centroids(pad[1:].reshape(al.shape), cells_al, method="iwcog", background="border", threshold=0.2)
    for k in M.QUANTITIES:
        same_bits(b[k], a[k])


def test_c_abi_errors():
    import ctypes as C

    import torch

    from barc4dip_amd import _ffi

    x = torch.zeros((1, 64, 64), dtype=torch.float32, device="cuda")
    out = torch.zeros((1, 2, 2, 14), dtype=torch.float64, device="cuda")
    good = np.array([0, 32, 64], dtype=np.int32)

    def call(ye=good, xe=good, mode=3, value=0.0, thr=0.1, method=0, sigma=8.0, its=8, sat=np.inf, ny=64):
        return _ffi.lib().b4d_spot_centroids(C.c_void_p(x.data_ptr()), 1, ny, 64, ye.ctypes.data_as(C.c_void_p), ye.size - 1,
                                             xe.ctypes.data_as(C.c_void_p), xe.size - 1, mode, value, thr, method, sigma, its, sat,
                                             C.c_void_p(out.data_ptr()), _ffi.stream_ptr())

    assert call() == 0
    torch.cuda.synchronize()
    EINVAL, ESIZE = -1, -2
    assert call(ye=np.array([0, 32, 65], np.int32)) == EINVAL and call(ye=np.array([-1, 32, 64], np.int32)) == EINVAL
    assert call(xe=np.array([0, 40, 40], np.int32)) == EINVAL and call(xe=np.array([0, 40, 30], np.int32)) == EINVAL
    assert call(xe=np.array([0, 1, 64], np.int32)) == ESIZE
    assert call(mode=4) == EINVAL and call(mode=1, value=np.nan) == EINVAL and call(thr=1.0) == EINVAL and call(thr=np.nan) == EINVAL
    assert call(method=2) == EINVAL and call(method=1, sigma=0.0) == EINVAL and call(method=1, its=-1) == EINVAL
    assert call(sat=np.nan) == EINVAL
    with pytest.raises(_ffi.B4DError, match="b4d_spot_centroids"):
        _ffi.check(call(thr=1.0))


# ------------------------------------------------------------------------------------------------------------------ end to end
SHAPE, PITCH, ORIGIN = (246, 292), 24.0, (3.3, 1.7)      # 10 x 12 cells
# Noiseless spots on a zero background, measured as the bound of tests/test_hartmann_host.py is derived: the whole cell weighs in
# (background none, threshold 0), so what is left is the cut tail, 1e-4 px.  A threshold clips the spot's skirt unevenly over the
# pixel phase (the S-curve of the thresholded centre of gravity: 1e-2 px at the default 0.1 on these frames, from the model on
# the CPU); that is the estimator's bias on its default options, not a kernel error, and no 1e-3 px bound holds for it.
OPTS = dict(background="none", threshold=0.0)


def _programmed(y, x):
    """dy = a (y - yc), dx = b (x - xc) with a largest shift of 3 px (at the lattice's corners) along x and 2.4 px along y."""
    yc, xc = 0.5 * (y[0, 0] + y[-1, 0]), 0.5 * (x[0, 0] + x[0, -1])
    return 2.4 / (y[-1, 0] - yc) * (y - yc) + 0 * x, 3.0 / (x[0, -1] - xc) * (x - xc) + 0 * y


@pytest.fixture(scope="module")
def pair():
    from barc4dip_amd import synth

    ref = synth.hartmann_frame(SHAPE, PITCH, ORIGIN, sigma=2.0)
    img = synth.hartmann_frame(SHAPE, PITCH, ORIGIN, _programmed, sigma=2.0)
    return ref, img


def test_lattice_of_the_reference(pair, observe):
    ref, _ = pair
    lat = hm().hartmann_lattice(ref, **OPTS)
    assert lat["shape"] == (10, 12)
    observe("hartmann_lattice_pitch_px", max(abs(lat["pitch"][0] - PITCH), abs(lat["pitch"][1] - PITCH)), 1e-3)
    observe("hartmann_lattice_origin_px", max(abs(lat["origin"][0] - ORIGIN[0]), abs(lat["origin"][1] - ORIGIN[1])), 1e-3)
    assert abs(lat["rotation"]) <= 1e-5
    given = hm().hartmann_lattice(ref, pitch=23.6, **OPTS)          # a pitch that is 2 % off still finds the lattice
    assert abs(given["pitch"][0] - PITCH) <= 1e-3 and abs(given["origin"][1] - ORIGIN[1]) <= 1e-3


def test_displacement_to_wavefront(pair, observe):
    from barc4dip_amd.signal import wavefront_from_displacement

    ref, img = pair
    h = hm()
    m = h.hartmann_displacement(ref, img, **OPTS)
    assert m["dy"].shape == (10, 12) and m["valid"].dtype == np.bool_ and m["valid"].all()
    ty, tx = _programmed(m["y"][:, None], m["x"][None, :])
    assert max(np.abs(ty).max(), np.abs(tx).max()) == pytest.approx(3.0, abs=0.01)
    observe("hartmann_displacement_px", max(np.abs(m["dy"] - ty).max(), np.abs(m["dx"] - tx).max()), 1e-3)
    assert m["peak"].max() == 1.0 and m["peak"].min() > 0.9 and np.all(m["snr"] >= 3.0)
    assert np.abs(m["transmission"] - 1.0).max() < 1e-3 and np.abs(m["dark_field"]).max() < 1e-2
    kw = dict(pixel_size=6.5e-6, distance=0.5)
    w = wavefront_from_displacement(m, weights="peak", mask=m["valid"], **kw)
    truth = dict(m, dy=ty, dx=tx)
    wt = wavefront_from_displacement(truth, weights="peak", mask=m["valid"], **kw)
    for k in ("radius_x", "radius_y"):
        assert np.isfinite(wt[k][0]) and wt[k][0] != 0.0
        observe(f"hartmann_{k}_rel", abs(w[k][0] / wt[k][0] - 1.0), 5e-3)
    # absolute mode on the image alone: shifts against the nominal positions of the programmed lattice
    cells = h.hartmann_cells(SHAPE, PITCH, ORIGIN)
    a = h.hartmann_displacement(None, img, cells=cells, **OPTS)
    assert a["valid"].all() and a["meta"]["absolute"]
    ty, tx = _programmed(cells["y"][:, None], cells["x"][None, :])
    observe("hartmann_absolute_px", max(np.abs(a["dy"] - ty).max(), np.abs(a["dx"] - tx).max()), 1e-3)
    assert np.isnan(a["transmission"]).all()
    # a stack of images, tensors out
    t = h.hartmann_displacement(ref, np.stack([img, ref]), cells=cells, return_tensors=True, **OPTS)
    assert t["dy"].shape == (2, 10, 12) and t["dy"].is_cuda and bool(t["valid"].all())
    assert float(t["dy"][1].abs().max()) == 0.0 and np.abs(t["dx"][0].cpu().numpy() - tx).max() <= 1e-3


def test_validity_on_the_edge_frame():
    frames, cells = DATA["edge"]
    h = hm()
    m = h.hartmann_displacement(None, frames, cells=cells, saturation=M.SATURATION)
    bad = [M.EDGE_CELLS[k] for k in ("constant", "all_nan", "saturated")]
    want = np.ones(cells["shape"], dtype=bool)
    for i, j in bad:
        want[i, j] = False
    assert np.array_equal(m["valid"], want), m["valid"]
    assert np.isnan(m["dy"][~want]).all() and np.isnan(m["dx"][~want]).all() and np.all(m["peak"][~want] == 0.0)
    assert np.isfinite(m["dy"][want]).all() and np.all(m["peak"][want] > 0.0) and m["peak"].max() == 1.0
    # against itself as the reference: zero shifts where valid
    r = h.hartmann_displacement(frames, frames, cells=cells, saturation=M.SATURATION)
    assert np.array_equal(r["valid"], want) and np.all(r["dy"][want] == 0.0) and np.all(r["transmission"][want] == 1.0)
