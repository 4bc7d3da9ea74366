"""Speckle scanning on the MI355X (b4d_speckle_scan through barc4dip_amd.signal.speckle_scan) against the float64 model of
tests/scanning_model.py on the same float32 input.

Bars.  Kernel and model differ in the order of float64 sums of at most 31^2 x 4096 terms (14 400 in the cases here) whose
cancellation after the shift by one pixel of the tile is at most about 100 x: below 2e-10 on rho.  So
  correlation                    1e-9 absolute          on all valid pixels
  transmission, dark_field       1e-9 relative          on all valid pixels
  integer parts of dy, dx        exact                  where the model's margin between best and second-best rho is above 1e-8
  sub-pixel parts                1e-6 px                where both model curvatures are at least 1e-3 in magnitude
                                                        (3 eps / |curvature| with eps = 1e-9)
  valid, edge, NaN pattern       exact                  everywhere
and each of the two exclusions may drop at most 1 % of a case's valid pixels.  Every deviation is reported through ``observe``
as a fraction of its bar; the observed maxima are listed in DESIGN.md section 24."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from scipy import ndimage

from scanning_model import band_limited, scan_model

pytestmark = pytest.mark.gpu

PLANES = ("dy", "dx", "correlation", "transmission", "dark_field")
BAR_RHO, BAR_REL, BAR_SUB = 1e-9, 1e-9, 1e-6
MIN_MARGIN, MIN_CURV, MAX_DROP = 1e-8, 1e-3, 0.01


@pytest.fixture(scope="module")
def scan():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import speckle_scan

    return speckle_scan


def _pair(v):
    return (int(v[0]), int(v[1])) if np.ndim(v) else (int(v), int(v))


@functools.lru_cache(maxsize=None)
def make_scan(N, shape, seed, search, dtype="float32", counts=None, contrast=None):
    """(reference, sample), read-only: a band-limited scan and the same scan resampled along a smooth field that reaches 0.85 x
    the search range (so that integer peaks land on its border), times a smooth gain, plus a little noise."""
    H, W = shape
    sy, sx = _pair(search)
    R = band_limited((N, H, W), seed)
    if counts:
        R = counts * (1.0 + contrast * (R - 100.0) / 25.0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fy = 0.85 * sy * np.sin(x / 9.0 + 0.3)
    fx = -0.85 * sx * np.cos(y / 7.0)
    S = np.stack([ndimage.map_coordinates(R[n], [y - fy, x - fx], order=3, mode="nearest") for n in range(N)])
    S = S * (0.8 + 0.1 * np.sin(y / 15.0) * np.cos(x / 13.0))
    S = S + 0.02 * R.std() * np.random.default_rng(seed + 1).standard_normal(S.shape)
    if np.dtype(dtype).kind in "ui":
        R, S = np.rint(R), np.rint(S)
    R, S = R.astype(dtype), S.astype(dtype)
    R.setflags(write=False)
    S.setflags(write=False)
    return R, S


def _freeze(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, np.ndarray)) else v) for k, v in kw.items()))


_MODELS = {}


def model_of(key, R, S, **kw):
    """The model of one scan, computed once per (input name, arguments)."""
    k = (key, _freeze(kw))
    if k not in _MODELS:
        kw = dict(kw)
        if "weights" in kw and kw["weights"] is not None:
            kw["weights"] = list(kw["weights"])
        _MODELS[k] = scan_model(R, S, **dict(kw, subpixel=True))
    return _MODELS[k]


def compare(observe, name, scan, key, R, S, **kw):
    """Device against model for one scan, sub-pixel step on and off."""
    kw = {k: v for k, v in kw.items() if k != "subpixel"}
    want = model_of(key, R, S, **kw)
    on = scan(R, S, subpixel=True, **kw)
    off = scan(R, S, subpixel=False, **kw)
    H, W = R.shape[-2:]
    assert on["meta"]["step"] == (1, 1) and on["meta"]["n_positions"] == R.shape[0] and on["meta"]["subpixel"] is True
    np.testing.assert_array_equal(on["y"], np.arange(H, dtype=np.float64))
    np.testing.assert_array_equal(on["x"], np.arange(W, dtype=np.float64))
    ok = ~np.isnan(want["correlation"])
    nv = int(ok.sum())
    mc = kw.get("min_correlation")
    for got in (on, off):
        for pl in PLANES:
            assert got[pl].dtype == np.float64 and got[pl].shape == (H, W)
            np.testing.assert_array_equal(np.isnan(got[pl]), ~ok, err_msg=f"{name}: NaN pattern of {pl}")
        np.testing.assert_array_equal(got["edge"], want["edge"], err_msg=f"{name}: edge")
        assert got["peak"] is got["correlation"] or np.array_equal(got["peak"], got["correlation"], equal_nan=True)
        if mc is None:
            np.testing.assert_array_equal(got["valid"], ok, err_msg=f"{name}: valid")
        else:   # a correlation within the bar of the threshold may fall on either side
            sure = ~ok | (np.abs(np.where(ok, want["correlation"], 0.0) - mc) > BAR_RHO)
            np.testing.assert_array_equal(got["valid"][sure], want["valid"][sure], err_msg=f"{name}: valid")
            assert (~sure).sum() <= MAX_DROP * nv
    for pl in ("correlation", "transmission", "dark_field"):     # the integer run reports the same peak values
        np.testing.assert_array_equal(on[pl], off[pl])
    if nv == 0:
        return want, on
    observe(f"scanning.{name}.correlation", np.max(np.abs(on["correlation"] - want["correlation"])[ok]) / BAR_RHO, 1.0)
    for pl in ("transmission", "dark_field"):
        observe(f"scanning.{name}.{pl}", np.max(np.abs(on[pl] / want[pl] - 1.0)[ok]) / BAR_REL, 1.0)
    clear = ok & (want["margin"] > MIN_MARGIN)
    assert (ok & ~clear).sum() <= MAX_DROP * nv, f"{name}: {(ok & ~clear).sum()} of {nv} pixels have a margin below {MIN_MARGIN}"
    np.testing.assert_array_equal(off["dy"][clear], want["uy"][clear].astype(np.float64), err_msg=f"{name}: integer dy")
    np.testing.assert_array_equal(off["dx"][clear], want["ux"][clear].astype(np.float64), err_msg=f"{name}: integer dx")
    cy, cx = want["curv_y"], want["curv_x"]
    with np.errstate(invalid="ignore"):
        curved = clear & (np.isnan(cy) | (np.abs(cy) >= MIN_CURV)) & (np.isnan(cx) | (np.abs(cx) >= MIN_CURV))
    assert (clear & ~curved).sum() <= MAX_DROP * nv, f"{name}: {(clear & ~curved).sum()} of {nv} pixels have a curvature below {MIN_CURV}"
    print(f"{name}: {nv} valid, smallest margin {np.nanmin(want['margin']):.2e}, smallest curvature "
          f"{np.nanmin(np.abs(np.stack([cy, cx]))) if np.isfinite(np.stack([cy, cx])).any() else np.nan:.2e}")
    for ax, u in (("dy", "uy"), ("dx", "ux")):
        d_got = on[ax][curved] - off[ax][curved]
        d_want = want[ax][curved] - want[u][curved]
        assert np.all(np.abs(d_got) <= 0.5)
        if d_got.size:
            observe(f"scanning.{name}.sub{ax[1]}", np.max(np.abs(d_got - d_want)) / BAR_SUB, 1.0)
    return want, on


# ---- a: the base case, every option
@pytest.mark.parametrize("taper", ["flat", "hann"])
def test_a_tapers(scan, observe, taper):
    R, S = make_scan(4, (40, 48), 1, 2)
    want, got = compare(observe, f"a.{taper}", scan, "a", R, S, window=5, search=2, taper=taper)
    assert want["edge"].sum() > 20 and (want["valid"] & ~want["edge"]).sum() > 200      # peaks on the search border occur here
    assert got["meta"] == {"window": (5, 5), "step": (1, 1), "search": (2, 2), "taper": taper, "subpixel": True, "n_positions": 4,
                           "min_correlation": None}


def test_a_weights_and_threshold(scan, observe):
    R, S = make_scan(4, (40, 48), 1, 2)
    g = (1.0, 0.0, 2.5, 0.5)
    want, _ = compare(observe, "a.weights", scan, "a", R, S, window=5, search=2, weights=g)
    drop = scan(R[[0, 2, 3]], S[[0, 2, 3]], window=5, search=2, weights=[1.0, 2.5, 0.5])
    unit = model_of("a", R, S, window=5, search=2)
    assert not np.array_equal(want["correlation"], unit["correlation"], equal_nan=True)
    ok = want["valid"]
    assert np.max(np.abs(drop["correlation"] - want["correlation"])[ok]) <= BAR_RHO    # weight 0 is a position left out
    want, got = compare(observe, "a.min_correlation", scan, "a", R, S, window=5, search=2, min_correlation=0.9)
    assert 0 < got["valid"].sum() < (~np.isnan(got["correlation"])).sum()              # the threshold cuts, the planes stay


# ---- b ... e: shapes
@pytest.mark.parametrize("name, N, shape, window, search, taper", [
    ("b", 5, (37, 61), (3, 7), (1, 3), "hann"),      # rectangular, sides that divide by nothing
    ("c", 3, (70, 150), 9, 4, "hann"),               # crosses every tile border on both axes
    ("d", 2, (64, 80), 31, 16, "hann"),              # the limits: 2 x 18 valid pixels, 16-px tiles
    ("d0", 2, (64, 80), 31, 0, "flat"),              # search 0: one candidate, every pixel on the border
    ("e", 1, (40, 48), 7, 2, "flat"),                # a single position
    ("w15", 2, (50, 70), (15, 3), (2, 5), "flat"),   # the largest window of the 32-px tile
    ("w17", 2, (50, 70), (3, 17), (5, 0), "hann"),   # the smallest of the 16-px tile; search 0 on one axis
])
def test_shapes(scan, observe, name, N, shape, window, search, taper):
    R, S = make_scan(N, shape, sum(map(ord, name)), search)
    want, _ = compare(observe, name, scan, name, R, S, window=window, search=search, taper=taper)
    (wy, wx), (sy, sx) = _pair(window), _pair(search)
    assert want["valid"].sum() == (shape[0] - 2 * (wy // 2 + sy)) * (shape[1] - 2 * (wx // 2 + sx))
    if name == "d":
        assert want["valid"].sum() == 2 * 18
    if name == "d0":
        assert want["edge"][want["valid"]].all()


# ---- f: detector words at low contrast
def test_f_low_contrast_uint16(scan, observe):
    R, S = make_scan(4, (40, 48), 7, 2, dtype="uint16", counts=30000.0, contrast=0.01)
    assert R.dtype == np.uint16 and 0.009 < R.std() / R.mean() < 0.011 and 29000 < R.mean() < 31000
    want, _ = compare(observe, "f", scan, "f", R, S, window=5, search=2)
    assert want["valid"].sum() == 32 * 40


# ---- g: the smallest frame
@pytest.mark.parametrize("window, search", [(5, 2), ((3, 7), (1, 3)), (1, 1)])
def test_g_one_valid_pixel(scan, observe, window, search):
    (wy, wx), (sy, sx) = _pair(window), _pair(search)
    shape = (wy + 2 * sy, wx + 2 * sx)
    R, S = make_scan(3, shape, 21, search)
    name = f"g.{wy}x{wx}"
    want, got = compare(observe, name, scan, name, R, S, window=window, search=search, taper="flat")
    assert want["valid"].sum() == 1 and got["valid"][shape[0] // 2, shape[1] // 2]


# ---- h: batches and input kinds
def test_h_batch_and_input_kinds(scan):
    import torch

    R, S0 = make_scan(4, (40, 48), 1, 2)
    S = np.stack([S0, make_scan(4, (40, 48), 2, 2)[1], make_scan(4, (40, 48), 3, 2)[1]])
    kw = dict(window=5, search=2)
    batch = scan(R, S, **kw)
    keys = PLANES + ("peak", "edge", "valid")
    for m in range(3):
        alone = scan(R, S[m], **kw)
        for k in keys:
            assert batch[k].shape == (3, 40, 48) and alone[k].shape == (40, 48)
            np.testing.assert_array_equal(batch[k][m], alone[k], err_msg=f"scan {m}, {k}")
    assert not np.array_equal(batch["dy"][0], batch["dy"][1], equal_nan=True)
    f64 = scan(R.astype(np.float64), S.astype(np.float64), **kw)
    dev = scan(torch.from_numpy(R.copy()).cuda(), torch.from_numpy(S.copy()).cuda(), **kw)
    ten = scan(torch.from_numpy(R.copy()).cuda(), torch.from_numpy(S.copy()).cuda(), return_tensors=True, **kw)
    for k in keys:
        np.testing.assert_array_equal(f64[k], batch[k])
        np.testing.assert_array_equal(dev[k], batch[k])
        assert ten[k].is_cuda and ten[k].dtype == (torch.bool if k in ("edge", "valid") else torch.float64)
        np.testing.assert_array_equal(ten[k].cpu().numpy(), batch[k])
    assert isinstance(ten["y"], np.ndarray) and ten["meta"] == batch["meta"]


# ---- i: values that are not finite
def test_i_non_finite_values(scan, observe):
    R0, S0 = make_scan(4, (40, 48), 1, 2)
    kw = dict(window=5, search=2)
    # (array, position, y, x, value): (30, 30) is the pixel whose value a 32-px tile subtracts before its sums
    plants = [("R", 1, 20, 25, np.nan), ("S", 2, 12, 30, np.inf), ("R", 0, 30, 30, np.nan), ("S", 0, 33, 9, -np.inf)]
    R, S, Rz, Sz = R0.copy(), S0.copy(), R0.copy(), S0.copy()
    named = np.zeros((40, 48), bool)
    yy, xx = np.mgrid[0:40, 0:48]
    for arr, n, y, x, v in plants:
        (R if arr == "R" else S)[n, y, x] = v
        (Rz if arr == "R" else Sz)[n, y, x] = 0.0
        reach = 2 if arr == "R" else 4            # the window; the window grown by the search
        named |= (np.abs(yy - y) <= reach) & (np.abs(xx - x) <= reach)
    inside = np.zeros((40, 48), bool)
    inside[4:36, 4:44] = True
    got, zero = scan(R, S, **kw), scan(Rz, Sz, **kw)
    for k in PLANES:
        np.testing.assert_array_equal(np.isnan(got[k]), named | ~inside, err_msg=k)
        np.testing.assert_array_equal(got[k][~named], zero[k][~named], err_msg=k)     # bit for bit
        assert not np.isnan(zero[k][inside]).any()
    for k in ("valid", "edge"):
        assert not got[k][named].any()
        np.testing.assert_array_equal(got[k][~named], zero[k][~named])
    compare(observe, "i", scan, "i", R, S, **kw)                                      # and the model agrees on all of it
    # a value that is not finite in a position of weight 0 changes nothing
    g = [1.0, 1.0, 0.0, 2.0]
    Rn, Sn = R0.copy(), S0.copy()
    Rn[2, 18, 18], Sn[2, 22, 30], Sn[2, 0, 0] = np.nan, np.inf, np.nan
    a, b = scan(Rn, Sn, weights=g, **kw), scan(R0, S0, weights=g, **kw)
    for k in PLANES + ("valid", "edge"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["valid"][18, 18] and a["valid"][22, 30]


# ---- j: a patch without contrast
def test_j_constant_patch(scan, observe):
    R, S0 = make_scan(4, (40, 48), 1, 2)
    S = S0.copy()
    S[:, 14:26, 20:32] = 80.0
    want, got = compare(observe, "j", scan, "j", R, S, window=5, search=2)
    dead = np.zeros((40, 48), bool)
    dead[18:22, 24:28] = True                     # window + search inside the patch: no candidate is defined
    np.testing.assert_array_equal(np.isnan(got["dy"][4:36, 4:44]), dead[4:36, 4:44])
    assert not got["valid"][dead].any() and not got["edge"][dead].any()
    assert got["valid"][17, 25] and got["valid"][22, 28]      # some candidates defined: compared with the model above


# ---- k: ground truth
def test_k_ground_truth_and_downstream(scan, observe):
    from barc4dip_amd.signal import wavefront_from_displacement

    a, b = 0.7, 12.5
    R = band_limited((3, 128, 128), 31)
    S = np.empty_like(R)
    shifts = {(0, 0): (3, -2), (0, 1): (-3, 3), (1, 0): (0, 1), (1, 1): (-1, 0)}
    uy, ux = np.zeros((128, 128)), np.zeros((128, 128))
    for (ty, tx), (dy, dx) in shifts.items():
        sl = (slice(None), slice(64 * ty, 64 * ty + 64), slice(64 * tx, 64 * tx + 64))
        S[sl] = a * np.roll(R[sl], (dy, dx), axis=(1, 2)) + b            # S[p + u] = a R[p] + b
        uy[sl[1:]], ux[sl[1:]] = dy, dx
    R, S = R.astype(np.float32), S.astype(np.float32)
    m = scan(R, S, window=5, search=4, subpixel=False)
    t = np.arange(128) % 64
    one = (t >= 6 + 3) & (t < 64 - 6 - 3)                                # reach 2 + 4 and a 3-px wrap inside one tile
    inside = one[:, None] & one[None, :]
    assert m["valid"][inside].all()
    np.testing.assert_array_equal(m["dy"][inside], uy[inside])
    np.testing.assert_array_equal(m["dx"][inside], ux[inside])
    observe("scanning.k.correlation", np.max(np.abs(m["correlation"][inside] - 1.0)) / BAR_RHO, 1.0)
    observe("scanning.k.slope", np.max(np.abs(m["dark_field"] * m["transmission"] - a)[inside]) / 1e-6, 1.0)
    sub = scan(R, S, window=5, search=4)
    np.testing.assert_array_equal(np.rint(sub["dy"][inside]), uy[inside])
    np.testing.assert_array_equal(np.rint(sub["dx"][inside]), ux[inside])
    w = wavefront_from_displacement(sub, pixel_size=1e-6, distance=0.5, mask=sub["valid"])
    assert isinstance(w, dict)
    from barc4dip_amd.preprocessing.distortion import correct_distortion

    back = correct_distortion(S[0], m)                                   # the sample displaced by the field matches the reference
    assert back.shape == (128, 128)
    assert np.max(np.abs(back - (a * R[0] + b))[inside]) < 1e-2          # float32 cubic interpolation at integer shifts
