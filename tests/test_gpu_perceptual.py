"""GPU tier of SSIM, MS-SSIM, the pair errors and pool2 (csrc/b4d_perceptual.hip) against the float64 models of
tests/perceptual_model.py on the float64 cast of the same float32 frames.

The SSIM kernel works on 32 x 32 tiles.  The base pair (3, 70, 150) is ragged in both axes with an odd row length and crosses the
tile edges; its [:, :, :148] slice takes the 16-byte path; (2, 9, 13) is shorter than the 11-tap window; the (1, 70, 150) pair at
16-bit detector levels (Poisson 40 000) is the case that float32 window sums fail by 1e-2; (2, 176, 200) halves to 11 x 12 at the
fifth scale of MS-SSIM.

Bounds, all formed from the data by perceptual_model: one float32 ulp of the model's value for the maps plus
the propagated float64 rounding of the five window sums through the two quotients; for the means that rounding averaged plus the
summation term; n 2^-53 sum |terms| for the error sums.  pool2 and the identities compare bits.  Every comparison prints the
largest fraction of its bound that was reached."""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceptual_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = sorted(M.MODES)
RNG = np.random.default_rng(28)


def noisy(r, sd):
    return (r + RNG.normal(0.0, sd, r.shape)).astype(np.float32)


REF = RNG.poisson(40.0, (3, 70, 150)).astype(np.float32)
IMG = noisy(REF, 4.0)
DATA = {
    "base": (REF, IMG),
    "w148": (np.ascontiguousarray(REF[:, :, :148]), np.ascontiguousarray(IMG[:, :, :148])),
    "small": (lambda r: (r, noisy(r, 4.0)))(RNG.poisson(40.0, (2, 9, 13)).astype(np.float32)),
    "u16": (lambda r: (r, noisy(r, 200.0)))(RNG.poisson(40000.0, (1, 70, 150)).astype(np.float32)),
    "ms": (lambda r: (r, noisy(r, 4.0)))(RNG.poisson(40.0, (2, 176, 200)).astype(np.float32)),
}
L = {"base": 64.0, "w148": 64.0, "small": 64.0, "u16": 65535.0, "ms": 64.0}
K1, K2 = 0.01, 0.03
# name -> (keyword arguments of metrics.ssim, (sy, sx), taps or None, cov_norm)
WINDOWS = {
    "gauss11": ({}, (11, 11), True, 1.0),
    "box7": ({"window": "box", "size": 7}, (7, 7), False, 1.0),
    "box7s": ({"window": "box", "size": 7, "sample_covariance": True}, (7, 7), False, 49.0 / 48.0),
    "box3x9": ({"window": "box", "size": (3, 9)}, (3, 9), False, 1.0),
    "box6": ({"window": "box", "size": 6}, (6, 6), False, 1.0),
    "box52": ({"window": "box", "size": 52}, (52, 52), False, 1.0),       # the largest square window the LDS holds
    "box63x25": ({"window": "box", "size": (63, 25)}, (63, 25), False, 1.0),
}


def metrics():
    import barc4dip_amd.metrics as m
    return m


def f64(x):
    return np.asarray(x, dtype=np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def within(got, ref, bound, what=""):
    """NaN in the same places, and |got - ref| <= bound elsewhere; prints and returns the largest fraction of the bound."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN footprint differs"
    ok = ~np.isnan(ref)
    with np.errstate(invalid="ignore"):
        skip = ~ok | (np.isinf(ref) & (got == ref))
        d = np.where(skip, 0.0, np.abs(got - ref))
        b = np.where(skip, 1.0, np.maximum(np.broadcast_to(bound, d.shape), 1e-300))
    frac = float(np.max(d / b)) if d.size else 0.0
    print(f"{what}: {frac:.3f} of the bound")
    assert frac <= 1.0, f"{what}: {frac:.3f} of the bound"
    return frac


@functools.lru_cache(maxsize=None)
def model(data, win, mode="reflect", cval=0.0, crop_border=True, shared=False):
    """The model of DATA[data] under WINDOWS[win], computed once and shared; shared: frame 0 of the reference serves every frame."""
    r, x = DATA[data]
    _, (sy, sx), gauss, cov = WINDOWS[win]
    taps = M.ssim_taps() if gauss else None
    crop = ((sy - 1) // 2, (sx - 1) // 2) if crop_border else (0, 0)
    return M.model_ssim(r[0] if shared else r, x, sy, sx, taps, taps, mode, cval, (K1 * L[data]) ** 2, (K2 * L[data]) ** 2, cov, crop)


def call(data, win, mode="reflect", cval=0.0, crop_border=True, shared=False, **kw):
    r, x = DATA[data]
    return metrics().ssim(r[0] if shared else r, x, data_range=L[data], mode=mode, cval=cval, crop_border=crop_border, full=True,
                          **WINDOWS[win][0], **kw)


def check(got, m, what):
    assert got["ssim_map"].dtype == np.float32 and got["ssim"].dtype == np.float64
    for k in ("ssim_map", "cs_map", "ssim", "cs"):
        within(got[k], m[k], m["tol_" + k], f"{what} {k}")


# ------------------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("win", sorted(WINDOWS))
def test_ssim_matches_the_model(mode, win):
    check(call("base", win, mode, 2.0), model("base", win, mode, 2.0), f"{win} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_the_16_byte_path_and_the_short_frame(mode):
    check(call("w148", "gauss11", mode, 2.0), model("w148", "gauss11", mode, 2.0), f"148 wide {mode}")
    check(call("w148", "box6", mode, 2.0), model("w148", "box6", mode, 2.0), f"148 wide box 6 {mode}")
    # 9 x 13, shorter than the window: the borders reflect or wrap more than once; no interior is left to crop to
    check(call("small", "gauss11", mode, 2.0, crop_border=False), model("small", "gauss11", mode, 2.0, crop_border=False), f"9 x 13 {mode}")
    with pytest.raises(ValueError, match="crop_border"):
        call("small", "gauss11", mode)


def test_sixteen_bit_levels_need_the_float64_sums():
    """Poisson 40 000: the variances are differences of window sums near 1.6e9; float32 sums move this map by up to 9e-3."""
    for win in ("gauss11", "box7s"):
        m = model("u16", win)
        check(call("u16", win), m, f"16-bit {win}")
        assert float(np.max(m["tol_ssim_map"])) < 1e-6      # the bound itself is five orders below the float32 failure


def test_crop_border_false_averages_the_whole_frame():
    got, m = call("base", "gauss11", crop_border=False), model("base", "gauss11", crop_border=False)
    check(got, m, "whole frame")
    within(got["ssim"], m["ssim_map"].mean(axis=(1, 2)), m["tol_ssim"], "whole-frame mean")
    cropped = call("base", "gauss11")
    assert same_bits(cropped["ssim_map"], got["ssim_map"]) and not np.array_equal(cropped["ssim"], got["ssim"])


# ------------------------------------------------------------------------------------------------------------ identities, bit for bit
@pytest.mark.parametrize("win", ["gauss11", "box7s", "box3x9", "box52"])
def test_identical_frames_score_exactly_one(win):
    m = metrics()
    for name in ("base", "w148", "u16"):
        r = DATA[name][0]
        for mode in ("reflect", "constant"):
            got = m.ssim(r, r.copy(), data_range=L[name], mode=mode, cval=3.0, full=True, **WINDOWS[win][0])
            assert np.all(got["ssim_map"] == np.float32(1.0)) and np.all(got["cs_map"] == np.float32(1.0)), (name, mode)
            assert np.all(got["ssim"] == 1.0) and np.all(got["cs"] == 1.0), (name, mode)


@pytest.mark.parametrize("win", ["gauss11", "box7s"])
def test_exchanging_reference_and_image_gives_the_same_bits(win):
    m = metrics()
    for name in ("base", "u16"):
        r, x = DATA[name]
        a = m.ssim(r, x, data_range=L[name], full=True, **WINDOWS[win][0])
        b = m.ssim(x, r, data_range=L[name], full=True, **WINDOWS[win][0])
        for k in a:
            assert same_bits(a[k], b[k]), (name, k)


def test_shared_reference_batches_and_single_frames():
    m = metrics()
    r, x = DATA["base"]
    shared = call("base", "gauss11", shared=True)
    check(shared, model("base", "gauss11", shared=True), "shared reference")
    repeated = m.ssim(np.repeat(r[:1], 3, axis=0), x, data_range=64.0, full=True)
    paired = call("base", "gauss11")
    for k in shared:
        assert same_bits(shared[k], repeated[k]), k
    for t in range(3):
        alone = m.ssim(r[t], x[t], data_range=64.0, full=True)
        assert alone["ssim"].shape == () and alone["ssim_map"].shape == (70, 150)
        for k in alone:
            assert same_bits(np.asarray(alone[k]), np.asarray(paired[k][t])), (t, k)
    score = m.ssim(r, x, data_range=64.0)
    assert score.shape == (3,) and score.dtype == np.float64 and same_bits(score, paired["ssim"])


def test_access_widths_agree_where_the_windows_see_the_same_data():
    """The 16-byte path (148 columns) against the dword path on the same values: five columns of cval appended by hand under
    mode "constant" (153 columns, an odd row length), and the 148-wide pair on a base that is one float past a 16-byte boundary."""
    import torch

    m = metrics()
    r, x = DATA["w148"]
    kw = dict(data_range=64.0, mode="constant", cval=7.0, full=True)
    wide = m.ssim(r, x, **kw)
    pad = np.full((3, 70, 5), 7.0, dtype=np.float32)
    ragged = m.ssim(np.concatenate([r, pad], axis=2), np.concatenate([x, pad], axis=2), **kw)
    for k in ("ssim_map", "cs_map"):
        assert same_bits(wide[k], np.ascontiguousarray(ragged[k][:, :, :148])), k

    def offset(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        t = buf[1:].view(a.shape)
        t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % 16 != 0
        return t

    off = m.ssim(offset(r), offset(x), **kw)
    for k in wide:
        assert same_bits(wide[k], off[k]), k
    e = m.frame_errors(r, x)
    eo = m.frame_errors(offset(r), offset(x))
    for k in e:
        assert same_bits(e[k], eo[k]), k


def test_nan_poisons_its_footprint_and_its_frame_only():
    m = metrics()
    r, x = DATA["base"]
    x = x.copy()
    x[1, 30, 70] = np.nan
    for win, (kw, (sy, sx), gauss, cov) in (("gauss11", WINDOWS["gauss11"]), ("box3x9", WINDOWS["box3x9"])):
        taps = M.ssim_taps() if gauss else None
        ref = M.model_ssim(r, x, sy, sx, taps, taps, "reflect", 0.0, (K1 * 64.0) ** 2, (K2 * 64.0) ** 2, cov, ((sy - 1) // 2, (sx - 1) // 2))
        assert int(np.isnan(ref["ssim_map"]).sum()) == sy * sx
        got = m.ssim(r, x, data_range=64.0, full=True, **kw)
        check(got, ref, f"NaN {win}")
        assert np.isnan(got["ssim"][1]) and np.isnan(got["cs"][1]) and not np.isnan(got["ssim"][[0, 2]]).any()
        assert int(np.isnan(got["ssim_map"]).sum()) == sy * sx == int(np.isnan(got["cs_map"][1]).sum())
    rn = r.copy()
    rn[2, 0, 149] = np.nan
    e = m.frame_errors(rn, x, data_range=64.0)
    assert np.isnan(e["mse"][1:]).all() and np.isnan(e["max_abs"][1:]).all() and not np.isnan(e["mse"][0])
    from barc4dip_amd.metrics import perceptual as P
    import torch

    raw = P.run_pair_errors(torch.from_numpy(rn).cuda(), 70 * 150, torch.from_numpy(x).cuda(), 3, 70, 150).cpu().numpy()
    assert not np.isnan(raw[0]).any()
    assert np.isnan(raw[1, [0, 1, 2, 7]]).all() and not np.isnan(raw[1, [3, 4, 5, 6]]).any()      # the NaN is in x
    assert np.isnan(raw[2, [0, 1, 2, 3, 4, 5, 6]]).all() and not np.isnan(raw[2, 7])               # the NaN is in r
    with pytest.raises(ValueError, match="data_range"):
        m.ssim(rn, x)


# ------------------------------------------------------------------------------------------------------------ C ABI
def _abi():
    import torch
    from barc4dip_amd import _ffi

    r, x = (torch.from_numpy(a).cuda() for a in DATA["base"])
    return torch, _ffi.lib(), _ffi.stream_ptr(), r, x


def test_null_output_combinations_and_means_only():
    torch, lib, st, r, x = _abi()
    null = C.c_void_p(0)
    wy = M.ssim_taps()
    wp = wy.ctypes.data_as(C.c_void_p)
    c1, c2 = (K1 * 64.0) ** 2, (K2 * 64.0) ** 2

    def run(s, c, m, box=False):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else null  # noqa: E731
        return lib.b4d_ssim(p(r), 70 * 150, p(x), 3, 70, 150, 7 if box else 11, 7 if box else 11, null if box else wp, null if box else wp, 1, 0.0, c1, c2, 1.0, 5, 5,
                            p(s), p(c), p(m), st)

    for box in (False, True):
        full = {"s": torch.empty_like(x), "c": torch.empty_like(x), "m": torch.empty((3, 2), dtype=torch.float64, device="cuda")}
        assert run(full["s"], full["c"], full["m"], box) == 0
        for keep in ("s", "c", "m", "sm", "cm", "sc"):
            outs = {k: torch.full_like(full[k], -1.0) for k in keep}
            assert run(outs.get("s"), outs.get("c"), outs.get("m"), box) == 0
            for k in keep:
                assert torch.equal(outs[k], full[k]), (keep, k, box)
        assert run(None, None, None, box) == -1


def test_c_abi_argument_errors_leave_the_outputs_untouched():
    torch, lib, st, r, x = _abi()
    null = C.c_void_p(0)
    w = M.ssim_taps()
    wp = w.ctypes.data_as(C.c_void_p)
    smap = torch.full_like(x, -5.0)
    means = torch.full((3, 2), -5.0, dtype=torch.float64, device="cuda")
    errs = torch.full((3, 8), -5.0, dtype=torch.float64, device="cuda")
    pooled = torch.full((3, 35, 75), -5.0, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def ssim(ref=P(r), stride=70 * 150, img=P(x), batch=3, ny=70, nx=150, sy=11, sx=11, wy=wp, wx=wp, mode=1, c1=0.4, c2=3.7, cov=1.0, cy=5, cx=5,
             s=P(smap), c=null, m=P(means)):
        return lib.b4d_ssim(ref, stride, img, batch, ny, nx, sy, sx, wy, wx, mode, 0.0, c1, c2, cov, cy, cx, s, c, m, st)

    einval = [dict(ref=null), dict(img=null), dict(batch=0), dict(ny=0), dict(nx=0), dict(sy=0), dict(sx=64), dict(wy=null), dict(wx=null), dict(mode=5),
              dict(mode=-1), dict(c1=0.0), dict(c2=-1.0), dict(c1=float("nan")), dict(cov=0.0), dict(cy=-1), dict(cy=35), dict(cx=75),
              dict(s=null, m=null), dict(s=P(x)), dict(c=P(r)), dict(s=P(r)), dict(stride=5)]
    for kw in einval:
        assert ssim(**kw) == -1, kw
        assert lib.b4d_last_error()
    assert ssim(sy=53, sx=53, wy=null, wx=null, cy=26, cx=26) == -2 and ssim(sy=63, sx=26, wy=null, wx=null, cy=31, cx=12) == -2
    assert ssim(batch=1, ny=65536, nx=32768) == -2

    def perr(ref=P(r), stride=70 * 150, img=P(x), batch=3, ny=70, nx=150, out=P(errs)):
        return lib.b4d_pair_errors(ref, stride, img, batch, ny, nx, out, st)

    for kw in [dict(ref=null), dict(img=null), dict(out=null), dict(batch=0), dict(ny=0), dict(nx=-1), dict(stride=-1), dict(stride=100), dict(out=P(x))]:
        assert perr(**kw) == -1, kw
    assert perr(batch=1, ny=65536, nx=32768) == -2

    def pool(in_=P(x), batch=3, ny=70, nx=150, out=P(pooled)):
        return lib.b4d_pool2(in_, batch, ny, nx, out, st)

    for kw in [dict(in_=null), dict(out=null), dict(batch=0), dict(ny=1), dict(nx=1), dict(ny=0), dict(out=P(x))]:
        assert pool(**kw) == -1, kw
    torch.cuda.synchronize()
    for t in (smap, means, errs, pooled):
        assert bool(torch.all(t == -5.0))
    assert ssim() == 0 and ssim(cy=34, cx=74) == 0 and ssim(cy=40, m=null) == 0 and perr() == 0 and perr(stride=0) == 0 and pool() == 0
    torch.cuda.synchronize()
    for t in (smap, means, errs, pooled):
        assert not bool(torch.any(t == -5.0))


# ------------------------------------------------------------------------------------------------------------ pool2, MS-SSIM
@pytest.mark.parametrize("shape", [(3, 70, 150), (1, 71, 151), (2, 2, 3)])
def test_pool2_bit_for_bit(shape):
    import torch
    from barc4dip_amd.metrics import perceptual as P

    x = RNG.normal(40.0, 10.0, shape).astype(np.float32)
    got = P.run_pool2(torch.from_numpy(x).cuda(), *shape).cpu().numpy()
    assert same_bits(got, M.pool2(x))


def test_ms_ssim_matches_the_model():
    m = metrics()
    r, x = DATA["ms"]
    taps = M.ssim_taps()
    ref = M.model_ms_ssim(r, x, sy=11, sx=11, wy=taps, wx=taps, c1=(K1 * 64.0) ** 2, c2=(K2 * 64.0) ** 2, crop=(5, 5))
    got = m.ms_ssim(r, x, data_range=64.0, full=True)
    assert got["ssim"].shape == (2, 5) and got["ms_ssim"].shape == (2,) and got["ms_ssim"].dtype == np.float64
    for k in ("ms_ssim", "ssim", "cs"):
        within(got[k], ref[k], ref["tol_" + k], f"ms_ssim {k}")
    assert np.all((got["ms_ssim"] > 0.0) & (got["ms_ssim"] < 1.0))
    assert same_bits(m.ms_ssim(r, x, data_range=64.0), got["ms_ssim"])
    one = m.ms_ssim(r[0], x[0], data_range=64.0, full=True)
    assert one["ms_ssim"].shape == () and one["ssim"].shape == (5,) and same_bits(np.asarray(one["ssim"]), got["ssim"][0])
    assert same_bits(got["ssim"][:, 0].copy(), m.ssim(r, x, data_range=64.0))       # scale 0 is ssim itself
    assert np.all(m.ms_ssim(r, r.copy(), data_range=64.0) == 1.0)
    ref3 = M.model_ms_ssim(r, x, weights=(0.2, 0.3, 0.5), sy=7, sx=7, c1=(K1 * 64.0) ** 2, c2=(K2 * 64.0) ** 2, cov_norm=49.0 / 48.0, crop=(3, 3))
    got3 = m.ms_ssim(r, x, weights=(0.2, 0.3, 0.5), window="box", size=7, sample_covariance=True, data_range=64.0, full=True)
    for k in ("ms_ssim", "ssim", "cs"):
        within(got3[k], ref3[k], ref3["tol_" + k], f"ms_ssim box, three scales {k}")
    with pytest.raises(ValueError, match="176"):
        m.ms_ssim(r[:, :175], x[:, :175], data_range=64.0)
    with pytest.raises(ValueError, match="176"):
        m.ms_ssim(DATA["base"][0], DATA["base"][1], data_range=64.0)


# ------------------------------------------------------------------------------------------------------------ frame errors
@pytest.mark.parametrize("name", ["base", "w148", "small", "u16", "ms"])
def test_frame_errors_match_the_model(name):
    import torch
    from barc4dip_amd.metrics import perceptual as P

    m = metrics()
    r, x = DATA[name]
    b, ny, nx = r.shape
    pe = M.model_pair_errors(r, x)
    raw = P.run_pair_errors(torch.from_numpy(r).cuda(), ny * nx, torch.from_numpy(x).cuda(), b, ny, nx).cpu().numpy()
    within(raw, pe["out"], pe["tol"], f"{name} pair errors")
    for col in (2, 5, 6):
        assert np.array_equal(raw[:, col], pe["out"][:, col])        # the extrema are exact
    for dr in (None, L[name]):
        ref = M.model_frame_errors(r, x, dr)
        got = m.frame_errors(r, x, data_range=dr)
        assert set(got) == {"mse", "rmse", "mae", "max_abs", "psnr", "nrmse"}
        for k in got:
            assert got[k].dtype == np.float64 and got[k].shape == (b,)
            within(got[k], ref[k], ref["tol"][k], f"{name} {k} data_range={dr}")
        within(m.psnr(r, x, data_range=dr), ref["psnr"], ref["tol"]["psnr"], f"{name} psnr()")
    ref = M.model_frame_errors(r, x)
    assert ref["data_range"] == float(r.max() - r.min())
    within(m.mse(r, x), ref["mse"], ref["tol"]["mse"], f"{name} mse()")
    within(m.nrmse(r, x), ref["nrmse"], ref["tol"]["nrmse"], f"{name} nrmse()")
    rmse, t = ref["rmse"], ref["tol"]["rmse"]
    span = f64(r).max(axis=(1, 2)) - f64(r).min(axis=(1, 2))
    within(m.nrmse(r, x, normalization="min-max"), rmse / span, t / span + M.EPS * rmse / span, f"{name} nrmse min-max")
    mean = pe["out"][:, 4] / (ny * nx)
    t_mean = pe["tol"][:, 4] / (ny * nx)
    within(m.nrmse(r, x, normalization="mean"), rmse / mean, t / mean + rmse / mean * t_mean / mean + 2 * M.EPS * rmse / mean, f"{name} nrmse mean")
    # a shared reference frame, one frame, identical frames
    sh = m.frame_errors(r[0], x, data_range=L[name])
    ref = M.model_frame_errors(r[0], x, L[name])
    for k in sh:
        within(sh[k], ref[k], ref["tol"][k], f"{name} shared {k}")
    one = m.frame_errors(r[0], x[0], data_range=L[name])
    assert one["mse"].shape == () and all(same_bits(np.asarray(one[k]), np.asarray(sh[k][0])) for k in one)
    same = m.frame_errors(r, r.copy())
    assert np.all(same["mse"] == 0.0) and np.all(same["psnr"] == np.inf) and np.all(same["max_abs"] == 0.0) and np.all(same["nrmse"] == 0.0)
    assert np.all(m.psnr(r, r.copy()) == np.inf)


def test_data_range_none_is_the_reference_range():
    m = metrics()
    r, x = DATA["base"]
    span = float(r.max() - r.min())
    assert same_bits(m.ssim(r, x), m.ssim(r, x, data_range=span))
    assert same_bits(m.ssim(r[1], x), m.ssim(r[1], x, data_range=float(r[1].max() - r[1].min())))
    assert same_bits(m.ms_ssim(*DATA["ms"]), m.ms_ssim(*DATA["ms"], data_range=float(DATA["ms"][0].max() - DATA["ms"][0].min())))
    with pytest.raises(ValueError, match="data_range"):
        m.ssim(np.full((40, 40), 3.0, dtype=np.float32), np.ones((40, 40), dtype=np.float32))
    with pytest.raises(ValueError, match="data_range"):
        m.psnr(np.full((40, 40), 3.0, dtype=np.float32), np.ones((40, 40), dtype=np.float32))


def test_device_tensors_stay_on_the_device():
    import torch

    m = metrics()
    r, x = (torch.from_numpy(a).cuda() for a in DATA["base"])
    got = m.ssim(r, x, data_range=64.0, full=True, return_tensors=True)
    assert all(v.is_cuda for v in got.values()) and got["ssim"].dtype == torch.float64 and got["ssim_map"].shape == (3, 70, 150)
    host = call("base", "gauss11")
    for k in got:
        assert same_bits(got[k].cpu().numpy(), host[k]), k
    assert m.ssim(r[0], x[0], data_range=64.0, return_tensors=True).shape == ()


# ------------------------------------------------------------------------------------------------------------ streams
def test_back_to_back_calls_keep_their_taps_and_scratch():
    """Calls with different windows (and the error sums between them) queued on one stream without a synchronisation, and the same
    on two streams: a later call must not overwrite the taps or the scratch partials of an earlier one."""
    import torch

    m = metrics()
    r = torch.from_numpy(RNG.poisson(40.0, (8, 256, 256)).astype(np.float32)).cuda()
    x = (r + 3.0 * torch.randn_like(r)).contiguous()
    calls = {
        "g15": lambda: m.ssim(r, x, data_range=64.0, return_tensors=True),
        "g10": lambda: m.ssim(r, x, data_range=64.0, sigma=1.0, return_tensors=True),
        "b7": lambda: m.ssim(r[0], x, data_range=64.0, window="box", size=7, return_tensors=True),
    }
    from barc4dip_amd.metrics import perceptual as P

    errs = lambda: P.run_pair_errors(r, 256 * 256, x, 8, 256, 256)  # noqa: E731
    want = {k: f().clone() for k, f in calls.items()}
    want_e = errs().clone()
    torch.cuda.synchronize()
    assert not torch.equal(want["g15"], want["g10"]) and not torch.equal(want["g15"], want["b7"])
    a, e1, b, c, e2 = calls["g15"](), errs(), calls["g10"](), calls["b7"](), errs()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        d = calls["g15"]()
    with torch.cuda.stream(s2):
        e = calls["g10"]()
    with torch.cuda.stream(s1):
        f = calls["b7"]()
    torch.cuda.synchronize()
    for got, k in ((a, "g15"), (b, "g10"), (c, "b7"), (d, "g15"), (e, "g10"), (f, "b7")):
        assert torch.equal(got, want[k]), k
    assert torch.equal(e1, want_e) and torch.equal(e2, want_e)
