"""GPU tier of the separable filters and local statistics (csrc/b4d_smooth.hip) against scipy.ndimage in float64 and the float64
models of tests/smoothing_model.py, on the float64 cast of the same float32 frames.

Tiles of the kernels: fused route 64 x 64 outputs per workgroup (half-widths up to 4; up to 24 with ``_fused=True``); two-pass route 512 x 8 (row
kernel) and 32 x 256 (column kernel); local statistics 32 x 32.  The base stack (3, 70, 150) is ragged in both axes with an odd row
length and crosses the 64-, 32- and 8-wide tile edges; its [:, :, :148] slice takes the 16-byte path; TALL (1, 262, 522) crosses
the 256-row and the 512-column edge of the two-pass kernels.

Bounds, all formed from the data by smoothing_model: |out - ref| <= 1.01 u M A_y A_x ((K_y + 4) + (K_x + 4))
for the filter, E + u |out| for the subtracting and |x| E / g^2 + 2 u |out| for the dividing epilogue; local statistics one float32
ulp of the model plus the cancellation term.  Exact tests compare bits."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smoothing_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = sorted(M.MODES)
RNG = np.random.default_rng(26)
STACK = RNG.poisson(40.0, (3, 70, 150)).astype(np.float32)
STACK148 = np.ascontiguousarray(STACK[:, :, :148])
TALL = RNG.poisson(40.0, (1, 262, 522)).astype(np.float32)
SMALL = RNG.poisson(40.0, (2, 9, 13)).astype(np.float32)
ROUTES = ({}, {"_general": True}, {"_fused": True})      # default route; two-pass everywhere; fused up to 49 taps
TWO_PASS = ({},)                                         # beyond 49 taps per axis


def prep():
    import barc4dip_amd.preprocessing as p
    return p


def f64(x):
    return np.asarray(x, dtype=np.float64)


def within(got, ref, bound, what=""):
    """NaN in the same places, and |got - ref| <= bound elsewhere; returns the largest fraction of the bound."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN footprint differs"
    ok = ~np.isnan(ref)
    with np.errstate(invalid="ignore"):
        skip = ~ok | (np.isinf(ref) & (got == ref))
        d = np.where(skip, 0.0, np.abs(got - ref))
        b = np.where(skip, 1.0, np.maximum(np.broadcast_to(bound, d.shape), 1e-300))
    frac = float(np.max(d / b))
    print(f"{what}: {frac:.3f} of the bound")
    assert frac <= 1.0, f"{what}: {frac:.3f} of the bound"
    return frac


def emulate_f32(x, wy, wx, mode, cval):
    """The kernels' arithmetic restated: taps rounded to float32; a sum starts from -0 and adds fma(w[k], x, acc) in ascending k;
    rows first.  The fma is formed in float64 (the product of two float32 is exact there) and rounded to float32."""
    def axis_pass(a, w, axis):
        w = np.asarray(w, dtype=np.float64).astype(np.float32)
        n = a.shape[axis]
        pos = np.arange(n) - w.size // 2
        acc = np.full(a.shape, -0.0, dtype=np.float32)
        for k in range(w.size):
            src = M._take(a, M.border_index(pos + k, n, mode), axis, np.float32(cval))
            with np.errstate(invalid="ignore", over="ignore"):
                acc = (acc.astype(np.float64) + np.float64(w[k]) * src.astype(np.float64)).astype(np.float32)
        return acc
    return axis_pass(axis_pass(np.asarray(x, dtype=np.float32), wx, x.ndim - 1), wy, x.ndim - 2)


# ------------------------------------------------------------------------------------------------------------ 1, 2: exact
@pytest.mark.parametrize("n", [1, 2, 5, 8, 33, 64])
def test_impulse_is_the_outer_product_of_the_taps(n):
    """A single 1.0 in a zero frame: away from the borders the output is float32(wy)[:, None] * float32(wx)[None, :] rounded once,
    reversed and placed as the model places it, bit for bit; near each corner under every mode (the impulse's mirror images fall
    into the window) it is the kernels' restated arithmetic, bit for bit.  Pins tap extent, even-size offset, order and borders."""
    p = prep()
    wy, wx = RNG.standard_normal(n), RNG.standard_normal(n)
    routes = ROUTES if n <= 33 else TWO_PASS
    x = np.zeros((1, 140, 150), dtype=np.float32)
    x[0, 70, 75] = 1.0
    prod = (wy.astype(np.float32)[:, None] * wx.astype(np.float32)[None, :]).astype(np.float32)
    want = np.zeros_like(x)
    lo, hi = n // 2, n - 1 - n // 2         # out[i] = w[k] at i = 70 + n // 2 - k
    want[0, 70 - hi:70 + lo + 1, 75 - hi:75 + lo + 1] = prod[::-1, ::-1]
    for g in routes:
        got = p.separable_filter(x, wy, wx, **g)
        assert np.array_equal(got, want), f"route {g}"
    frame = np.zeros((4, 70, 150), dtype=np.float32)
    for i, (r, c) in enumerate([(1, 2), (0, 148), (68, 0), (69, 149)]):
        frame[i, r, c] = 1.0
    for mode in MODES:
        want = emulate_f32(frame, wy, wx, mode, 0.0)
        for g in routes:
            got = p.separable_filter(frame, wy, wx, mode=mode, **g)
            assert np.array_equal(got, want), f"{mode}, route {g}"


@pytest.mark.parametrize("mode", MODES)
def test_dyadic_taps_are_exact(mode):
    """Taps {1/4, 1/2, 1/4} and boxes of 2, 4, 8 on small-integer frames: every partial sum is representable, so the result is
    SciPy's float64 result cast to float32, on both routes and both access widths."""
    p = prep()
    ints = RNG.integers(0, 64, (2, 70, 150)).astype(np.float32)
    for x in (ints, np.ascontiguousarray(ints[:, :, :148])):
        w = np.array([0.25, 0.5, 0.25])
        ref = ndi.correlate1d(ndi.correlate1d(f64(x), w, axis=-1, mode=mode, cval=3.0), w, axis=-2, mode=mode, cval=3.0)
        for g in ROUTES:
            assert np.array_equal(p.separable_filter(x, w, w, mode=mode, cval=3.0, **g), ref.astype(np.float32))
        for size in (2, 4, 8):
            ref = ndi.uniform_filter(f64(x), size=(1, size, size), mode=mode, cval=3.0)
            for g in ROUTES:
                assert np.array_equal(p.uniform_filter(x, size, mode=mode, cval=3.0, **g), ref.astype(np.float32)), (size, g)


# ------------------------------------------------------------------------------------------------------------ 3, 4: bounds
def gauss_case(x, sigma, order, mode, general, cval=0.0):
    p = prep()
    sy, sx = (sigma, sigma) if np.ndim(sigma) == 0 else sigma
    oy, ox = order
    ref = ndi.gaussian_filter(f64(x), sigma=(0, sy, sx), order=(0, oy, ox), mode=mode, cval=cval)
    got = p.gaussian_filter(x, sigma, order=order, mode=mode, cval=cval, **general)
    assert got.dtype == np.float32
    bound = M.bound_separable(x, M.gaussian_taps(sy, oy), M.gaussian_taps(sx, ox))
    return within(got, ref, bound, f"gaussian sigma={sigma} order={order} {mode} route {general}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sigma", [0.8, 1.0, 1.25, 2.0, 4.0, 4.25, 10.0, 30.0])
def test_gaussian_filter_within_the_bound(mode, sigma):
    """Half-widths 3, 8, 16 on the fused and the two-pass route, 17, 40, 120 on the two-pass route, and 4, 5: either side of the
    boundary between the routes that a plain call takes.  cval = 0 under "constant" with derivative orders (the pass order, see preprocessing/smooth.py)."""
    for x in (STACK, STACK148):
        for g in (ROUTES if sigma <= 4.0 else TWO_PASS):
            gauss_case(x, sigma, (0, 0), mode, g, cval=1.5)
    gauss_case(STACK, sigma, (1, 0), mode, {})
    gauss_case(STACK, sigma, (0, 2), mode, {})


@pytest.mark.parametrize("mode", MODES)
def test_anisotropic_and_one_axis(mode):
    for g in ROUTES:
        gauss_case(STACK, (1.5, 6.0), (0, 0), mode, g, cval=1.5)      # 13 x 49 taps: two-pass; x beyond the fused limit
        gauss_case(STACK, (6.0, 1.5), (0, 0), mode, g, cval=1.5)
        gauss_case(STACK, (0.0, 2.0), (0, 0), mode, g, cval=1.5)      # identity along y
        gauss_case(STACK148, (2.0, 0.0), (0, 0), mode, g, cval=1.5)   # identity along x
    p = prep()
    assert np.array_equal(p.gaussian_filter(STACK, 0.0), STACK) and np.array_equal(p.gaussian_filter(STACK, 0.0, _general=True), STACK)


@pytest.mark.parametrize("size", [3, 6, 63, 511])
def test_uniform_filter_within_the_bound(size):
    p = prep()
    for mode in MODES:
        ref = ndi.uniform_filter(f64(STACK), size=(1, size, size), mode=mode, cval=1.5)
        bound = M.bound_separable(STACK, M.box_taps(size), M.box_taps(size))
        for g in (ROUTES if size <= 33 else TWO_PASS):
            within(p.uniform_filter(STACK, size, mode=mode, cval=1.5, **g), ref, bound, f"uniform {size} {mode} route {g}")


def test_tile_edges_of_the_two_pass_kernels():
    p = prep()
    for sigma in (4.25, 2.0):
        ref = ndi.gaussian_filter(f64(TALL), sigma=(0, sigma, sigma))
        bound = M.bound_separable(TALL, M.gaussian_taps(sigma), M.gaussian_taps(sigma))
        within(p.gaussian_filter(TALL, sigma, _general=True), ref, bound, f"tall sigma={sigma}")
    m = M.model_local_stats(f64(TALL), 7, 7)
    from barc4dip_amd.metrics import local_contrast
    got = local_contrast(TALL, 7)
    tol = M.tolerances_local_stats(m, 7, 7)
    for k in ("mean", "variance", "contrast"):
        within(got[k], m[k].astype(np.float32), tol[k], f"tall local {k}")


@pytest.mark.parametrize("mode", MODES)
def test_overhang_longer_than_the_frame(mode):
    """9 x 13 frames, half-width 20: the window reflects or wraps several times."""
    p = prep()
    w = M.gaussian_taps(5.0, 0, radius=20)
    ref = M.model_separable(f64(SMALL), w, w, mode, 2.5)
    bound = M.bound_separable(SMALL, w, w)
    within(p.gaussian_filter(SMALL, 5.0, radius=20, mode=mode, cval=2.5), ref, bound, f"overhang 20 {mode}")
    w = M.gaussian_taps(5.0, 0, radius=16)
    ref = M.model_separable(f64(SMALL), w, w, mode, 2.5)
    bound = M.bound_separable(SMALL, w, w)
    for g in ROUTES:
        within(p.gaussian_filter(SMALL, 5.0, radius=16, mode=mode, cval=2.5, **g), ref, bound, f"overhang 16 {mode} route {g}")


def _offset_by_one_float(x):
    """x on the device, on a base that is one float past a 16-byte boundary."""
    import torch

    buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 != 0
    return t


@pytest.mark.parametrize("mode", MODES)
def test_halo_wider_than_one_axis_and_one_past_a_tile_edge(mode):
    """The tile stager where its paths meet: one axis of 5 samples under windows of up to 511 taps, the other one element past a
    tile edge (1029 = 2 x 512 + 5 and 16 x 64 + 5; 517 = 2 x 256 + 5 and 8 x 64 + 5; 70 x 516: 516 = 512 + 4 = 16 x 32 + 4), rows
    of 1029 and 5 floats (element by element) and of 516 floats (16 bytes) on an aligned base and on one offset by a float.  Every
    route gives the bits of the restated arithmetic and stays within the bound of the float64 model."""
    from barc4dip_amd.metrics import local_contrast

    p = prep()
    rng = np.random.default_rng(28)
    taps = {n: rng.uniform(0.2, 1.0, n) / n for n in (1, 9, 12, 49, 511)}
    for shape in ((5, 1029), (517, 5), (70, 516)):
        x = rng.poisson(40.0, shape).astype(np.float32)
        off = _offset_by_one_float(x) if shape[1] % 4 == 0 else None
        cases = [(taps[n], taps[n], ROUTES) for n in (1, 9, 12, 49)]
        cases.append((taps[511], None, TWO_PASS) if shape[0] > shape[1] else (None, taps[511], TWO_PASS))
        for wy, wx, routes in cases:
            my, mx = (np.ones(1) if w is None else w for w in (wy, wx))
            want = emulate_f32(x, my, mx, mode, 2.5)
            within(want, M.model_separable(f64(x), my, mx, mode, 2.5), M.bound_separable(x, my, mx), f"{shape} {my.size} x {mx.size} taps {mode}")
            for g in routes:
                assert np.array_equal(p.separable_filter(x, wy, wx, mode=mode, cval=2.5, **g).view(np.uint32), want.view(np.uint32)), (shape, my.size, mx.size, g)
                if off is not None:
                    got = p.separable_filter(off, wy, wx, mode=mode, cval=2.5, **g)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, my.size, mx.size, g, "offset base")
        for size in (63, (3, 9)):
            got, _ = local_case(x, size=size, mode=mode, cval=2.0)
            if off is not None:
                again = local_contrast(off, size, mode=mode, cval=2.0)
                for k in got:
                    assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), (shape, size, k, "offset base")


# ------------------------------------------------------------------------------------------------------------ 5: batches, widths
@pytest.mark.parametrize("sigma,general", [(1.0, {}), (2.0, {"_general": True}), (2.0, {"_fused": True}), (10.0, {})])
def test_batch_independence_and_access_widths(sigma, general):
    import torch

    p = prep()
    whole = p.gaussian_filter(STACK, sigma, **general)
    alone = p.gaussian_filter(STACK[1], sigma, **general)
    assert np.array_equal(whole[1].view(np.uint32), alone.view(np.uint32))
    # the 16-byte path against the dword path on the same values: columns of cval appended by hand, mode "constant"
    lw = int(4.0 * sigma + 0.5)
    wide = p.gaussian_filter(STACK148, sigma, mode="constant", cval=7.0, **general)
    padded = np.concatenate([STACK148, np.full((3, 70, lw + (lw % 2 == 0)), 7.0, dtype=np.float32)], axis=2)
    assert padded.shape[2] % 4 != 0
    ragged = p.gaussian_filter(padded, sigma, mode="constant", cval=7.0, **general)
    assert np.array_equal(wide.view(np.uint32), ragged[:, :, :148].view(np.uint32))
    # ... and on a base that is not 16-byte aligned
    buf = torch.empty(STACK148.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(STACK148.shape)
    t.copy_(torch.from_numpy(STACK148))
    assert t.data_ptr() % 16 != 0
    off = p.gaussian_filter(t, sigma, mode="constant", cval=7.0, **general, return_tensors=True)
    assert np.array_equal(off.cpu().numpy().view(np.uint32), wide.view(np.uint32))
    ref = ndi.gaussian_filter(f64(STACK148), sigma=(0, sigma, sigma), mode="constant", cval=7.0)
    within(wide, ref, M.bound_separable(STACK148, M.gaussian_taps(sigma), M.gaussian_taps(sigma)), "aligned path")


# ------------------------------------------------------------------------------------------------------------ 6: non-finite
@pytest.mark.parametrize("sigma,general", [(1.0, {}), (1.0, {"_general": True}), (3.0, {"_fused": True}), (6.0, {})])
def test_non_finite_input_poisons_its_footprint(sigma, general):
    p = prep()
    x = STACK.copy()
    x[0, 30, 70] = np.nan
    x[1, 2, 147] = np.inf
    x[2, 69, 0] = np.nan
    for mode in ("reflect", "constant", "wrap"):
        w = M.gaussian_taps(sigma)
        ref = M.model_separable(f64(x), w, w, mode, 0.0)
        assert 0 < np.isnan(ref).sum() < ref.size // 2
        got = p.gaussian_filter(x, sigma, mode=mode, **general)
        within(got, ref, M.bound_separable(x, w, w), f"non-finite sigma={sigma} {mode}")
    wz = np.array([0.0, 0.5, 0.0, 0.25, 0.0])      # zero taps poison too
    ref = M.model_separable(f64(x), wz, wz, "reflect")
    for g in ROUTES:
        within(p.separable_filter(x, wz, wz, **g), ref, M.bound_separable(x, wz, wz), "zero taps")


# ------------------------------------------------------------------------------------------------------------ 7: epilogues
@pytest.mark.parametrize("sigma,general", [(1.0, {}), (2.0, {"_general": True}), (2.0, {"_fused": True}), (30.0, {})])
def test_remove_envelope(sigma, general):
    p = prep()
    x = (STACK + 10.0).astype(np.float32)
    w = M.gaussian_taps(sigma)
    g = M.model_separable(f64(x), w, w, "reflect")
    e = M.bound_separable(x, w, w)
    sub = f64(x) - g
    within(p.remove_envelope(x, sigma, method="subtract", **general), sub, M.bound_subtract(e, sub), "subtract")
    div = f64(x) / g
    within(p.remove_envelope(x, sigma, **general), div, M.bound_divide(e, f64(x), g, div), "divide")
    big = p.remove_envelope(x, sigma, eps=1024.0, **general)          # g < eps everywhere: x / eps, rounded once
    assert np.array_equal(big, (x / np.float32(1024.0)).astype(np.float32))
    third = p.remove_envelope(x, sigma, eps=3000.0, **general)
    assert np.array_equal(third, (x / np.float32(3000.0)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ 8: local statistics
def local_case(x, size=None, sigma=None, mode="reflect", cval=0.0):
    from barc4dip_amd.metrics import local_contrast

    if sigma is None:
        sy, sx = (size, size) if np.ndim(size) == 0 else size
        wy = wx = None
        got = local_contrast(x, size, mode=mode, cval=cval)
    else:
        wy = wx = M.gaussian_taps(sigma, 0, 3.0)
        sy = sx = wy.size
        got = local_contrast(x, window="gaussian", sigma=sigma, mode=mode, cval=cval)
    m = M.model_local_stats(f64(x), sy, sx, wy, wx, mode, cval)
    tol = M.tolerances_local_stats(m, sy, sx)
    for k in ("mean", "variance", "contrast"):
        assert got[k].dtype == np.float32 and got[k].shape == x.shape
        within(got[k], m[k].astype(np.float32), tol[k], f"local {k} size={size} sigma={sigma} {mode}")
    return got, m


@pytest.mark.parametrize("mode", MODES)
def test_local_statistics_match_the_model(mode):
    for size in (3, 7, 15, 63, (3, 9)):
        got, m = local_case(STACK, size=size, mode=mode, cval=2.0)
        # integer-valued frames under the box window: the sums are exact and the mean is the model's, cast once
        assert np.array_equal(got["mean"], m["mean"].astype(np.float32))
    for sigma in (1.0, 3.0):
        local_case(STACK148, sigma=sigma, mode=mode, cval=2.0)


def test_local_statistics_edge_values():
    from barc4dip_amd.metrics import local_contrast

    const = np.full((2, 40, 70), 37.0, dtype=np.float32)
    for size in (3, 7, 63):
        got = local_contrast(const, size)
        assert np.all(got["variance"] == 0.0) and np.all(got["contrast"] == 0.0) and np.all(got["mean"] == 37.0)
    z = local_contrast(np.zeros((40, 70), dtype=np.float32), 5)
    assert np.all(np.isnan(z["contrast"])) and np.all(z["mean"] == 0.0) and np.all(z["variance"] == 0.0)
    x = STACK.copy()
    x[0, 30, 70] = np.nan
    x[1, 1, 148] = np.nan
    local_case(x, size=(3, 9))
    local_case(x, sigma=1.0, mode="wrap")


def test_local_stats_null_outputs_through_the_c_abi():
    import torch
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    t = torch.from_numpy(STACK).cuda()
    null = C.c_void_p(0)
    full = {k: torch.empty_like(t) for k in ("m", "v", "c")}
    st = _ffi.stream_ptr()
    assert lib.b4d_local_stats(t.data_ptr(), 3, 70, 150, 5, 7, null, null, 1, 0.0, full["m"].data_ptr(), full["v"].data_ptr(),
                               full["c"].data_ptr(), st) == 0
    for keep in ("m", "v", "c", "mc"):
        outs = {k: torch.full_like(t, -1.0) for k in keep}
        ptr = lambda k: C.c_void_p(outs[k].data_ptr()) if k in outs else null  # noqa: E731
        assert lib.b4d_local_stats(t.data_ptr(), 3, 70, 150, 5, 7, null, null, 1, 0.0, ptr("m"), ptr("v"), ptr("c"), st) == 0
        for k in keep:
            assert torch.equal(outs[k], full[k])
    assert lib.b4d_local_stats(t.data_ptr(), 3, 70, 150, 5, 7, null, null, 1, 0.0, null, null, null, st) == -1


# ------------------------------------------------------------------------------------------------------------ 9: streams
def test_back_to_back_calls_keep_their_taps_and_scratch():
    """Two calls with different sigma queued on one stream without a synchronisation between them, and the same on two streams:
    a later call must not overwrite the taps or the intermediate of an earlier one."""
    import torch

    p = prep()
    x = torch.from_numpy(RNG.poisson(40.0, (8, 512, 512)).astype(np.float32)).cuda()
    want = {s: p.gaussian_filter(x, s, return_tensors=True).clone() for s in (10.0, 7.0, 3.0)}
    torch.cuda.synchronize()
    a = p.gaussian_filter(x, 10.0, return_tensors=True)
    b = p.gaussian_filter(x, 7.0, return_tensors=True)
    c = p.gaussian_filter(x, 3.0, return_tensors=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        d = p.gaussian_filter(x, 10.0, return_tensors=True)
    with torch.cuda.stream(s2):
        e = p.gaussian_filter(x, 7.0, return_tensors=True)
    with torch.cuda.stream(s1):
        f = p.gaussian_filter(x, 7.0, return_tensors=True)
    torch.cuda.synchronize()
    for got, s in ((a, 10.0), (b, 7.0), (c, 3.0), (d, 10.0), (e, 7.0), (f, 7.0)):
        assert torch.equal(got, want[s]), f"sigma {s}"
    ref = ndi.gaussian_filter(f64(x[:1].cpu().numpy()), sigma=(0, 10.0, 10.0))
    xs = x[:1].cpu().numpy()
    within(a[:1].cpu().numpy(), ref, M.bound_separable(xs, M.gaussian_taps(10.0), M.gaussian_taps(10.0)), "stream sigma 10")


# ------------------------------------------------------------------------------------------------------------ 10: C ABI errors
def test_c_abi_argument_errors_leave_the_output_untouched():
    import torch
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    t = torch.from_numpy(STACK).cuda()
    out = torch.full_like(t, -5.0)
    w = np.ones(3) / 3.0
    big = np.ones(512) / 512.0
    wp, bp = w.ctypes.data_as(C.c_void_p), big.ctypes.data_as(C.c_void_p)
    null = C.c_void_p(0)
    st = _ffi.stream_ptr()
    i, o = C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())

    def sep(in_=i, batch=3, ny=70, nx=150, wy=wp, n_y=3, wx=wp, n_x=3, mode=1, epi=0, out_=o):
        return lib.b4d_separable_filter(in_, batch, ny, nx, wy, n_y, wx, n_x, mode, 0.0, epi, 1e-30, 0, out_, st)

    einval = [dict(n_y=0), dict(n_x=0), dict(wy=bp, n_y=512), dict(wx=bp, n_x=512), dict(mode=5), dict(mode=-1), dict(epi=3), dict(epi=-1),
              dict(batch=0), dict(ny=0), dict(nx=0), dict(out_=i), dict(out_=null), dict(in_=null), dict(wy=null), dict(wx=null)]
    for kw in einval:
        assert sep(**kw) == -1, kw
        assert lib.b4d_last_error()
    assert sep(batch=1, ny=65536, nx=32768) == -2
    torch.cuda.synchronize()
    assert bool(torch.all(out == -5.0))
    assert sep() == 0

    def stats(in_=i, batch=3, ny=70, nx=150, sy=3, sx=3, wy=null, wx=null, mode=1, m=o, v=null, c=null):
        return lib.b4d_local_stats(in_, batch, ny, nx, sy, sx, wy, wx, mode, 0.0, m, v, c, st)

    torch.cuda.synchronize()
    out.fill_(-5.0)
    for kw in [dict(sy=0), dict(sx=64), dict(mode=5), dict(batch=0), dict(ny=0), dict(in_=null), dict(m=null), dict(m=i), dict(v=i),
               dict(wy=wp), dict(wx=wp)]:
        assert stats(**kw) == -1, kw
    assert stats(batch=1, ny=65536, nx=32768) == -2
    torch.cuda.synchronize()
    assert bool(torch.all(out == -5.0))
    assert stats() == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out == -5.0))
