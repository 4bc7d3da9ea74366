"""GPU tier of the spatial rank filters, the range-only variant, outlier repair and the utils functions
(csrc/b4d_rankfilt.hip through barc4dip_amd.preprocessing.rank and barc4dip_amd.utils).

No tolerance appears here: a rank filter is a selection, the outlier test is a chain of singly rounded float32 operations and
the counts are integers, so every comparison is exact equality -- with scipy.ndimage where SciPy defines the result, with the
sort-based NumPy model of tests/test_rank_filter_host.py (itself checked against SciPy and the reference there) where NaN is
involved or SciPy has no such function.  Only percentile_minmax_range keeps the bar that test_gpu_metrics.py and
test_gpu_stats_edges.py use for percentiles_batch (rtol 1e-12 against np.nanpercentile of the float64 cast).

Shapes follow the kernels' tiles: 128 x 32 outputs per workgroup on the register route, 64 x 16 on the general route."""
import ctypes as C

import numpy as np
import pytest
import scipy.ndimage as ndi

from test_rank_filter_host import (MODES, counts_frame, model_filtered_minmax_range, model_median_filter, model_percentile_minmax_range,
                                   model_rank_filter, model_remove_outliers, model_to_uint16, outlier_frame, percentile_rank,
                                   special_frame, window_pair)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi, utils
    from barc4dip_amd.preprocessing import rank

    class E:
        pass

    e = E()
    e.torch, e.D, e.ffi, e.lib, e.R, e.U = torch, D, _ffi, _ffi.lib(), rank, utils
    return e


@pytest.fixture(scope="module")
def stack():
    """(3, 70, 150): 3 x 2 register-route tiles and 5 x 3 general-route tiles, ragged in both axes, odd row length."""
    return np.random.default_rng(21).poisson(40, (3, 70, 150)).astype(np.float32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ a .. e: the filters
@pytest.mark.parametrize("mode", MODES)
def test_a_counts_frame_equals_scipy(env, mode):
    f = counts_frame()
    for size in (3, 5, 7):
        ref = ndi.median_filter(f, size=size, mode=mode, cval=7.0)
        for general in (False, True):
            got = env.R.median_filter(f, size, mode=mode, cval=7.0, _general=general)
            assert got.dtype == np.float32 and np.array_equal(got, ref), (mode, size, general)


@pytest.mark.parametrize("size", [3, 5, 7])
def test_b_stack_over_several_tiles(env, stack, size):
    ref = ndi.median_filter(stack, size=(1, size, size))
    got = env.R.median_filter(stack, size)
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    assert np.array_equal(env.R.median_filter(stack, size, _general=True), got)
    aligned = np.ascontiguousarray(stack[:, :, :148])         # rows of a multiple of four: 16-byte loads and stores
    assert np.array_equal(env.R.median_filter(aligned, size), ndi.median_filter(aligned, size=(1, size, size)))


@pytest.mark.parametrize("mode", MODES)
def test_c_frames_smaller_than_the_window(env, mode):
    rng = np.random.default_rng(22)
    for shape, size in (((4, 5), 7), ((1, 9), 3), ((9, 1), 5), ((1, 1), 3), ((2, 3), 15), ((4, 5), (2, 6))):
        f = rng.normal(size=shape).astype(np.float32)
        ref = ndi.median_filter(f, size=size, mode=mode, cval=-2.5)
        for general in (False, True):
            assert np.array_equal(env.R.median_filter(f, size, mode=mode, cval=-2.5, _general=general), ref), (shape, size, mode, general)


@pytest.mark.parametrize("mode", MODES)
def test_c_halo_wider_than_one_axis_and_one_past_a_tile_edge(env, mode):
    """The tile stager where its paths meet: one axis shorter than the halo (3 rows or 3 columns under windows up to 15 x 15), the
    other one element past a tile edge (261 = 2 x 128 + 5 = 8 x 32 + 5: both routes' tiles; 35 rows, 132 columns), rows of 261 and
    3 floats (element by element), and rows of 132 floats (16 bytes) on an aligned base and on a base offset by one float."""
    rng = np.random.default_rng(27)
    for shape in ((3, 261), (261, 3), (35, 132)):
        f = rng.poisson(40, shape).astype(np.float32)
        f[rng.integers(0, shape[0], 6), rng.integers(0, shape[1], 6)] = 4000.0
        inputs = [f]
        if shape[1] % 4 == 0:
            buf = env.torch.empty(f.size + 1, dtype=env.torch.float32, device="cuda")
            off = buf[1:].view(shape)
            off.copy_(env.torch.from_numpy(f))
            assert off.data_ptr() % 16 != 0
            inputs.append(off)
        refs = {size: ndi.median_filter(f, size=size, mode=mode, cval=7.0) for size in (3, 5, 7)}
        ranks = {(15, 100): ndi.rank_filter(f, 100, size=15, mode=mode, cval=7.0), ((2, 6), 5): ndi.rank_filter(f, 5, size=(2, 6), mode=mode, cval=7.0)}
        want, wmask, wcount = model_remove_outliers(f, 7, scale="mad", threshold=4.0, mode=mode, cval=7.0)
        for x in inputs:
            for size, ref in refs.items():
                for general in (False, True):
                    assert np.array_equal(env.R.median_filter(x, size, mode=mode, cval=7.0, _general=general), ref), (shape, size, general)
            for (size, rank), ref in ranks.items():
                assert np.array_equal(env.R.rank_filter(x, rank, size, mode=mode, cval=7.0), ref), (shape, size)
            got, info = env.R.remove_outliers(x, 7, scale="mad", threshold=4.0, mode=mode, cval=7.0, return_mask=True)
            assert same(got, want) and np.array_equal(info["mask"], wmask) and np.array_equal(info["count"], wcount), shape


@pytest.mark.parametrize("size", [(3, 5), (4, 4), 9, 11, 15])
def test_d_general_route_ranks_and_percentiles(env, stack, size):
    f = stack[0, :37, :83]
    n = int(np.prod(window_pair(size)))
    for mode in ("reflect", "wrap"):
        for rank in (0, -1, 7):
            assert np.array_equal(env.R.rank_filter(f, rank, size, mode=mode), ndi.rank_filter(f, rank, size=size, mode=mode)), (size, rank)
        for p in (10, 99.9, -20):
            assert np.array_equal(env.R.percentile_filter(f, p, size, mode=mode), ndi.percentile_filter(f, p, size=size, mode=mode)), (size, p)
    assert np.array_equal(env.R.median_filter(f, size), ndi.median_filter(f, size=size))
    assert np.array_equal(env.R.percentile_filter(f, 100, size), ndi.maximum_filter(f, size=size))
    assert percentile_rank(n, 100) == n - 1


def test_e_nan_inf_and_signed_zero_both_routes(env):
    f = special_frame()
    assert np.isnan(f).sum() >= 27 and np.isinf(f).sum() == 6
    for size in (3, 5, 7):
        for mode in ("reflect", "constant"):
            want = model_median_filter(f, size, mode, np.nan if mode == "constant" else 0.0)
            for general in (False, True):
                got = env.R.median_filter(f, size, mode=mode, cval=np.nan if mode == "constant" else 0.0, _general=general)
                assert same(got, want), (size, mode, general)
    for rank in (0, -1, 5):
        assert same(env.R.rank_filter(f, rank, (3, 4)), model_rank_filter(f, rank, (3, 4)))
    allnan = np.full((5, 6), np.nan, np.float32)
    assert np.isnan(env.R.median_filter(allnan, 3)).all() and np.isnan(env.R.median_filter(allnan, 3, _general=True)).all()


# ------------------------------------------------------------------------------------------------ f: inputs
def test_f_dtypes_layouts_and_tensors(env):
    rng = np.random.default_rng(23)
    base = rng.integers(0, 4000, (2, 40, 140))
    cases = {"uint16": base.astype(np.uint16), "int32": (base - 2000).astype(np.int32), "float64": base / 7.0,
             "byte-swapped": base.astype(">u2"), "byte-swapped f4": (base / 3.0).astype(">f4"),
             "strided": base.astype(np.float32)[:, ::2, 3:131:3], "transposed": base.astype(np.int16).transpose(0, 2, 1)}
    for name, a in cases.items():
        before = a.copy()
        got = env.R.median_filter(a, 3)
        assert same(got, ndi.median_filter(np.asarray(a).astype(np.float32), size=(1, 3, 3))), name
        assert np.array_equal(a, before) and a.dtype == before.dtype, name
    f = base[0].astype(np.float32)
    t = env.torch.from_numpy(f).cuda()
    keep = t.clone()
    ref = ndi.median_filter(f, size=5)
    got = env.R.median_filter(t, 5)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref)
    dev = env.R.median_filter(t, 5, return_tensors=True)
    assert env.torch.is_tensor(dev) and dev.is_cuda and dev.dtype == env.torch.float32 and dev.data_ptr() != t.data_ptr()
    assert np.array_equal(dev.cpu().numpy(), ref) and env.torch.equal(t, keep)
    odd = t[1:, 3:]                                            # a strided device view, odd row length
    assert np.array_equal(env.R.median_filter(odd, 3), ndi.median_filter(f[1:, 3:], size=3)) and env.torch.equal(t, keep)
    repaired, info = env.R.remove_outliers(t, 3, scale="absolute", threshold=1500.0, return_mask=True, return_tensors=True)
    assert repaired.is_cuda and info["mask"].dtype == env.torch.bool and info["count"].dtype == env.torch.int64 and env.torch.equal(t, keep)


# ------------------------------------------------------------------------------------------------ g: range only
def _frame_ranges(env, frames, size, general=False):
    t = env.torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).cuda()
    t3 = t if t.ndim == 3 else t[None]
    sy, sx = window_pair(size)
    _, mm = env.R.run_rank_filter(t3, int(t3.shape[0]), int(t3.shape[1]), int(t3.shape[2]), sy, sx, (sy * sx) // 2, 1, 0.0,
                                  general=general, want_out=False, want_range=True)
    return mm.cpu().numpy()


def test_g_range_only_variant(env, stack, tmp_path):
    special = special_frame()
    special[:9, :9] = np.nan                                   # the filtered frame has NaN of its own
    for frames, sizes in ((counts_frame(), (3, 5, 7)), (stack, (3, 5, 7, 4)), (special, (3, 5))):
        for size in sizes:
            ref = model_median_filter(frames, size)
            ref3 = ref if ref.ndim == 3 else ref[None]
            want = np.stack([[np.nanmin(r), np.nanmax(r)] for r in ref3]).astype(np.float32)
            for general in (False, True):
                got = _frame_ranges(env, frames, size, general)
                assert got.dtype == np.float32 and np.array_equal(got, want), (frames.shape, size, general)
    allnan = np.full((2, 6, 7), np.nan, np.float32)
    allnan[1, 2:5, 2:6] = 3.0
    got = _frame_ranges(env, allnan, 3)
    assert np.isnan(got[0]).all() and np.array_equal(got[1], [3.0, 3.0])

    for img in (stack, stack[1], special, stack.astype(np.uint16)):
        for size in (3, 5):
            assert env.U.filtered_minmax_range(img, size) == model_filtered_minmax_range(img, size)
    path = tmp_path / "stack.npy"
    big = np.concatenate([stack, stack[::-1] + 1.0, stack[:1] * 2.0]).astype(">u2")      # 7 frames: chunks of 2 leave a ragged last one
    np.save(path, big)
    mapped = np.load(path, mmap_mode="r")
    assert env.U.filtered_minmax_range_streaming(mapped, 3, chunk_frames=2) == model_filtered_minmax_range(big, 3)
    assert env.U.filtered_minmax_range_streaming(mapped, 5) == model_filtered_minmax_range(big, 5)
    assert env.U.filtered_minmax_range_streaming(stack[0], 3) == model_filtered_minmax_range(stack[0], 3)
    for bad in (np.full((12, 12), 4.0, np.float32), np.full((2, 5, 5), np.nan, np.float32)):
        with pytest.raises(ValueError):
            env.U.filtered_minmax_range(bad)
        with pytest.raises(ValueError):
            env.U.filtered_minmax_range_streaming(bad, chunk_frames=1)
    inf = stack[0].copy()
    inf[20:30, 20:30] = np.inf
    with pytest.raises(ValueError):
        env.U.filtered_minmax_range(inf)


# ------------------------------------------------------------------------------------------------ h: outlier repair
@pytest.mark.parametrize("size", [3, 5])
@pytest.mark.parametrize("scale", ["absolute", "mad", "poisson"])
def test_h_outlier_repair_equals_the_model(env, scale, size):
    """Frames, mask and count equal the model exactly.  The detection claim -- all 40 planted pixels and at most 6 others -- is
    asserted of the model first, for 5 x 5 / mad / 6 and 3 x 3 / poisson / 5 / min_scale 1.  3 x 3 mad flags dozens of ordinary
    pixels on this frame (a nine-sample MAD is noisy): it is tested for equality with the model only."""
    f, idx = outlier_frame()
    g = f.copy()
    g[5, 7] = np.nan                                           # one non-finite centre: always an outlier
    kw = {"absolute": dict(threshold=300.0), "mad": dict(threshold=6.0), "poisson": dict(threshold=5.0, min_scale=1.0)}[scale]
    if (scale, size) in (("mad", 5), ("poisson", 3)):
        _, mask, count = model_remove_outliers(f, size, scale=scale, **kw)
        assert mask.reshape(-1)[idx].all() and 40 <= int(count[0]) <= 46
    for frame in (f, g, np.stack([f, g, f[::-1]])):
        for polarity in ("both", "hot", "dead"):
            want, wmask, wcount = model_remove_outliers(frame, size, scale=scale, polarity=polarity, **kw)
            got, info = env.R.remove_outliers(frame, size, scale=scale, polarity=polarity, return_mask=True, **kw)
            assert info["mask"].dtype == np.bool_ and np.array_equal(info["mask"], wmask), (scale, size, polarity)
            assert info["count"].dtype == np.int64 and np.array_equal(info["count"], wcount), (scale, size, polarity)
            assert same(got, want), (scale, size, polarity)
            assert same(env.R.remove_outliers(frame, size, scale=scale, polarity=polarity, **kw), want)


def test_h_outlier_repair_size7_modes_and_ragged_rows(env, stack):
    frames = stack[:2, :45, :131].copy()
    frames[0, 0, 0] = 5000.0
    frames[1, 44, 130] = -np.inf
    for mode in ("reflect", "constant", "wrap"):
        want, wmask, wcount = model_remove_outliers(frames, 7, scale="mad", threshold=4.0, mode=mode, cval=40.0)
        got, info = env.R.remove_outliers(frames, 7, scale="mad", threshold=4.0, mode=mode, cval=40.0, return_mask=True)
        assert same(got, want) and np.array_equal(info["mask"], wmask) and np.array_equal(info["count"], wcount), mode
        assert wmask[0, 0, 0] and wmask[1, 44, 130]


# ------------------------------------------------------------------------------------------------ i: uint16 and percentile bounds
def test_i_to_uint16_and_percentile_range(env):
    rng = np.random.default_rng(24)
    low = rng.gamma(2.0, 1.5, (3, 33, 50)).astype(np.float32)              # mean 3: the scaling branch
    low[1, 4, 5] = 400.0
    low[2, 7, 7] = np.nan                                                  # NaN -> 0
    for scaling in (1 / np.sqrt(2), 0.5, np.float32(0.5)):                 # NumPy float64 scalar, Python float, NumPy float32 scalar
        for img in (low, low[0], low[:, :, :49]):
            got = env.U.to_uint16(img, scaling=scaling)
            assert got.dtype == np.uint16 and np.array_equal(got, model_to_uint16(img, scaling=scaling)), repr(scaling)
    assert env.U.to_uint16(low)[2, 7, 7] == 0 and env.U.to_uint16(low)[1, 4, 5] == 65535
    assert np.array_equal(env.U.to_uint16(low, median_size=5, scaling=0.9), model_to_uint16(low, median_size=5, scaling=0.9))
    counts = rng.poisson(300, (2, 16, 25)).astype(np.float32) * 220.25     # fractions are truncated, about half is clipped
    counts[0, 0, 0] = -3.5
    for img in (counts, counts.astype(np.int32), counts[0]):
        got = env.U.to_uint16(img)
        assert got.dtype == np.uint16 and got.shape == img.shape and np.array_equal(got, model_to_uint16(img))
    u16 = counts.astype(np.uint16)
    assert env.U.to_uint16(u16) is u16

    for img in (low[0], low, counts):
        got = env.U.percentile_minmax_range(img)
        with np.errstate(all="ignore"):
            want = (np.nanpercentile(img.astype(np.float64), 0.05), np.nanpercentile(img.astype(np.float64), 99.95))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert isinstance(got[0], float) and got[0] < got[1]
    np.testing.assert_allclose(env.U.percentile_minmax_range(counts, 1.0, 90.0), model_percentile_minmax_range(counts.astype(np.float64), 1.0, 90.0),
                               rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ j: C ABI misuse
def test_j_cabi_misuse_returns_einval(env):
    """Bad arguments return B4D_EINVAL and launch nothing: the output buffers keep their fill."""
    torch, D, lib = env.torch, env.D, env.lib
    t = torch.from_numpy(counts_frame()).cuda()
    ny, nx = (int(v) for v in t.shape)
    out = torch.full_like(t, -7.0)
    mm = torch.full((1, 2), -7.0, dtype=torch.float32, device="cuda")
    mask = torch.full((ny, nx), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    u16 = torch.full((ny * nx,), 9, dtype=torch.int16, device="cuda")
    st, null = env.ffi.stream_ptr(), C.c_void_p(0)

    def rank(size_y=3, size_x=3, rank=4, mode=1, src=t, dst=out, rng=mm, batch=1):
        return lib.b4d_rank_filter(D.ptr(src) if src is not None else null, batch, ny, nx, size_y, size_x, rank, mode, 0.0, 0,
                                   D.ptr(dst) if dst is not None else null, D.ptr(rng) if rng is not None else null, st)

    def desp(size=3, scale=1, thr=6.0, pol=0, mode=1, src=t, dst=out, batch=1):
        return lib.b4d_despeckle(D.ptr(src), batch, ny, nx, size, scale, thr, 0.0, pol, mode, 0.0, D.ptr(dst) if dst is not None else null,
                                 D.ptr(mask), D.ptr(cnt), st)

    bad = [rank(size_y=0), rank(size_x=0), rank(size_y=16), rank(size_x=16), rank(rank=9), rank(rank=-1), rank(size_y=4, size_x=4, rank=16),
           rank(mode=5), rank(mode=-1), rank(batch=0), rank(src=None), rank(dst=t), rank(dst=None, rng=None), rank(dst=t[1:]),
           desp(size=4), desp(size=9), desp(scale=3), desp(pol=3), desp(thr=-1.0), desp(thr=float("nan")), desp(mode=7), desp(batch=0),
           desp(dst=t), desp(dst=None),
           lib.b4d_scale_to_u16(D.ptr(t), 0, 0.0, 1.0, 0, D.ptr(u16), st), lib.b4d_scale_to_u16(null, 8, 0.0, 1.0, 0, D.ptr(u16), st),
           lib.b4d_scale_to_u16(D.ptr(t), 8, 0.0, 1.0, 0, null, st), lib.b4d_scale_to_u16(D.ptr(t), 8, 0.0, 1.0, 0, D.ptr(t), st)]
    assert bad == [-1] * len(bad), bad
    assert b"b4d_scale_to_u16" in lib.b4d_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((mm == -7.0).all()) and bool((mask == 9).all()) and int(cnt[0]) == 9 and bool((u16 == 9).all())
    assert torch.equal(t.cpu(), torch.from_numpy(counts_frame()))
    assert rank() == 0 and rank(dst=None) == 0 and rank(rng=None) == 0 and desp() == 0      # and the same calls with good arguments run
    torch.cuda.synchronize()
    ref = ndi.median_filter(counts_frame(), size=3)
    assert same(out.cpu().numpy(), model_remove_outliers(counts_frame(), 3)[0])            # the last writer of out: desp()
    assert np.array_equal(mm.cpu().numpy()[0], [np.nanmin(ref), np.nanmax(ref)])
