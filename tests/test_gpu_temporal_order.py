"""GPU tier of the temporal order statistics (csrc/b4d_torder.hip through barc4dip_amd.metrics.order and
barc4dip_amd.preprocessing.combine) against the NumPy model of tests/temporal_order_model.py, itself checked against NumPy in
tests/test_temporal_order_host.py.

Every quantile, median, scale, n_valid, n_kept, rejected and cleaned comparison is exact (np.array_equal on values, equal NaN
pattern): selections are exact and the interpolation and the rejection test are chains of singly rounded operations that the model
repeats.  Only `mean` has a bar, 2^-23 relative: its float64 sum runs in eight partial sums where the model's runs in frame
order, so the quotient may differ in its last place before it is rounded once to float32 (half a float32 ulp, 2^-24, from the
rounding and as much again from a sum that lands on the other side of a tie).

Shapes are the smallest at which the kernels can go wrong: the register route's lanes own 4, 2 or 1 pixels (T <= 16, 32, 64) and
take wide or dword accesses; the general route works in tiles of 32 pixels."""
import ctypes as C

import numpy as np
import pytest

import temporal_order_model as M
from test_temporal_order_host import with_nans

pytestmark = pytest.mark.gpu

QS = [0.0, 10.0, 37.5, 50.0, 99.0, 100.0]
MEAN_BAR = 2.0 ** -23


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi, metrics, preprocessing
    from barc4dip_amd.metrics import order

    class E:
        pass

    e = E()
    e.torch, e.D, e.ffi, e.lib, e.O, e.metrics, e.P = torch, D, _ffi, _ffi.lib(), order, metrics, preprocessing
    return e


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def dev(env, x):
    return env.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def check_quantiles(env, x, methods=M.METHODS, general=False, qs=QS):
    """every method and both NaN policies of temporal_percentile on the host array x against the model"""
    for method in methods:
        for ignore in (False, True):
            got, cnt = env.O.temporal_percentile(x, qs, method=method, ignore_nan=ignore, return_count=True, _general=general)
            ref, nv = M.quantiles(x, np.asarray(qs) / 100.0, method, ignore)
            assert got.dtype == np.float32 and same(got, ref), (x.shape, method, ignore, general)
            assert cnt.dtype == np.int32 and same(cnt, nv.astype(np.int32)), (x.shape, method, ignore, general)


def robust_outputs(env, x, scale, polarity, threshold, min_scale=0.0, general=False):
    """all six outputs of b4d_temporal_robust_mean as host arrays"""
    res = env.O.run_robust_mean(dev(env, x), M.SCALES.index(scale), threshold, min_scale, M.POLARITIES.index(polarity), general=general,
                                want_info=True, want_mask=True, want_cleaned=True)
    return dict(zip(("mean", "median", "scale", "n_kept", "rejected", "cleaned"), (r.cpu().numpy() for r in res)))


def check_robust(got, ref, observe, what):
    for k in ("median", "scale", "cleaned"):
        assert got[k].dtype == np.float32 and same(got[k], ref[k]), (what, k)
    assert same(got["n_kept"].astype(np.int64), ref["n_kept"]) and same(got["rejected"].astype(bool), ref["rejected"]), what
    assert same(np.isnan(got["mean"]), np.isnan(ref["mean"])), what
    ok = ~np.isnan(ref["mean"])
    if ok.any():
        with np.errstate(all="ignore"):
            rel = np.abs(got["mean"][ok].astype(np.float64) - ref["mean"][ok]) / np.abs(ref["mean"][ok].astype(np.float64))
        rel = np.where(got["mean"][ok] == ref["mean"][ok], 0.0, rel)
        print(f"{what}: mean within {float(rel.max()):.3e} relative")
        observe("torder.mean", float(rel.max()), MEAN_BAR)


# ------------------------------------------------------------------------------------------------ a: register route
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64])
def test_a_register_route_padding_edges(env, T):
    """5 x 7: 35 pixels, dword accesses; 8 x 12: under one wave, wide accesses; 37 x 64: several waves and a tail."""
    for shape in ((5, 7), (8, 12), (37, 64)):
        x = M.counts_stack(T, shape, seed=T)
        check_quantiles(env, x)
        check_quantiles(env, with_nans(x, T))
    x = M.counts_stack(T, (5, 7), seed=T)
    assert same(env.metrics.temporal_median(x), np.median(x, axis=0))


# ------------------------------------------------------------------------------------------------ b: general route
@pytest.mark.parametrize("T", [65, 100, 256, 257, 1024])
def test_b_general_route(env, T, observe):
    """3 x 33: three full tiles of 32 pixels and a ragged one; 40 pixels: one full tile and a quarter."""
    for shape in ((3, 33), (5, 8)):
        x = with_nans(M.counts_stack(T, shape, seed=T), T)
        check_quantiles(env, x)
        z, _, _ = M.zinger_stack(T, shape, seed=T)
        z[T // 2, 0, 1] = np.nan
        for scale, thr in (("mad", 6.0), ("poisson", 6.0)):
            check_robust(robust_outputs(env, z, scale, "both", thr, 1.0), M.robust_mean(z, thr, scale, "both", 1.0), observe, (T, shape, scale))
    x = M.counts_stack(T, (3, 33), seed=T)
    assert same(env.metrics.temporal_median(x), np.median(x, axis=0))


@pytest.mark.parametrize("T", [1, 5, 16, 33, 64])
def test_b_forced_general_route_is_bit_identical(env, T, observe):
    lib, D, torch = env.lib, env.D, env.torch
    for shape in ((3, 33), (4, 24)):
        x = with_nans(M.counts_stack(T, shape, seed=50 + T), T)
        t = dev(env, x)
        fr = np.asarray(QS) / 100.0
        for method in range(5):
            for policy in (0, 1):
                a, na = env.O.run_quantiles(t, fr, method, policy, general=False, want_count=True)
                b, nb = env.O.run_quantiles(t, fr, method, policy, general=True, want_count=True)
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(na, nb), (T, shape, method, policy)
        check_quantiles(env, x, general=True)
        z, _, _ = M.zinger_stack(T, shape, seed=T)
        z[0, 0, 0] = np.inf
        for scale, thr in (("absolute", 300.0), ("mad", 6.0), ("poisson", 6.0)):
            for pol in M.POLARITIES:
                r = robust_outputs(env, z, scale, pol, thr, 1.0)
                g = robust_outputs(env, z, scale, pol, thr, 1.0, general=True)
                assert all(np.array_equal(r[k].view(np.uint8), g[k].view(np.uint8)) for k in r), (T, shape, scale, pol)
            check_robust(g, M.robust_mean(z, thr, scale, "dead", 1.0), observe, ("forced", T, shape, scale))


# ------------------------------------------------------------------------------------------------ c: special values
def special_stack(T):
    """(T, 2, 8): pixels with one NaN, all NaN, +Inf, -Inf and both, -0 / +0, integer ties, constants."""
    rng = np.random.default_rng(T)
    x = rng.normal(size=(T, 16)).astype(np.float32)
    x[T // 2, 0] = np.nan
    x[:, 1] = np.nan
    x[0, 2] = np.inf
    x[T - 1, 3] = -np.inf
    x[0, 4], x[T // 3, 4], x[T - 1, 4] = np.inf, -np.inf, np.inf
    x[:, 5] = np.where(np.arange(T) % 2 == 0, -0.0, 0.0)
    x[:, 6] = np.where(np.arange(T) % 3 == 0, -0.0, x[:, 6])
    x[:, 7] = rng.integers(0, 3, T)
    x[:, 8] = rng.integers(-2, 2, T)
    x[:, 9] = 4.25
    x[:, 10] = -1e30
    x[:, 11] = np.inf
    x[:, 12] = np.where(np.arange(T) % 2 == 0, np.nan, 3.0)
    return x.reshape(T, 2, 8)


@pytest.mark.parametrize("T,general", [(9, False), (9, True), (32, False), (32, True), (70, True)])
def test_c_special_values(env, T, general, observe):
    x = special_stack(T)
    inf_pixels = np.isinf(x).any(axis=0)
    check_quantiles(env, x, methods=("lower", "higher", "nearest"), general=general)          # +-Inf: selections only
    y = np.where(inf_pixels[None], np.float32(1.0), x).astype(np.float32)
    check_quantiles(env, y, general=general)
    for ignore in (False, True):
        with np.errstate(all="ignore"):
            assert same(env.O.temporal_median(y, ignore_nan=ignore, _general=general), M.median(y, ignore))
    for scale, thr, floor_ in (("absolute", 1.0, 0.0), ("mad", 3.0, 0.0), ("mad", 3.0, 0.5), ("poisson", 2.0, 0.25)):
        for pol in M.POLARITIES:
            check_robust(robust_outputs(env, x, scale, pol, thr, floor_, general=general), M.robust_mean(x, thr, scale, pol, floor_), observe,
                         (T, general, scale, pol))
    r = robust_outputs(env, x, "mad", "both", 3.0, general=general)                         # the documented degeneracy, and n_kept = 0
    assert r["scale"][1, 1] == 0.0 and r["n_kept"][1, 1] == T and np.isnan(r["mean"][0, 1]) and r["n_kept"][0, 1] == 0
    assert r["rejected"][:, 0, 1].all() and r["rejected"][:, 1, 3].all() and r["n_kept"][1, 3] == 0


# ------------------------------------------------------------------------------------------------ d: layout
@pytest.mark.parametrize("T", [9, 20, 64, 80])
def test_d_strides_alignment_and_variants_give_identical_bits(env, T):
    torch, D, lib = env.torch, env.D, env.lib
    h, w = 6, 12
    npix, st, null = h * w, env.ffi.stream_ptr(), C.c_void_p(0)
    x = with_nans(M.counts_stack(T, (h, w), seed=T), T)
    x[1, 0, 3] = np.inf
    fr = np.asarray([0.1, 0.5, 0.99], dtype=np.float64)

    def quant(src, fs, out, nv):
        env.ffi.check(lib.b4d_temporal_quantiles(D.ptr(src), T, fs, npix, fr.ctypes.data_as(C.c_void_p), 3, 0, 1, 0, D.ptr(out), D.ptr(nv), st))

    def robust(src, fs, outs, os_):
        env.ffi.check(lib.b4d_temporal_robust_mean(D.ptr(src), T, fs, npix, 1, 4.0, 0.5, 0, 0, *(D.ptr(o) for o in outs), os_, st))

    def robust_buffers(os_, off):
        f32 = lambda n: torch.full((n + 8,), -7.0, dtype=torch.float32, device="cuda")[off:off + n]  # noqa: E731
        return [f32(npix), f32(npix), f32(npix), torch.full((npix + 8,), -7, dtype=torch.int16, device="cuda")[off:off + npix],
                torch.full((T * os_ + 8,), 9, dtype=torch.uint8, device="cuda")[off:off + T * os_], f32(T * os_)]

    base = dev(env, x).reshape(T, npix)
    q0 = torch.empty((3, npix), dtype=torch.float32, device="cuda")
    n0 = torch.empty((npix,), dtype=torch.int16, device="cuda")
    quant(base, npix, q0, n0)
    ref, nv = M.quantiles(x.reshape(T, npix), fr, "linear", True)
    assert same(q0.cpu().numpy(), ref) and same(n0.cpu().numpy().astype(np.int64), nv)
    r0 = robust_buffers(npix, 0)
    robust(base, npix, r0, npix)
    for fs, off in ((npix + 4, 0), (npix + 3, 0), (npix, 1), (npix + 5, 1)):      # wide; odd stride; unaligned base; both
        buf = torch.full((T * fs + 8,), float("nan"), dtype=torch.float32, device="cuda")
        view = buf[off:off + T * fs].view(T, fs)
        view[:, :npix] = base
        q1 = torch.full((3 * npix + 8,), -7.0, dtype=torch.float32, device="cuda")[off:off + 3 * npix].view(3, npix)
        n1 = torch.full((npix + 8,), -7, dtype=torch.int16, device="cuda")[off:off + npix]
        quant(view, fs, q1, n1)
        assert torch.equal(q1.view(torch.int32), q0.view(torch.int32)) and torch.equal(n1, n0), (T, fs, off)
        os_ = npix + (4 if off == 0 else 3)
        r1 = robust_buffers(os_, off)
        robust(view, fs, r1, os_)
        for k in range(4):
            assert torch.equal(r1[k].view(torch.int32) if k < 3 else r1[k], r0[k].view(torch.int32) if k < 3 else r0[k]), (T, fs, off, k)
        rej1, cl1 = r1[4].view(T, os_), r1[5].view(T, os_)
        assert torch.equal(rej1[:, :npix], r0[4].view(T, npix)) and torch.equal(cl1[:, :npix].view(torch.int32), r0[5].view(T, npix).view(torch.int32))
        assert bool((rej1[:, npix:] == 9).all()) and bool((cl1[:, npix:] == -7.0).all())            # the gaps between rows stay as they were


def test_d_input_kinds(env):
    torch = env.torch
    rng = np.random.default_rng(8)
    base = rng.poisson(300, (11, 6, 10))
    ref = M.percentile(base.astype(np.float32), [25.0, 75.0])
    for arr in (base.astype(np.uint16), base.astype(np.int32), base.astype(np.float64), base.astype(">u2")):
        assert same(env.metrics.temporal_percentile(arr, [25.0, 75.0]), ref), arr.dtype
        assert same(env.metrics.temporal_median(arr), np.median(base.astype(np.float32), axis=0))
    t = torch.from_numpy(base.astype(np.float32)).cuda()
    got = env.metrics.temporal_percentile(t, [25.0, 75.0], return_tensors=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and same(got.cpu().numpy(), ref)
    one = env.metrics.temporal_percentile(t, 25.0, return_tensors=True)
    assert tuple(one.shape) == (6, 10) and same(one.cpu().numpy(), ref[0])
    mean, info = env.metrics.temporal_robust_mean(t, return_mask=True, return_tensors=True)
    m = M.robust_mean(base.astype(np.float32))
    assert mean.is_cuda and info["rejected"].dtype == torch.bool and same(info["rejected"].cpu().numpy(), m["rejected"])
    assert same(info["median"].cpu().numpy(), m["median"]) and same(info["n_kept"].cpu().numpy().astype(np.int64), m["n_kept"])
    many = np.linspace(0.0, 100.0, 19)                          # more than 8 values go down in groups of 8
    assert same(env.metrics.temporal_percentile(base.astype(np.float32), many), M.percentile(base.astype(np.float32), many))


def test_d_offsets_past_2_31_elements(env, observe):
    """A stack of 33 x (2^26 + 40) samples, 8.9 GB: element offsets of the last frames and of `cleaned` exceed 2^31 (and 2^32 in
    bytes) on both routes.  The first and the last 2048 pixels are compared with the model."""
    torch, O = env.torch, env.O
    T, npix, edge = 33, (1 << 26) + 40, 2048
    assert T * npix > 1 << 31
    stack = torch.empty((T, 1, npix), dtype=torch.float32, device="cuda").uniform_(0.0, 200.0).floor_()
    stack[T - 1, 0, npix - 1] = float("nan")
    stack[5, 0, npix - 2] = 5000.0
    cols = torch.cat([stack[:, 0, :edge], stack[:, 0, npix - edge:]], dim=1).cpu().numpy()
    fr = np.asarray([0.25, 0.5], dtype=np.float64)
    ref, nv = M.quantiles(cols, fr, "linear", True)
    rob = M.robust_mean(cols, 5.0, "mad", "both", 1.0)
    pick = lambda t: torch.cat([t[..., :edge], t[..., npix - edge:]], dim=-1).cpu().numpy()  # noqa: E731
    for general in (False, True):
        out, cnt = O.run_quantiles(stack, fr, 0, 1, general=general, want_count=True)
        assert same(pick(out[:, 0]), ref) and same(pick(cnt[0]).astype(np.int64), nv), general
        del out, cnt
        res = O.run_robust_mean(stack, 1, 5.0, 1.0, 0, general=general, want_info=True, want_mask=True, want_cleaned=True)
        got = dict(zip(("mean", "median", "scale", "n_kept", "rejected", "cleaned"), (pick(r[..., 0, :]) for r in res)))
        check_robust(got, rob, observe, ("2^31", general))
        assert got["rejected"][5, -2] and got["rejected"][T - 1, -1]
        del res
    del stack
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ e: robust mean
@pytest.mark.parametrize("T", [9, 32, 64, 100])
def test_e_robust_mean_scales_and_polarities(env, T, observe):
    for shape in ((6, 11), (4, 24)):
        x, hot, dead = M.zinger_stack(T, shape, seed=10 + T)
        for scale, thr, floor_ in (("absolute", 300.0, 0.0), ("mad", 6.0, 0.0), ("poisson", 6.0, 1.0)):
            for pol in M.POLARITIES:
                ref = M.robust_mean(x, thr, scale, pol, floor_)
                got = robust_outputs(env, x, scale, pol, thr, floor_)
                check_robust(got, ref, observe, (T, shape, scale, pol))
                if pol != "dead":
                    assert got["rejected"].astype(bool)[hot].all()
                if pol != "hot":
                    assert got["rejected"].astype(bool)[dead].all()
    mean, info = env.metrics.temporal_robust_mean(x, threshold=6.0, scale="mad", return_info=True)
    ref = M.robust_mean(x, 6.0, "mad")
    assert set(info) == {"median", "scale", "n_kept"} and same(info["scale"], ref["scale"]) and same(np.isnan(mean), np.isnan(ref["mean"]))


def test_e_remove_zingers_and_combine_frames(env):
    x, hot, dead = M.zinger_stack(20, (9, 13), seed=3)
    ref = M.robust_mean(x, 5.0, "mad", "hot")
    cleaned, info = env.P.remove_zingers(x, return_mask=True)
    assert cleaned.dtype == np.float32 and same(cleaned, ref["cleaned"]) and same(info["mask"], ref["rejected"])
    assert info["count"].dtype == np.int64 and same(info["count"], ref["rejected"].sum(axis=(1, 2))) and info["mask"][hot].all()
    assert not info["mask"][dead].any() and same(env.P.remove_zingers(x), cleaned)
    ct, it = env.P.remove_zingers(x, return_mask=True, return_tensors=True)
    assert ct.is_cuda and same(ct.cpu().numpy(), cleaned) and same(it["count"].cpu().numpy(), info["count"])
    med = env.P.combine_frames(x, method="median")
    assert med.dtype == np.float32 and med.shape == (9, 13) and same(med, M.median(x))
    assert same(env.P.combine_frames(x, "mean"), x.mean(axis=0, dtype=np.float32))
    rob = env.P.combine_frames(x, "robust", threshold=6.0)
    assert same(np.isnan(rob), np.isnan(ref["mean"])) and np.allclose(rob, M.robust_mean(x, 6.0)["mean"], rtol=MEAN_BAR, atol=0.0, equal_nan=True)
    images = np.random.default_rng(4).poisson(200, (3, 9, 13)).astype(np.float32)
    flats = x + np.float32(1)
    got = env.P.flat_field_correction(images, flats=env.P.combine_frames(flats, "median"))
    assert same(got, env.P.flat_field_correction(images, flats=M.median(flats)))
    assert not same(got, env.P.flat_field_correction(images, flats=flats))                       # the mean of the flats keeps the zingers


# ------------------------------------------------------------------------------------------------ f: banded source
def test_f_memory_mapped_source_in_bands(env, tmp_path):
    rng = np.random.default_rng(6)
    data = rng.poisson(50, (12, 10, 16)).astype(np.uint16)
    data[3, 4, 5] = 60000
    path = tmp_path / "stack.npy"
    np.save(path, data)
    mm = np.load(path, mmap_mode="r")
    band = 3 * 4 * 12 * 16                                      # three rows of the float32 image
    assert env.O.row_bands(mm.shape, band) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert same(env.metrics.temporal_median(mm, max_bytes=band), env.metrics.temporal_median(data))
    assert same(env.metrics.temporal_median(mm, max_bytes=band), np.median(data.astype(np.float32), axis=0))
    for a, b in zip(env.metrics.temporal_percentile(mm, [5.0, 95.0], return_count=True, max_bytes=band),
                    env.metrics.temporal_percentile(data, [5.0, 95.0], return_count=True)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    m1, i1 = env.metrics.temporal_robust_mean(mm, return_mask=True, max_bytes=band)
    m2, i2 = env.metrics.temporal_robust_mean(data, return_mask=True)
    assert np.array_equal(m1.view(np.uint8), m2.view(np.uint8)) and all(same(i1[k], i2[k]) for k in i2) and i1["rejected"][3, 4, 5]
    c1, j1 = env.P.remove_zingers(mm, return_mask=True, max_bytes=band)
    c2, j2 = env.P.remove_zingers(data, return_mask=True)
    assert c1.shape == (12, 10, 16) and same(c1, c2) and same(j1["mask"], j2["mask"]) and same(j1["count"], j2["count"])
    tt = env.metrics.temporal_median(mm, max_bytes=band, return_tensors=True)
    assert tt.is_cuda and same(tt.cpu().numpy(), env.metrics.temporal_median(data))


# ------------------------------------------------------------------------------------------------ g: C-ABI misuse
def test_g_cabi_misuse_returns_einval(env):
    """Bad arguments return B4D_EINVAL / B4D_ESIZE and launch nothing: the output buffers keep their fill."""
    torch, D, lib = env.torch, env.D, env.lib
    T, npix = 9, 40
    x = M.counts_stack(T, (5, 8), seed=1)
    t = dev(env, x).reshape(T, npix)
    out = torch.full((8, npix), -7.0, dtype=torch.float32, device="cuda")
    nv = torch.full((npix,), -7, dtype=torch.int16, device="cuda")
    f = [torch.full((npix,), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    nk = torch.full((npix,), -7, dtype=torch.int16, device="cuda")
    rej = torch.full((T, npix), 9, dtype=torch.uint8, device="cuda")
    cl = torch.full((T, npix), -7.0, dtype=torch.float32, device="cuda")
    st, null = env.ffi.stream_ptr(), C.c_void_p(0)
    P = lambda v: D.ptr(v) if v is not None else null  # noqa: E731

    def quant(q=(0.5,), n_q=None, method=0, policy=0, flags=0, T=T, fs=npix, npix=npix, src=t, dst=out, cnt=nv, qnull=False):
        qa = np.asarray(q, dtype=np.float64)
        return lib.b4d_temporal_quantiles(P(src), T, fs, npix, null if qnull else qa.ctypes.data_as(C.c_void_p), len(q) if n_q is None else n_q,
                                          method, policy, flags, P(dst), P(cnt), st)

    def rob(kind=1, thr=5.0, floor_=0.0, pol=0, flags=0, T=T, fs=npix, os_=npix, npix=npix, src=t, mean=f[0], med=f[1], sc=f[2], cnt=nk, r=rej, c=cl):
        return lib.b4d_temporal_robust_mean(P(src), T, fs, npix, kind, thr, floor_, pol, flags, P(mean), P(med), P(sc), P(cnt), P(r), P(c), os_, st)

    nan, inf = float("nan"), float("inf")
    bad = [quant(fs=npix - 1), quant(q=(-0.01,)), quant(q=(1.01,)), quant(q=(0.2, nan)), quant(q=(inf,)), quant(n_q=0), quant(q=(0.5,) * 9),
           quant(method=5), quant(method=-1), quant(policy=2), quant(policy=-1), quant(flags=2), quant(T=0), quant(npix=0), quant(src=None),
           quant(dst=None), quant(qnull=True), quant(dst=t), quant(dst=t[T - 1:]), quant(cnt=t.view(torch.int16)),
           rob(fs=npix - 1), rob(os_=npix - 1), rob(kind=3), rob(kind=-1), rob(pol=3), rob(pol=-1), rob(flags=4), rob(thr=-1.0), rob(thr=nan),
           rob(floor_=-0.5), rob(floor_=nan), rob(T=0), rob(npix=0), rob(src=None), rob(mean=None), rob(mean=t), rob(med=t[2:]), rob(sc=t[T - 1:]),
           rob(cnt=t.view(torch.int16)), rob(r=t.view(torch.uint8)), rob(c=t)]
    assert bad == [-1] * len(bad), bad
    assert b"b4d_temporal_robust_mean" in lib.b4d_last_error()
    assert [quant(T=1025), rob(T=1025), quant(T=4096, flags=1)] == [-2, -2, -2]
    assert b"1024" in lib.b4d_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((nv == -7).all()) and all(bool((v == -7.0).all()) for v in f + [cl])
    assert bool((nk == -7).all()) and bool((rej == 9).all()) and same(t.cpu().numpy(), x.reshape(T, npix))
    assert quant() == 0 and quant(cnt=None, flags=1) == 0 and rob() == 0 and rob(med=None, sc=None, cnt=None, r=None, c=None, flags=1) == 0
    torch.cuda.synchronize()                                    # and the same calls with good arguments run
    assert same(out[0].cpu().numpy(), M.quantiles(x.reshape(T, npix), [0.5], "linear")[0][0]) and bool((out[1:] == -7.0).all())
    assert same(f[1].cpu().numpy(), M.median(x.reshape(T, npix)))


# ------------------------------------------------------------------------------------------------ one outlier rule
def window_stack(image, size):
    """(size * size, H, W): frame dy * size + dx holds, for every pixel, the element (dy, dx) of its reflect-mode size x size
    window; frame size * size // 2 is the image.  Along T a pixel has the samples remove_outliers sees in its window."""
    r = size // 2
    p = np.pad(image, r, mode="symmetric")
    H, W = image.shape
    return np.stack([p[dy:dy + H, dx:dx + W] for dy in range(size) for dx in range(size)]).astype(np.float32)


def test_spatial_and_temporal_units_apply_one_rule(env):
    """remove_outliers on an image and temporal_robust_mean (both routes) on the stack of the image's window offsets see the same
    samples per pixel, so the one rule of b4d_keys.hpp must give the same decision and the same repaired value, bit for bit: the
    mask equals rejected[centre] and the repaired frame equals cleaned[centre].  13 x 17 Poisson(50) counts with planted 4000
    (corner), 900 (edge), 0, 1 (interior) and 51.5 (corner); sizes 3 and 5; every scale, polarity and three settings."""
    img = np.random.default_rng(50).poisson(50, (13, 17)).astype(np.float32)
    img[0, 0], img[0, 8], img[6, 6], img[9, 12], img[12, 16] = 4000.0, 900.0, 0.0, 1.0, 51.5
    for size in (3, 5):
        stack, c = window_stack(img, size), size * size // 2
        assert stack.shape == (size * size, 13, 17) and same(stack[c], img)
        flagged = dict.fromkeys(M.SCALES, 0)
        for scale in M.SCALES:
            for polarity in M.POLARITIES:
                for threshold, min_scale in ((5.0, 0.0), (3.0, 1.0), (20.0, 0.0)):
                    what = (size, scale, polarity, threshold, min_scale)
                    out, info = env.P.remove_outliers(img, size, threshold=threshold, scale=scale, polarity=polarity, min_scale=min_scale,
                                                      return_mask=True)
                    flagged[scale] += int(info["mask"].sum())
                    for general in (False, True):
                        got = robust_outputs(env, stack, scale, polarity, threshold, min_scale, general=general)
                        assert same(info["mask"], got["rejected"][c].astype(bool)), (what, general)
                        assert out.dtype == np.float32 and got["cleaned"].dtype == np.float32, (what, general)
                        assert np.array_equal(out.view(np.uint32), got["cleaned"][c].view(np.uint32)), (what, general)
        print(f"size {size}: flagged pixels per scale {flagged}")
        assert all(0 < n < 9 * img.size for n in flagged.values()), flagged
