"""GPU tier: the select and reduction kernels of csrc/b4d_stats.hip on edge inputs -- unusual values (+-0, denormals, +-inf,
NaN shares, ties, one key bin), sizes around the single- / multi-workgroup switch, unaligned frames, tiny and ragged
shapes -- each compared with the float64 NumPy model of the same entry point (oracle/stats_np.py) on the same float32 input.

Bars: a quantity that already has a bar in test_gpu_stats.py / test_gpu_metrics.py keeps it; the raw sums of b4d_psd_stats and
the Laplacian variance of a paraboloid had none and go through `observe` (bar = 2 x the largest value seen on the MI355X,
rounded up to one digit)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from barc4dip_amd import synth
from oracle import stats_np as SN

pytestmark = pytest.mark.gpu

QS = [0.0, 0.05, 1.0, 5.0, 25.0, 33.3, 50.0, 75.0, 95.0, 98.0, 99.0, 99.95, 100.0]
QS16 = QS + [10.0, 66.6, 90.0]
# observed on the MI355X (the maxima the `observe` fixture records), bar = 2 x max rounded up to one significant digit.  Both sides sum
# the same float32 inputs in float64 and the kernels reduce in a fixed order (no float atomics in these outputs), so the difference
# is a few float64 roundings and does not vary from run to run.
BAR_PSD_SUMS = 3e-15              # observed 1.31e-15 over 858 sums (largest: sum P^2 of a 512 x 300 speckle PSD)
BAR_LAPVAR_PARABOLOID = 4e-16     # observed 1.62e-16


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd.metrics import kernels

    class E:
        pass

    e = E()
    e.torch, e.D, e.ffi, e.K, e.lib = torch, D, _ffi, kernels, _ffi.lib()
    return e


def _dev(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ percentiles
def _raw_rows(env, t, q):
    """(B, nq, 4) rows of b4d_percentiles for a (B, n) device tensor."""
    qs = np.ascontiguousarray(q, dtype=np.float64)
    out = env.torch.empty((int(t.shape[0]), qs.size, 4), dtype=env.torch.float64, device=t.device)
    env.ffi.check(env.lib.b4d_percentiles(env.D.ptr(t), int(t.shape[0]), int(t.shape[1]), qs.ctypes.data_as(C.c_void_p),
                                          int(qs.size), env.D.ptr(out), env.ffi.stream_ptr()))
    return out.cpu().numpy()


def _check_select(env, frames, q, tag):
    t = _dev(env, frames)
    if frames.shape[1] % 4:     # batch 3: frames 1 and 2 start off a 16-byte boundary
        assert any((t.data_ptr() + 4 * frames.shape[1] * b) % 16 for b in (1, 2))
    raw = _raw_rows(env, t, q)
    model = SN.select_rows(frames, q)
    np.testing.assert_array_equal(raw[..., 3], model[..., 3], err_msg=f"{tag}: n_valid")
    np.testing.assert_array_equal(raw[..., 0], model[..., 0], err_msg=f"{tag}: x_lo")
    np.testing.assert_array_equal(raw[..., 1], model[..., 1], err_msg=f"{tag}: x_hi")
    np.testing.assert_array_equal(raw[..., 2], model[..., 2], err_msg=f"{tag}: fraction")
    got = env.K.percentiles_batch(t, q)
    assert got.shape == (frames.shape[0], len(q)) and got.dtype == np.float64
    np.testing.assert_array_equal(got, env.K.finish_percentiles(model[..., 0], model[..., 1], model[..., 2]), err_msg=tag)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")      # All-NaN slice / invalid value: NumPy still defines the result (NaN)
        ref = np.stack([np.nanpercentile(f.astype(np.float64), q) for f in frames])
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)


SIZES = [1, 2, 3, 5, 41, 61, 101, 1023, 1025, 2001, 24601, 131071, 131072, 131073, 262145]


@pytest.mark.parametrize("n", SIZES)
def test_percentiles_every_family(env, n):
    """Sizes up to the last single-workgroup one (131071) and the first multi-workgroup ones x every input family."""
    for fam in SN.SELECT_FAMILIES:
        _check_select(env, SN.select_family(fam, n), QS, f"{fam} n={n}")


@pytest.mark.parametrize("fam", ["squares", "low10", "nan50", "inf"])
def test_percentiles_largest_size(env, fam):
    n = (1 << 22) + 3
    _check_select(env, SN.select_family(fam, n), QS, f"{fam} n={n}")


@pytest.mark.parametrize("n", [5, 2001, 131071, 131073])
def test_percentiles_sixteen_queries_and_nq_limits(env, n):
    for fam in ("squares", "three", "nan50"):
        _check_select(env, SN.select_family(fam, n), QS16, f"{fam} n={n} nq=16")
    t = _dev(env, SN.select_family("normal", n))
    with pytest.raises(env.ffi.B4DError):
        env.K.percentiles_batch(t, QS16 + [42.0])
    with pytest.raises(env.ffi.B4DError):
        env.K.percentiles_batch(t, [])


@pytest.mark.parametrize("n, q", [(41, 95.0), (61, 95.0), (101, 95.0), (2001, 33.3), (24601, 99.0)])
def test_percentile_rank_next_to_integers(env, n, q):
    """Sizes where floor(q/100*(n-1)) and floor(NumPy's virtual index) differ (unshuffled squares: the value names the rank)."""
    x = (np.arange(n, dtype=np.float64) ** 2).astype(np.float32)[None]
    got = env.K.percentiles_batch(_dev(env, x), [q])
    assert got[0, 0] == pytest.approx(float(np.nanpercentile(x[0].astype(np.float64), q)), rel=1e-12)
    raw = _raw_rows(env, _dev(env, x), [q])[0, 0]
    assert raw[0] == float(np.float32(np.floor(SN.virtual_index(n, q)) ** 2))


@pytest.mark.parametrize("n", [10, 11, 1025, 131074, 131075])
def test_median_f32_odd_and_even_counts(env, n):
    from barc4dip_amd.preprocessing.normalize import _median_f32

    rng = np.random.default_rng(n)
    for n_nan in (3, 4):        # one of the two valid counts is odd, the other even
        x = (rng.standard_normal(n) * 1000.0).astype(np.float32)
        x[rng.choice(n, size=n_nan, replace=False)] = np.nan
        med, cnt = _median_f32(_dev(env, x))
        ref = np.nanmedian(x)
        assert cnt == n - n_nan and isinstance(med, np.float32) and ref.dtype == np.float32
        assert med == ref, (n, n_nan, med, ref)
    med, cnt = _median_f32(_dev(env, np.full(n, np.nan, np.float32)))
    assert np.isnan(med) and cnt == 0


# ------------------------------------------------------------------------------------------------ moments
EPS32 = float(np.float32(1e-6))
SAT = 3000.0
MOM_FAMILIES = ("constant", "offset", "eps_sat", "negzero", "sprinkled", "nofinite", "skewed")


def _mom_frame(fam, npix, rng):
    if fam == "constant":
        x = np.full(npix, 1234.5677)
    elif fam == "offset":
        x = 1e6 + rng.standard_normal(npix)
    elif fam == "eps_sat":
        x = rng.choice(np.array([EPS32, -EPS32, 0.5 * EPS32, 2.0 * EPS32, SAT, 2.0 * SAT, 0.999 * SAT, 10.0]), size=npix)
    elif fam == "negzero":
        x = rng.choice(np.array([-0.0, 0.0, 1.0, -3.0]), size=npix)
        x[0] = -0.0
    elif fam == "nofinite":
        x = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=npix)
    else:
        x = rng.exponential(100.0, size=npix)
    x = x.astype(np.float32)
    if fam == "eps_sat":
        x[:3] = (EPS32, -EPS32, SAT)
    if fam == "sprinkled":
        u = rng.random(npix)
        x[u < 0.1] = np.nan
        x[(u >= 0.1) & (u < 0.15)] = np.inf
        x[(u >= 0.15) & (u < 0.2)] = -np.inf
    return x


def _check_moment_rows(got, frames, fams, tag):
    model = SN.moments_rows(frames, eps=EPS32, saturation=SAT)
    for b, fam in enumerate(fams):
        k, m, t = got[b], model[b], f"{tag} frame {b} ({fam})"
        assert k[0] == m[0] and k[5] == m[5] and k[6] == m[6] and k[7] == 0.0, t      # counts exact
        if m[0] == 0:
            assert np.array_equal(k, np.zeros(8)), t       # the documented row of a frame without a finite value
            continue
        assert k[1] == pytest.approx(m[1], rel=1e-12), t
        if fam == "constant":
            assert k[1] == float(frames[b, 0]) and k[2] == 0.0 and k[3] == 0.0 and k[4] == 0.0, t
            continue
        v = frames[b].astype(np.float64)
        d = np.abs(v[np.isfinite(v)] - m[1])
        # only the summation order (and fma) differs: a few float64 roundings of the sum of magnitudes
        for j, p in ((2, 2), (3, 3), (4, 4)):
            assert abs(k[j] - m[j]) <= 1e-12 * np.sum(d ** p), (t, j, k[j], m[j])
        if m[2] > 0:
            assert np.sqrt(k[2] / k[0]) == pytest.approx(np.sqrt(m[2] / m[0]), rel=1e-12), t
        if frames.shape[1] >= 4096 and fam in ("offset", "eps_sat", "negzero", "sprinkled", "skewed"):
            vk, vm = k[2] / k[0], m[2] / m[0]
            assert (k[3] / k[0]) / vk ** 1.5 == pytest.approx((m[3] / m[0]) / vm ** 1.5, rel=1e-10), t
            assert (k[4] / k[0]) / vk ** 2 - 3.0 == pytest.approx((m[4] / m[0]) / vm ** 2 - 3.0, rel=1e-10), t
    if "eps_sat" in fams:
        b = fams.index("eps_sat")
        assert got[b, 5] >= 2 and got[b, 6] >= 1     # |x| == eps and x == saturation are counted


@pytest.mark.parametrize("batch, npix", [(1, 4), (1, 8), (1, 4096), (1, 4100), (1, 1 << 22), (3, 4), (3, 8), (3, 4100),
                                         (3, 1 << 22), (300, 8), (300, 4096), (300, 4100), (2049, 4), (2049, 8), (2049, 4096)])
def test_moments_batch_edges(env, batch, npix):
    rng = np.random.default_rng([batch, npix])
    nf = len(MOM_FAMILIES)
    starts = range(0, nf, batch) if batch < nf else (0,)
    if npix == 1 << 22 and batch > 1:
        starts = (0, 3)          # constant / offset / eps_sat and negzero / sprinkled / nofinite
    for s in starts:
        fams = [MOM_FAMILIES[(s + i) % nf] for i in range(batch)]
        frames = np.stack([_mom_frame(f, npix, rng) for f in fams])
        got = env.K.moments_batch(_dev(env, frames), eps=EPS32, saturation=SAT).cpu().numpy()
        _check_moment_rows(got, frames, fams, f"batch={batch} npix={npix}")


@pytest.mark.parametrize("shape", [(3, 5), (171,), (33, 31), (2, 3)])
def test_distribution_moments_pixel_count_not_multiple_of_4(env, shape):
    from barc4dip_amd.metrics import distribution_moments
    from oracle import metrics_np as M

    rng = np.random.default_rng(shape[0])
    img = rng.exponential(50.0, size=shape).astype(np.float32)
    img.flat[2] = np.nan
    img.flat[4] = 0.0
    got, ref = distribution_moments(img, saturation_value=100.0), M.distribution_moments(img, saturation_value=100.0)
    assert got["mean"] == pytest.approx(ref["mean"], rel=1e-12) and got["std"] == pytest.approx(ref["std"], rel=1e-12)
    assert got["frac_zero"] == ref["frac_zero"] and got["frac_sat"] == ref["frac_sat"]
    assert got["skewness"] == pytest.approx(ref["skewness"], rel=1e-10)
    assert got["kurtosis"] == pytest.approx(ref["kurtosis"], rel=1e-10)


def test_moments_cabi_rejects_ragged_and_unaligned(env):
    t = env.torch.ones(16, dtype=env.torch.float32, device="cuda")
    out = env.torch.full((1, 8), -7.0, dtype=env.torch.float64, device="cuda")
    call = lambda p, npix: env.lib.b4d_moments(p, 1, npix, 0.0, 1.0, env.D.ptr(out), env.ffi.stream_ptr())  # noqa: E731
    assert call(env.D.ptr(t), 6) == -1                       # B4D_EINVAL: npix % 4 != 0
    assert call(env.D.ptr(t[1:]), 8) == -1                   # B4D_EINVAL: frames 4 bytes off a 16-byte boundary
    assert call(env.D.ptr(t), 8) == 0
    env.torch.cuda.synchronize()
    assert out.cpu().numpy()[0, 0] == 8.0
    with pytest.raises(NotImplementedError):
        env.K.moments_batch(np.ones((2, 6), np.float32))


# ------------------------------------------------------------------------------------------------ Sobel / Laplace
def _check_sobel(got, model, tag):
    for b in range(got.shape[0]):
        t = f"{tag} frame {b}"
        assert got[b, 0] == pytest.approx(model[b, 0], rel=1e-12), t
        assert got[b, 1] == pytest.approx(model[b, 1], rel=1e-12), t
        assert abs(got[b, 2] - model[b, 2]) <= 1e-12 * np.sqrt(model[b, 3]), t
        assert got[b, 3] == pytest.approx(model[b, 3], rel=1e-12), t
        assert got[b, 3] - got[b, 2] ** 2 == pytest.approx(model[b, 3] - model[b, 2] ** 2, rel=1e-10), t


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (3, 65), (16, 64), (17, 65), (33, 129), (1000, 3)])
def test_sobel_laplace_small_and_ragged_shapes(env, shape):
    rng = np.random.default_rng(shape)
    frames = (500.0 + 100.0 * rng.standard_normal((5,) + shape)).astype(np.float32)
    got = env.K.sobel_laplace_batch(_dev(env, frames)).cpu().numpy()
    _check_sobel(got, SN.sobel_laplace_rows(frames), str(shape))
    if shape[0] == 1:
        assert np.all(got[:, 1] == 0.0)        # one row: the reflected rows are the row itself
    if shape[1] == 1:
        assert np.all(got[:, 0] == 0.0)


@pytest.mark.parametrize("shape", [(17, 65), (33, 129)])
def test_sobel_laplace_non_finite_neighbours(env, shape):
    """A non-finite pixel is left out as a centre, but its neighbours see it: NaN / inf propagate as in scipy."""
    rng = np.random.default_rng(shape)
    frames = (500.0 + 100.0 * rng.standard_normal((3,) + shape)).astype(np.float32)
    frames[0, shape[0] // 2, shape[1] // 2] = np.nan
    frames[0, 0, 0] = np.inf
    frames[1, 0, shape[1] - 1] = np.inf          # inf alone
    got = env.K.sobel_laplace_batch(_dev(env, frames)).cpu().numpy()
    model = SN.sobel_laplace_rows(frames)
    np.testing.assert_allclose(got[[0, 2]], model[[0, 2]], rtol=1e-12, equal_nan=True)
    assert np.isnan(got[0]).all() and np.isfinite(got[2]).all()
    # inf alone: the Laplacian statistics are +inf on both sides.  The Sobel ones are +inf here and NaN in scipy, whose
    # derivative pass multiplies the inf centre by its zero weight (0 * inf) and so hands NaN to the neighbouring rows; the
    # kernel has no zero-weight term.  Neither is a number: only non-finiteness is asserted for them.
    np.testing.assert_array_equal(got[1, 2:], model[1, 2:])
    assert np.all(got[1] == np.inf) and not np.isfinite(model[1, :2]).any()


def test_laplacian_variance_of_paraboloid_plus_noise(env, observe):
    """a (x^2 + y^2) + noise with a = 0.37: 4a in the interior, one-sided differences of order a x size on the reflecting
    border rows.  With reflecting borders the Laplacian of an all-finite frame sums to zero (every difference appears twice
    with opposite signs), so mean lap stays ~0 even here and mean lap^2 - (mean lap)^2 does not cancel; what the case adds
    over speckle frames is a Laplacian spread over several decades.  Only the summation order differs from the model; the
    observed difference sets the bar."""
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:100, 0:150].astype(np.float64)
    frames = np.stack([0.37 * ((xx - 70 - b) ** 2 + (yy - 40) ** 2) + rng.standard_normal(xx.shape) for b in range(3)]).astype(np.float32)
    got = env.K.sobel_laplace_batch(_dev(env, frames)).cpu().numpy()
    model = SN.sobel_laplace_rows(frames)
    _check_sobel(got, model, "paraboloid")
    for b in range(3):
        vk, vm = got[b, 3] - got[b, 2] ** 2, model[b, 3] - model[b, 2] ** 2
        assert vm > 50.0 and abs(model[b, 2]) < 1e-3
        print(f"lap var paraboloid: frame {b} mean lap {got[b, 2]!r} / {model[b, 2]!r} kernel {vk!r} model {vm!r} rel {abs(vk - vm) / vm:.3e}")
        observe("lap_var_paraboloid_rel", abs(vk - vm) / vm, BAR_LAPVAR_PARABOLOID)


# ------------------------------------------------------------------------------------------------ radial profile
@pytest.mark.parametrize("shape", [(2, 2), (3, 3), (127, 127), (128, 96), (97, 131)])
def test_radial_profile_sampling_edges(env, shape):
    from barc4dip_amd.maths.radial import radial_mean_interpolated, radial_profile_batch

    rng = np.random.default_rng(shape)
    maps = rng.standard_normal((3,) + shape).astype(np.float32)
    const = np.full(shape, 3.5, np.float32)
    half = float(min(shape[1] - 1 - shape[1] // 2, shape[1] // 2, shape[0] - 1 - shape[0] // 2, shape[0] // 2))
    half_default = float(min(shape[0] // 2, shape[1] // 2))
    for r_max in (0.5, None, 1.5 * half_default):
        nr_default = int(np.floor(half_default if r_max is None else r_max)) + 1
        for nr in (2, None):
            if nr is None and nr_default < 2:
                with pytest.raises(ValueError):
                    radial_profile_batch(maps, r_max=r_max)
                with pytest.raises(ValueError):
                    SN.radial_profile(maps, r_max=r_max)
                nr = 3
            for ntheta in (4, 255, 256, 257, 1130):
                tag = f"{shape} r_max={r_max} nr={nr} ntheta={ntheta}"
                got, r = radial_profile_batch(maps, r_max=r_max, nr=nr, ntheta=ntheta)
                ref, rr = SN.radial_profile(maps, r_max=r_max, nr=nr, ntheta=ntheta)
                np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12, err_msg=tag)
                np.testing.assert_array_equal(r, rr)
                for fill in (0.0, 2.5):
                    p1, _ = radial_mean_interpolated(maps[1], r_max=r_max, nr=nr, ntheta=ntheta, fill_value=fill)
                    q1, _ = SN.radial_profile(maps[1:2], r_max=r_max, nr=nr, ntheta=ntheta, fill_value=fill)
                    np.testing.assert_allclose(p1, q1[0], rtol=1e-9, atol=1e-12, err_msg=f"{tag} fill={fill}")
                pc, rc = radial_mean_interpolated(const, r_max=r_max, nr=nr, ntheta=ntheta)
                inside = rc <= half
                assert inside[0]
                np.testing.assert_allclose(pc[inside], 3.5, rtol=1e-9, atol=1e-12, err_msg=tag)


# ------------------------------------------------------------------------------------------------ PSD statistics
PSD_SHAPES = [(64, 64), (65, 65), (171, 171), (512, 512), (100, 37), (512, 300)]


def _check_psd_rows(env, maps, observe, tag):
    """All eight outputs of b4d_psd_stats against the model; returns (kernel rows, model rows)."""
    got = env.K.psd_stats_batch(_dev(env, maps))
    model = SN.psd_stats_rows(maps)
    assert got.shape == model.shape == (maps.shape[0], 8)
    for b in range(maps.shape[0]):
        for j in range(7):
            if model[b, j] == 0.0:
                assert got[b, j] == 0.0, (tag, b, j)
            else:
                rel = abs(got[b, j] - model[b, j]) / abs(model[b, j])
                print(f"psd sums: {tag} frame {b} out[{j}] kernel {got[b, j]!r} model {model[b, j]!r} rel {rel:.3e}")
                observe("psd_stats_sums_rel", rel, BAR_PSD_SUMS)
        if maps.shape[1] != maps.shape[2]:
            assert np.isnan(got[b, 7]) and np.isnan(model[b, 7]), (tag, b)
        elif np.isnan(model[b, 7]):
            assert np.isnan(got[b, 7]) or got[b, 7] == 0.0, (tag, b)
        else:
            assert got[b, 7] == pytest.approx(model[b, 7], rel=1e-12), (tag, b)
    return got, model


def _speckle_psd(shape, seed):
    from oracle import signal_np as S

    img = synth.speckle_frame(512, seed)[:shape[0], :shape[1]].astype(np.float64)
    return np.asarray(S.psd2d(img - img.mean(), scale=True)[0]).astype(np.float32)


@pytest.mark.parametrize("shape", PSD_SHAPES)
def test_psd_stats_speckle_and_dc(env, observe, shape):
    base = np.stack([_speckle_psd(shape, 40 + b) for b in range(3)])
    # a different f95 ring in every frame: damp the spectrum beyond a frame-dependent radius
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    rr = np.hypot(yy - shape[0] // 2, xx - shape[1] // 2)
    for b in range(3):
        base[b] *= np.exp(-rr / (0.05 * (b + 1) * min(shape))).astype(np.float32)
    got, model = _check_psd_rows(env, base, observe, f"speckle {shape}")
    if shape[0] == shape[1]:
        assert len(set(got[:, 7])) == 3
    # NaN, +inf and a large value at the DC bin count as 0; so does a non-finite bin elsewhere
    odd = base.copy()
    for b, v in enumerate((np.nan, np.inf, 3e37)):
        odd[b, shape[0] // 2, shape[1] // 2] = v
    got2, _ = _check_psd_rows(env, odd, observe, f"dc {shape}")
    assert np.array_equal(got2, got, equal_nan=True)
    odd[0, 1, 2], odd[1, 2, 1] = np.nan, -np.inf
    _check_psd_rows(env, odd, observe, f"nonfinite {shape}")


@pytest.mark.parametrize("shape", PSD_SHAPES)
def test_psd_stats_single_bins_rings_and_disc_edge(env, observe, shape):
    ny, nx = shape
    cy, cx = ny // 2, nx // 2
    # one non-zero bin per frame: f95 is exactly that bin's radius
    offs = [(0, 1), (3, -4), (-(min(shape) // 4), min(shape) // 5)]
    one = np.zeros((3, ny, nx), np.float32)
    for b, (dy, dx) in enumerate(offs):
        one[b, cy + dy, cx + dx] = 7.0
    got, _ = _check_psd_rows(env, one, observe, f"single {shape}")
    if ny == nx:
        for b, (dy, dx) in enumerate(offs):
            assert got[b, 7] == pytest.approx(np.sqrt(float(dy * dy + dx * dx)) / nx, rel=1e-12)
            assert got[b, 0] == 7.0 and got[b, 4] == 49.0 and got[b, 5] == 7.0
    # two rings holding 94.9 % / 5.1 % (f95 on the outer one) and 95.1 % / 4.9 % (f95 on the inner one)
    for inner, outer, where in ((94.9, 5.1, "outer"), (95.1, 4.9, "inner")):
        two = np.zeros((3, ny, nx), np.float32)
        radii = [(2 + b, 5 + 2 * b) for b in range(3)]
        for b, (r1, r2) in enumerate(radii):
            two[b, cy, cx + r1] = inner
            two[b, cy - r2, cx] = outer
        got, _ = _check_psd_rows(env, two, observe, f"rings {where} {shape}")
        if ny == nx:
            for b, (r1, r2) in enumerate(radii):
                assert got[b, 7] == pytest.approx((r2 if where == "outer" else r1) / nx, rel=1e-12)
    # power on the bin with fr == f_max exactly (inside the disc) and in the corners (outside: S_all only)
    edge = np.zeros((3, ny, nx), np.float32)
    on_x = (nx // 2) / nx <= (ny // 2) / ny
    for b in range(3):
        if on_x:
            edge[b, cy, 0] = 11.0 + b          # fx = -(nx // 2) / nx
        else:
            edge[b, 0, cx] = 11.0 + b
        edge[b, 0, 0] = 5.0
        edge[b, ny - 1, nx - 1] = 2.0
    got, _ = _check_psd_rows(env, edge, observe, f"edge {shape}")
    for b in range(3):
        assert got[b, 0] == 11.0 + b and got[b, 5] == 18.0 + b
        if ny == nx:
            assert got[b, 7] == pytest.approx((nx // 2) / nx, rel=1e-12)


@pytest.mark.parametrize("shape", [(64, 64), (65, 65), (100, 37)])
def test_psd_stats_all_zero_map(env, observe, shape):
    from barc4dip_amd.metrics import speckles

    got, _ = _check_psd_rows(env, np.zeros((3,) + shape, np.float32), observe, f"zero {shape}")
    assert np.array_equal(got[:, :7], np.zeros((3, 7)))
    with pytest.raises(ValueError):
        speckles._bandwidth_from(got[0])
    with pytest.raises(ValueError):
        speckles.bandwidth(np.zeros((128, 96) if shape[0] != shape[1] else (64, 64), np.float32))


# ------------------------------------------------------------------------------------------------ temporal
def _edge_stack(T, shape, seed):
    rng = np.random.default_rng(seed)
    stack = rng.poisson(700.0, size=(T,) + shape).astype(np.float32)
    stack[T // 2, 1, 2] = np.nan
    stack[T - 1, 2, 1] = np.inf
    stack[:, 3, 3] = 0.0
    return stack


@pytest.mark.parametrize("T", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("shape", [(6, 10), (5, 7)])
def test_temporal_stats_nan_inf_and_zero_pixels(env, T, shape):
    """The four-frame unroll and its remainder, on 16-byte frames (6 x 10) and on odd ones (5 x 7: the dword kernel)."""
    from barc4dip_amd.metrics import temporal_stats
    from oracle import temporal_np as Tn

    stack = _edge_stack(T, shape, T)
    with np.errstate(all="ignore"):
        ref = Tn.temporal_stats(stack)
    for chunk in (2, 1024):
        got = temporal_stats(stack, chunk=chunk)
        for g, r in zip(got, ref):
            assert g.shape == shape and g.dtype == np.float32
            np.testing.assert_allclose(g, r, rtol=2e-6, atol=1e-6, equal_nan=True)
        mean, var, con = got
        assert np.isnan(var[1, 2]) and np.isnan(var[2, 1]) and np.isnan(mean[1, 2]) and mean[2, 1] == np.inf
        assert mean[3, 3] == 0.0 and var[3, 3] == 0.0 and np.isnan(con[3, 3])


@pytest.mark.parametrize("T", [1, 3, 4, 5, 9])
def test_temporal_accumulate_range_direct(env, T):
    stride = 64
    stack = _edge_stack(T, (8, 8), 50 + T)
    t = _dev(env, stack.reshape(T, stride))
    assert t.data_ptr() % 16 == 0

    def run(pix0, npix):
        acc = env.torch.full((2, npix + 8), -3.0, dtype=env.torch.float64, device="cuda")
        acc[:, 4:4 + npix] = 0.0
        rc = env.lib.b4d_temporal_accumulate_range(env.D.ptr(t), T, stride, pix0, npix, env.D.ptr(acc[0, 4:]), env.D.ptr(acc[1, 4:]),
                                                   env.ffi.stream_ptr())
        env.ffi.check(rc)
        return acc.cpu().numpy()

    # whole frames; an aligned range of 16-byte groups; an unaligned start; a ragged count; the last pixels
    for pix0, npix in ((0, 64), (8, 32), (3, 32), (8, 30), (5, 7), (60, 4), (63, 1)):
        a = run(pix0, npix)
        sx, sxx = SN.temporal_sums_range(stack, pix0, npix)
        np.testing.assert_array_equal(a[0, 4:4 + npix], sx, err_msg=f"{pix0}+{npix}")      # integer counts sum exactly
        np.testing.assert_array_equal(a[1, 4:4 + npix], sxx, err_msg=f"{pix0}+{npix}")
        assert np.all(a[:, :4] == -3.0) and np.all(a[:, 4 + npix:] == -3.0)               # nothing written around the range
    for pix0, npix in ((61, 4), (0, 65), (64, 1)):
        with pytest.raises(env.ffi.B4DError):
            run(pix0, npix)


def test_temporal_accumulate_range_two_workgroups(env):
    """1028 pixels are 257 groups of four: two workgroups of the 16-byte kernel, the second with one live lane; five of the dword
    kernel on the unaligned range."""
    T, stride = 5, 1028
    stack = _edge_stack(T, (4, 257), 71)
    t = _dev(env, stack.reshape(T, stride))
    assert t.data_ptr() % 16 == 0
    for pix0, npix in ((0, 1028), (4, 1024), (1, 1027)):
        acc = env.torch.full((2, npix + 8), -3.0, dtype=env.torch.float64, device="cuda")
        acc[:, 4:4 + npix] = 0.0
        env.ffi.check(env.lib.b4d_temporal_accumulate_range(env.D.ptr(t), T, stride, pix0, npix, env.D.ptr(acc[0, 4:]),
                                                            env.D.ptr(acc[1, 4:]), env.ffi.stream_ptr()))
        a = acc.cpu().numpy()
        sx, sxx = SN.temporal_sums_range(stack, pix0, npix)
        np.testing.assert_array_equal(a[0, 4:4 + npix], sx, err_msg=f"{pix0}+{npix}")
        np.testing.assert_array_equal(a[1, 4:4 + npix], sxx, err_msg=f"{pix0}+{npix}")
        assert np.all(a[:, :4] == -3.0) and np.all(a[:, 4 + npix:] == -3.0)               # nothing written around the range


def test_temporal_finalize_count_and_null_outputs(env):
    T = 5
    stack = _edge_stack(T, (6, 10), 9)
    sx, sxx = SN.temporal_sums_range(stack, 0, 60)
    want = SN.temporal_finalize(sx, sxx, T)
    dsx, dsxx = _dev(env, sx), _dev(env, sxx)
    f32 = lambda: env.torch.full((60,), -3.0, dtype=env.torch.float32, device="cuda")  # noqa: E731
    mean, var, con = f32(), f32(), f32()
    fin = env.lib.b4d_temporal_finalize
    for count in (0.0, -1.0, float("nan")):
        with pytest.raises(env.ffi.B4DError):
            env.ffi.check(fin(env.D.ptr(dsx), env.D.ptr(dsxx), count, 60, env.D.ptr(mean), env.D.ptr(var), env.D.ptr(con),
                              env.ffi.stream_ptr()))
    env.ffi.check(fin(env.D.ptr(dsx), env.D.ptr(dsxx), float(T), 60, env.D.ptr(mean), env.D.ptr(var), env.D.ptr(con),
                      env.ffi.stream_ptr()))
    mean2 = f32()
    env.ffi.check(fin(env.D.ptr(dsx), env.D.ptr(dsxx), float(T), 60, env.D.ptr(mean2), None, None, env.ffi.stream_ptr()))
    cnt = _dev(env, np.array([float(T)]))
    m3, v3, c3 = f32(), f32(), f32()
    env.ffi.check(env.lib.b4d_temporal_finalize_dev(env.D.ptr(dsx), env.D.ptr(dsxx), env.D.ptr(cnt), 60, env.D.ptr(m3), env.D.ptr(v3),
                                                    env.D.ptr(c3), env.ffi.stream_ptr()))
    env.torch.cuda.synchronize()
    for g, r in zip((mean, var, con), want):
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-6, atol=1e-6, equal_nan=True)
    assert np.array_equal(mean.cpu().numpy(), mean2.cpu().numpy(), equal_nan=True)
    for a, b in zip((mean, var, con), (m3, v3, c3)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    v = var.cpu().numpy().reshape(6, 10)
    assert np.isnan(v[1, 2]) and np.isnan(v[2, 1]) and v[3, 3] == 0.0
    # a variance that rounds below zero is still clamped: identical frames of a value whose square is inexact
    same = np.full((3, 8), 0.1, np.float32)
    sx, sxx = SN.temporal_sums_range(same, 0, 8)
    sxx = sxx - 1e-12
    m, v, c = f32(), f32(), f32()
    dsx, dsxx = _dev(env, sx), _dev(env, sxx)
    env.ffi.check(fin(env.D.ptr(dsx), env.D.ptr(dsxx), 3.0, 8, env.D.ptr(m), env.D.ptr(v), env.D.ptr(c), env.ffi.stream_ptr()))
    env.torch.cuda.synchronize()
    assert np.all(v.cpu().numpy()[:8] == 0.0) and np.all(c.cpu().numpy()[:8] == 0.0)
