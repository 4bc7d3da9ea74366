"""Host tier: the NumPy model of the reduction / selection kernels (oracle/stats_np.py) against what the project
already trusts -- oracle.metrics_np for the PSD statistics, np.nanpercentile for the order statistics -- so that the GPU
tier (tests/test_gpu_stats_edges.py) can compare raw kernel outputs with the model."""
import numpy as np
import pytest

from barc4dip_amd import synth
from barc4dip_amd.metrics.kernels import finish_percentiles
from oracle import metrics_np as M
from oracle import signal_np as S
from oracle import stats_np as SN

QS = [0.0, 0.05, 1.0, 5.0, 25.0, 33.3, 50.0, 75.0, 95.0, 98.0, 99.0, 99.95, 100.0]


def _squares(n, seed, nan_every=0):
    """n distinct, widely spaced values in random order; every `nan_every`-th element NaN."""
    x = np.arange(n, dtype=np.float64) ** 2
    np.random.default_rng(seed).shuffle(x)
    if nan_every:
        x[::nan_every] = np.nan
    return x


def _finished(x, q):
    r = SN.select_rows(x[None], q)[0]
    return finish_percentiles(r[:, 0], r[:, 1], r[:, 2]), r


@pytest.mark.parametrize("shape", [(256, 256), (300, 420)])
def test_psd_stats_rows_reproduce_bandwidth_and_entropy(shape):
    img = synth.speckle_frame(512, 77)[:shape[0], :shape[1]].astype(np.float64)
    ref = M.bandwidth(img)
    sq = S.pad_to_square(img, fill_value=np.mean(img))
    P = S.psd2d(sq - float(np.nanmean(sq)), dx=1.0, dy=1.0, scale=True)[0]
    got = SN.bandwidth_from_row(SN.psd_stats_rows(np.asarray(P)[None])[0])
    for k in ("feq", "sig_fx", "sig_fy", "f95", "spr"):
        assert got[k] == pytest.approx(ref[k], rel=1e-12), k
    # spectral entropy: no padding (like the reference), so the 300 x 420 map is a non-square one
    Pe = np.asarray(S.psd2d(img - float(np.mean(img)), scale=False)[0])
    row = SN.psd_stats_rows(Pe[None])[0]
    assert SN.entropy_from_row(row, Pe.size) == pytest.approx(M.spectral_entropy(img), rel=1e-12)
    assert np.isnan(row[7]) == (shape[0] != shape[1])


def test_psd_stats_rows_edges():
    P = np.zeros((2, 8, 8))
    P[0, 4, 4] = np.inf          # DC: ignored
    P[0, 4, 0] = 3.0             # fx = -0.5 = f_max: inside the disc
    P[0, 0, 0] = 5.0             # corner: outside, counted in S_all only
    P[0, 1, 1] = np.nan
    r = SN.psd_stats_rows(P)
    assert r[0, 0] == 3.0 and r[0, 5] == 8.0 and r[0, 7] == 0.5 and r[0, 4] == 9.0
    assert r[0, 6] == pytest.approx(3 * np.log(3) + 5 * np.log(5), rel=1e-15)
    assert np.array_equal(r[1, :7], np.zeros(7)) and np.isnan(r[1, 7])
    with pytest.raises(ValueError):
        M.bandwidth(np.full((8, 8), 3.0))


def test_select_rows_and_finish_vs_nanpercentile():
    """Every n in 1..3000 (and three large sizes) x 13 percentiles: rank, fraction and the finishing interpolation
    reproduce np.nanpercentile at the suite's percentile bar.  Taking the rank from floor(q/100*(n-1)) and the fraction
    from NumPy's virtual index (the earlier arithmetic) misses this bar at 64 of these sizes by a whole gap between
    neighbouring order statistics; see test_mixed_rank_formulas_bracket_the_wrong_pair."""
    for n in list(range(1, 3001)) + [24601, 33451, 131073]:
        x = _squares(n, n, nan_every=5 if n % 3 == 0 and n > 5 else 0)
        got, r = _finished(x, QS)
        np.testing.assert_allclose(got, np.nanpercentile(x, QS), rtol=1e-12, atol=0, err_msg=f"n={n}")
        assert np.all(r[:, 3] == np.count_nonzero(~np.isnan(x)))
        assert np.all((r[:, 2] >= 0.0) & (r[:, 2] <= 1.0)) and np.all(r[:, 0] <= r[:, 1])


@pytest.mark.parametrize("n, q, want", [(41, 95.0, 1444.0), (61, 95.0, 3249.0), (101, 95.0, 9025.0),
                                        (2001, 33.3, 443556.0), (24601, 99.0, 593117316.0)])
def test_mixed_rank_formulas_bracket_the_wrong_pair(n, q, want):
    """The sizes where floor(q/100*(n-1)) and floor(NumPy's virtual index) differ: the model (and the kernels, which
    share its arithmetic) follow NumPy; a rank from the former with a fraction from the latter is off by a whole gap."""
    x = np.arange(n, dtype=np.float64) ** 2
    ref = float(np.nanpercentile(x, q))
    assert ref == pytest.approx(want, rel=3e-10)
    got, r = _finished(x, [q])
    assert got[0] == pytest.approx(ref, rel=1e-12)
    # the earlier arithmetic, on the same sorted data
    lo_old = int(np.floor(q / 100.0 * (n - 1)))
    vi = SN.virtual_index(n, q)
    frac = float(vi - np.floor(vi))
    old = finish_percentiles(x[lo_old], x[min(lo_old + 1, n - 1)], frac)
    assert lo_old != int(np.floor(vi))
    assert abs(float(old) - ref) > 1e-5 * ref          # 1521 vs 1444 at n = 41; the bar is 1e-12


def test_select_rows_edge_values():
    inf = np.inf
    x = np.array([[np.nan] * 4, [np.nan, 2.0, np.nan, np.nan], [-inf, 1.0, 2.0, inf], [-0.0, 0.0, -0.0, 0.0]])
    r = SN.select_rows(x, [0.0, 50.0, 100.0])
    assert np.isnan(r[0, :, :2]).all() and np.all(r[0, :, 2:] == 0.0)
    assert np.all(r[1, :, :2] == 2.0) and np.all(r[1, :, 3] == 1.0)
    with np.errstate(invalid="ignore"):
        want = np.nanpercentile(x[2], [0.0, 50.0, 100.0])
    np.testing.assert_array_equal(finish_percentiles(r[2, :, 0], r[2, :, 1], r[2, :, 2]), want)     # NaN, 1.5, NaN
    assert np.isnan(want[0]) and want[1] == 1.5
    assert np.all(finish_percentiles(r[3, :, 0], r[3, :, 1], r[3, :, 2]) == 0.0)


def test_moments_and_sobel_models_vs_metrics_oracle():
    img = synth.speckle_frame(128, 5)[:100, :77].copy()
    img[3, 4] = np.nan
    img[50, 6] = np.inf
    img[:2, :2] = 0.0
    n, mean, m2, m3, m4, nz, ns, _ = SN.moments_rows(img[None], saturation=3000.0)[0]
    ref = M.distribution_moments(img, saturation_value=3000.0)
    var = m2 / n
    assert mean == pytest.approx(ref["mean"], rel=1e-14) and np.sqrt(var) == pytest.approx(ref["std"], rel=1e-13)
    assert (m3 / n) / var ** 1.5 == pytest.approx(ref["skewness"], rel=1e-12)
    assert (m4 / n) / var ** 2 - 3.0 == pytest.approx(ref["kurtosis"], rel=1e-12)
    assert nz / n == ref["frac_zero"] and ns / n == ref["frac_sat"]
    assert np.array_equal(SN.moments_rows(np.full((1, 8), np.nan, np.float32)), np.zeros((1, 8)))
    clean = synth.speckle_frame(128, 6)[:33, :65]
    row = SN.sobel_laplace_rows(clean[None])[0]
    t = M.tenengrad(clean)
    assert row[0] == pytest.approx(t["ex"], rel=1e-14) and row[1] == pytest.approx(t["ey"], rel=1e-14)
    assert row[3] - row[2] ** 2 == pytest.approx(M.laplacian_variance(clean), rel=1e-11)


def test_temporal_model_keeps_nan_variance():
    stack = np.random.default_rng(3).poisson(50.0, size=(5, 2, 3)).astype(np.float32)
    stack[2, 0, 0] = np.nan
    stack[1, 0, 1] = np.inf
    stack[:, 1, 1] = 0.0
    sx, sxx = SN.temporal_sums_range(stack, 0, 6)
    mean, var, con = SN.temporal_finalize(sx, sxx, 5)
    from oracle import temporal_np as Tn
    with np.errstate(invalid="ignore"):
        rm, rv, rc = Tn.temporal_stats(stack)
    np.testing.assert_allclose(mean.reshape(2, 3), rm, rtol=1e-14, equal_nan=True)
    np.testing.assert_allclose(var.reshape(2, 3), rv, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert np.isnan(var[0]) and np.isnan(var[1]) and var[4] == 0.0 and np.isnan(con[4])
