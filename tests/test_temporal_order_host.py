"""Host tier of the temporal order statistics (barc4dip_amd.metrics.order, barc4dip_amd.preprocessing.combine): the NumPy model
that the GPU tier (tests/test_gpu_temporal_order.py) compares the kernels with, checked here against np.percentile /
np.nanpercentile / np.median / np.nanmedian; the robust-mean model on planted outliers; the sorting networks of
csrc/b4d_sortnet.hpp, proved as host code by a small C++ program; and the Python layer's plumbing.

Bars.  lower / higher / nearest and the median are selections (the median of an even count: one float32 addition and an exact
halving): exact equality with NumPy.  linear / midpoint: the model rounds the exact value once (after three float64 operations
that are exact or far below a float32 ulp), so it is within half a float32 ulp of the exact value; NumPy's lerp a + (b - a) g of
same-sign data, cast to float32, is within 1.5 ulps even where it runs in float32 (three roundings).  Bar: 2 ulps."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import temporal_order_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = [2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 100]
QS = [0.0, 10.0, 25.0, 37.5, 50.0, 62.5, 99.0, 100.0]


def with_nans(x, seed):
    """x with NaN samples: pixel 0 all NaN, pixel 1 one NaN, a tenth of the rest sprinkled."""
    rng = np.random.default_rng(seed)
    y = x.copy()
    y[rng.random(y.shape) < 0.1] = np.nan
    flat = y.reshape(y.shape[0], -1)
    flat[:, 0] = np.nan
    flat[:, 1] = x.reshape(x.shape[0], -1)[:, 1]
    flat[0, 1] = np.nan
    return y


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the model against NumPy
@pytest.mark.parametrize("T", TS)
def test_model_selection_methods_equal_numpy(T):
    x = M.counts_stack(T, (6, 7), seed=T)
    xn = with_nans(x, T)
    for method in ("lower", "higher", "nearest"):
        got = M.percentile(x, QS, method)
        assert got.dtype == np.float32 and same(got, np.percentile(x, QS, axis=0, method=method)), (T, method)
        with _quiet():
            assert same(M.percentile(xn, QS, method, ignore_nan=True), np.nanpercentile(xn, QS, axis=0, method=method)), (T, method)
            assert same(M.percentile(xn, QS, method), np.percentile(xn, QS, axis=0, method=method)), (T, method)


@pytest.mark.parametrize("T", TS)
def test_model_median_equals_numpy(T):
    x = M.counts_stack(T, (6, 7), seed=100 + T)
    xn = with_nans(x, T)
    assert same(M.median(x), np.median(x, axis=0))
    with _quiet():
        assert same(M.median(xn), np.median(xn, axis=0))                             # propagate: any NaN -> NaN
        assert same(M.median(xn, ignore_nan=True), np.nanmedian(xn, axis=0))         # omit; the all-NaN pixel is NaN
    assert np.isnan(M.median(xn, ignore_nan=True).reshape(-1)[0]) and not np.isnan(M.median(xn, ignore_nan=True).reshape(-1)[1])
    assert M.median(x).dtype == np.float32 and same(M.median(x), M.percentile(x, 50.0, "midpoint"))


@pytest.mark.parametrize("T", TS)
def test_model_interpolating_methods_within_two_ulps_of_numpy(T):
    x = M.counts_stack(T, (6, 7), seed=200 + T)
    xn = with_nans(x, T)
    worst = 0
    for method in ("linear", "midpoint"):
        ref = np.percentile(x, QS, axis=0, method=method).astype(np.float32)
        worst = max(worst, int(M.ulp_distance(M.percentile(x, QS, method), ref).max()))
        with _quiet():
            refn = np.nanpercentile(xn, QS, axis=0, method=method).astype(np.float32)
            got = M.percentile(xn, QS, method, ignore_nan=True)
            assert np.array_equal(np.isnan(got), np.isnan(refn))
            worst = max(worst, int(M.ulp_distance(got, refn).max()))
            assert same(np.isnan(M.percentile(xn, QS, method)), np.isnan(np.percentile(xn, QS, axis=0, method=method)))
    print(f"T={T}: largest distance to NumPy {worst} ulp")
    assert worst <= 2


def test_model_scalar_and_sequence_and_count():
    x = with_nans(M.counts_stack(9, (4, 5), seed=3), 3)
    assert M.percentile(x, 30.0).shape == (4, 5) and M.percentile(x, [30.0]).shape == (1, 4, 5)
    res, nv = M.quantiles(x, [0.3, 0.6], "linear", ignore_nan=True)
    assert res.shape == (2, 4, 5) and same(nv, np.count_nonzero(~np.isnan(x), axis=0)) and nv.reshape(-1)[0] == 0
    i, g = M.quantile_position(0.5, np.array([0, 1, 2, 3, 4]), "nearest")           # h = -, 0, 0.5, 1, 1.5 -> half to even
    assert list(i) == [0, 0, 0, 1, 2] and not g.any()
    i, g = M.quantile_position(0.5, np.array([2, 3]), "midpoint")
    assert list(i) == [0, 1] and list(g) == [0.5, 0.0]


class _quiet:
    """NumPy warns about all-NaN slices and invalid values; they are the cases under test."""

    def __enter__(self):
        import warnings

        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore")
        self._e = np.errstate(all="ignore")
        self._e.__enter__()

    def __exit__(self, *a):
        self._e.__exit__(*a)
        self._w.__exit__(*a)


# ------------------------------------------------------------------------------------------------ the robust model
@pytest.mark.parametrize("scale,kw", [("absolute", dict(threshold=300.0)), ("mad", dict(threshold=6.0)),
                                      ("poisson", dict(threshold=6.0, min_scale=1.0))])
def test_robust_model_finds_planted_samples(scale, kw):
    x, hot, dead = M.zinger_stack(40, (8, 9), seed=5)
    assert hot.any() and dead.any() and not (hot & dead).any()
    both = M.robust_mean(x, scale=scale, polarity="both", **kw)
    assert both["rejected"][hot | dead].all() and np.count_nonzero(both["rejected"] & ~(hot | dead)) <= x.size // 200
    r_hot = M.robust_mean(x, scale=scale, polarity="hot", **kw)["rejected"]
    r_dead = M.robust_mean(x, scale=scale, polarity="dead", **kw)["rejected"]
    assert r_hot[hot].all() and not r_hot[dead].any() and r_dead[dead].all() and not r_dead[hot].any()
    assert same(both["n_kept"], 40 - both["rejected"].sum(axis=0))
    assert np.all(np.abs(both["mean"] - 400.0) < 25.0) and both["mean"].dtype == np.float32
    assert same(both["cleaned"][~both["rejected"]], x[~both["rejected"]])
    assert same(both["cleaned"][both["rejected"]], np.broadcast_to(both["median"], x.shape)[both["rejected"]])
    assert same(both["median"], np.median(x, axis=0))


def test_robust_model_mad_degeneracy_nonfinite_and_empty():
    x = np.full((9, 4), 7.0, np.float32)
    x[3, 0] = 7.5                                     # pixel 0: eight equal samples and one that differs by little
    x[:, 1] = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    x[2, 2], x[5, 2] = np.inf, np.nan                 # pixel 2: non-finite samples are always rejected
    x[:, 3] = np.nan                                  # pixel 3: nothing takes part
    x[0, 3] = -np.inf
    r = M.robust_mean(x, threshold=5.0, scale="mad")
    assert r["scale"][0] == 0.0 and r["rejected"][:, 0].sum() == 1 and r["rejected"][3, 0] and r["mean"][0] == 7.0   # mad = 0
    floor_ = M.robust_mean(x, threshold=5.0, scale="mad", min_scale=0.2)
    assert floor_["scale"][0] == np.float32(5.0) * np.float32(0.2) and not floor_["rejected"][:, 0].any()
    assert not r["rejected"][:, 1].any() and r["mean"][1] == 5.0 and r["n_kept"][1] == 9
    for pol in M.POLARITIES:
        for scale in M.SCALES:
            q = M.robust_mean(x, threshold=1e9, scale=scale, polarity=pol)
            assert q["rejected"][2, 2] and q["rejected"][5, 2] and q["rejected"][:, 2].sum() == 2 and q["n_kept"][2] == 7
            assert q["mean"][2] == 7.0 and q["cleaned"][2, 2] == 7.0
            assert q["n_kept"][3] == 0 and np.isnan(q["mean"][3]) and np.isnan(q["median"][3]) and q["rejected"][:, 3].all()


# ------------------------------------------------------------------------------------------------ the networks as host code
SORTNET_PROGRAM = r"""
// Proves the sorting networks of b4d_sortnet.hpp as host code.  Zero-one principle: a network of min / max exchanges that sorts
// every 0-1 input sorts every input; 64 patterns are evaluated at a time (lo = AND, hi = OR on 64-bit words).  N <= 16: every
// 0-1 input.  N = 32, 64: the network sorts its halves with the network of half the size (proved before) and merges them, so
// the merge is run on every pair of sorted 0-1 halves, (N / 2 + 1)^2 inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "b4d_sortnet.hpp"
using namespace b4d::rankfilt;
namespace sn = b4d::sortnet;

struct BitOps {
    typedef uint64_t T;
    static T lo(T a, T b) { return a & b; }
    static T hi(T a, T b) { return a | b; }
};
static long g_count = 0;
struct CountOps {
    typedef uint32_t T;
    static T lo(T a, T b) { ++g_count; return a < b ? a : b; }
    static T hi(T a, T b) { return a < b ? b : a; }
};
static const uint64_t LANE_BITS[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                      0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
// a sorted 0-1 word: output j holds a one in the patterns with more than N - 1 - j ones
template <int N>
static long exhaustive() {
    long bad = 0;
    const uint64_t words = N > 6 ? (1ull << (N - 6)) : 1;
    const uint64_t valid = N >= 6 ? ~0ull : ((1ull << (1 << N)) - 1);
    for (uint64_t base = 0; base < words; ++base) {
        uint64_t v[N];
        for (int i = 0; i < N; ++i) v[i] = i < 6 ? LANE_BITS[i] : (((base >> (i - 6)) & 1) ? ~0ull : 0ull);
        sn::sortnet<BitOps, N>(v);
        for (int j = 0; j < N; ++j) {
            uint64_t want = 0;
            for (int lane = 0; lane < 64; ++lane)
                if (__builtin_popcountll(((base << 6) | (uint64_t)lane) & (N >= 64 ? ~0ull : ((1ull << N) - 1))) > N - 1 - j) want |= 1ull << lane;
            if ((v[j] ^ want) & valid) ++bad;
        }
    }
    std::printf("sortnet %d: all 2^%d zero-one inputs, %ld bad words\n", N, N, bad);
    return bad;
}
// every pair of sorted 0-1 halves: the lower half has a ones, the upper half b ones
template <int N>
static long merges() {
    long bad = 0, inputs = 0;
    for (int a = 0; a <= N / 2; ++a)
        for (int b = 0; b <= N / 2; ++b, ++inputs) {
            uint64_t v[N];
            for (int i = 0; i < N / 2; ++i) {
                v[i] = i >= N / 2 - a ? 1ull : 0ull;
                v[N / 2 + i] = i >= N / 2 - b ? 1ull : 0ull;
            }
            sn::odd_even_merge<BitOps, N, 0, N>(v);
            for (int j = 0; j < N; ++j)
                if (v[j] != (j >= N - a - b ? 1ull : 0ull)) ++bad;
        }
    std::printf("merge %d: %ld pairs of sorted zero-one halves, %ld bad outputs\n", N, inputs, bad);
    return bad + (inputs != (long)(N / 2 + 1) * (N / 2 + 1));
}
static float random_value(std::mt19937_64& rng) {
    const int kind = rng() % 16;
    if (kind == 0) return std::numeric_limits<float>::quiet_NaN();
    if (kind == 1) return -std::numeric_limits<float>::quiet_NaN();
    if (kind == 2) return 0.0f;
    if (kind == 3) return -0.0f;
    if (kind == 4) return std::numeric_limits<float>::infinity();
    if (kind == 5) return -std::numeric_limits<float>::infinity();
    if (kind < 11) return (float)((int)(rng() % 7) - 3);          // ties
    return (float)((double)(rng() % 2000001) / 1000.0 - 1000.0);
}
// random float keys, the last `pad` of them the pad key 0xFFFFFFFF, against std::sort
template <int N>
static long random_keys(long trials, std::mt19937_64& rng) {
    long bad = 0;
    for (long k = 0; k < trials; ++k) {
        uint32_t v[N];
        std::vector<uint32_t> s(N);
        const int pad = (int)(rng() % N);
        for (int i = 0; i < N; ++i) v[i] = s[i] = i < N - pad ? to_key(random_value(rng)) : 0xFFFFFFFFu;
        std::sort(s.begin(), s.end());
        sn::sortnet<KeyOps, N>(v);
        for (int i = 0; i < N; ++i)
            if (v[i] != s[i]) { ++bad; break; }
        if (pad < N && !(KEY_NAN < 0xFFFFFFFFu && v[N - pad - 1] <= KEY_NAN)) ++bad;   // data and NaNs first, then the pad
    }
    std::printf("sortnet %d: %ld random key sets against std::sort, %ld bad\n", N, trials, bad);
    return bad;
}
template <int N>
static long counted(long want) {
    uint32_t v[N];
    for (int i = 0; i < N; ++i) v[i] = (uint32_t)(N - i);
    g_count = 0;
    sn::sortnet<CountOps, N>(v);
    const long bad = (g_count != want) + (sn::exchanges(N) != want);
    std::printf("sortnet %d: %ld exchanges (expected %ld)\n", N, g_count, want);
    return bad;
}
static long positions() {      // quantile_position on a few hand-made cases
    long bad = 0;
    int i;
    double g;
    sn::quantile_position(0.5, 4, sn::METHOD_LINEAR, i, g);   bad += !(i == 1 && g == 0.5);
    sn::quantile_position(0.5, 4, sn::METHOD_LOWER, i, g);    bad += !(i == 1 && g == 0.0);
    sn::quantile_position(0.5, 4, sn::METHOD_HIGHER, i, g);   bad += !(i == 2 && g == 0.0);
    sn::quantile_position(0.5, 4, sn::METHOD_NEAREST, i, g);  bad += !(i == 2 && g == 0.0);   // 1.5 -> 2
    sn::quantile_position(0.5, 2, sn::METHOD_NEAREST, i, g);  bad += !(i == 0 && g == 0.0);   // 0.5 -> 0 (half to even)
    sn::quantile_position(0.5, 4, sn::METHOD_MIDPOINT, i, g); bad += !(i == 1 && g == 0.5);
    sn::quantile_position(0.5, 5, sn::METHOD_MIDPOINT, i, g); bad += !(i == 2 && g == 0.0);
    sn::quantile_position(1.0, 7, sn::METHOD_LINEAR, i, g);   bad += !(i == 6 && g == 0.0);
    sn::quantile_position(0.7, 0, sn::METHOD_LINEAR, i, g);   bad += !(i == 0 && g == 0.0);
    std::printf("quantile_position: %ld bad\n", bad);
    return bad;
}

int main() {
    std::mt19937_64 rng(4321);
    long bad = 0;
    bad += exhaustive<1>() + exhaustive<2>() + exhaustive<4>() + exhaustive<8>() + exhaustive<16>();
    bad += merges<32>() + merges<64>();
    bad += merges<2>() + merges<4>() + merges<8>() + merges<16>();
    bad += counted<2>(1) + counted<4>(5) + counted<8>(19) + counted<16>(63) + counted<32>(191) + counted<64>(543);
    bad += random_keys<8>(20000, rng) + random_keys<16>(20000, rng) + random_keys<32>(20000, rng) + random_keys<64>(20000, rng);
    bad += positions();
    std::printf("TOTAL BAD %ld\n", bad);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def sortnet_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("torder_sortnet")
    src, exe = d / "sortnet.cpp", d / "sortnet"
    src.write_text(SORTNET_PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the networks
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_sorting_networks_as_host_code(sortnet_program):
    """Zero-one principle: every 0-1 input for N <= 16; for N = 32 and 64 the final merge on every pair of sorted 0-1 halves
    (the halves are sorted by the proved network of half the size); exchange counts 1, 5, 19, 63, 191, 543; random float keys
    with NaN, +-Inf, +-0 and pad keys against std::sort; quantile_position by hand."""
    r = subprocess.run([sortnet_program], capture_output=True, text=True)
    assert r.returncode == 0 and "TOTAL BAD 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sortnet 64: 543 exchanges" in r.stdout and "merge 64: 1089 pairs" in r.stdout and "merge 32: 289 pairs" in r.stdout


# ------------------------------------------------------------------------------------------------ plumbing
def test_exports_and_argument_errors_come_before_the_device():
    from barc4dip_amd import metrics, preprocessing
    from barc4dip_amd.metrics import order

    for name in ("temporal_median", "temporal_percentile", "temporal_robust_mean", "order"):
        assert name in metrics.__all__ and getattr(metrics, name) is not None
    for name in ("combine_frames", "remove_zingers"):
        assert name in preprocessing.__all__ and callable(getattr(preprocessing, name))
    s = np.ones((4, 3, 5), np.float32)
    for bad in (lambda: metrics.temporal_percentile(s, 101.0), lambda: metrics.temporal_percentile(s, -1.0),
                lambda: metrics.temporal_percentile(s, float("nan")), lambda: metrics.temporal_percentile(s, [10.0, 200.0]),
                lambda: metrics.temporal_percentile(s, []), lambda: metrics.temporal_percentile(s, 50.0, method="hazen"),
                lambda: metrics.temporal_percentile(s[0], 50.0), lambda: metrics.temporal_median(s[0]),
                lambda: metrics.temporal_median(np.ones((0, 3, 5), np.float32)), lambda: metrics.temporal_median(s, max_bytes=0),
                lambda: metrics.temporal_robust_mean(s, scale="sigma"), lambda: metrics.temporal_robust_mean(s, polarity="cold"),
                lambda: metrics.temporal_robust_mean(s, threshold=-1.0), lambda: metrics.temporal_robust_mean(s, min_scale=float("nan")),
                lambda: metrics.temporal_robust_mean(s[0]), lambda: preprocessing.combine_frames(s, method="mode"),
                lambda: preprocessing.combine_frames(s, method="robust", return_mask=True),
                lambda: preprocessing.remove_zingers(s, scale="sigma"), lambda: preprocessing.remove_zingers(s, threshold=-2.0),
                lambda: preprocessing.remove_zingers(s[0])):
        with pytest.raises(ValueError):
            bad()
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(order.MAX_T + 1, 2, 2), strides=(0, 0, 0))
    for fn in (metrics.temporal_median, metrics.temporal_robust_mean, preprocessing.remove_zingers,
               lambda a: metrics.temporal_percentile(a, 10.0), lambda a: preprocessing.combine_frames(a, "median")):
        with pytest.raises(NotImplementedError, match="1024"):
            fn(big)


def test_row_bands():
    from barc4dip_amd.metrics.order import row_bands

    assert row_bands((12, 10, 16), 1 << 30) == [(0, 10)]
    assert row_bands((12, 10, 16), 4 * 12 * 10 * 16) == [(0, 10)]
    assert row_bands((12, 10, 16), 4 * 12 * 10 * 16 - 1) == [(0, 9), (9, 10)]
    assert row_bands((12, 10, 16), 3 * 4 * 12 * 16) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert row_bands((12, 10, 16), 3 * 4 * 12 * 16 + 100) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert row_bands((12, 3, 16), 1) == [(0, 1), (1, 2), (2, 3)]          # a band has at least one row
    for shape, mb in (((7, 33, 5), 1000), ((64, 100, 3), 5000)):
        b = row_bands(shape, mb)
        assert b[0][0] == 0 and b[-1][1] == shape[1] and all(x[1] == y[0] for x, y in zip(b, b[1:]))
        assert all(4 * shape[0] * shape[2] * (r1 - r0) <= max(mb, 4 * shape[0] * shape[2]) for r0, r1 in b)
    with pytest.raises(ValueError):
        row_bands((2, 2, 2), 0)
