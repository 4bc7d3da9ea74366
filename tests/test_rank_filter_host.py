"""Host tier of the spatial rank filters (barc4dip_amd.preprocessing.rank, barc4dip_amd.utils): the NumPy models that the GPU
tier (tests/test_gpu_rank_filter.py) compares the kernels with, each checked here against what the project already trusts --
scipy.ndimage for the filters, the reference for the utils functions -- and the selection networks of
csrc/b4d_rankfilt.hpp, run as host code by a small C++ program.

A rank filter is a selection, so every comparison in both tiers is exact equality.  On NaN the model is the definition
(np.sort's order: NaN above +Inf); SciPy leaves it unspecified."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi
from numpy.lib.stride_tricks import sliding_window_view

from temporal_order_model import outlier_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["reflect", "constant", "nearest", "mirror", "wrap"]
_PAD = {"reflect": "symmetric", "mirror": "reflect", "nearest": "edge", "wrap": "wrap", "constant": "constant"}


# ------------------------------------------------------------------------------------------------ models
def window_pair(size):
    return (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))


def sorted_windows(frame, size, mode="reflect", cval=0.0):
    """(H, W, sy * sx) sorted windows of a 2-D float32 frame, placed as SciPy places them (offsets -(s // 2) .. s - 1 - s // 2)."""
    sy, sx = window_pair(size)
    f = np.asarray(frame, dtype=np.float32)
    pads = ((sy // 2, sy - 1 - sy // 2), (sx // 2, sx - 1 - sx // 2))
    kw = {"constant_values": np.float32(cval)} if mode == "constant" else {}
    p = np.pad(f, pads, mode=_PAD[mode], **kw)
    w = sliding_window_view(p, (sy, sx)).reshape(f.shape[0], f.shape[1], sy * sx)
    return np.sort(w, axis=-1)


def percentile_rank(n, percentile):
    p = float(percentile)
    if p < 0.0:
        p += 100.0
    return n - 1 if p == 100.0 else int(float(n) * p / 100.0)


def model_rank_filter(images, rank, size, mode="reflect", cval=0.0):
    """rank_filter of a frame or, frame by frame, a stack: float32."""
    a = np.asarray(images).astype(np.float32)
    if a.ndim == 3:
        return np.stack([model_rank_filter(f, rank, size, mode, cval) for f in a])
    sy, sx = window_pair(size)
    r = rank + sy * sx if rank < 0 else rank
    return np.ascontiguousarray(sorted_windows(a, size, mode, cval)[..., r])


def model_median_filter(images, size, mode="reflect", cval=0.0):
    sy, sx = window_pair(size)
    return model_rank_filter(images, (sy * sx) // 2, size, mode, cval)


def model_remove_outliers(images, size=3, threshold=6.0, scale="mad", polarity="both", min_scale=0.0, mode="reflect", cval=0.0):
    """(frames, mask, count) of remove_outliers in its float32 operation order; every operation is rounded on its own."""
    a = np.asarray(images).astype(np.float32)
    if a.ndim == 3:
        parts = [model_remove_outliers(f, size, threshold, scale, polarity, min_scale, mode, cval) for f in a]
        return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    with np.errstate(all="ignore"):
        win = sorted_windows(a, size, mode, cval)
        med = win[..., win.shape[-1] // 2]
        mad = lambda: np.sort(np.abs(win - med[..., None]), axis=-1)[..., win.shape[-1] // 2]
        _, out = outlier_rule(a, med, mad, threshold, scale, polarity, min_scale)
    return np.where(out, med, a).astype(np.float32), out, np.array([np.count_nonzero(out)], dtype=np.int64)


def model_filtered_minmax_range(image, size=3):
    with np.errstate(all="ignore"):
        ref = model_median_filter(image, size)
        vmin, vmax = float(np.nanmin(ref)), float(np.nanmax(ref))
    if not np.isfinite(vmin) or not np.isfinite(vmax) or vmax <= vmin:
        raise ValueError(f"Invalid range after filtering: vmin={vmin}, vmax={vmax}")
    return vmin, vmax


def model_percentile_minmax_range(image, p_low=0.05, p_high=99.95):
    arr = np.asarray(image)
    return float(np.nanpercentile(arr, p_low)), float(np.nanpercentile(arr, p_high))


def model_round_uint16_bounds(vmin, vmax, k=1000):
    return max(0, int(np.floor(vmin / k) * k)), min(65535, int(np.ceil(vmax / k) * k))


def model_scale_to_u16(x32, vmin, inv, mul_f64):
    """b4d_scale_to_u16 element by element: float32 subtraction, one rounded product, clip, truncate; NaN -> 0."""
    x = np.asarray(x32, dtype=np.float32) - np.float32(vmin)
    with np.errstate(all="ignore"):
        y = (x.astype(np.float64) * np.float64(inv)).astype(np.float32) if mul_f64 else x * np.float32(inv)
        y = np.where(np.isnan(y), np.float32(0), np.clip(y, np.float32(0), np.float32(65535)))
    return y.astype(np.uint16)


def model_to_uint16(data, median_size=3, counts_threshold=10.0, scaling=1 / np.sqrt(2)):
    if data.dtype == np.uint16:
        return data
    x32 = data.astype(np.float32)
    if float(np.nanmean(data)) > counts_threshold:
        return model_scale_to_u16(x32, 0.0, 1.0, False)
    vmin, vmax = model_filtered_minmax_range(data, median_size)
    vmin *= 0.95
    vmax /= 0.95
    inv = 65535 * scaling / (vmax - vmin)
    return model_scale_to_u16(x32, vmin, float(inv), isinstance(inv, np.generic))


# ------------------------------------------------------------------------------------------------ inputs shared with the GPU tier
def counts_frame(shape=(37, 53), seed=1):
    """poisson(5) counts (ties everywhere) with one +Inf."""
    f = np.random.default_rng(seed).poisson(5, shape).astype(np.float32)
    f[shape[0] // 3, shape[1] // 2] = np.inf
    return f


def special_frame(shape=(41, 67), seed=2):
    """normal values with 1 % NaN, some +-Inf and -0.0 / +0.0 entries."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=shape).astype(np.float32)
    flat = f.reshape(-1)
    idx = rng.choice(flat.size, flat.size // 100 + 12, replace=False)
    flat[idx[:-12]] = np.nan
    flat[idx[-12:-9]] = np.inf
    flat[idx[-9:-6]] = -np.inf
    flat[idx[-6:-3]] = -0.0
    flat[idx[-3:]] = 0.0
    return f


def outlier_frame():
    """poisson(1000) on 64 x 96 with 20 pixels at 1e4 and 20 at 0; returns (frame, flat indices of the 40)."""
    rng = np.random.default_rng(7)
    f = rng.poisson(1000, (64, 96)).astype(np.float32)
    idx = rng.choice(64 * 96, 40, replace=False)
    f.reshape(-1)[idx[:20]] = 1e4
    f.reshape(-1)[idx[20:]] = 0.0
    return f, idx


# ------------------------------------------------------------------------------------------------ the models against SciPy
@pytest.mark.parametrize("mode", MODES)
def test_model_equals_scipy_median(mode):
    f = counts_frame()
    small = np.random.default_rng(3).normal(size=(4, 5)).astype(np.float32)
    for size in (3, 4, 5, 7, 9, 11, (3, 5)):
        for frame in (f, small):
            got = model_median_filter(frame, size, mode, 7.0)
            ref = ndi.median_filter(frame, size=size, mode=mode, cval=7.0)
            assert got.dtype == np.float32 and np.array_equal(got, ref), (mode, size, frame.shape)


@pytest.mark.parametrize("mode", MODES)
def test_model_equals_scipy_rank_and_percentile(mode):
    f = counts_frame((23, 31), 4)
    for size in (3, 5, (4, 4), 9):
        n = int(np.prod(window_pair(size)))
        for rank in (0, 3, -1, min(24, n - 1)):
            assert np.array_equal(model_rank_filter(f, rank, size, mode, 7.0), ndi.rank_filter(f, rank, size=size, mode=mode, cval=7.0))
        for p in (0, 10, 50, 99.9, 100, -20):
            assert np.array_equal(model_rank_filter(f, percentile_rank(n, p), size, mode, 7.0),
                                  ndi.percentile_filter(f, p, size=size, mode=mode, cval=7.0)), (mode, size, p)


def test_model_stack_is_frame_by_frame():
    s = np.random.default_rng(5).poisson(5, (3, 12, 17)).astype(np.float32)
    assert np.array_equal(model_median_filter(s, 5), ndi.median_filter(s, size=(1, 5, 5)))


def test_model_nan_order_and_signed_zero():
    """NaN above +Inf: a window with k NaN entries loses its k largest ranks to them; -0.0 and +0.0 compare equal."""
    f = np.arange(25, dtype=np.float32).reshape(5, 5)
    f[2, 2] = np.nan
    out = model_rank_filter(f, -1, 3)
    assert np.isnan(out[1:4, 1:4]).all() and not np.isnan(model_rank_filter(f, -2, 3)).any()
    assert model_median_filter(f, 3)[2, 2] == 13.0          # of 6 7 8 11 NaN 13 16 17 18 the fifth smallest
    z = np.array([[-0.0, 0.0, -0.0]], dtype=np.float32)
    assert np.array_equal(model_median_filter(z, 3), np.zeros((1, 3), np.float32))


# ------------------------------------------------------------------------------------------------ outlier repair
def test_outlier_model_finds_the_planted_pixels():
    """The condition the GPU tier's frame must meet under the model alone: all 40 planted pixels flagged and at most 6 others
    (0.1 %), for 5 x 5 / mad / 6 and for 3 x 3 / poisson / 5 / min_scale 1."""
    f, idx = outlier_frame()
    for kw in (dict(size=5, scale="mad", threshold=6.0), dict(size=3, scale="poisson", threshold=5.0, min_scale=1.0)):
        out, mask, count = model_remove_outliers(f, **kw)
        assert mask.reshape(-1)[idx].all(), kw
        assert 40 <= int(count[0]) <= 46 and int(count[0]) == np.count_nonzero(mask), (kw, count)
        assert np.array_equal(out[~mask], f[~mask]) and np.array_equal(out[mask], model_median_filter(f, kw["size"])[mask])
        assert out.dtype == np.float32 and abs(float(out.max()) - 1000) < 200 and float(out.min()) > 800


def test_outlier_model_polarity_and_nonfinite():
    f, idx = outlier_frame()
    hot = model_remove_outliers(f, 5, scale="mad", polarity="hot")[1].reshape(-1)
    dead = model_remove_outliers(f, 5, scale="mad", polarity="dead")[1].reshape(-1)
    assert hot[idx[:20]].all() and not hot[idx[20:]].any() and dead[idx[20:]].all() and not dead[idx[:20]].any()
    g = f.copy()
    g[10, 10] = np.nan
    for polarity in ("both", "hot", "dead"):
        out, mask, _ = model_remove_outliers(g, 3, scale="absolute", threshold=1e9, polarity=polarity)
        assert mask[10, 10] and np.count_nonzero(mask) == 1 and np.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ utils
def _utils_inputs():
    rng = np.random.default_rng(11)
    low = rng.gamma(2.0, 1.5, (3, 20, 28)).astype(np.float32)            # mean 3: the scaling branch
    low[1, 4, 5] = 400.0                                                  # a zinger that the median filter removes from the range
    counts = rng.poisson(300, (2, 16, 24)).astype(np.float32) * 220.0     # about half above 65535: clipped
    counts[0, 0, 0] = -3.5
    return low, counts


def test_utils_models_basics():
    low, counts = _utils_inputs()
    vmin, vmax = model_filtered_minmax_range(low)
    assert vmin > 0 and vmax < 100 and (vmin, vmax) == (float(np.min(ndi.median_filter(low, size=(1, 3, 3)))),
                                                       float(np.max(ndi.median_filter(low, size=(1, 3, 3)))))
    with pytest.raises(ValueError):
        model_filtered_minmax_range(np.full((6, 6), 2.0, np.float32))
    assert model_round_uint16_bounds(1234.5, 50001.0) == (1000, 51000) and model_round_uint16_bounds(-5.0, 7e4) == (0, 65535)
    u = model_to_uint16(counts)
    assert u.dtype == np.uint16 and u[0, 0, 0] == 0 and u.max() == 65535 and u[1, 3, 3] == int(min(counts[1, 3, 3], 65535))
    s = model_to_uint16(low)
    assert s.dtype == np.uint16 and s[1, 4, 5] == 65535 and 0 < int(np.median(s)) < 65535


@pytest.mark.needs_reference
def test_utils_models_equal_the_reference():
    from oracle import load_reference

    load_reference.load()
    ref_range = importlib.import_module("barc4dip.utils.range")
    ref_dtype = importlib.import_module("barc4dip.utils.dtype")
    low, counts = _utils_inputs()
    for img in (low, low[0], counts):
        for size in (3, 5):
            assert model_filtered_minmax_range(img, size) == ref_range.filtered_minmax_range(img, size)
            assert model_filtered_minmax_range(img, size) == ref_range.filtered_minmax_range_streaming(img, size)
        assert model_percentile_minmax_range(img) == ref_range.percentile_minmax_range(img)
        assert model_percentile_minmax_range(img, 1.0, 90.0) == ref_range.percentile_minmax_range(img, 1.0, 90.0)
    for args in ((1234.5, 50001.0), (-5.0, 7e4), (999.0, 1000.0, 250)):
        assert model_round_uint16_bounds(*args) == ref_dtype.round_uint16_bounds(*args)
    for scaling in (1 / np.sqrt(2), 0.5, np.float32(0.5)):              # NumPy float64 scalar, Python float, NumPy float32 scalar
        for img in (low, low[0]):
            assert np.array_equal(model_to_uint16(img, scaling=scaling), ref_dtype.to_uint16(img, scaling=scaling)), repr(scaling)
    for img in (counts, counts.astype(np.int32), low.astype(np.float32) * 0 + np.arange(28, dtype=np.float32) * 3000):
        assert np.array_equal(model_to_uint16(img), ref_dtype.to_uint16(img))
    u16 = counts.astype(np.uint16)
    assert model_to_uint16(u16) is u16 and ref_dtype.to_uint16(u16) is u16
    with pytest.raises(ValueError):
        ref_range.filtered_minmax_range(np.full((6, 6), 2.0, np.float32))


# ------------------------------------------------------------------------------------------------ the networks as host code
NETWORK_PROGRAM = r"""
// Runs the selection networks of b4d_rankfilt.hpp as host code.  Zero-one principle: a network of min / max exchanges that is
// right on every 0-1 input is right on every input; 64 patterns are evaluated at a time (lo = AND, hi = OR on 64-bit words).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "b4d_rankfilt.hpp"
using namespace b4d::rankfilt;

struct BitOps {
    typedef uint64_t T;
    static T lo(T a, T b) { return a & b; }
    static T hi(T a, T b) { return a | b; }
};
template <class O>
typename O::T median9_cols(typename O::T (&v)[9]) {   // the 3 x 3 route of the kernels: v[3 * row + column]
    for (int c = 0; c < 3; ++c) sort3<O>(v[c], v[3 + c], v[6 + c]);
    return median9_sorted_cols<O>(v[0], v[3], v[6], v[1], v[4], v[7], v[2], v[5], v[8]);
}
template <int N>
struct Forgetful {
    template <class O>
    static typename O::T run(typename O::T (&v)[N]) { return median_forgetful<O, N>(v); }
};
struct Cols9 {
    template <class O>
    static typename O::T run(typename O::T (&v)[9]) { return median9_cols<O>(v); }
};
template <int S>
struct SortedCols {   // the 5 x 5 and 7 x 7 route of the kernels: v[S * row + column], columns sorted first
    template <class O>
    static typename O::T run(typename O::T (&v)[S * S]) {
        typename O::T cols[S][S];
        for (int j = 0; j < S; ++j) {
            typename O::T c[S];
            for (int i = 0; i < S; ++i) c[i] = v[S * i + j];
            sort_small<O, S>(c);
            for (int i = 0; i < S; ++i) cols[j][i] = c[i];
        }
        return median_sorted_cols<O, S>(cols);
    }
};
static const uint64_t LANE_BITS[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                      0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
// every one of the 2^N patterns: pattern p = 64 * base + lane, input i holds bit i of p
template <int N, class Net>
static long exhaustive(const char* name) {
    long bad = 0;
    const uint64_t words = N > 6 ? (1ull << (N - 6)) : 1;
    for (uint64_t base = 0; base < words; ++base) {
        uint64_t v[N], want = 0;
        for (int i = 0; i < N; ++i) v[i] = i < 6 ? LANE_BITS[i] : (((base >> (i - 6)) & 1) ? ~0ull : 0ull);
        for (int lane = 0; lane < 64; ++lane)
            if (__builtin_popcountll((base << 6) | (uint64_t)lane) > N / 2) want |= 1ull << lane;
        const uint64_t got = Net::template run<BitOps>(v);
        const uint64_t valid = N >= 6 ? ~0ull : ((1ull << (1 << N)) - 1);
        if ((got ^ want) & valid) ++bad;
    }
    std::printf("%s exhaustive 2^%d patterns: %ld bad words\n", name, N, bad);
    return bad;
}
template <int N, class Net>
static long random_patterns(const char* name, long patterns, std::mt19937_64& rng) {
    long bad = 0;
    for (long k = 0; k < patterns / 64; ++k) {
        uint64_t v[N], in[N], want = 0;
        for (int i = 0; i < N; ++i) {                      // three densities of ones: 1/2, 1/4, 3/4
            const uint64_t a = rng(), b = rng();
            v[i] = in[i] = k % 3 == 0 ? a : (k % 3 == 1 ? (a & b) : (a | b));
        }
        for (int lane = 0; lane < 64; ++lane) {
            int ones = 0;
            for (int i = 0; i < N; ++i) ones += (in[i] >> lane) & 1;
            if (ones > N / 2) want |= 1ull << lane;
        }
        if (Net::template run<BitOps>(v) != want) ++bad;
    }
    std::printf("%s random 0-1 patterns %ld: %ld bad words\n", name, patterns, bad);
    return bad;
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
template <int N, class Net>
static long random_floats(const char* name, long trials, std::mt19937_64& rng) {
    long bad = 0;
    for (long k = 0; k < trials; ++k) {
        uint32_t v[N];
        std::vector<uint32_t> s(N);
        for (int i = 0; i < N; ++i) v[i] = s[i] = to_key(random_value(rng));
        std::nth_element(s.begin(), s.begin() + N / 2, s.end());
        if (Net::template run<KeyOps>(v) != s[N / 2]) ++bad;
    }
    std::printf("%s random float windows %ld: %ld bad\n", name, trials, bad);
    return bad;
}
static long keys_and_bitwise(std::mt19937_64& rng) {
    long bad = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float order[] = {-inf, -3.5f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1.0f, 3.4e38f, inf, nan};
    for (int i = 0; i + 1 < 10; ++i)
        if (!(to_key(order[i]) < to_key(order[i + 1]))) ++bad;
    if (to_key(-nan) != KEY_NAN || to_key(nan) != KEY_NAN) ++bad;
    for (int i = 0; i < 9; ++i)
        if (float_bits(from_key(to_key(order[i]))) != float_bits(order[i])) ++bad;
    for (int k = 0; k < 20000; ++k) {                       // select_bitwise against nth_element, any n <= 225 and rank
        const int n = 1 + (int)(rng() % 225), rank = (int)(rng() % n);
        std::vector<uint32_t> w(n);
        for (int i = 0; i < n; ++i) w[i] = to_key(random_value(rng));
        const uint32_t got = select_bitwise(rank, [&](uint32_t t) {
            int c = 0;
            for (int i = 0; i < n; ++i) c += w[i] < t ? 1 : 0;
            return c;
        });
        std::nth_element(w.begin(), w.begin() + rank, w.end());
        if (got != w[rank]) ++bad;
    }
    std::printf("keys and bitwise selection: %ld bad\n", bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "border")) {      // index table for the Python side: n, mode, i, source index
        for (int n = 1; n <= 6; ++n)
            for (int mode = 0; mode <= 4; ++mode)
                for (int i = -20; i < n + 20; ++i) std::printf("%d %d %d %d\n", n, mode, i, border_index(i, n, mode));
        return 0;
    }
    if (argc > 2 && !std::strcmp(argv[1], "keys")) {        // key table for the Python side: bits, to_key, key_bits, bits of from_key(to_key)
        std::FILE* f = std::fopen(argv[2], "r");
        if (!f) return 2;
        unsigned u;
        while (std::fscanf(f, "%x", &u) == 1) {
            const float x = bits_float(u);
            std::printf("%08x %08x %08x %08x\n", u, to_key(x), key_bits(x), float_bits(from_key(to_key(x))));
        }
        std::fclose(f);
        return 0;
    }
    std::mt19937_64 rng(12345);
    long bad = keys_and_bitwise(rng);
    bad += exhaustive<9, Cols9>("median9 (sorted columns)");
    bad += exhaustive<9, Forgetful<9>>("forgetful 9");
    bad += exhaustive<9, SortedCols<3>>("sorted columns 3 x 3");
    bad += exhaustive<25, Forgetful<25>>("forgetful 25");
    bad += exhaustive<25, SortedCols<5>>("sorted columns 5 x 5");
    bad += random_patterns<49, Forgetful<49>>("forgetful 49", 1000000, rng);
    bad += random_patterns<49, SortedCols<7>>("sorted columns 7 x 7", 1000000, rng);
    bad += random_floats<25, SortedCols<5>>("sorted columns 5 x 5", 100000, rng);
    bad += random_floats<49, SortedCols<7>>("sorted columns 7 x 7", 100000, rng);
    if (rows_kept(3) != 3 || rows_kept(5) != 13 || rows_kept(7) != 29) ++bad;
    bad += random_floats<9, Cols9>("median9 (sorted columns)", 100000, rng);
    bad += random_floats<25, Forgetful<25>>("forgetful 25", 100000, rng);
    bad += random_floats<49, Forgetful<49>>("forgetful 49", 100000, rng);
    std::printf("TOTAL BAD %ld\n", bad);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def network_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("rankfilt_networks")
    src, exe = d / "networks.cpp", d / "networks"
    src.write_text(NETWORK_PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the networks
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_selection_networks_as_host_code(network_program):
    """Zero-one principle, exhaustively for 9 and 25 inputs (2^9, 2^25 patterns); for 49 inputs 10^6 random 0-1 patterns and
    10^5 random float windows with ties, NaN and +-0 against std::nth_element on the keys -- for the selection from sorted
    columns that the median kernels run and for the forgetful selection behind it (alone: the MAD of the outlier repair); key
    order and bitwise selection."""
    r = subprocess.run([network_program], capture_output=True, text=True)
    assert r.returncode == 0 and "TOTAL BAD 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_border_index_equals_numpy_pad(network_program):
    """The halo's index rule for any overhang (repeated reflection / wrap) against np.pad of an index ramp."""
    r = subprocess.run([network_program, "border"], capture_output=True, text=True, check=True)
    rows = np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()])
    codes = {0: "nearest", 1: "reflect", 2: "mirror", 3: "constant", 4: "wrap"}
    assert len(rows) == sum((n + 40) * 5 for n in range(1, 7))
    for n in range(1, 7):
        for code, mode in codes.items():
            sel = rows[(rows[:, 0] == n) & (rows[:, 1] == code)]
            kw = {"constant_values": -1} if mode == "constant" else {}
            want = np.pad(np.arange(n), (20, 20), mode=_PAD[mode], **kw)
            assert np.array_equal(sel[:, 2], np.arange(-20, n + 20)) and np.array_equal(sel[:, 3], want), (n, mode)


def test_float_keys_follow_numpy_sort(network_program, tmp_path):
    """The float-to-key map of b4d_keys.hpp on +-0, the extreme denormals and normals, +-1, +-Inf, quiet and signalling NaNs of
    both signs with payloads and 4096 random bit patterns: to_key orders as np.sort does (ties between NaNs only), key_bits is
    to_key away from NaN, from_key returns the bits of every non-NaN, and every NaN has the key KEY_NAN."""
    fixed = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,
             0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC12345, 0x7F800001, 0xFF800001,
             0x7FA54321, 0xFFA54321, 0x7FFFFFFF, 0xFFFFFFFF]
    bits = np.concatenate([np.array(fixed, dtype=np.uint32),
                           np.random.default_rng(21).integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)])
    path = tmp_path / "bits.txt"
    path.write_text("\n".join(f"{int(b):08x}" for b in bits) + "\n")
    r = subprocess.run([network_program, "keys", str(path)], capture_output=True, text=True, check=True)
    rows = np.array([[int(v, 16) for v in line.split()] for line in r.stdout.splitlines()], dtype=np.uint64)
    assert rows.shape == (bits.size, 4) and np.array_equal(rows[:, 0], bits)
    key, raw, back = rows[:, 1], rows[:, 2], rows[:, 3]
    x = bits.view(np.float32)
    nan = np.isnan(x)
    assert nan.sum() >= 10 and (~nan).sum() >= 4000
    assert np.all(key[nan] == 0xFFC00000) and np.all(key[~nan] < 0xFFC00000)
    assert np.array_equal(raw[~nan], key[~nan]) and np.array_equal(back[~nan], bits[~nan])
    by_key = x[np.argsort(key, kind="stable")]
    assert np.array_equal(by_key, np.sort(x), equal_nan=True)
    # ties between NaNs only: different bits have different keys, -0 below +0
    ub, first = np.unique(bits[~nan], return_index=True)
    assert np.unique(key[~nan][first]).size == ub.size and key[1] < key[0]


# ------------------------------------------------------------------------------------------------ interface
def test_exports_and_argument_errors():
    import barc4dip_amd
    from barc4dip_amd import preprocessing, utils
    from barc4dip_amd.preprocessing import rank

    for name in ("median_filter", "rank_filter", "percentile_filter", "remove_outliers"):
        assert name in preprocessing.__all__ and callable(getattr(preprocessing, name))
    for name in ("filtered_minmax_range", "filtered_minmax_range_streaming", "percentile_minmax_range", "round_uint16_bounds", "to_uint16"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    assert barc4dip_amd.utils is utils and utils.range.filtered_minmax_range is utils.filtered_minmax_range
    assert utils.dtype.to_uint16 is utils.to_uint16
    f = np.zeros((8, 8), np.float32)
    for bad in (lambda: rank.median_filter(f, 0), lambda: rank.median_filter(f, 16), lambda: rank.median_filter(f, (3, 5, 7)),
                lambda: rank.median_filter(f, 2.5), lambda: rank.median_filter(f, 3, mode="periodic"),
                lambda: rank.rank_filter(f, 9, 3), lambda: rank.rank_filter(f, -10, 3), lambda: rank.rank_filter(f, 1.5, 3),
                lambda: rank.percentile_filter(f, 101, 3), lambda: rank.percentile_filter(f, -101, 3),
                lambda: rank.remove_outliers(f, 4), lambda: rank.remove_outliers(f, 9), lambda: rank.remove_outliers(f, scale="sigma"),
                lambda: rank.remove_outliers(f, polarity="cold"), lambda: rank.remove_outliers(f, threshold=-1.0),
                lambda: rank.remove_outliers(f, mode="periodic"),
                lambda: utils.filtered_minmax_range(np.zeros(8, np.float32)), lambda: utils.filtered_minmax_range(f, 16),
                lambda: utils.filtered_minmax_range_streaming(np.zeros((2, 2, 2, 2), np.float32)),
                lambda: utils.to_uint16(np.zeros(8, np.float32))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        utils.to_uint16([[1.0, 2.0]])
    u = np.arange(6, dtype=np.uint16).reshape(2, 3)
    assert utils.to_uint16(u) is u
    assert utils.round_uint16_bounds(1234.5, 50001.0) == (1000, 51000) and utils.round_uint16_bounds(-5.0, 7e4) == (0, 65535)
    assert utils.round_uint16_bounds(999.0, 1000.0, 250) == model_round_uint16_bounds(999.0, 1000.0, 250)
