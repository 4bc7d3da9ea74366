// b4d_keys.hpp -- the three decisions every order statistic of the library shares: how a float32 becomes an ordered integer key,
// how a value is selected among keys without sorting, and when a sample is an outlier.  Everything here is __host__ __device__
// and free of HIP types, so a plain C++ program can include it (tests/test_rank_filter_host.py, tests/test_outlier_rule_host.py).
// Users: b4d_select.hpp (radix select of b4d_stats.hip, b4d_track.hip, b4d_displace.hip: key_bits / from_key), b4d_rankfilt.hpp
// and b4d_sortnet.hpp (the networks of b4d_rankfilt.hip and b4d_torder.hip: to_key, KeyOps, cex, select_bitwise), and the
// outlier rule of b4d_despeckle and b4d_temporal_robust_mean.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define B4D_HD __host__ __device__ __forceinline__
#else
#define B4D_HD inline
#endif
#if defined(__clang__)
#define B4D_HD_UNROLL _Pragma("unroll")
#define B4D_HD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define B4D_HD_UNROLL
#define B4D_HD_NO_CONTRACT
#endif

namespace b4d {
namespace keys {

B4D_HD uint32_t float_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
B4D_HD float bits_float(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// np.sort's order as an unsigned integer order: -Inf < ... < -0 < +0 < ... < +Inf < NaN.  Negative values have all bits flipped,
// the others the sign bit set.  key_bits is the raw map, for callers that have already skipped NaNs (a NaN with the sign bit set
// would land below -Inf); to_key first makes every NaN the positive quiet NaN, whose key KEY_NAN lies above +Inf's.
constexpr uint32_t KEY_NAN = 0xFFC00000u;
B4D_HD uint32_t key_bits(float x) {
    const uint32_t u = float_bits(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
B4D_HD uint32_t to_key(float x) {
    uint32_t u = float_bits(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0x7FC00000u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
B4D_HD float from_key(uint32_t k) { return bits_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// A network is written against an operations policy O (O::T, O::lo, O::hi): the kernels run it on 32-bit keys with integer
// min / max, the host tests also on 64 zero-one patterns at a time (lo = AND, hi = OR).
struct KeyOps {
    typedef uint32_t T;
    static B4D_HD T lo(T a, T b) { return a < b ? a : b; }
    static B4D_HD T hi(T a, T b) { return a < b ? b : a; }
};
template <class O>
B4D_HD void cex(typename O::T& a, typename O::T& b) {
    const typename O::T l = O::lo(a, b), h = O::hi(a, b);
    a = l;
    b = h;
}

// rank-th smallest (0-based) of n keys by bitwise selection: the answer is the largest t with #(key < t) <= rank, built from
// the top bit down.  count(t) returns #(key < t) over the window.  32 counting passes, no sorting, any n.
template <class Count>
B4D_HD uint32_t select_bitwise(int rank, Count count) {
    uint32_t t = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t trial = t | (1u << bit);
        if (count(trial) <= rank) t = trial;
    }
    return t;
}

// ------------------------------------------------------------------------------------------------ the outlier rule
// A sample x is an outlier against the median med of its neighbourhood (a window, or the frames of a stack) when
//   absolute: |x - med| > threshold          mad: |x - med| > threshold * max(1.4826 mad, min_scale)
//   poisson : (x - med)^2 > threshold^2 * max(med, min_scale)
// and the sign of x - med fits the polarity; a sample that is not finite always is.  Every float32 operation is rounded on its
// own (no product feeds an add), in this order, so a NumPy model reproduces the decision exactly.
struct OutlierRule {
    int scale_kind;    // 0 absolute, 1 mad, 2 poisson
    float threshold;   // poisson: threshold * threshold (make_outlier_rule)
    float min_scale;
    int polarity;      // 0 both, 1 hot, 2 dead
};
#if defined(__HIP_DEVICE_COMPILE__)
B4D_HD float sub_rn(float a, float b) { return __fsub_rn(a, b); }
B4D_HD float mul_rn(float a, float b) { return __fmul_rn(a, b); }
#else
B4D_HD float sub_rn(float a, float b) {
    B4D_HD_NO_CONTRACT
    return a - b;
}
B4D_HD float mul_rn(float a, float b) {
    B4D_HD_NO_CONTRACT
    return a * b;
}
#endif
B4D_HD OutlierRule make_outlier_rule(int scale_kind, float threshold, float min_scale, int polarity) {
    return OutlierRule{scale_kind, scale_kind == 2 ? mul_rn(threshold, threshold) : threshold, min_scale, polarity};
}
// np.maximum(s, floor): NaN stays NaN
B4D_HD float max_keep_nan(float s, float floor_) { return s < floor_ ? floor_ : s; }
// right-hand side of the test (the `scale` output of the robust mean); mad is read for scale_kind 1 only
B4D_HD float outlier_rhs(const OutlierRule& r, float med, float mad) {
    if (r.scale_kind == 1) return mul_rn(r.threshold, max_keep_nan(mul_rn(1.4826f, mad), r.min_scale));
    if (r.scale_kind == 2) return mul_rn(r.threshold, max_keep_nan(med, r.min_scale));
    return r.threshold;
}
B4D_HD bool outlier_rejected(const OutlierRule& r, float x, float med, float rhs) {
    const float d = sub_rn(x, med);
    bool o = r.scale_kind == 2 ? mul_rn(d, d) > rhs : __builtin_fabsf(d) > rhs;
    if (r.polarity == 1) o = o && d > 0.f;
    if (r.polarity == 2) o = o && d < 0.f;
    return o || (float_bits(x) & 0x7F800000u) == 0x7F800000u;   // last: a sample that is not finite is always an outlier
}

}  // namespace keys

// The keys began in the spatial filters' namespace: b4d::rankfilt sees all of the above, here already, so that code written
// against it (the host programs of the tests among it) compiles with either header.
namespace rankfilt {
using namespace keys;
}
}  // namespace b4d
