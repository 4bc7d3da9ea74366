// b4d_sortnet.hpp -- compile-time sorting networks of the temporal order statistics (b4d_torder.hip): Batcher's odd-even merge
// sort of N = 2^k values held in registers.  Like b4d_keys.hpp, everything here is __host__ __device__, free of HIP types and
// written against an operations policy O (O::T, O::lo, O::hi), so a plain C++ program can include it and prove the networks by
// the zero-one principle (tests/test_temporal_order_host.py).
//
// The network is built the way it is proved: sort_range sorts the two halves of a range with the network of half the size and
// joins them with odd_even_merge.  A merge that is right on every pair of sorted 0-1 halves, together with a half-size network
// that is right, makes the whole network right.  Exchanges: 1, 5, 19, 63, 191, 543 for N = 2, 4, .. 64 (exchanges()).
#pragma once
#include "b4d_keys.hpp"

namespace b4d {
namespace sortnet {

using keys::cex;

// One level of the odd-even merge of v[OFF .. OFF + M), whose halves are sorted: the exchanges at distance K, then the levels
// K / 2 .. 1.  Level K = M / 2 compares the halves element by element; a level below it exchanges v[j + i] with v[j + i + K] for
// j = K, 3K, 5K, .. and i < K.  All indices are compile-time after unrolling: v lives in registers.
template <class O, int N, int OFF, int M, int K>
B4D_HD void merge_level(typename O::T (&v)[N]) {
    constexpr int P = M / 2;
    B4D_HD_UNROLL
    for (int j = K % P; j <= M - 1 - K; j += 2 * K) {
        B4D_HD_UNROLL
        for (int i = 0; i < K; ++i)
            if (i + j + K <= M - 1) cex<O>(v[OFF + i + j], v[OFF + i + j + K]);
    }
    if constexpr (K > 1) merge_level<O, N, OFF, M, K / 2>(v);
}
// v[OFF .. OFF + M / 2) and v[OFF + M / 2 .. OFF + M) sorted -> v[OFF .. OFF + M) sorted
template <class O, int N, int OFF, int M>
B4D_HD void odd_even_merge(typename O::T (&v)[N]) {
    static_assert(M >= 2 && (M & (M - 1)) == 0 && OFF >= 0 && OFF + M <= N, "a power-of-two range inside v");
    merge_level<O, N, OFF, M, M / 2>(v);
}
template <class O, int N, int OFF, int M>
B4D_HD void sort_range(typename O::T (&v)[N]) {
    if constexpr (M >= 2) {
        sort_range<O, N, OFF, M / 2>(v);
        sort_range<O, N, OFF + M / 2, M / 2>(v);
        odd_even_merge<O, N, OFF, M>(v);
    }
}
// v[0] <= v[1] <= .. <= v[N - 1] afterwards; N a power of two
template <class O, int N>
B4D_HD void sortnet(typename O::T (&v)[N]) {
    static_assert(N >= 1 && (N & (N - 1)) == 0, "N must be a power of two");
    sort_range<O, N, 0, N>(v);
}

constexpr int merge_exchanges(int M) {   // of odd_even_merge over M values
    int c = 0;
    for (int k = M / 2; k >= 1; k /= 2)
        for (int j = k % (M / 2); j <= M - 1 - k; j += 2 * k)
            for (int i = 0; i < k; ++i) c += (i + j + k <= M - 1) ? 1 : 0;
    return c;
}
constexpr int exchanges(int N) { return N < 2 ? 0 : 2 * exchanges(N / 2) + merge_exchanges(N); }

// Quantile position (NumPy's methods "linear", "lower", "higher", "nearest", "midpoint"): with h = q (n - 1) in float64 the
// result lies between the sorted samples s[i] and s[i + 1] at the fraction g; g == 0 means s[i] itself.  n < 1: i = 0, g = 0.
enum { METHOD_LINEAR = 0, METHOD_LOWER = 1, METHOD_HIGHER = 2, METHOD_NEAREST = 3, METHOD_MIDPOINT = 4 };
B4D_HD void quantile_position(double q, int n, int method, int& i, double& g) {
    i = 0;
    g = 0.0;
    if (n < 1) return;
    const double h = q * (double)(n - 1);
    const double fl = __builtin_floor(h);
    if (method == METHOD_HIGHER) i = (int)__builtin_ceil(h);
    else if (method == METHOD_NEAREST) i = (int)__builtin_rint(h);   // half to even
    else i = (int)fl;
    if (method == METHOD_LINEAR) g = h - fl;
    if (method == METHOD_MIDPOINT) g = h > fl ? 0.5 : 0.0;
}

}  // namespace sortnet
}  // namespace b4d
