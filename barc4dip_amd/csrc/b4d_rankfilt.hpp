// b4d_rankfilt.hpp -- what is spatial in the rank filters (b4d_rankfilt.hip): the selection networks of the 3 x 3 .. 7 x 7
// windows.  The border rule comes from b4d_tile.hpp; the keys, the operations policy O and cex come from b4d_keys.hpp.  Everything here is __host__ __device__
// and free of HIP types, so a plain C++ program can include it and test the networks (tests/test_rank_filter_host.py).
#pragma once
#include "b4d_keys.hpp"
#include "b4d_tile.hpp"

namespace b4d {
namespace rankfilt {   // (sees namespace keys: b4d_keys.hpp)

template <class O>
B4D_HD typename O::T med3(typename O::T a, typename O::T b, typename O::T c) {
    return O::hi(O::lo(a, b), O::lo(O::hi(a, b), c));
}
// a <= b <= c afterwards (3 exchanges)
template <class O>
B4D_HD void sort3(typename O::T& a, typename O::T& b, typename O::T& c) {
    cex<O>(a, b);
    cex<O>(b, c);
    cex<O>(a, b);
}
// Median of a 3 x 3 window from its three SORTED columns (lo_i <= mid_i <= hi_i): the two smaller column minima have at least
// five elements above them, the two larger column maxima five below, and of the column medians only the middle one can be the
// median of nine -- so it is med3(max lo, med3 mid, min hi).  A column sort is shared by the three windows the column belongs to.
template <class O>
B4D_HD typename O::T median9_sorted_cols(typename O::T l0, typename O::T m0, typename O::T h0, typename O::T l1, typename O::T m1,
                                            typename O::T h1, typename O::T l2, typename O::T m2, typename O::T h2) {
    const typename O::T a = O::hi(O::hi(l0, l1), l2);
    const typename O::T b = med3<O>(m0, m1, m2);
    const typename O::T c = O::lo(O::lo(h0, h1), h2);
    return med3<O>(a, b, c);
}

// Median of N (odd) values by forgetful selection: of any M = (N + 1) / 2 + 1 values neither the smallest nor the largest can
// be the median of all N, so both are dropped and one more value joins; after (N - 3) / 2 rounds three values are left and
// their middle one is the median.  A round on m values: exchange v[i] with v[m-1-i] (small ones to the front), then carry the
// minimum of the front half to v[0] and the maximum of the back half to v[m-1]; the next value takes v[0]'s place and
// v[m-1] falls off the end.  v is destroyed.  All indices are compile-time after unrolling: v lives in registers.
template <class O, int N>
B4D_HD typename O::T median_forgetful(typename O::T (&v)[N]) {
    static_assert(N % 2 == 1 && N >= 3, "odd N");
    constexpr int M0 = (N + 1) / 2 + 1;
    int nxt = M0 < N ? M0 : N;
    B4D_HD_UNROLL
    for (int m = (M0 < N ? M0 : N); m >= 3; --m) {
        B4D_HD_UNROLL
        for (int i = 0; i < m / 2; ++i) cex<O>(v[i], v[m - 1 - i]);
        B4D_HD_UNROLL
        for (int i = 1; i < (m + 1) / 2; ++i) cex<O>(v[0], v[i]);
        B4D_HD_UNROLL
        for (int i = m / 2; i < m - 1; ++i) cex<O>(v[i], v[m - 1]);
        if (m > 3) v[0] = v[nxt++];
    }
    return v[1];
}

// optimal sorting networks of 5 (9 exchanges) and 7 (16 exchanges) values
template <class O>
B4D_HD void sort5(typename O::T (&a)[5]) {
    cex<O>(a[0], a[1]); cex<O>(a[3], a[4]); cex<O>(a[2], a[4]); cex<O>(a[2], a[3]); cex<O>(a[1], a[4]);
    cex<O>(a[0], a[3]); cex<O>(a[0], a[2]); cex<O>(a[1], a[3]); cex<O>(a[1], a[2]);
}
template <class O>
B4D_HD void sort7(typename O::T (&a)[7]) {
    cex<O>(a[0], a[6]); cex<O>(a[2], a[3]); cex<O>(a[4], a[5]); cex<O>(a[0], a[2]); cex<O>(a[1], a[4]); cex<O>(a[3], a[6]);
    cex<O>(a[0], a[1]); cex<O>(a[2], a[5]); cex<O>(a[3], a[4]); cex<O>(a[1], a[2]); cex<O>(a[4], a[6]); cex<O>(a[2], a[3]);
    cex<O>(a[4], a[5]); cex<O>(a[1], a[2]); cex<O>(a[3], a[4]); cex<O>(a[5], a[6]);
}
template <class O, int S>
B4D_HD void sort_small(typename O::T (&a)[S]) {
    static_assert(S == 3 || S == 5 || S == 7, "3, 5 or 7 values");
    if constexpr (S == 3) sort3<O>(a[0], a[1], a[2]);
    if constexpr (S == 5) sort5<O>(a);
    if constexpr (S == 7) sort7<O>(a);
}

// Median of an S x S window from its S SORTED columns (col[j][i] <= col[j][i + 1]); the column sorts are shared by the S windows
// a column belongs to.  Row i holds the i-th smallest value of every column.  The k-th smallest value e of row i is <= the
// entries i .. S-1 of the S-k+1 columns whose row-i entry is >= e: where (S-k+1)(S-i) >= (N+3)/2, more than half of the N = S*S
// values lie at or above e and e is dropped as too small; by symmetry the largest values of row S-1-i are dropped as too large.
// As many go on either side, so the median of the rest (3 of 9: the classic med3 form; 13 of 25; 29 of 49) is the median of the
// window.  Each row is sorted by a network of its own (the exchanges behind values that are dropped fall away as dead code) and
// the rest goes through forgetful selection.
constexpr int rows_dropped_low(int S, int i) {
    int k = 0;
    while (k < S && (S - k) * (S - i) >= (S * S + 3) / 2) ++k;   // the (k + 1)-th smallest has S - k columns at or above it
    return k;
}
constexpr int rows_kept(int S) {
    int n = 0;
    for (int i = 0; i < S; ++i) n += S - rows_dropped_low(S, i) - rows_dropped_low(S, S - 1 - i);
    return n;
}
template <class O, int S>
B4D_HD typename O::T median_sorted_cols(const typename O::T (&col)[S][S]) {
    constexpr int K = rows_kept(S);
    typename O::T keep[K];
    int n = 0;
    B4D_HD_UNROLL
    for (int i = 0; i < S; ++i) {
        typename O::T row[S];
        B4D_HD_UNROLL
        for (int j = 0; j < S; ++j) row[j] = col[j][i];
        sort_small<O, S>(row);
        B4D_HD_UNROLL
        for (int k = rows_dropped_low(S, i); k < S - rows_dropped_low(S, S - 1 - i); ++k) keep[n++] = row[k];
    }
    return median_forgetful<O, K>(keep);
}

using b4d::border_index;   // the border rule (b4d_tile.hpp), under the name it had here

}  // namespace rankfilt
}  // namespace b4d
