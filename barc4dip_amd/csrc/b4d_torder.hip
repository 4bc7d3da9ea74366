// b4d_torder.hip -- per-pixel order statistics along the frame axis of a stack (barc4dip_amd.metrics.order,
// barc4dip_amd.preprocessing.combine): quantiles with NumPy's methods linear / lower / higher / nearest /
// midpoint under the NaN policies "propagate" and "omit", and a robust mean that rejects samples by their distance from the
// per-pixel median (absolute, MAD or Poisson scale; the outlier rule of b4d_keys.hpp, which b4d_despeckle applies over a window).
//
// Semantics.  A stack is (T, npix) float32, frames frame_stride elements apart.  Per pixel the samples are sorted in np.sort's
// order (to_key of b4d_keys.hpp: NaN above +Inf).  With s[0 .. n) the sorted samples that take part, q in [0, 1] and
// h = q (n - 1) in float64, quantile_position (b4d_sortnet.hpp) gives the index i and the fraction g of the method; g == 0 gives
// s[i] itself, otherwise (float) (a + (b - a) g) with a = (double) s[i], b = (double) s[i + 1], the difference, product and sum
// each rounded once in float64.  Selections are exact, so both routes below give the same bits.
//
// Register route, T <= 64: a lane owns PPL adjacent pixels, reads every frame once with streaming loads, pads the T keys to
// TP in {8, 16, 32, 64} with 0xFFFFFFFF (above the NaN key: data, then NaNs, then pad after the sort) and sorts them in
// registers by Batcher's odd-even merge sort.  A sorted value at a run-time index is picked by compare-and-select over the TP
// registers.  The robust mean keeps the unsorted samples in registers as well: the stack is read once.
// General route, 64 < T <= 1024 (or flags bit 0): a workgroup stages the keys of 32 pixels x T samples in dynamic LDS (128 T
// bytes), a wave owns 8 pixels with 8 lanes each, a lane takes the samples t = sub, sub + 8, .. -- one conflict-free read of
// LDS into registers; every order statistic is found by select_bitwise (32 counting steps on those registers), the partial
// counts joined by three butterfly steps inside the wave.  No barrier after the staging.
// No atomics, no address that depends on data, every loop bounded by an argument, plain vector stores only.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "b4d_common.hpp"
#include "b4d_sortnet.hpp"

// a product and a sum that are written apart stay apart: the interpolation is three singly rounded float64 operations
#pragma clang fp contract(off)

namespace b4d {

using namespace keys;
using sortnet::quantile_position;

constexpr int TO_THREADS = 256;
constexpr int TO_MAX_T = 1024, TO_MAX_REG_T = 64, TO_MAX_Q = 8;
constexpr int TO_TILE = 32;           // pixels per workgroup of the general route
constexpr int TO_GROUP = 8;           // lanes per pixel of the general route; also the partial sums of the robust mean
constexpr uint32_t KEY_PAD = 0xFFFFFFFFu;

struct QuantArgs {
    double q[TO_MAX_Q];
    int n_q, method, nan_policy;
};

__device__ __forceinline__ float to_nan() { return bits_float(0x7FC00000u); }
__device__ __forceinline__ bool to_finite(float x) { return (float_bits(x) & 0x7F800000u) != 0x7F800000u; }

// the value between the sorted keys ka <= kb at fraction g
__device__ __forceinline__ float to_interpolate(uint32_t ka, uint32_t kb, double g) {
    if (g == 0.0) return from_key(ka);
    const double a = (double)from_key(ka), b = (double)from_key(kb);
    const double d = b - a;
    const double p = d * g;
    return (float)(a + p);
}
// position of the midpoint median of n samples: s[(n - 1) / 2], halfway to the next one for even n
__device__ __forceinline__ void to_median_position(int n, int& i, double& g) {
    i = n > 0 ? (n - 1) >> 1 : 0;
    g = (n > 0 && (n & 1) == 0) ? 0.5 : 0.0;
}

// ------------------------------------------------------------------------------------------------ register route
// VEC: one PPL-wide access per lane and frame (npix and the strides multiples of PPL, every base aligned to the access);
// otherwise dword accesses on clamped addresses and guarded stores.  The arithmetic is the same code: the same bits.
template <int PPL, bool VEC>
__device__ __forceinline__ void to_load(const float* frame, size_t i0, size_t npix, float (&v)[PPL]) {
    if constexpr (VEC && PPL == 4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 q = __builtin_nontemporal_load(reinterpret_cast<const f4*>(frame + i0));
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else if constexpr (VEC && PPL == 2) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const f2 q = __builtin_nontemporal_load(reinterpret_cast<const f2*>(frame + i0));
        v[0] = q.x, v[1] = q.y;
    } else {
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const size_t i = i0 + j < npix ? i0 + j : npix - 1;
            v[j] = __builtin_nontemporal_load(frame + i);
        }
    }
}
template <int PPL, bool VEC, class V>
__device__ __forceinline__ void to_store(V* row, size_t i0, size_t npix, const V (&v)[PPL]) {
    if constexpr (VEC && PPL > 1) {
        typedef V vv __attribute__((ext_vector_type(PPL)));
        vv q;
#pragma unroll
        for (int j = 0; j < PPL; ++j) q[j] = v[j];
        *reinterpret_cast<vv*>(row + i0) = q;
    } else {
#pragma unroll
        for (int j = 0; j < PPL; ++j)
            if (i0 + j < npix) row[i0 + j] = v[j];
    }
}
// the frames t0 .. t0 + 8 of a lane's pixels, eight loads in flight; frames beyond T repeat frame T - 1 and are not used
template <int PPL, bool VEC>
__device__ __forceinline__ void to_load8(const float* stack, int T, size_t fs, size_t i0, size_t npix, int t0, float (&v)[8][PPL]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;
        to_load<PPL, VEC>(stack + (size_t)t * fs, i0, npix, v[u]);
    }
}
template <int TP>
__device__ __forceinline__ uint32_t to_pick(const uint32_t (&k)[TP], int i) {
    uint32_t r = 0u;
#pragma unroll
    for (int j = 0; j < TP; ++j) r = j == i ? k[j] : r;
    return r;
}
template <int TP>
__device__ __forceinline__ float to_sorted_median(const uint32_t (&k)[TP], int n) {
    int i;
    double g;
    to_median_position(n, i, g);
    const float m = to_interpolate(to_pick<TP>(k, i), to_pick<TP>(k, i + 1), g);
    return n > 0 ? m : to_nan();
}

// grid ceil(npix / PPL / 256)
template <int TP, int PPL, bool VEC>
__global__ void __launch_bounds__(TO_THREADS) k_tq_reg(const float* __restrict__ stack, int T, size_t fs, size_t npix, QuantArgs a,
                                                       float* __restrict__ out, unsigned short* __restrict__ n_valid) {
    const size_t i0 = ((size_t)blockIdx.x * TO_THREADS + threadIdx.x) * PPL;
    if (i0 >= npix) return;
    uint32_t k[PPL][TP];
    int nn[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) nn[j] = 0;
#pragma unroll
    for (int t0 = 0; t0 < TP; t0 += 8) {
        if (t0 < T) {
            float v[8][PPL];
            to_load8<PPL, VEC>(stack, T, fs, i0, npix, t0, v);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    const uint32_t key = t0 + u < T ? to_key(v[u][j]) : KEY_PAD;
                    nn[j] += key < KEY_NAN ? 1 : 0;
                    k[j][t0 + u] = key;
                }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < PPL; ++j) k[j][t0 + u] = KEY_PAD;
        }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) sortnet::sortnet<KeyOps, TP>(k[j]);
    for (int iq = 0; iq < a.n_q; ++iq) {
        float r[PPL];
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const int n = a.nan_policy ? nn[j] : T;
            int i;
            double g;
            quantile_position(a.q[iq], n, a.method, i, g);
            const float val = to_interpolate(to_pick<TP>(k[j], i), to_pick<TP>(k[j], i + 1), g);
            r[j] = (n < 1 || (!a.nan_policy && nn[j] < T)) ? to_nan() : val;
        }
        to_store<PPL, VEC>(out + (size_t)iq * npix, i0, npix, r);
    }
    if (n_valid) {
        unsigned short nv[PPL];
#pragma unroll
        for (int j = 0; j < PPL; ++j) nv[j] = (unsigned short)nn[j];
        to_store<PPL, VEC>(n_valid, i0, npix, nv);
    }
}

template <int TP, int PPL, bool VEC>
__global__ void __launch_bounds__(TO_THREADS) k_tr_reg(const float* __restrict__ stack, int T, size_t fs, size_t npix, OutlierRule a,
                                                       float* __restrict__ mean, float* __restrict__ median, float* __restrict__ scale,
                                                       unsigned short* __restrict__ n_kept, unsigned char* __restrict__ rejected,
                                                       float* __restrict__ cleaned, size_t os) {
    const size_t i0 = ((size_t)blockIdx.x * TO_THREADS + threadIdx.x) * PPL;
    if (i0 >= npix) return;
    float x[PPL][TP];      // the samples in frame order, NaN for one that is not finite (and for the pad)
    uint32_t k[PPL][TP];
    int nn[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) nn[j] = 0;
#pragma unroll
    for (int t0 = 0; t0 < TP; t0 += 8) {
        if (t0 < T) {
            float v[8][PPL];
            to_load8<PPL, VEC>(stack, T, fs, i0, npix, t0, v);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    const bool in = t0 + u < T;
                    const float xv = in && to_finite(v[u][j]) ? v[u][j] : to_nan();
                    x[j][t0 + u] = xv;
                    const uint32_t key = in ? to_key(xv) : KEY_PAD;
                    nn[j] += key < KEY_NAN ? 1 : 0;
                    k[j][t0 + u] = key;
                }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    x[j][t0 + u] = to_nan();
                    k[j][t0 + u] = KEY_PAD;
                }
        }
    }
    float med[PPL], rhs[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        sortnet::sortnet<KeyOps, TP>(k[j]);
        med[j] = to_sorted_median<TP>(k[j], nn[j]);
    }
    if (a.scale_kind == 1) {
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
#pragma unroll
            for (int t = 0; t < TP; ++t) k[j][t] = t < T ? to_key(fabsf(__fsub_rn(x[j][t], med[j]))) : KEY_PAD;
            sortnet::sortnet<KeyOps, TP>(k[j]);
            rhs[j] = outlier_rhs(a, med[j], to_sorted_median<TP>(k[j], nn[j]));
        }
    } else {
#pragma unroll
        for (int j = 0; j < PPL; ++j) rhs[j] = outlier_rhs(a, med[j], 0.f);
    }
    // the kept samples are added in TO_GROUP partial sums, partial s over t = s, s + 8, .. in ascending t, joined as
    // ((P0 + P1) + (P2 + P3)) + ((P4 + P5) + (P6 + P7)): the order of the general route's lanes and butterfly
    double acc[PPL][TO_GROUP];
    int kept[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        kept[j] = 0;
#pragma unroll
        for (int s = 0; s < TO_GROUP; ++s) acc[j][s] = 0.0;
    }
#pragma unroll
    for (int t = 0; t < TP; ++t) {
        if (t < T) {
            unsigned char rj[PPL];
            float cl[PPL];
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                const bool o = outlier_rejected(a, x[j][t], med[j], rhs[j]);
                rj[j] = o ? 1 : 0;
                cl[j] = o ? med[j] : x[j][t];
                acc[j][t % TO_GROUP] += o ? 0.0 : (double)x[j][t];
                kept[j] += o ? 0 : 1;
            }
            if (rejected) to_store<PPL, VEC>(rejected + (size_t)t * os, i0, npix, rj);
            if (cleaned) to_store<PPL, VEC>(cleaned + (size_t)t * os, i0, npix, cl);
        }
    }
    float mo[PPL];
    unsigned short nk[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const double s01 = acc[j][0] + acc[j][1], s23 = acc[j][2] + acc[j][3], s45 = acc[j][4] + acc[j][5], s67 = acc[j][6] + acc[j][7];
        const double lo = s01 + s23, hi = s45 + s67;
        const double s = lo + hi;
        mo[j] = kept[j] > 0 ? (float)(s / (double)kept[j]) : to_nan();
        nk[j] = (unsigned short)kept[j];
    }
    to_store<PPL, VEC>(mean, i0, npix, mo);
    if (median) to_store<PPL, VEC>(median, i0, npix, med);
    if (scale) to_store<PPL, VEC>(scale, i0, npix, rhs);
    if (n_kept) to_store<PPL, VEC>(n_kept, i0, npix, nk);
}

// ------------------------------------------------------------------------------------------------ general route
// LDS: T rows of 32 keys, row t rotated by 8 (t mod 4) words.  A 32-lane half of a wave reads 8 adjacent pixels in 4 consecutive
// rows (ds_read_b32: 32 banks, conflicts counted per half): the rotation puts the four rows on the bank octets 0, 8, 16, 24 in
// some order, so the 32 addresses fall on 32 different banks without a padded row stride (T = 1024: 128 KiB, not 160).
__device__ __forceinline__ int tg_slot(int t, int p) { return t * TO_TILE + ((p + 8 * (t & 3)) & (TO_TILE - 1)); }

// keys of the tile: pixels beyond npix repeat the last pixel (computed, never stored); ROBUST: NaN for a sample that is not finite
template <bool ROBUST>
__device__ __forceinline__ void tg_stage(uint32_t* lds, const float* __restrict__ stack, int T, size_t fs, size_t npix, size_t tile0) {
    for (int idx = threadIdx.x; idx < T * TO_TILE; idx += TO_THREADS) {
        const int t = idx / TO_TILE, p = idx % TO_TILE;
        const size_t pix = tile0 + p < npix ? tile0 + p : npix - 1;
        float v = __builtin_nontemporal_load(stack + (size_t)t * fs + pix);
        if (ROBUST && !to_finite(v)) v = to_nan();
        lds[tg_slot(t, p)] = to_key(v);
    }
    __syncthreads();
}
// the three butterfly steps over the TO_GROUP lanes of a pixel (lane = sub * 8 + pixel): every lane of the group gets the result
__device__ __forceinline__ int tg_join_sum(int c) {
    c += __shfl_xor(c, 8, 64);
    c += __shfl_xor(c, 16, 64);
    c += __shfl_xor(c, 32, 64);
    return c;
}
__device__ __forceinline__ double tg_join_sum(double c) {
    c += __shfl_xor(c, 8, 64);
    c += __shfl_xor(c, 16, 64);
    c += __shfl_xor(c, 32, 64);
    return c;
}
__device__ __forceinline__ uint32_t tg_join_min(uint32_t c) {
    c = min(c, (uint32_t)__shfl_xor((int)c, 8, 64));
    c = min(c, (uint32_t)__shfl_xor((int)c, 16, 64));
    c = min(c, (uint32_t)__shfl_xor((int)c, 32, 64));
    return c;
}
// After the staging a lane copies its KPL >= ceil(T / 8) keys (samples t = sub, sub + 8, ..; the pad key beyond T) from LDS into
// registers, once and free of bank conflicts; the counting steps then run on registers.  key_at(m) is the m-th key of the lane.
template <int KPL>
__device__ __forceinline__ void tg_fetch(const uint32_t* lds, int T, int sub, int p, uint32_t (&kk)[KPL]) {
#pragma unroll
    for (int m = 0; m < KPL; ++m) {
        const int t = sub + m * TO_GROUP;
        kk[m] = t < T ? lds[tg_slot(t, p)] : KEY_PAD;
    }
}
// #(key < trial) over the samples of a pixel (the pad key is below no trial).  All 64 lanes of the wave call.
template <int KPL, class KeyAt>
__device__ __forceinline__ int tg_count_below(uint32_t trial, KeyAt key_at) {
    int c = 0;
#pragma unroll
    for (int m = 0; m < KPL; ++m) c += key_at(m) < trial ? 1 : 0;
    return tg_join_sum(c);
}
// the sorted keys s[i] and s[i + 1] (the pad key where i + 1 is beyond the samples): s[i] by 32 counting steps; s[i + 1] is
// the smallest key above s[i], unless more than i + 1 keys lie at or below s[i] -- then it is the same value again
template <int KPL, class KeyAt>
__device__ __forceinline__ void tg_select_pair(int i, KeyAt key_at, uint32_t& ka, uint32_t& kb) {
    ka = select_bitwise(i, [&](uint32_t trial) { return tg_count_below<KPL>(trial, key_at); });
    const int at_or_below = tg_count_below<KPL>(ka + 1u, key_at);   // no sample key exceeds KEY_NAN: ka + 1 does not wrap
    uint32_t above = KEY_PAD;
#pragma unroll
    for (int m = 0; m < KPL; ++m) {
        const uint32_t key = key_at(m);
        above = key > ka && key < above ? key : above;
    }
    above = tg_join_min(above);
    kb = at_or_below > i + 1 ? ka : above;
}
template <int KPL, class KeyAt>
__device__ __forceinline__ float tg_median(int n, KeyAt key_at) {
    int i;
    double g;
    to_median_position(n, i, g);
    uint32_t ka, kb;
    tg_select_pair<KPL>(i, key_at, ka, kb);
    const float m = to_interpolate(ka, kb, g);
    return n > 0 ? m : to_nan();
}

// grid ceil(npix / 32), dynamic LDS 128 T bytes; T <= 8 KPL
template <int KPL>
__global__ void __launch_bounds__(TO_THREADS) k_tq_gen(const float* __restrict__ stack, int T, size_t fs, size_t npix, QuantArgs a,
                                                       float* __restrict__ out, unsigned short* __restrict__ n_valid) {
    extern __shared__ __attribute__((aligned(16))) uint32_t to_lds[];
    const size_t tile0 = (size_t)blockIdx.x * TO_TILE;
    tg_stage<false>(to_lds, stack, T, fs, npix, tile0);
    const int lane = threadIdx.x & 63, p = (threadIdx.x >> 6) * 8 + (lane & 7), sub = lane >> 3;
    const size_t pix = tile0 + p;
    const bool writer = sub == 0 && pix < npix;
    uint32_t kk[KPL];
    tg_fetch<KPL>(to_lds, T, sub, p, kk);
    auto key_at = [&](int m) { return kk[m]; };
    const int nv = tg_count_below<KPL>(KEY_NAN, key_at);
    const int n = a.nan_policy ? nv : T;
    for (int iq = 0; iq < a.n_q; ++iq) {
        int i;
        double g;
        quantile_position(a.q[iq], n, a.method, i, g);
        uint32_t ka, kb;
        tg_select_pair<KPL>(i, key_at, ka, kb);
        const float val = to_interpolate(ka, kb, g);
        if (writer) out[(size_t)iq * npix + pix] = (n < 1 || (!a.nan_policy && nv < T)) ? to_nan() : val;
    }
    if (n_valid && writer) n_valid[pix] = (unsigned short)nv;
}

template <int KPL>
__global__ void __launch_bounds__(TO_THREADS) k_tr_gen(const float* __restrict__ stack, int T, size_t fs, size_t npix, OutlierRule a,
                                                       float* __restrict__ mean, float* __restrict__ median, float* __restrict__ scale,
                                                       unsigned short* __restrict__ n_kept, unsigned char* __restrict__ rejected,
                                                       float* __restrict__ cleaned, size_t os) {
    extern __shared__ __attribute__((aligned(16))) uint32_t to_lds[];
    const size_t tile0 = (size_t)blockIdx.x * TO_TILE;
    tg_stage<true>(to_lds, stack, T, fs, npix, tile0);
    const int lane = threadIdx.x & 63, p = (threadIdx.x >> 6) * 8 + (lane & 7), sub = lane >> 3;
    const size_t pix = tile0 + p;
    const bool inside = pix < npix, writer = sub == 0 && inside;
    uint32_t kk[KPL];
    tg_fetch<KPL>(to_lds, T, sub, p, kk);
    auto key_at = [&](int m) { return kk[m]; };
    const int n = tg_count_below<KPL>(KEY_NAN, key_at);
    const float med = tg_median<KPL>(n, key_at);
    float mad = 0.f;
    if (a.scale_kind == 1)      // the keys of |x - med|, formed on the fly
        mad = tg_median<KPL>(n, [&](int m) { return kk[m] == KEY_PAD ? KEY_PAD : to_key(fabsf(__fsub_rn(from_key(kk[m]), med))); });
    const float rhs = outlier_rhs(a, med, mad);
    double acc = 0.0;      // partial `sub` of the kept samples, ascending t
    int kept = 0;
    for (int t = sub; t < T; t += TO_GROUP) {      // the last pass reads the tile again: a rolled loop, the key registers are free
        const float x = from_key(to_lds[tg_slot(t, p)]);
        const bool o = outlier_rejected(a, x, med, rhs);
        acc += o ? 0.0 : (double)x;
        kept += o ? 0 : 1;
        if (rejected && inside) rejected[(size_t)t * os + pix] = o ? 1 : 0;
        if (cleaned && inside) cleaned[(size_t)t * os + pix] = o ? med : x;
    }
    acc = tg_join_sum(acc);
    kept = tg_join_sum(kept);
    if (writer) {
        mean[pix] = kept > 0 ? (float)(acc / (double)kept) : to_nan();
        if (median) median[pix] = med;
        if (scale) scale[pix] = rhs;
        if (n_kept) n_kept[pix] = (unsigned short)kept;
    }
}

// ------------------------------------------------------------------------------------------------ host side
constexpr long long TO_MAX_NPIX = (long long)1 << 36;   // 2^31 tiles of the general route

// pixels per lane of the register route by padded length (the resource table)
template <int TP> struct ToPpl { static constexpr int quant = TP <= 16 ? 4 : (TP == 32 ? 2 : 1), robust = TP <= 8 ? 4 : (TP == 16 ? 2 : 1); };

template <int TP>
static int launch_tq_reg(const float* stack, int T, size_t fs, size_t npix, const QuantArgs& a, float* out, unsigned short* nv, hipStream_t st) {
    constexpr int PPL = ToPpl<TP>::quant;
    const bool vec = PPL > 1 && npix % PPL == 0 && fs % PPL == 0 && ptr_aligned(stack, 4 * PPL) && ptr_aligned(out, 4 * PPL) && ptr_aligned(nv, 2 * PPL);
    const dim3 grid((unsigned)((npix + (size_t)PPL * TO_THREADS - 1) / ((size_t)PPL * TO_THREADS)));
    if (vec) return launch(k_tq_reg<TP, PPL, true>, grid, dim3(TO_THREADS), 0, st, stack, T, fs, npix, a, out, nv);
    return launch(k_tq_reg<TP, PPL, false>, grid, dim3(TO_THREADS), 0, st, stack, T, fs, npix, a, out, nv);
}
template <int TP>
static int launch_tr_reg(const float* stack, int T, size_t fs, size_t npix, const OutlierRule& a, float* mean, float* median, float* scale,
                         unsigned short* nk, unsigned char* rej, float* cleaned, size_t os, hipStream_t st) {
    constexpr int PPL = ToPpl<TP>::robust;
    const bool vec = PPL > 1 && npix % PPL == 0 && fs % PPL == 0 && os % PPL == 0 && ptr_aligned(stack, 4 * PPL) && ptr_aligned(mean, 4 * PPL) &&
                     ptr_aligned(median, 4 * PPL) && ptr_aligned(scale, 4 * PPL) && ptr_aligned(nk, 2 * PPL) && ptr_aligned(rej, PPL) &&
                     ptr_aligned(cleaned, 4 * PPL);
    const dim3 grid((unsigned)((npix + (size_t)PPL * TO_THREADS - 1) / ((size_t)PPL * TO_THREADS)));
    if (vec) return launch(k_tr_reg<TP, PPL, true>, grid, dim3(TO_THREADS), 0, st, stack, T, fs, npix, a, mean, median, scale, nk, rej, cleaned, os);
    return launch(k_tr_reg<TP, PPL, false>, grid, dim3(TO_THREADS), 0, st, stack, T, fs, npix, a, mean, median, scale, nk, rej, cleaned, os);
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_temporal_quantiles(const float* stack, int T, long long frame_stride, long long npix, const double* q, int n_q, int method,
                                      int nan_policy, int flags, float* out, unsigned short* n_valid, void* stream) {
    if (!stack || !out || !q || T < 1 || npix < 1) return fail(B4D_EINVAL, "b4d_temporal_quantiles: null pointer or empty shape");
    if (T > TO_MAX_T) return fail(B4D_ESIZE, "b4d_temporal_quantiles: more than 1024 frames");
    if (npix >= TO_MAX_NPIX) return fail(B4D_ESIZE, "b4d_temporal_quantiles: 2^36 pixels or more");
    if (frame_stride < npix) return fail(B4D_EINVAL, "b4d_temporal_quantiles: frame_stride < npix");
    if (n_q < 1 || n_q > TO_MAX_Q) return fail(B4D_EINVAL, "b4d_temporal_quantiles: n_q must be in 1 .. 8");
    if (method < 0 || method > 4 || nan_policy < 0 || nan_policy > 1 || (flags & ~1))
        return fail(B4D_EINVAL, "b4d_temporal_quantiles: method must be 0 .. 4, nan_policy 0 or 1, flags 0 or 1");
    QuantArgs a;
    for (int i = 0; i < TO_MAX_Q; ++i) a.q[i] = 0.0;
    for (int i = 0; i < n_q; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(B4D_EINVAL, "b4d_temporal_quantiles: every q must be a fraction in [0, 1]");
        a.q[i] = q[i];
    }
    a.n_q = n_q, a.method = method, a.nan_policy = nan_policy;
    const size_t fs = (size_t)frame_stride, np = (size_t)npix, sbytes = ((size_t)(T - 1) * fs + np) * sizeof(float);
    if (ranges_overlap(stack, sbytes, out, (size_t)n_q * np * sizeof(float)) || ranges_overlap(stack, sbytes, n_valid, np * sizeof(unsigned short)))
        return fail(B4D_EINVAL, "b4d_temporal_quantiles: an output overlaps the stack");
    hipStream_t st = (hipStream_t)stream;
    if (T > TO_MAX_REG_T || (flags & 1)) {
        const dim3 grid((unsigned)((np + TO_TILE - 1) / TO_TILE));
        const size_t lds = (size_t)T * TO_TILE * sizeof(uint32_t);
        if (T <= 128) return launch(k_tq_gen<16>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, out, n_valid);
        if (T <= 256) return launch(k_tq_gen<32>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, out, n_valid);
        if (T <= 512) return launch(k_tq_gen<64>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, out, n_valid);
        return launch(k_tq_gen<128>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, out, n_valid);
    }
    if (T <= 8) return launch_tq_reg<8>(stack, T, fs, np, a, out, n_valid, st);
    if (T <= 16) return launch_tq_reg<16>(stack, T, fs, np, a, out, n_valid, st);
    if (T <= 32) return launch_tq_reg<32>(stack, T, fs, np, a, out, n_valid, st);
    return launch_tq_reg<64>(stack, T, fs, np, a, out, n_valid, st);
}

extern "C" int b4d_temporal_robust_mean(const float* stack, int T, long long frame_stride, long long npix, int scale_kind, float threshold,
                                        float min_scale, int polarity, int flags, float* mean, float* median, float* scale,
                                        unsigned short* n_kept, unsigned char* rejected, float* cleaned, long long out_stride, void* stream) {
    if (!stack || !mean || T < 1 || npix < 1) return fail(B4D_EINVAL, "b4d_temporal_robust_mean: null pointer or empty shape");
    if (T > TO_MAX_T) return fail(B4D_ESIZE, "b4d_temporal_robust_mean: more than 1024 frames");
    if (npix >= TO_MAX_NPIX) return fail(B4D_ESIZE, "b4d_temporal_robust_mean: 2^36 pixels or more");
    if (frame_stride < npix || out_stride < npix) return fail(B4D_EINVAL, "b4d_temporal_robust_mean: frame_stride or out_stride < npix");
    if (scale_kind < 0 || scale_kind > 2 || polarity < 0 || polarity > 2 || (flags & ~1))
        return fail(B4D_EINVAL, "b4d_temporal_robust_mean: scale_kind / polarity must be 0, 1 or 2, flags 0 or 1");
    if (!(threshold >= 0.f) || !(min_scale >= 0.f)) return fail(B4D_EINVAL, "b4d_temporal_robust_mean: threshold and min_scale must be >= 0");
    const size_t fs = (size_t)frame_stride, os = (size_t)out_stride, np = (size_t)npix;
    const size_t sbytes = ((size_t)(T - 1) * fs + np) * sizeof(float), obytes = (size_t)(T - 1) * os + np;
    if (ranges_overlap(stack, sbytes, mean, np * 4) || ranges_overlap(stack, sbytes, median, np * 4) || ranges_overlap(stack, sbytes, scale, np * 4) ||
        ranges_overlap(stack, sbytes, n_kept, np * 2) || ranges_overlap(stack, sbytes, rejected, obytes) || ranges_overlap(stack, sbytes, cleaned, obytes * 4))
        return fail(B4D_EINVAL, "b4d_temporal_robust_mean: an output overlaps the stack");
    const OutlierRule a = make_outlier_rule(scale_kind, threshold, min_scale, polarity);
    hipStream_t st = (hipStream_t)stream;
    if (T > TO_MAX_REG_T || (flags & 1)) {
        const dim3 grid((unsigned)((np + TO_TILE - 1) / TO_TILE));
        const size_t lds = (size_t)T * TO_TILE * sizeof(uint32_t);
        if (T <= 128) return launch(k_tr_gen<16>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os);
        if (T <= 256) return launch(k_tr_gen<32>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os);
        if (T <= 512) return launch(k_tr_gen<64>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os);
        return launch(k_tr_gen<128>, grid, dim3(TO_THREADS), lds, st, stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os);
    }
    if (T <= 8) return launch_tr_reg<8>(stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os, st);
    if (T <= 16) return launch_tr_reg<16>(stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os, st);
    if (T <= 32) return launch_tr_reg<32>(stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os, st);
    return launch_tr_reg<64>(stack, T, fs, np, a, mean, median, scale, n_kept, rejected, cleaned, os, st);
}
