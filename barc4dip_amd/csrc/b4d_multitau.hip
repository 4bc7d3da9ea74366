// b4d_multitau.hip -- multi-tau correlation of long and streamed speckle stacks (include/b4d.h: b4d_multi_tau_*; DESIGN.md
// section 21).
//
// The correlator keeps a fixed amount of state per used pixel and takes the stack in pushes of any length.  Level 0 is the stack,
// level l the pairwise float32 average of level l - 1; every level correlates each new frame with its last m - 1 frames.
//   scan    bad[p] |= "x[t, p] is not finite for some t of this chunk"
//   init    effective labels, pixels per (span, region), prefix -> the region-ordered pixel list pix[q] (raster order within a
//           region, every region starts on a wave boundary, the rest of its last wave is padding, pix = -1); state zeroed
//   push    one launch per level that receives a frame (k_mt_push).  A lane owns one pixel of the list: it holds the level's last
//           m - 1 values and the MT_RUN new ones in registers, does m (level 0) or m / 2 (above) multiply-adds per new value
//           for P = sum I[k] I[k + j] and Q = sum (I[k] I[k + j])^2 in float32, and moves them into float64 after every MT_RUN
//           frames.  At the end of the push the float64 sums are added across the wave (xor butterfly) and into the wave's slot.
//           Frames before the level's first one read as 0, so the loop has no lag-dependent bounds.  The level's averaged frames
//           go to a scratch buffer (two buffers, used in turn), its last m - 1 frames to a ring of m slots in the workspace.
//           The partner sums A = sum I[k], B = sum I[k + j] are not accumulated per lag: A_j = S - (the last j frames),
//           B_j = S - (the first j frames), with S the sum of all frames of the level.  S and the first m - 1 frames' sums are
//           stored per wave as the frames pass; the last m - 1 are read from the ring at the end.
//   finish  the ring's frame sums per wave; every per-wave column summed per region in wave order (lanes in index order, fixed
//           tree); g2, g2_err, mean, n_pixels.
// One wave per workgroup: a slot has one writer, there are no atomics, and every sum runs in an order fixed by T, the frame size,
// the label map, m and the sequence of push lengths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_reduce.hpp"
#include "b4d_regions.hpp"

namespace b4d {

constexpr int MT_RUN = 8;         // frames per float32 run of a lane's sums
constexpr int MT_MAX_R = RG_MAX_R;
constexpr int MT_MAX_LEVELS = 24;

struct MTLayout {
    int W;                        // waves (upper bound): npix / 64 + R
    long long Q;                  // lanes: 64 W
    long long span;               // pixels per span (multiple of 64)
    int nspan;
    int NS;                       // lag slots: m + (n_levels - 1) m / 2
    int ncols;                    // per-wave float64 columns: P[NS] Q[NS] S[L] head[L m] tail[L m]
    int cap0, cap1;               // frames of the two scratch buffers
    size_t o_pix, o_lab, o_cnt, o_base, o_meta, o_ring, o_buf0, o_buf1, o_cols, o_red, bytes;
    int c_P, c_Q, c_S, c_head, c_tail;
};

static bool mt_layout(long long npix, int R, int m, int L, int max_push, MTLayout& y) {
    if (npix < 1 || npix >= (1ll << 31) || R < 1 || R > MT_MAX_R || (m != 8 && m != 16 && m != 32) || L < 1 || L > MT_MAX_LEVELS ||
        max_push < 1)
        return false;
    y.W = (int)(npix / 64 + R);
    y.Q = 64ll * y.W;
    y.span = 64 * ((npix + 64 * 4096ll - 1) / (64 * 4096ll));
    y.nspan = (int)((npix + y.span - 1) / y.span);
    y.NS = m + (L - 1) * (m / 2);
    y.c_P = 0;
    y.c_Q = y.NS;
    y.c_S = 2 * y.NS;
    y.c_head = y.c_S + L;
    y.c_tail = y.c_head + L * m;
    y.ncols = y.c_tail + L * m;
    y.cap0 = (max_push + 1) / 2;
    y.cap1 = (y.cap0 + 1) / 2;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align256(bytes);
        return at;
    };
    y.o_pix = take(sizeof(int) * (size_t)y.Q);
    y.o_lab = take((size_t)npix);
    y.o_cnt = take(sizeof(int) * (size_t)y.nspan * R);
    y.o_base = take(sizeof(int) * (size_t)y.nspan * R);
    y.o_meta = take(sizeof(RegionMeta));
    y.o_ring = take(sizeof(float) * (size_t)L * m * (size_t)y.Q);
    y.o_buf0 = take(L > 1 ? sizeof(float) * (size_t)y.cap0 * (size_t)y.Q : 0);
    y.o_buf1 = take(L > 2 ? sizeof(float) * (size_t)y.cap1 * (size_t)y.Q : 0);
    y.o_cols = take(sizeof(double) * (size_t)y.ncols * y.W);
    y.o_red = take(sizeof(double) * (size_t)y.ncols * R);
    y.bytes = o;
    return true;
}

// levels in use for T frames: level 0, and every l >= 1 with floor(T / 2^l) >= m / 2 + 1, up to max_level (< 0: no cap)
static int mt_levels(long long T, int m, int max_level) {
    int L = 1;
    while (L < 40 && (T >> L) >= m / 2 + 1 && (max_level < 0 || L <= max_level)) ++L;
    return L;
}

// ---- scan: grid (ceil(npix / 256), ceil(n / 32)).  Every writer stores the same byte.
__global__ void __launch_bounds__(256) k_mt_scan(const float* __restrict__ x, int n, long long npix, uint8_t* __restrict__ bad) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int t0 = blockIdx.y * 32, t1 = min(n, t0 + 32);
    bool fin = true;
    for (int t = t0; t < t1; ++t) fin = fin && isfinite(x[(size_t)t * (size_t)npix + (size_t)p]);
    if (!fin) bad[p] = 1;
}

// ---- init, after region_list: pixel p of region r lands at lane 64 start[r] + (pixels of r before p).  pix was filled with -1.
// grid (nspan), one wave
__global__ void __launch_bounds__(64) k_mt_fill(const uint8_t* __restrict__ lab, long long npix, int R, long long span,
                                                const int* __restrict__ base, const RegionMeta* __restrict__ meta,
                                                int* __restrict__ pix) {
    __shared__ int run[RG_MAX_R + 1];
    const int lane = threadIdx.x;
    for (int r = lane; r < R; r += 64) run[r + 1] = base[(size_t)blockIdx.x * R + r];
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * span, p1 = min(npix, p0 + span);
    for (long long g = p0; g < p1; g += 64) {
        const long long p = g + lane;
        for_each_label(p < p1 ? (int)lab[p] : 0, [&](int r, int lead, bool mine, unsigned long long mask) {
            const long long dst = region_slot<64>(meta, run, r, lead, lane, mask);
            if (mine) pix[dst] = (int)p;
        });
    }
}

// ---- push, one level: grid (W), one wave per workgroup.  M lags per level, J0 the first lag (0 on level 0, M / 2 above).
// src: the level's n new frames, frame k at src + k * stride; pix: the pixel list (level 0) or null (src is in list order).
// c: frames the level has received before.  ring: this level's M slots of Q floats, frame i in slot i & (M - 1).
// out: the next level's new frames in list order (null on the last level), cap of them.  P, Qs: this level's M - J0 columns;
// S: one column; head: M columns (the sums of the level's frames 0 .. M - 2).
template <int M, int J0>
__global__ void __launch_bounds__(64) k_mt_push(const float* __restrict__ src, long long stride, const int* __restrict__ pix, int c,
                                                int n, long long Q, int W, int R, const RegionMeta* __restrict__ meta,
                                                float* __restrict__ ring, float* __restrict__ out, int cap, double* __restrict__ P,
                                                double* __restrict__ Qs, double* __restrict__ S, double* __restrict__ head) {
    constexpr int NL = M - J0;
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= meta->start[R]) return;
    const long long q = 64ll * w + lane;
    const long long off = pix ? (long long)pix[q] : q;
    const bool live = off >= 0;
    float win[M - 1 + MT_RUN];
#pragma unroll
    for (int i = 0; i < M - 1; ++i) {
        const int idx = c - (M - 1) + i;
        win[i] = idx >= 0 ? ring[(size_t)(idx & (M - 1)) * (size_t)Q + (size_t)q] : 0.f;
    }
    float pf[NL], qf[NL];
    double pd[NL], qd[NL], sd = 0.0;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        pf[j] = qf[j] = 0.f;
        pd[j] = qd[j] = 0.0;
    }
    for (int k = 0; k < n; k += MT_RUN) {
#pragma unroll
        for (int u = 0; u < MT_RUN; ++u)
            win[M - 1 + u] = (live && k + u < n) ? src[(size_t)(k + u) * (size_t)stride + (size_t)off] : 0.f;
        float sf = 0.f;
#pragma unroll
        for (int u = 0; u < MT_RUN; ++u) {
            const float v = win[M - 1 + u];
            sf += v;
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const float h = win[M - 1 + u - (J0 + j)];
                const float pr = v * h;
                pf[j] = fmaf(v, h, pf[j]);
                qf[j] = fmaf(pr, pr, qf[j]);
            }
            const int a = c + k + u;        // the frame's index in its level; the branches below are the same in every lane
            if (k + u < n) {
                if (a < M - 1) {
                    const double s = wave_sum_all((double)v);
                    if (lane == 0) head[(size_t)a * W + w] = s;
                }
                if (out && (a & 1)) {
                    const int e = (a >> 1) - (c >> 1);
                    if (e < cap) out[(size_t)e * (size_t)Q + (size_t)q] = 0.5f * (win[M - 2 + u] + v);
                }
                if (k + u >= n - (M - 1)) ring[(size_t)(a & (M - 1)) * (size_t)Q + (size_t)q] = v;
            }
        }
        sd += (double)sf;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            pd[j] += (double)pf[j];
            qd[j] += (double)qf[j];
            pf[j] = qf[j] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < M - 1; ++i) win[i] = win[i + MT_RUN];
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const double a = wave_sum_all(pd[j]), b = wave_sum_all(qd[j]);
        if (lane == 0) {
            P[(size_t)j * W + w] += a;
            Qs[(size_t)j * W + w] += b;
        }
    }
    sd = wave_sum_all(sd);
    if (lane == 0) S[w] += sd;
}

// ---- finish a: tail[(l m + i) W + w] = the wave's sum of the i-th last frame of level l (0 where the level has fewer).
// grid (W, L), one wave
__global__ void __launch_bounds__(64) k_mt_tail(const float* __restrict__ ring, int T, int m, long long Q, int W, int R,
                                                const RegionMeta* __restrict__ meta, double* __restrict__ tail) {
    const int w = blockIdx.x, l = blockIdx.y, lane = threadIdx.x;
    if (w >= meta->start[R]) return;
    const int Tl = T >> l;
    const float* rl = ring + (size_t)l * m * (size_t)Q + (size_t)(64ll * w + lane);
    for (int i = 0; i < m - 1; ++i) {
        const int idx = Tl - 1 - i;
        const double s = wave_sum_all(idx >= 0 ? (double)rl[(size_t)(idx & (m - 1)) * (size_t)Q] : 0.0);
        if (lane == 0) tail[((size_t)l * m + i) * W + w] = s;
    }
}

// ---- finish b: red[col R + r] = sum of column col over the region's waves: thread t adds the waves t, t + 256, ... of the region in
// order, then a fixed tree.  grid (ncols, R), block 256
__global__ void __launch_bounds__(256) k_mt_colsum(const double* __restrict__ cols, int W, int R, const RegionMeta* __restrict__ meta,
                                                   double* __restrict__ red) {
    __shared__ double sh[256];
    const int col = blockIdx.x, r = blockIdx.y;
    const int w0 = meta->start[r], w1 = meta->start[r + 1];
    double a = 0.0;
    for (int w = w0 + threadIdx.x; w < w1; w += 256) a += cols[(size_t)col * W + w];
    a = block_tree_sum256(a, sh, false);
    if (threadIdx.x == 0) red[(size_t)col * R + r] = a;
}

// ---- finish c: one thread per (region, lag).  grid ceil(R n_lags / 64)
__global__ void __launch_bounds__(64) k_mt_final(const double* __restrict__ red, int T, int m, int L, int R, int n_lags, int NS,
                                                 const RegionMeta* __restrict__ meta, double* __restrict__ g2, double* __restrict__ g2_err,
                                                 double* __restrict__ mean, long long* __restrict__ n_pixels) {
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= R * n_lags) return;
    const int r = id / n_lags;
    int k = id % n_lags, l = 0, j = 0;
    for (; l < L; ++l) {        // lag k -> (level, j), in the order of b4d_multi_tau_lags
        const int Tl = T >> l, j0 = l ? m / 2 : 0;
        const int cnt = max(0, min(m, Tl) - j0);
        if (k < cnt) {
            j = j0 + k;
            break;
        }
        k -= cnt;
    }
    if (l >= L) return;
    const int c_S = 2 * NS, c_head = c_S + L, c_tail = c_head + L * m;
    const int slot = l ? m + (l - 1) * (m / 2) + (j - m / 2) : j;
    const double N = (double)meta->N[r];
    const double nn = N * (double)((T >> l) - j);
    double g = NAN, ge = NAN;
    if (N > 0.0) {
        const double S = red[(size_t)(c_S + l) * R + r];
        double A = S, B = S;
        for (int i = 0; i < j; ++i) {
            A -= red[(size_t)(c_tail + l * m + i) * R + r];
            B -= red[(size_t)(c_head + l * m + i) * R + r];
        }
        const double p = red[(size_t)slot * R + r] / nn, q = red[(size_t)(NS + slot) * R + r] / nn;
        const double den = (A / nn) * (B / nn);
        if (den > 0.0) {
            g = p / den;
            ge = sqrt(fmax(q - p * p, 0.0) / nn) / den;
        }
    }
    g2[id] = g;
    g2_err[id] = ge;
    if (id % n_lags == 0) {
        mean[r] = N > 0.0 ? red[(size_t)c_S * R + r] / (N * (double)T) : NAN;
        n_pixels[r] = meta->N[r];
    }
}

template <int M>
static void mt_launch_level(bool first, int W, hipStream_t st, const float* src, long long stride, const int* pix, int c, int n,
                            long long Q, int R, const RegionMeta* meta, float* ring, float* out, int cap, double* P, double* Qs, double* S,
                            double* head) {
    if (first)
        hipLaunchKernelGGL((k_mt_push<M, 0>), dim3(W), dim3(64), 0, st, src, stride, pix, c, n, Q, W, R, meta, ring, out, cap, P, Qs, S,
                           head);
    else
        hipLaunchKernelGGL((k_mt_push<M, M / 2>), dim3(W), dim3(64), 0, st, src, stride, pix, c, n, Q, W, R, meta, ring, out, cap, P, Qs,
                           S, head);
}

static int mt_check(long long npix, int n_regions, int m, int n_levels, int max_push, MTLayout& y) {
    if (npix < 1 || n_regions < 1 || n_levels < 1 || max_push < 1)
        return fail(B4D_EINVAL, "multi-tau: npix, n_regions, n_levels and max_push must be at least 1");
    if ((m != 8 && m != 16 && m != 32) || n_regions > MT_MAX_R || npix >= (1ll << 31) || n_levels > MT_MAX_LEVELS)
        return fail(B4D_ESIZE, "multi-tau: lags_per_level 8, 16 or 32, n_regions <= 64, fewer than 2^31 pixels per frame and at most 24 "
                               "levels");
    if (!mt_layout(npix, n_regions, m, n_levels, max_push, y)) return fail(B4D_ESIZE, "multi-tau: unsupported shape");
    return B4D_OK;
}

}  // namespace b4d

using namespace b4d;

extern "C" size_t b4d_multi_tau_workspace_bytes(long long npix, int n_regions, int m, int n_levels, int max_push) {
    MTLayout y;
    return mt_layout(npix, n_regions, m, n_levels, max_push, y) ? y.bytes : 0;
}

extern "C" int b4d_multi_tau_lags(long long T, int m, int max_level, long long* lags, int* levels, long long* n_pairs, int* n_levels) {
    if (T < 2) return fail(B4D_EINVAL, "multi-tau: T >= 2");
    if (m != 8 && m != 16 && m != 32) return fail(B4D_ESIZE, "multi-tau: lags_per_level must be 8, 16 or 32");
    if (T >= (1ll << 31)) return fail(B4D_ESIZE, "multi-tau: T < 2^31");
    const int L = mt_levels(T, m, max_level);
    if (L > MT_MAX_LEVELS) return fail(B4D_ESIZE, "multi-tau: more than 24 levels (set max_level)");
    int k = 0;
    for (int l = 0; l < L; ++l) {
        const long long Tl = T >> l;
        for (int j = l ? m / 2 : 0; j < m && Tl - j >= 1; ++j, ++k) {
            if (lags) lags[k] = (long long)j << l;
            if (levels) levels[k] = l;
            if (n_pairs) n_pairs[k] = Tl - j;
        }
    }
    if (n_levels) *n_levels = L;
    return k;
}

extern "C" int b4d_multi_tau_scan(const float* frames, int n, long long npix, unsigned char* bad, void* stream) {
    if (!frames || !bad) return fail(B4D_EINVAL, "null argument");
    if (n < 1 || npix < 1) return fail(B4D_EINVAL, "multi-tau scan: n >= 1 and npix >= 1");
    if (npix >= (1ll << 31) || (n + 31) / 32 > 65535) return fail(B4D_ESIZE, "multi-tau scan: npix < 2^31 and n <= 2 097 120 frames a call");
    hipLaunchKernelGGL(k_mt_scan, dim3((unsigned)((npix + 255) / 256), (n + 31) / 32), dim3(256), 0, (hipStream_t)stream, frames, n, npix,
                       bad);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_multi_tau_init(const int* labels, const unsigned char* bad, long long npix, int n_regions, int m, int n_levels,
                                  int max_push, void* workspace, void* stream) {
    if (!workspace) return fail(B4D_EINVAL, "null argument");
    if (!labels && n_regions != 1) return fail(B4D_EINVAL, "multi-tau: without a label map there is one region");
    MTLayout y;
    if (int rc = mt_check(npix, n_regions, m, n_levels, max_push, y)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* w = static_cast<char*>(workspace);
    const int R = n_regions;
    uint8_t* lab = reinterpret_cast<uint8_t*>(w + y.o_lab);
    int* pix = reinterpret_cast<int*>(w + y.o_pix);
    int* cnt = reinterpret_cast<int*>(w + y.o_cnt);
    int* base = reinterpret_cast<int*>(w + y.o_base);
    RegionMeta* meta = reinterpret_cast<RegionMeta*>(w + y.o_meta);
    B4D_HIP(hipMemsetAsync(pix, 0xFF, sizeof(int) * (size_t)y.Q, st));
    B4D_HIP(hipMemsetAsync(w + y.o_ring, 0, sizeof(float) * (size_t)n_levels * m * (size_t)y.Q, st));
    B4D_HIP(hipMemsetAsync(w + y.o_cols, 0, sizeof(double) * (size_t)y.ncols * y.W, st));
    region_list(labels, false, bad, npix, R, y.span, y.nspan, 64, lab, cnt, base, meta, nullptr, st);
    hipLaunchKernelGGL(k_mt_fill, dim3(y.nspan), dim3(64), 0, st, lab, npix, R, y.span, base, meta, pix);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_multi_tau_push(const float* frames, long long t0, int n, long long npix, int n_regions, int m, int n_levels,
                                  int max_push, void* workspace, void* stream) {
    if (!frames || !workspace) return fail(B4D_EINVAL, "null argument");
    MTLayout y;
    if (int rc = mt_check(npix, n_regions, m, n_levels, max_push, y)) return rc;
    if (n < 1 || n > max_push || t0 < 0) return fail(B4D_EINVAL, "multi-tau push: 1 <= n <= max_push and t0 >= 0");
    if (t0 + n >= (1ll << 31)) return fail(B4D_ESIZE, "multi-tau push: T < 2^31");
    hipStream_t st = (hipStream_t)stream;
    char* w = static_cast<char*>(workspace);
    const int* pix = reinterpret_cast<const int*>(w + y.o_pix);
    const RegionMeta* meta = reinterpret_cast<const RegionMeta*>(w + y.o_meta);
    float* ring = reinterpret_cast<float*>(w + y.o_ring);
    float* buf[2] = {reinterpret_cast<float*>(w + y.o_buf0), reinterpret_cast<float*>(w + y.o_buf1)};
    double* cols = reinterpret_cast<double*>(w + y.o_cols);
    int cap = max_push;                         // most frames level l can receive in a push
    for (int l = 0; l < n_levels; ++l) {
        const int c = (int)(t0 >> l), nl = (int)((t0 + n) >> l) - c;
        const int cap_out = (cap + 1) / 2;
        if (nl < 1) break;                      // the levels above receive nothing either
        const bool last = l == n_levels - 1;
        const float* src = l ? buf[(l - 1) & 1] : frames;
        const int slot = l ? m + (l - 1) * (m / 2) : 0;
        float* rl = ring + (size_t)l * m * (size_t)y.Q;
        double* P = cols + (size_t)(y.c_P + slot) * y.W;
        double* Qs = cols + (size_t)(y.c_Q + slot) * y.W;
        double* S = cols + (size_t)(y.c_S + l) * y.W;
        double* head = cols + (size_t)(y.c_head + l * m) * y.W;
        float* out = last ? nullptr : buf[l & 1];
        const long long stride = l ? y.Q : npix;
        if (m == 8)
            mt_launch_level<8>(l == 0, y.W, st, src, stride, l ? nullptr : pix, c, nl, y.Q, n_regions, meta, rl, out, cap_out, P, Qs, S,
                               head);
        else if (m == 16)
            mt_launch_level<16>(l == 0, y.W, st, src, stride, l ? nullptr : pix, c, nl, y.Q, n_regions, meta, rl, out, cap_out, P, Qs, S,
                                head);
        else
            mt_launch_level<32>(l == 0, y.W, st, src, stride, l ? nullptr : pix, c, nl, y.Q, n_regions, meta, rl, out, cap_out, P, Qs, S,
                                head);
        cap = cap_out;
    }
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_multi_tau_finish(long long T, long long npix, int n_regions, int m, int n_levels, int max_push, void* workspace,
                                    double* g2, double* g2_err, double* mean, long long* n_pixels, void* stream) {
    if (!workspace || !g2 || !g2_err || !mean || !n_pixels) return fail(B4D_EINVAL, "null argument");
    MTLayout y;
    if (int rc = mt_check(npix, n_regions, m, n_levels, max_push, y)) return rc;
    if (T < 2) return fail(B4D_EINVAL, "multi-tau: T >= 2");
    if (T >= (1ll << 31)) return fail(B4D_ESIZE, "multi-tau: T < 2^31");
    if (n_levels > mt_levels(T, m, -1)) return fail(B4D_EINVAL, "multi-tau finish: T frames do not fill n_levels levels");
    const int n_lags = b4d_multi_tau_lags(T, m, n_levels - 1, nullptr, nullptr, nullptr, nullptr);
    if (n_lags < 0) return n_lags;
    hipStream_t st = (hipStream_t)stream;
    char* w = static_cast<char*>(workspace);
    const RegionMeta* meta = reinterpret_cast<const RegionMeta*>(w + y.o_meta);
    const float* ring = reinterpret_cast<const float*>(w + y.o_ring);
    double* cols = reinterpret_cast<double*>(w + y.o_cols);
    double* red = reinterpret_cast<double*>(w + y.o_red);
    const int R = n_regions;
    hipLaunchKernelGGL(k_mt_tail, dim3(y.W, n_levels), dim3(64), 0, st, ring, (int)T, m, y.Q, y.W, R, meta,
                       cols + (size_t)y.c_tail * y.W);
    hipLaunchKernelGGL(k_mt_colsum, dim3(y.ncols, R), dim3(256), 0, st, cols, y.W, R, meta, red);
    hipLaunchKernelGGL(k_mt_final, dim3((R * n_lags + 63) / 64), dim3(64), 0, st, red, (int)T, m, n_levels, R, n_lags, y.NS, meta, g2,
                       g2_err, mean, n_pixels);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
