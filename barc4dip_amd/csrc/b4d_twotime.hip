// b4d_twotime.hip -- two-time correlation of a speckle stack (include/b4d.h: b4d_two_time).
//
// Per region r (the pixels that carry label r and are finite in all T frames) the T x T matrix of covariances is a symmetric
// rank-k update over the region's pixels.  The stages, all on the caller's stream:
//   1. scan     one wave per (pixel span, frame slice): float64 sums and counts of the finite pixels per (span, region, frame),
//               and a flag per labelled pixel that is non-finite in some frame.  Offsets c[r][t] = float32(provisional mean).
//   2. pack     the region list (b4d_regions.hpp) with a chunk as granule -> every pixel's place in its region's raster order;
//               Xc[t][q] = x[t][p] - c[r][t] (float32), regions one after the other, each padded with zeros to whole chunks
//               of TT_KC pixels; s[r][t] = float64 sum of the stored values.
//   3. product  split-K SYRK on v_mfma_f32_32x32x2_f32: one workgroup per (chunk, frame-block pair bi <= bj inside the band),
//               128 x 128 tile, four waves in 2 x 2 of 64 x 64 (lane maps: b4d_mfma.hpp), K staged 32 deep
//               through LDS with the next stage prefetched into registers; the accumulators are added into a second set and
//               cleared every TT_RUN products (short fma chains).  The partial tile goes to the workspace: no communication
//               between workgroups, no atomics.
//   4. reduce   float64 sum of a region's partial tiles in chunk order, cov = Gc / N - (s_i / N)(s_j / N), m = c + s / N;
//               then the normalisation, written to both triangles from one value.
//   5. lags     g2 and its standard error along the diagonals (b4d_two_time_lags).
// Every sum runs in an order fixed by (T, npix, max_lag) and the region's own pixel list: spans are cut by pixel position,
// chunks by the position in the region's list.  No f32 accumulator sees more than TT_KC products.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_mfma.hpp"
#include "b4d_reduce.hpp"
#include "b4d_regions.hpp"

namespace b4d {

constexpr int TT_KC = 2048;       // pixels per chunk (one f32 accumulation)
constexpr int TT_RUN = 256;       // products per float32 fma chain: the chunk's eight runs are added up once each
constexpr int TT_TILE = 128;      // frame block
constexpr int TT_U = 8;           // frames per step of the scan and pack loops
constexpr int TT_MAX_T = 2048;
constexpr int TT_MAX_R = RG_MAX_R;

struct TTLayout {
    int nb, W, npairs;            // frame blocks, largest block distance inside the band, block pairs
    long long span;               // pixels per span (multiple of 64)
    int nscan, fz, tz;            // spans, frames per slice (multiple of TT_U), slices
    long long nchunks, ktot;      // upper bound of the chunks in use; row length of Xc
    size_t o_xc, o_part, o_psum, o_pcnt, o_lab, o_bad, o_cnt, o_base, o_c, o_s, o_meta, bytes;
};

static bool tt_layout(int T, long long npix, int R, int L, TTLayout& y) {
    if (T < 2 || T > TT_MAX_T || npix < 1 || npix >= (1ll << 31) || R < 1 || R > TT_MAX_R || L < 0 || L > T - 1) return false;
    y.nb = (T + TT_TILE - 1) / TT_TILE;
    y.W = (L + TT_TILE - 1) / TT_TILE;
    y.npairs = 0;
    for (int bi = 0; bi < y.nb; ++bi) y.npairs += std::min(y.nb - 1, bi + y.W) - bi + 1;
    const long long smax = std::max(64, std::min(4096, (1 << 20) / T));
    y.span = 64 * ((npix + 64 * smax - 1) / (64 * smax));
    y.nscan = (int)((npix + y.span - 1) / y.span);
    y.fz = TT_U * ((T + TT_U * 8 - 1) / (TT_U * 8));
    y.tz = (T + y.fz - 1) / y.fz;
    y.nchunks = npix / TT_KC + R;
    y.ktot = y.nchunks * TT_KC;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align256(bytes);
        return at;
    };
    y.o_xc = take(sizeof(float) * (size_t)T * (size_t)y.ktot);
    y.o_part = take(sizeof(float) * (size_t)y.nchunks * y.npairs * TT_TILE * TT_TILE);
    y.o_psum = take(sizeof(double) * (size_t)y.nscan * R * T);
    y.o_pcnt = take(sizeof(double) * (size_t)y.nscan * R * T);
    y.o_lab = take((size_t)npix);
    y.o_bad = take((size_t)npix);
    y.o_cnt = take(sizeof(int) * (size_t)y.nscan * R);
    y.o_base = take(sizeof(int) * (size_t)y.nscan * R);
    y.o_c = take(sizeof(float) * (size_t)R * T);
    y.o_s = take(sizeof(double) * (size_t)R * T);
    y.o_meta = take(sizeof(RegionMeta));
    y.bytes = o;
    return true;
}

// ---- labels as bytes: 0 outside 1 .. R; without a label map every pixel is region 1.  grid ceil(npix / 256)
__global__ void __launch_bounds__(256) k_tt_labels(const int* __restrict__ labels, long long npix, int R, uint8_t* __restrict__ lab) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    lab[p] = (uint8_t)region_label(labels, p, R);
}

// ---- 1. scan: grid (nscan, tz), one wave.  psum / pcnt[(span * R + r) * T + t] += sum / count over the span's pixels of label
// r + 1 that are finite in frame t (only this wave touches the slot); bad[p] = 1 for a labelled pixel with a non-finite frame.
__global__ void __launch_bounds__(64) k_tt_scan(const float* __restrict__ x, int T, long long npix, int R, long long span, int fz,
                                                const uint8_t* __restrict__ lab, uint8_t* __restrict__ bad,
                                                double* __restrict__ psum, double* __restrict__ pcnt) {
    const int lane = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * span, p1 = min(npix, p0 + span);
    const int t0 = blockIdx.y * fz, t1 = min(T, t0 + fz);
    for (long long g = p0; g < p1; g += 64) {
        const long long p = g + lane;
        const int l = p < p1 ? (int)lab[p] : 0;
        bool allfin = true;
        for_each_label(l, [&](int r, int, bool mine, unsigned long long) {
            for (int t = t0; t < t1; t += TT_U) {
                float v[TT_U];
#pragma unroll
                for (int u = 0; u < TT_U; ++u) v[u] = (mine && t + u < t1) ? x[(size_t)(t + u) * (size_t)npix + (size_t)p] : 0.f;
                double ms = 0.0, mc = 0.0;
#pragma unroll
                for (int u = 0; u < TT_U; ++u) {
                    const bool fin = isfinite(v[u]);
                    if (!fin) allfin = false;
                    const bool use = mine && fin && t + u < t1;
                    const double s = wave_sum_all(use ? (double)v[u] : 0.0);
                    const double c = (double)__popcll(__ballot(use));
                    if (lane == u) {
                        ms = s;
                        mc = c;
                    }
                }
                if (lane < TT_U && t + lane < t1) {
                    const size_t at = ((size_t)blockIdx.x * R + (r - 1)) * T + t + lane;
                    psum[at] += ms;
                    pcnt[at] += mc;
                }
            }
        });
        if (l > 0 && !allfin) bad[p] = 1;
    }
}

// ---- column sums of the per-span partials, one wave per (r, t): lane l adds the spans l, l + 64, ... in order, then the lanes are
// summed in a fixed tree.  With counts: c = float32(sum / count) (0 without pixels); without: s = sum.  grid (R * T)
__global__ void __launch_bounds__(64) k_tt_colsum(const double* __restrict__ psum, const double* __restrict__ pcnt, int nscan,
                                                  int R, int T, float* __restrict__ c, double* __restrict__ s) {
    const int rt = blockIdx.x, r = rt / T, t = rt % T;
    double a = 0.0, n = 0.0;
    for (int b = threadIdx.x; b < nscan; b += 64) {
        const size_t at = ((size_t)b * R + r) * T + t;
        a += psum[at];
        if (pcnt) n += pcnt[at];
    }
    a = wave_sum_all(a);
    if (pcnt) n = wave_sum_all(n);
    if (threadIdx.x == 0) {
        if (pcnt)
            c[rt] = n > 0.0 ? (float)(a / n) : 0.f;
        else
            s[rt] = a;
    }
}

// ---- 2. pack, after region_list: grid (nscan, tz), one wave.  Pixel p of region r lands at column start[r] * TT_KC + (pixels of r
// before p).
__global__ void __launch_bounds__(64) k_tt_pack(const float* __restrict__ x, int T, long long npix, int R, long long span, int fz,
                                                const uint8_t* __restrict__ lab, const int* __restrict__ base,
                                                const RegionMeta* __restrict__ meta, const float* __restrict__ c, float* __restrict__ Xc,
                                                long long ktot, double* __restrict__ psum) {
    __shared__ int run[RG_MAX_R + 1];
    const int lane = threadIdx.x;
    for (int r = lane; r < R; r += 64) run[r + 1] = base[(size_t)blockIdx.x * R + r];
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * span, p1 = min(npix, p0 + span);
    const int t0 = blockIdx.y * fz, t1 = min(T, t0 + fz);
    for (long long g = p0; g < p1; g += 64) {
        const long long p = g + lane;
        const int l = p < p1 ? (int)lab[p] : 0;
        for_each_label(l, [&](int r, int lead, bool mine, unsigned long long mask) {
            const long long dst = region_slot<TT_KC>(meta, run, r, lead, lane, mask);
            for (int t = t0; t < t1; t += TT_U) {
                double ms = 0.0;
#pragma unroll
                for (int u = 0; u < TT_U; ++u) {
                    float v = 0.f;
                    if (mine && t + u < t1) {
                        v = x[(size_t)(t + u) * (size_t)npix + (size_t)p] - c[(size_t)(r - 1) * T + t + u];
                        Xc[(size_t)(t + u) * (size_t)ktot + (size_t)dst] = v;
                    }
                    const double s = wave_sum_all((double)v);
                    if (lane == u) ms = s;
                }
                if (lane < TT_U && t + lane < t1) psum[((size_t)blockIdx.x * R + (r - 1)) * T + t + lane] += ms;
            }
        });
    }
}

// ---- 2b. zeros behind each region's last pixel, up to the end of its last chunk.  grid (R, T)
__global__ void __launch_bounds__(256) k_tt_padzero(const RegionMeta* __restrict__ meta, float* __restrict__ Xc, long long ktot) {
    const int r = blockIdx.x;
    const long long a = (long long)meta->start[r] * TT_KC + meta->N[r], b = (long long)meta->start[r + 1] * TT_KC;
    float* row = Xc + (size_t)blockIdx.y * (size_t)ktot;
    for (long long q = a + threadIdx.x; q < b; q += 256) row[q] = 0.f;
}

// pair index -> frame blocks (bi <= bj <= bi + W), in the order the host counts them
__device__ __forceinline__ void tt_pair(int pair, int nb, int W, int& bi, int& bj) {
    bi = 0;
    for (; bi < nb - 1; ++bi) {
        const int len = min(nb - 1, bi + W) - bi + 1;
        if (pair < len) break;
        pair -= len;
    }
    bj = bi + pair;
}

// ---- 3. product: grid (nchunks * npairs), pair fastest so that the pairs of a chunk run side by side; block 256 = 4 waves in 2 x 2,
// each a 64 x 64 tile (4 accumulators of 16 registers).  part[(chunk * npairs + pair)][128][128] = A_bi A_bj^T over the chunk.
__global__ void __launch_bounds__(256, 2) k_tt_syrk(const float* __restrict__ Xc, long long ktot, int T, int R, int nb, int W, int npairs,
                                                 const RegionMeta* __restrict__ meta, float* __restrict__ part) {
    __shared__ float As[32][129];
    __shared__ float Bs[32][129];
    const int chunk = blockIdx.x / npairs, pair = blockIdx.x % npairs;
    if (chunk >= meta->start[R]) return;
    int bi, bj;
    tt_pair(pair, nb, W, bi, bj);
    const bool diag = bi == bj;
    const WaveTile t = wave_tile(threadIdx.x);
    const int m0 = bi * TT_TILE, n0 = bj * TT_TILE;
    // thread -> (row, 4 consecutive k) of the 128 x 32 stage, four rows 32 apart
    const int srow = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 4;
    const float* col = Xc + (size_t)chunk * TT_KC + sk;
    float4 ra[4], rb[4];
#define TT_FETCH(k0)                                                                                                        \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                         \
        const int ia = m0 + srow + 32 * q, ib = n0 + srow + 32 * q;                                                         \
        ra[q] = make_float4(0.f, 0.f, 0.f, 0.f);                                                                            \
        rb[q] = make_float4(0.f, 0.f, 0.f, 0.f);                                                                            \
        if (ia < T) ra[q] = *reinterpret_cast<const float4*>(col + (size_t)ia * (size_t)ktot + (k0));                       \
        if (!diag && ib < T) rb[q] = *reinterpret_cast<const float4*>(col + (size_t)ib * (size_t)ktot + (k0));              \
    }
    f32x16 acc[2][2], tot[2][2];
    zero(acc);
    zero(tot);
    const float* Bp = diag ? &As[0][0] : &Bs[0][0];
    TT_FETCH(0)
    for (int k0 = 0; k0 < TT_KC; k0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = srow + 32 * q;
            As[sk][row] = ra[q].x;
            As[sk + 1][row] = ra[q].y;
            As[sk + 2][row] = ra[q].z;
            As[sk + 3][row] = ra[q].w;
            if (!diag) {
                Bs[sk][row] = rb[q].x;
                Bs[sk + 1][row] = rb[q].y;
                Bs[sk + 2][row] = rb[q].z;
                Bs[sk + 3][row] = rb[q].w;
            }
        }
        __syncthreads();
        if (k0 + 32 < TT_KC) {
            TT_FETCH(k0 + 32)
        }
        // mma_slab of b4d_mfma.hpp written out: B is read through the flat pointer that selects the A slab on diagonal pairs
#pragma unroll
        for (int kk = 0; kk < 32; kk += 2) {
            const float a0 = As[kk + t.lk][64 * t.wr + t.li], a1 = As[kk + t.lk][64 * t.wr + 32 + t.li];
            const float b0 = Bp[(kk + t.lk) * 129 + 64 * t.wc + t.li], b1 = Bp[(kk + t.lk) * 129 + 64 * t.wc + 32 + t.li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if ((k0 + 32) % TT_RUN == 0) {
            tot[0][0] += acc[0][0], tot[0][1] += acc[0][1], tot[1][0] += acc[1][0], tot[1][1] += acc[1][1];
            zero(acc);
        }
    }
    float* out = part + ((size_t)chunk * npairs + pair) * (TT_TILE * TT_TILE);
    for_each(tot, t, 0, 0, [&](int row, int col, float v) { out[row * TT_TILE + col] = v; });
#undef TT_FETCH
}

// ---- 4a. covariances of the upper triangle inside the band, means and variances.  grid (64, npairs, R), block 256
__global__ void __launch_bounds__(256) k_tt_reduce(const float* __restrict__ part, int T, int R, int nb, int W, int npairs, int L,
                                                   const RegionMeta* __restrict__ meta, const float* __restrict__ c,
                                                   const double* __restrict__ s, double* __restrict__ out, double* __restrict__ mean,
                                                   double* __restrict__ var) {
    const int elem = blockIdx.x * 256 + threadIdx.x, pair = blockIdx.y, r = blockIdx.z;
    int bi, bj;
    tt_pair(pair, nb, W, bi, bj);
    const int i = bi * TT_TILE + (elem >> 7), j = bj * TT_TILE + (elem & 127);
    if (i >= T || j >= T || j < i || j - i > L) return;
    const long long N = meta->N[r];
    double cov = NAN, m = NAN;
    if (N > 0) {
        double G = 0.0;
        for (int ch = meta->start[r]; ch < meta->start[r + 1]; ++ch)
            G += (double)part[((size_t)ch * npairs + pair) * (TT_TILE * TT_TILE) + elem];
        const double n = (double)N, si = s[(size_t)r * T + i] / n, sj = s[(size_t)r * T + j] / n;
        cov = G / n - si * sj;
        m = (double)c[(size_t)r * T + i] + si;
    }
    out[((size_t)r * T + i) * T + j] = cov;
    if (i == j) {
        var[(size_t)r * T + i] = cov;
        mean[(size_t)r * T + i] = m;
    }
}

// ---- 4b. normalisation in place: the upper entry is read, both triangles are written from one value.  grid (ceil(T / 256), T, R)
__global__ void __launch_bounds__(256) k_tt_normalise(double* __restrict__ out, const double* __restrict__ mean,
                                                      const double* __restrict__ var, int T, int L, int norm) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, r = blockIdx.z;
    if (j >= T || j < i) return;
    double* M = out + (size_t)r * T * T;
    double v = NAN;
    if (j - i <= L) {
        const double cov = M[(size_t)i * T + j];
        if (norm == B4D_TWO_TIME_COVARIANCE) {
            v = cov;
        } else if (norm == B4D_TWO_TIME_PEARSON) {
            const double vi = var[(size_t)r * T + i], vj = var[(size_t)r * T + j];
            if (vi > 0.0 && vj > 0.0) v = i == j ? 1.0 : cov / sqrt(vi * vj);
        } else {
            const double d = mean[(size_t)r * T + i] * mean[(size_t)r * T + j];
            if (d > 0.0) v = 1.0 + cov / d;
        }
    }
    M[(size_t)i * T + j] = v;
    M[(size_t)j * T + i] = v;
}

// ---- 5. g2[r][tau] = mean of the diagonal j - i = tau, g2_err = population standard deviation / sqrt(T - tau).
// grid (L + 1, R), block 256; lane sums in index order, then a fixed tree
__global__ void __launch_bounds__(256) k_tt_lags(const double* __restrict__ M, int T, int L, double* __restrict__ g2,
                                                 double* __restrict__ g2_err) {
    __shared__ double sh[256];
    const int tau = blockIdx.x, r = blockIdx.y, n = T - tau;
    const double* D = M + (size_t)r * T * T + tau;
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += D[(size_t)i * (T + 1)];
    const double mu = block_tree_sum256(a, sh, true) / n;
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = D[(size_t)i * (T + 1)] - mu;
        q = fma(d, d, q);
    }
    const double ss = block_tree_sum256(q, sh, false);
    if (threadIdx.x == 0) {
        g2[(size_t)r * (L + 1) + tau] = mu;
        g2_err[(size_t)r * (L + 1) + tau] = sqrt(ss / n) / sqrt((double)n);
    }
}

}  // namespace b4d

using namespace b4d;

extern "C" size_t b4d_two_time_workspace_bytes(int T, long long npix, int n_regions, int max_lag) {
    TTLayout y;
    return tt_layout(T, npix, n_regions, max_lag, y) ? y.bytes : 0;
}

// ev: null, or five events recorded on the stream around the scan, pack, product and reduce stages
static int tt_run(const float* stack, int T, long long npix, const int* labels, int n_regions, int norm, int max_lag, void* workspace,
                  double* two_time, double* mean, double* var, long long* n_pixels, void* stream, hipEvent_t* ev) {
    if (!stack || !workspace || !two_time || !mean || !var || !n_pixels) return fail(B4D_EINVAL, "null argument");
    if (T < 2 || npix < 1 || n_regions < 1) return fail(B4D_EINVAL, "two-time: T >= 2, npix >= 1 and n_regions >= 1");
    if (!labels && n_regions != 1) return fail(B4D_EINVAL, "two-time: without a label map there is one region");
    if (norm < 0 || norm > 2) return fail(B4D_EINVAL, "two-time: norm must be 0 (pearson), 1 (intensity) or 2 (covariance)");
    if (max_lag < 0 || max_lag > T - 1) return fail(B4D_EINVAL, "two-time: max_lag must lie in 0 .. T - 1");
    if (T > TT_MAX_T || n_regions > TT_MAX_R || npix >= (1ll << 31))
        return fail(B4D_ESIZE, "two-time: T <= " + std::to_string(TT_MAX_T) + ", n_regions <= " + std::to_string(TT_MAX_R) +
                                   " and fewer than 2^31 pixels per frame");
    TTLayout y;
    if (!tt_layout(T, npix, n_regions, max_lag, y)) return fail(B4D_ESIZE, "two-time: unsupported shape");
    if (y.nchunks * y.npairs >= (1ll << 31)) return fail(B4D_ESIZE, "two-time: too many (chunk, frame-block pair) tiles for one launch");
    hipStream_t st = (hipStream_t)stream;
    const int R = n_regions, L = max_lag;
    char* w = static_cast<char*>(workspace);
    float* Xc = reinterpret_cast<float*>(w + y.o_xc);
    float* part = reinterpret_cast<float*>(w + y.o_part);
    double* psum = reinterpret_cast<double*>(w + y.o_psum);
    double* pcnt = reinterpret_cast<double*>(w + y.o_pcnt);
    uint8_t* lab = reinterpret_cast<uint8_t*>(w + y.o_lab);
    uint8_t* bad = reinterpret_cast<uint8_t*>(w + y.o_bad);
    int* cnt = reinterpret_cast<int*>(w + y.o_cnt);
    int* base = reinterpret_cast<int*>(w + y.o_base);
    float* c = reinterpret_cast<float*>(w + y.o_c);
    double* s = reinterpret_cast<double*>(w + y.o_s);
    RegionMeta* meta = reinterpret_cast<RegionMeta*>(w + y.o_meta);
    const size_t pbytes = sizeof(double) * (size_t)y.nscan * R * T;

    if (ev) B4D_HIP(hipEventRecord(ev[0], st));
    B4D_HIP(hipMemsetAsync(bad, 0, (size_t)npix, st));
    B4D_HIP(hipMemsetAsync(psum, 0, pbytes, st));
    B4D_HIP(hipMemsetAsync(pcnt, 0, pbytes, st));
    hipLaunchKernelGGL(k_tt_labels, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, labels, npix, R, lab);
    hipLaunchKernelGGL(k_tt_scan, dim3(y.nscan, y.tz), dim3(64), 0, st, stack, T, npix, R, y.span, y.fz, lab, bad, psum, pcnt);
    hipLaunchKernelGGL(k_tt_colsum, dim3(R * T), dim3(64), 0, st, psum, pcnt, y.nscan, R, T, c, s);
    if (ev) B4D_HIP(hipEventRecord(ev[1], st));
    region_list(nullptr, true, bad, npix, R, y.span, y.nscan, TT_KC, lab, cnt, base, meta, n_pixels, st);
    B4D_HIP(hipMemsetAsync(psum, 0, pbytes, st));
    hipLaunchKernelGGL(k_tt_pack, dim3(y.nscan, y.tz), dim3(64), 0, st, stack, T, npix, R, y.span, y.fz, lab, base, meta, c, Xc, y.ktot,
                       psum);
    hipLaunchKernelGGL(k_tt_padzero, dim3(R, T), dim3(256), 0, st, meta, Xc, y.ktot);
    hipLaunchKernelGGL(k_tt_colsum, dim3(R * T), dim3(64), 0, st, psum, (const double*)nullptr, y.nscan, R, T, c, s);
    if (ev) B4D_HIP(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_tt_syrk, dim3((unsigned)(y.nchunks * y.npairs)), dim3(256), 0, st, Xc, y.ktot, T, R, y.nb, y.W, y.npairs, meta,
                       part);
    if (ev) B4D_HIP(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_tt_reduce, dim3(TT_TILE * TT_TILE / 256, y.npairs, R), dim3(256), 0, st, part, T, R, y.nb, y.W, y.npairs, L,
                       meta, c, s, two_time, mean, var);
    hipLaunchKernelGGL(k_tt_normalise, dim3((T + 255) / 256, T, R), dim3(256), 0, st, two_time, mean, var, T, L, norm);
    if (ev) B4D_HIP(hipEventRecord(ev[4], st));
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_two_time(const float* stack, int T, long long npix, const int* labels, int n_regions, int norm, int max_lag,
                            void* workspace, double* two_time, double* mean, double* var, long long* n_pixels, void* stream) {
    return tt_run(stack, T, npix, labels, n_regions, norm, max_lag, workspace, two_time, mean, var, n_pixels, stream, nullptr);
}

extern "C" int b4d_two_time_timed(const float* stack, int T, long long npix, const int* labels, int n_regions, int norm, int max_lag,
                                  void* workspace, double* two_time, double* mean, double* var, long long* n_pixels, void* stream,
                                  float* stage_ms) {
    if (!stage_ms) return fail(B4D_EINVAL, "null argument");
    hipEvent_t ev[5];
    for (auto& e : ev) B4D_HIP(hipEventCreate(&e));
    int rc = tt_run(stack, T, npix, labels, n_regions, norm, max_lag, workspace, two_time, mean, var, n_pixels, stream, ev);
    if (rc == B4D_OK) {
        hipError_t e = hipEventSynchronize(ev[4]);
        for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventElapsedTime(stage_ms + k, ev[k], ev[k + 1]);
        if (e != hipSuccess) rc = fail(B4D_EHIP, std::string("two-time timing: ") + hipGetErrorString(e));
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return rc;
}

extern "C" int b4d_two_time_lags(const double* two_time, int n_regions, int T, int max_lag, double* g2, double* g2_err, void* stream) {
    if (!two_time || !g2 || !g2_err) return fail(B4D_EINVAL, "null argument");
    if (T < 2 || n_regions < 1) return fail(B4D_EINVAL, "two-time lags: T >= 2 and n_regions >= 1");
    if (max_lag < 0 || max_lag > T - 1) return fail(B4D_EINVAL, "two-time lags: max_lag must lie in 0 .. T - 1");
    if (T > TT_MAX_T || n_regions > TT_MAX_R) return fail(B4D_ESIZE, "two-time lags: T <= 2048 and n_regions <= 64");
    hipLaunchKernelGGL(k_tt_lags, dim3(max_lag + 1, n_regions), dim3(256), 0, (hipStream_t)stream, two_time, T, max_lag, g2, g2_err);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
