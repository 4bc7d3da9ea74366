// b4d_rankfilt.hip -- spatial median / rank / percentile filters (scipy.ndimage.median_filter, rank_filter, percentile_filter on
// (batch, ny, nx) float32 frames, frame by frame), the range-only variant behind utils/range.py:14-86 of the reference, the fused
// outlier repair and the uint16 scaling of utils/dtype.py:15-53.
//
// One workgroup per output tile.  The tile and its halo are staged ONCE in LDS as ordered integer keys (b4d_keys.hpp): the
// border rule runs only while the halo of an edge tile is filled, NaN rules cost nothing afterwards, and every compare-exchange
// is an integer min / max.  A rank filter is a selection, so on finite input the output is bit-identical to SciPy's.
//   register route: median of 3 x 3 / 5 x 5 / 7 x 7; a lane produces four outputs adjacent in x from S rows of twelve keys
//   general route : any sy x sx <= 15 x 15 and any rank, by 32 counting passes over the window in LDS (select_bitwise)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_reduce.hpp"
#include "b4d_rankfilt.hpp"

namespace b4d {
using namespace rankfilt;

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// register route: 128 x 32 outputs per workgroup, 32 lanes x 4 outputs across, 8 lane rows x 4 passes down; the halo in x is padded
// to 4 so that a lane's twelve keys of a row are three aligned 16-byte LDS reads
constexpr int RF_TX = 128, RF_TY = 32, RF_PAD = 4, RF_LW = RF_TX + 2 * RF_PAD;
// general route: 64 x 16 outputs per workgroup, halo up to 7 (padded to 8) each side
constexpr int GN_TX = 64, GN_TY = 16, GN_PAD = 8, GN_LW = GN_TX + 2 * GN_PAD, GN_ROWS = GN_TY + 14;

// keys of frame rows y0 - ylo + [0, rows) and columns x0 - PAD + 4 * [g0, g1) into lds (row pitch LW); 16-byte loads for groups
// of four that lie inside an aligned row, the border rule element by element for the others.  Two phases, both unrolled over the
// MAXIT groups a lane can own (rows * (g1 - g0) <= 256 * MAXIT): every load is issued before the first value is used, so a
// workgroup has its whole tile in flight at once instead of one 16-byte load per lane at a time.
template <int LW, int PAD, int MAXIT>
__device__ __forceinline__ void fill_tile(uint32_t* __restrict__ lds, const float* __restrict__ f, int ny, int nx, int x0, int y0, int ylo,
                                          int rows, int g0, int g1, int mode, float cval, bool vec) {
    const int ng = g1 - g0, total = rows * ng;
    v4f q[MAXIT];
    int at[MAXIT];
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int idx = threadIdx.x + 256 * it;
        q[it] = v4f{cval, cval, cval, cval};
        at[it] = -1;
        if (idx < total) {
            const int j = idx / ng, g = g0 + idx - j * ng;
            const int yy = border_index(y0 - ylo + j, ny, mode);
            const int xb = x0 - PAD + 4 * g;
            at[it] = j * LW + 4 * g;
            if (yy >= 0) {
                const float* row = f + (size_t)yy * nx;
                if (vec && xb >= 0 && xb + 3 < nx) {
                    q[it] = *reinterpret_cast<const v4f*>(row + xb);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int xx = border_index(xb + e, nx, mode);
                        if (xx >= 0) q[it][e] = row[xx];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < MAXIT; ++it)
        if (at[it] >= 0) *reinterpret_cast<v4u*>(lds + at[it]) = v4u{to_key(q[it][0]), to_key(q[it][1]), to_key(q[it][2]), to_key(q[it][3])};
}

// the S rows x 12 keys that hold the windows of a lane's four outputs (output c: columns 4 + c - S/2 .. 4 + c + S/2)
template <int S>
__device__ __forceinline__ void load_window(const uint32_t* __restrict__ lds, int ly, int tx, uint32_t (&w)[S][12]) {
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const v4u t = *reinterpret_cast<const v4u*>(lds + (ly + j) * RF_LW + 4 * tx + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[j][4 * q + e] = t[e];
        }
}

// medians of the four windows: the S + 3 columns they span are sorted once (w's columns are left sorted: the same multiset) and
// every window selects from its S sorted columns (b4d_rankfilt.hpp)
template <int S>
__device__ __forceinline__ void medians4(uint32_t (&w)[S][12], uint32_t (&med)[4]) {
    constexpr int R = S / 2;
    if constexpr (S == 3) {
#pragma unroll
        for (int c = 3; c < 9; ++c) sort3<KeyOps>(w[0][c], w[1][c], w[2][c]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            med[c] = median9_sorted_cols<KeyOps>(w[0][c + 3], w[1][c + 3], w[2][c + 3], w[0][c + 4], w[1][c + 4], w[2][c + 4], w[0][c + 5],
                                                 w[1][c + 5], w[2][c + 5]);
    } else {
#pragma unroll
        for (int c = 4 - R; c < 8 + R; ++c) {
            uint32_t col[S];
#pragma unroll
            for (int j = 0; j < S; ++j) col[j] = w[j][c];
            sort_small<KeyOps, S>(col);
#pragma unroll
            for (int j = 0; j < S; ++j) w[j][c] = col[j];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t cols[S][S];
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j) cols[i][j] = w[j][4 + c - R + i];
            med[c] = median_sorted_cols<KeyOps, S>(cols);
        }
    }
}

// per-workgroup NaN-aware range of the filtered keys -> integer atomics on the frame's key pair (deterministic: min / max of integers).
// In-wave exchange first, one LDS atomic pair per wave, and one device atomic pair per workgroup -- skipped where the pair in memory
// is already as wide: the pair only ever widens, so a stale read costs an atomic and never loses one (a frame's workgroups would
// otherwise queue a thousand atomics on one line).
__device__ __forceinline__ void reduce_range(uint32_t kmin, uint32_t kmax, uint32_t* s_mm, uint32_t* __restrict__ mm_frame) {
    kmin = wave_min_all(kmin);
    kmax = wave_max_all(kmax);
    // (no block reduction of b4d_reduce.hpp behind it: the waves meet in integer atomics, whose order does not matter)
    if ((threadIdx.x & 63) == 0 && kmin <= kmax) {
        atomicMin(&s_mm[0], kmin);
        atomicMax(&s_mm[1], kmax);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_mm[0] <= s_mm[1]) {
        if (s_mm[0] < __hip_atomic_load(mm_frame, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(mm_frame, s_mm[0]);
        if (s_mm[1] > __hip_atomic_load(mm_frame + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mm_frame + 1, s_mm[1]);
    }
}

// grid (ceil(nx / 128), ceil(ny / 32), frames); out and / or mm (frames x 2 keys, see k_range_init) may be null
template <int S>
__global__ void __launch_bounds__(256) k_median_reg(const float* __restrict__ in, int ny, int nx, int mode, float cval, float* __restrict__ out,
                                                    uint32_t* __restrict__ mm, int vec_in, int vec_out) {
    constexpr int R = S / 2;
    __shared__ __attribute__((aligned(16))) uint32_t lds[(RF_TY + 2 * R) * RF_LW];
    __shared__ uint32_t s_mm[2];
    const int x0 = blockIdx.x * RF_TX, y0 = blockIdx.y * RF_TY;
    const size_t fo = (size_t)blockIdx.z * ny * nx;
    const int th = min(RF_TY, ny - y0);
    if (threadIdx.x == 0) {
        s_mm[0] = 0xFFFFFFFFu;
        s_mm[1] = 0u;
    }
    fill_tile<RF_LW, RF_PAD, ((RF_TY + 2 * R) * (RF_LW / 4) + 255) / 256>(lds, in + fo, ny, nx, x0, y0, R, th + 2 * R, 0, RF_LW / 4, mode, cval, vec_in != 0);
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ox = x0 + 4 * tx;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    if (ox < nx) {
        for (int ly = ty; ly < th; ly += 8) {
            uint32_t w[S][12], med[4];
            load_window<S>(lds, ly, tx, w);
            medians4<S>(w, med);
            if (out)
                store4(out + fo + (size_t)(y0 + ly) * nx + ox, v4f{from_key(med[0]), from_key(med[1]), from_key(med[2]), from_key(med[3])}, nx - ox,
                       vec_out != 0, true);
            if (mm) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (ox + c < nx && med[c] != KEY_NAN) {
                        kmin = min(kmin, med[c]);
                        kmax = max(kmax, med[c]);
                    }
            }
        }
    }
    if (mm) reduce_range(kmin, kmax, s_mm, mm + 2 * (size_t)blockIdx.z);
}

// grid (ceil(nx / 64), ceil(ny / 16), frames): one output per lane and pass, rank-th smallest of the sy x sx window by counting
__global__ void __launch_bounds__(256) k_rank_general(const float* __restrict__ in, int ny, int nx, int sy, int sx, int rank, int mode,
                                                      float cval, float* __restrict__ out, uint32_t* __restrict__ mm, int vec_in) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[GN_ROWS * GN_LW];
    __shared__ uint32_t s_mm[2];
    const int x0 = blockIdx.x * GN_TX, y0 = blockIdx.y * GN_TY;
    const size_t fo = (size_t)blockIdx.z * ny * nx;
    const int th = min(GN_TY, ny - y0);
    const int ylo = sy / 2, xlo = sx / 2, xhi = sx - 1 - xlo;   // SciPy's placement: offsets -(size / 2) .. size - 1 - size / 2
    if (threadIdx.x == 0) {
        s_mm[0] = 0xFFFFFFFFu;
        s_mm[1] = 0u;
    }
    fill_tile<GN_LW, GN_PAD, (GN_ROWS * (GN_LW / 4) + 255) / 256>(lds, in + fo, ny, nx, x0, y0, ylo, th + sy - 1, (GN_PAD - xlo) / 4,
                                                                  (GN_PAD + GN_TX + xhi + 3) / 4, mode, cval, vec_in != 0);
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int ox = x0 + tx;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    if (ox < nx) {
        for (int ly = ty; ly < th; ly += 4) {
            const uint32_t* base = lds + ly * GN_LW + GN_PAD + tx - xlo;
            const uint32_t k = select_bitwise(rank, [&](uint32_t t) {
                int c = 0;
                for (int j = 0; j < sy; ++j)
                    for (int i = 0; i < sx; ++i) c += base[j * GN_LW + i] < t ? 1 : 0;
                return c;
            });
            if (out) out[fo + (size_t)(y0 + ly) * nx + ox] = from_key(k);
            if (k != KEY_NAN) {
                kmin = min(kmin, k);
                kmax = max(kmax, k);
            }
        }
    }
    if (mm) reduce_range(kmin, kmax, s_mm, mm + 2 * (size_t)blockIdx.z);
}

// the (frames, 2) float32 range array holds keys while the filter runs: {all ones, 0} = nothing seen yet
__global__ void __launch_bounds__(256) k_range_init(uint32_t* __restrict__ mm, int frames) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < frames) {
        mm[2 * i] = 0xFFFFFFFFu;
        mm[2 * i + 1] = 0u;
    }
}
// keys -> float32 in place; NaN for a frame whose filtered values are all NaN
__global__ void __launch_bounds__(256) k_range_final(uint32_t* __restrict__ mm, int frames) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < frames) {
        const uint32_t lo = mm[2 * i], hi = mm[2 * i + 1];
        const bool none = lo > hi;
        mm[2 * i] = none ? 0x7FC00000u : float_bits(from_key(lo));
        mm[2 * i + 1] = none ? 0x7FC00000u : float_bits(from_key(hi));
    }
}

// out = median where the centre pixel is an outlier (the rule of b4d_keys.hpp against the window's median and, for the mad scale
// only, the window's MAD), else the pixel: one read of the frame, one write.
template <int S>
__global__ void __launch_bounds__(256) k_despeckle(const float* __restrict__ in, int ny, int nx, int mode, float cval, float* __restrict__ out,
                                                   unsigned char* __restrict__ mask, unsigned long long* __restrict__ counts, OutlierRule a,
                                                   int vec_in, int vec_out, int vec_mask) {
    constexpr int R = S / 2;
    __shared__ __attribute__((aligned(16))) uint32_t lds[(RF_TY + 2 * R) * RF_LW];
    __shared__ unsigned s_cnt;
    const int x0 = blockIdx.x * RF_TX, y0 = blockIdx.y * RF_TY;
    const size_t fo = (size_t)blockIdx.z * ny * nx;
    const int th = min(RF_TY, ny - y0);
    if (threadIdx.x == 0) s_cnt = 0u;
    fill_tile<RF_LW, RF_PAD, ((RF_TY + 2 * R) * (RF_LW / 4) + 255) / 256>(lds, in + fo, ny, nx, x0, y0, R, th + 2 * R, 0, RF_LW / 4, mode, cval, vec_in != 0);
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ox = x0 + 4 * tx;
    unsigned cnt = 0u;
    if (ox < nx) {
        for (int ly = ty; ly < th; ly += 8) {
            uint32_t w[S][12], med[4];
            float x[4], res[4];
            unsigned char flag[4];
            load_window<S>(lds, ly, tx, w);
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = from_key(w[R][4 + c]);
            medians4<S>(w, med);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float m = from_key(med[c]);
                float mad = 0.f;
                if (a.scale_kind == 1) {
                    uint32_t v[S * S];
#pragma unroll
                    for (int j = 0; j < S; ++j)
#pragma unroll
                        for (int i = 0; i < S; ++i) v[j * S + i] = to_key(fabsf(__fsub_rn(from_key(w[j][4 + c - R + i]), m)));
                    mad = from_key(median_forgetful<KeyOps, S * S>(v));
                }
                const bool o = outlier_rejected(a, x[c], m, outlier_rhs(a, m, mad));
                res[c] = o ? m : x[c];
                flag[c] = o ? 1 : 0;
                if (ox + c < nx) cnt += flag[c];
            }
            const size_t po = fo + (size_t)(y0 + ly) * nx + ox;
            store4(out + po, v4f{res[0], res[1], res[2], res[3]}, nx - ox, vec_out != 0, true);
            if (mask) store4(mask + po, flag, nx - ox, vec_mask != 0);
        }
    }
    if (counts) {
        cnt = wave_sum_all(cnt);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (threadIdx.x == 0 && s_cnt) atomicAdd(counts + blockIdx.z, (unsigned long long)s_cnt);
    }
}

// utils/dtype.py:48-53: x = in - vmin; x *= inv (in float64 rounded once to float32 when mul_f64, as NumPy multiplies a float32
// array by a float64 scalar into a float32 output; else in float32); clip to [0, 65535]; truncate.  NaN -> 0 (our definition).
__device__ __forceinline__ unsigned short scale_u16(float v, float vmin, double inv, float invf, int mul_f64) {
    const float x = __fsub_rn(v, vmin);
    float y = mul_f64 ? (float)((double)x * inv) : __fmul_rn(x, invf);
    if (!(y > 0.f)) y = 0.f;   // NaN and negatives
    if (y > 65535.f) y = 65535.f;
    return (unsigned short)y;
}
__global__ void __launch_bounds__(256) k_scale_u16(const float* __restrict__ in, size_t n, float vmin, double inv, int mul_f64,
                                                   unsigned short* __restrict__ out) {
    const float invf = (float)inv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = scale_u16(in[i], vmin, inv, invf, mul_f64);
}
// four elements per lane: 16 bytes in, 8 out; in 16-byte and out 8-byte aligned
__global__ void __launch_bounds__(256) k_scale_u16_vec(const float* __restrict__ in, size_t nvec, float vmin, double inv, int mul_f64,
                                                       unsigned short* __restrict__ out) {
    typedef unsigned short v4h __attribute__((ext_vector_type(4)));
    const float invf = (float)inv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const v4f q = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(in) + i);
        v4h r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = scale_u16(q[e], vmin, inv, invf, mul_f64);
        __builtin_nontemporal_store(r, reinterpret_cast<v4h*>(out) + i);
    }
}

static dim3 rf_grid(int ny, int nx, int frames) { return dim3((nx + RF_TX - 1) / RF_TX, (ny + RF_TY - 1) / RF_TY, frames); }
// the register-route kernel of window size 3, 5 or 7
template <class... A>
static int launch_median_reg(int size, dim3 grid, hipStream_t st, const A&... args) {
    if (size == 3) return launch(k_median_reg<3>, grid, dim3(256), 0, st, args...);
    if (size == 5) return launch(k_median_reg<5>, grid, dim3(256), 0, st, args...);
    return launch(k_median_reg<7>, grid, dim3(256), 0, st, args...);
}
template <class... A>
static int launch_despeckle(int size, dim3 grid, hipStream_t st, const A&... args) {
    if (size == 3) return launch(k_despeckle<3>, grid, dim3(256), 0, st, args...);
    if (size == 5) return launch(k_despeckle<5>, grid, dim3(256), 0, st, args...);
    return launch(k_despeckle<7>, grid, dim3(256), 0, st, args...);
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_rank_filter(const float* in, int batch, int ny, int nx, int size_y, int size_x, int rank, int mode, float cval, int flags,
                               float* out, float* minmax, void* stream) {
    if (const int rc = check_stack("b4d_rank_filter", "null input or empty shape", in, batch, ny, nx, mode, false)) return rc;
    if (size_y < 1 || size_y > 15 || size_x < 1 || size_x > 15) return fail(B4D_EINVAL, "b4d_rank_filter: window sizes must be in 1 .. 15");
    if (rank < 0 || rank >= size_y * size_x) return fail(B4D_EINVAL, "b4d_rank_filter: rank must be in [0, size_y * size_x)");
    if (!out && !minmax) return fail(B4D_EINVAL, "b4d_rank_filter: out and minmax are both null");
    const size_t fpix = (size_t)ny * nx, bytes = fpix * batch * sizeof(float);
    if (ranges_overlap(in, bytes, out, bytes) || ranges_overlap(in, bytes, minmax, 8 * (size_t)batch) || ranges_overlap(out, bytes, minmax, 8 * (size_t)batch))
        return fail(B4D_EINVAL, "b4d_rank_filter: in, out and minmax must not overlap");
    if ((ny + GN_TY - 1) / GN_TY > 65535) return fail(B4D_ESIZE, "b4d_rank_filter: more than 65535 row tiles");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* mm = reinterpret_cast<uint32_t*>(minmax);
    const int vec_in = vec_ok(in, nx, 16), vec_out = vec_ok(out, nx, 16);
    const bool reg = !(flags & 1) && size_y == size_x && (size_y == 3 || size_y == 5 || size_y == 7) && rank == size_y * size_x / 2;
    if (mm)
        if (const int rc = launch(k_range_init, dim3((batch + 255) / 256), dim3(256), 0, st, mm, batch)) return rc;
    const int rc = for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        const float* pin = in + fpix * b0;
        float* pout = out ? out + fpix * b0 : nullptr;
        uint32_t* pmm = mm ? mm + 2 * (size_t)b0 : nullptr;
        if (reg) return launch_median_reg(size_y, rf_grid(ny, nx, nb), st, pin, ny, nx, mode, cval, pout, pmm, vec_in, vec_out);
        return launch(k_rank_general, dim3((nx + GN_TX - 1) / GN_TX, (ny + GN_TY - 1) / GN_TY, nb), dim3(256), 0, st, pin, ny, nx, size_y, size_x, rank,
                      mode, cval, pout, pmm, vec_in);
    });
    if (rc || !mm) return rc;
    return launch(k_range_final, dim3((batch + 255) / 256), dim3(256), 0, st, mm, batch);
}

extern "C" int b4d_despeckle(const float* in, int batch, int ny, int nx, int size, int scale_kind, float threshold, float min_scale, int polarity,
                             int mode, float cval, float* out, unsigned char* mask, long long* counts, void* stream) {
    if (const int rc = check_stack("b4d_despeckle", "null frames or empty shape", in && out, batch, ny, nx, mode, false)) return rc;
    if (size != 3 && size != 5 && size != 7) return fail(B4D_EINVAL, "b4d_despeckle: size must be 3, 5 or 7");
    if (scale_kind < 0 || scale_kind > 2 || polarity < 0 || polarity > 2) return fail(B4D_EINVAL, "b4d_despeckle: scale_kind / polarity must be 0, 1 or 2");
    if (!(threshold >= 0.f) || !(min_scale >= 0.f)) return fail(B4D_EINVAL, "b4d_despeckle: threshold and min_scale must be >= 0");
    const size_t fpix = (size_t)ny * nx, npix = fpix * batch, bytes = npix * sizeof(float);
    if (ranges_overlap(in, bytes, out, bytes) || ranges_overlap(in, bytes, mask, npix) || ranges_overlap(out, bytes, mask, npix) ||
        ranges_overlap(in, bytes, counts, 8 * (size_t)batch) || ranges_overlap(out, bytes, counts, 8 * (size_t)batch))
        return fail(B4D_EINVAL, "b4d_despeckle: buffers must not overlap");
    if ((ny + RF_TY - 1) / RF_TY > 65535) return fail(B4D_ESIZE, "b4d_despeckle: more than 65535 row tiles");
    hipStream_t st = (hipStream_t)stream;
    const OutlierRule a = make_outlier_rule(scale_kind, threshold, min_scale, polarity);
    const int vec_in = vec_ok(in, nx, 16), vec_out = vec_ok(out, nx, 16), vec_mask = vec_ok(mask, nx, 4);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (cnt) B4D_HIP(hipMemsetAsync(cnt, 0, 8 * (size_t)batch, st));
    return for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        return launch_despeckle(size, rf_grid(ny, nx, nb), st, in + fpix * b0, ny, nx, mode, cval, out + fpix * b0, mask ? mask + fpix * b0 : nullptr,
                                cnt ? cnt + b0 : nullptr, a, vec_in, vec_out, vec_mask);
    });
}

extern "C" int b4d_scale_to_u16(const float* in, size_t n, float vmin, double inv, int mul_f64, unsigned short* out, void* stream) {
    if (!in || !out || n < 1) return fail(B4D_EINVAL, "b4d_scale_to_u16: bad argument");
    if (ranges_overlap(in, n * sizeof(float), out, n * sizeof(unsigned short))) return fail(B4D_EINVAL, "b4d_scale_to_u16: in and out must not overlap");
    hipStream_t st = (hipStream_t)stream;
    size_t done = 0;
    if (ptr_aligned(in, 16) && ptr_aligned(out, 8) && n >= 4) {
        const size_t nvec = n / 4;
        if (const int rc = launch(k_scale_u16_vec, dim3((unsigned)std::min<size_t>((nvec + 255) / 256, 65535)), dim3(256), 0, st, in, nvec, vmin, inv, mul_f64, out))
            return rc;
        done = nvec * 4;
    }
    if (done < n)
        return launch(k_scale_u16, dim3((unsigned)std::min<size_t>((n - done + 255) / 256, 65535)), dim3(256), 0, st, in + done, n - done, vmin, inv, mul_f64,
                      out + done);
    return B4D_OK;
}
