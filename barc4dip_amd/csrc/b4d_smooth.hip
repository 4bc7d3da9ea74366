// b4d_smooth.hip -- linear separable filters (scipy.ndimage.correlate1d along x, then along y, on every frame of a (batch, ny, nx)
// float32 stack: Gaussian and box filters, their high-pass and envelope-division forms) and per-pixel windowed mean / variance /
// contrast in float64.
//
// The taps travel in the kernel arguments: the runtime copies them when the launch is queued, so a later call -- on this stream or
// on another -- can never overwrite the taps of a launch that has not run yet, and nothing waits for a host-to-device copy.
//   fused route   : half-widths <= SM_FUSED_HALF (4); one launch; tile + halo in LDS, row pass LDS -> LDS, column pass LDS -> registers
//   two-pass route: any window up to 511 taps; a row kernel writes the intermediate to the per-stream scratch buffer, a column
//                   kernel writes the output.  A lane produces 8 consecutive outputs along the filter axis from a register window
//                   of 16 samples: one 16-byte LDS read feeds 32 (rows) or 128 (columns: four columns wide) FMAs.
// Both routes add the products of one output in ascending tap order, so they give the same bits.
// The stager of all four kernels (`stage`, with the NoSwz layout) and the core of k_local_stats -- taps, LDS layout, row pass; the column
// pass by its contract, in loops of this kernel's own -- are b4d_window.hpp's, shared with k_ssim of b4d_perceptual.hip; Swz and Pair, the layouts of the separable kernels, stay here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_tile.hpp"
#include "b4d_window.hpp"

namespace b4d {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int SM_MAX_TAPS = 511;
// largest half-width on the fused route (A/B of both routes on 2048 x 2048 frames)
constexpr int SM_FUSED_HALF = 4;
constexpr int SM_FUSED_TAPS = 2 * SM_FUSED_HALF + 1;
// what the fused kernel can hold (flags bit 1 takes it that far, for the A/B of the boundary): half-widths up to 24
constexpr int SM_FUSED_CAP = 49, SM_FUSED_PAD = 56;
// row kernel: 512 x 8 outputs per workgroup, 64 lanes x 8 outputs across, 4 lane rows x 2 rows each (packed FMAs on row pairs)
constexpr int SR_TX = 512, SR_TY = 8;
// column kernel: 32 x 256 outputs per workgroup, 8 lanes x 4 columns across, 32 lane rows x 8 outputs down; row pitch 36: the
// lanes of a 16-byte LDS read (8 across, lane rows 8 x 36 words apart) fall on different banks
constexpr int SC_TX = 32, SC_TY = 256, SC_PITCH = SC_TX + 4;
// fused kernel: 64 x 64 outputs per workgroup; the row pass gives 8 outputs across per lane, the column pass 4 columns x 4 rows
constexpr int SF_T = 64, SF_PITCH_B = SF_T + 4;

struct Taps {   // one axis, float32, zero beyond n (never multiplied: 0 * NaN would widen a NaN's footprint)
    int n;
    float w[SM_MAX_TAPS + 1];
};
struct TapsFused {
    int ny, nx;
    float wy[SM_FUSED_PAD], wx[SM_FUSED_PAD];
};
struct Frame {   // what every kernel needs of the call
    const float* in;
    float* out;
    int ny, nx, tiles_x, mode;
    float cval;
    int vec_in, vec_out, epi;
    float eps;
};

constexpr int up8(int n) { return (n + 7) & ~7; }

// Where sample (row j, column c) of a staged tile lives in LDS (NoSwz, plain rows: b4d_window.hpp).
// Swz: rows of 8-output lanes that read 16 bytes at a time: four words of padding behind every 128 columns, so that lanes 16 apart
//   (128 words: the same bank without it) meet on one bank less often.  Monotonic; an aligned group of eight stays adjacent.
//   A row of w columns takes swz_width(w) words.
// Pair: rows 2 i and 2 i + 1 interleaved sample by sample ({a0, b0, a1, b1, ..}: a 16-byte read is two columns of both rows, the
//   operands of two packed FMAs), with four words of padding behind every 64 words: the sixteen lanes of a 16-byte read, 16 words
//   apart, then fall on sixteen different bank groups.  `pitch` is that of a row pair, pair_width(w) words for w columns.
struct Swz {
    __device__ static __forceinline__ int col(int c) { return c + ((c >> 7) << 2); }
    __device__ static __forceinline__ int at(int j, int c, int pitch) { return j * pitch + col(c); }
};
struct Pair {
    __device__ static __forceinline__ int col(int c2) { return c2 + ((c2 >> 6) << 2); }
    __device__ static __forceinline__ int at(int j, int c, int pitch) { return (j >> 1) * pitch + col(2 * c) + (j & 1); }
};
constexpr int swz_width(int w) { return w + ((w >> 7) << 2) + 4; }
constexpr int pair_width(int w) { return 2 * w + ((2 * w >> 6) << 2) + 4; }

// ---------------------------------------------------------------------------------------------- register windows
// A lane's R outputs along the filter axis, acc[j] = sum_k w[k] * s[j + k] with k ascending, from a window of 2 R samples in
// registers: R taps are R * R FMAs on the halves lo, hi (acc[j] += w[c] * s[c + j]); then hi takes lo's place and R new samples
// are read -- the loop is unrolled twice with the halves' roles swapped, so no sample is moved between registers.  A sample V is
// one float, two (the same column of two rows) or four (four columns of a row): pairs are packed FMAs, whose rate is the float32
// vector peak; a scalar FMA's is half of it.  load(o, v) reads samples o .. o + R - 1; samples up to upR(n) + R - 1 are read, and
// what lies beyond the window is never used.  The last, partial group of taps runs under uniform branches: a padding tap is never
// multiplied.  The sum starts from -0, which leaves a single product as it is, the sign of a zero included.
__device__ __forceinline__ float fma_w(float w, float s, float a) { return fmaf(w, s, a); }
__device__ __forceinline__ v2f fma_w(float w, v2f s, v2f a) { return __builtin_elementwise_fma(v2f{w, w}, s, a); }
__device__ __forceinline__ v4f fma_w(float w, v4f s, v4f a) {
    const v2f l = fma_w(w, v2f{s[0], s[1]}, v2f{a[0], a[1]}), h = fma_w(w, v2f{s[2], s[3]}, v2f{a[2], a[3]});
    return v4f{l[0], l[1], h[0], h[1]};
}
template <int R, bool TAIL, class V>
__device__ __forceinline__ void window_taps(const float* __restrict__ w, int rem, const V (&lo)[R], const V (&hi)[R], V (&acc)[R]) {
#pragma unroll
    for (int c = 0; c < R; ++c) {
        if (!TAIL || c < rem) {
            const float wc = w[c];
#pragma unroll
            for (int j = 0; j < R; ++j) acc[j] = fma_w(wc, c + j < R ? lo[c + j] : hi[c + j - R], acc[j]);
        }
    }
}
template <int R, class V, class Load>
__device__ __forceinline__ void window_conv(Load load, const float* __restrict__ w, int n, V (&acc)[R]) {
    V a[R], b[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = -0.f;
    const int nfull = n / R, rem = n % R;
    load(0, a);
    int i = 0;
    for (; i + 2 <= nfull; i += 2) {
        load(R * i + R, b);
        window_taps<R, false>(w + R * i, 0, a, b, acc);
        load(R * i + 2 * R, a);
        window_taps<R, false>(w + R * i + R, 0, b, a, acc);
    }
    if (i < nfull) {
        load(R * i + R, b);
        window_taps<R, false>(w + R * i, 0, a, b, acc);
        ++i;
        if (rem) {
            load(R * i + R, a);
            window_taps<R, true>(w + R * i, rem, b, a, acc);
        }
    } else if (rem) {
        load(R * i + R, b);
        window_taps<R, true>(w + R * i, rem, a, b, acc);
    }
}
// columns c .. c + 7 of a Swz row (c a multiple of 8: they share one group of 128)
__device__ __forceinline__ void load_x8(const float* __restrict__ row, int c, float (&v)[8]) {
    const int s = Swz::col(c);
    const v4f a = *reinterpret_cast<const v4f*>(row + s), b = *reinterpret_cast<const v4f*>(row + s + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = a[e];
        v[4 + e] = b[e];
    }
}
// columns c .. c + 7 of both rows of a Pair row pair (c a multiple of 8: the sixteen words share one group of 64)
__device__ __forceinline__ void load_x8x2(const float* __restrict__ prow, int c, v2f (&v)[8]) {
    const int s = Pair::col(2 * c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4f t = *reinterpret_cast<const v4f*>(prow + s + 4 * q);
        v[2 * q] = v2f{t[0], t[1]};
        v[2 * q + 1] = v2f{t[2], t[3]};
    }
}
// four columns of rows r .. r + R - 1
template <int R>
__device__ __forceinline__ void load_y(const float* __restrict__ p, int pitch, int r, v4f (&v)[R]) {
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = *reinterpret_cast<const v4f*>(p + (r + j) * pitch);
}

// 0: g   1: x - g   2: x / max(g, eps), max as np.maximum: a NaN g stays NaN
__device__ __forceinline__ float epilogue(int epi, float g, float x, float eps) {
    if (epi == 1) return __fsub_rn(x, g);
    if (epi == 2) return __fdiv_rn(x, g != g ? g : fmaxf(g, eps));
    return g;
}

// ---------------------------------------------------------------------------------------------- two-pass route
// grid (tiles_x * tiles_y, frames); dynamic LDS SR_TY / 2 row pairs of pitch pair_width(SR_TX + up8(n)).  A lane filters 8 outputs of
// two rows.  epi is applied when this is the only pass (-1: this is the first of two: plain stores, the intermediate is read again).
__global__ void __launch_bounds__(256) k_smooth_row(Frame a, Taps t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = t.n, lo = n / 2, pitch = pair_width(SR_TX + up8(n));
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * SR_TX, y0 = tile_y * SR_TY;
    const size_t fo = (size_t)blockIdx.y * a.ny * a.nx;
    const int tw = min(SR_TX, a.nx - x0), th = min(SR_TY, a.ny - y0);
    stage<Pair>(lds, pitch, a.in + fo, a.ny, a.nx, y0, th, x0 - lo, tw + n - 1, a.mode, a.cval, a.vec_in != 0, threadIdx.x);
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = 2 * (threadIdx.x >> 6), ox = x0 + 8 * lx;
    if (ox >= a.nx || ly >= th) return;
    v2f acc[8];
    const float* prow = lds + (ly >> 1) * pitch;
    window_conv<8>([&](int o, v2f(&v)[8]) { load_x8x2(prow, 8 * lx + o, v); }, t.w, n, acc);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (ly + r < th) {
            float g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = acc[j][r];
            if (a.epi > 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) g[j] = epilogue(a.epi, g[j], lds[Pair::at(ly + r, 8 * lx + lo + j, pitch)], a.eps);
            }
            float* o = a.out + fo + (size_t)(y0 + ly + r) * a.nx + ox;
            store4(o, v4f{g[0], g[1], g[2], g[3]}, a.nx - ox, a.vec_out != 0, a.epi >= 0);
            if (ox + 4 < a.nx) store4(o + 4, v4f{g[4], g[5], g[6], g[7]}, a.nx - ox - 4, a.vec_out != 0, a.epi >= 0);
        }
    }
}

// grid (tiles_x * tiles_y, frames); dynamic LDS (SC_TY + up8(n)) rows of pitch SC_PITCH.  a.in is what this pass filters (the
// intermediate, or the frames when the x axis is the identity), xin the frames for the epilogue.
__global__ void __launch_bounds__(256) k_smooth_col(Frame a, const float* __restrict__ xin, int vec_x, Taps t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = t.n, lo = n / 2;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * SC_TX, y0 = tile_y * SC_TY;
    const size_t fo = (size_t)blockIdx.y * a.ny * a.nx;
    const int tw = min(SC_TX, a.nx - x0), th = min(SC_TY, a.ny - y0);
    stage<NoSwz>(lds, SC_PITCH, a.in + fo, a.ny, a.nx, y0 - lo, th + n - 1, x0, tw, a.mode, a.cval, a.vec_in != 0, threadIdx.x);
    __syncthreads();
    const int lx = threadIdx.x & 7, r0 = 8 * (threadIdx.x >> 3), ox = x0 + 4 * lx;
    if (ox >= a.nx || r0 >= th) return;
    v4f acc[8];
    const float* col = lds + r0 * SC_PITCH + 4 * lx;
    window_conv<8>([&](int o, v4f(&v)[8]) { load_y<8>(col, SC_PITCH, o, v); }, t.w, n, acc);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (r0 + j < th) {
            const size_t po = fo + (size_t)(y0 + r0 + j) * a.nx + ox;
            if (a.epi) {
                v4f x = v4f{0.f, 0.f, 0.f, 0.f};
                if (vec_x && ox + 3 < a.nx) {
                    x = *reinterpret_cast<const v4f*>(xin + po);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (ox + e < a.nx) x[e] = xin[po + e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = epilogue(a.epi, acc[j][e], x[e], a.eps);
            }
            store4(a.out + po, acc[j], a.nx - ox, a.vec_out != 0, true);
        }
    }
}

// ---------------------------------------------------------------------------------------------- fused route
// grid (tiles_x * tiles_y, frames).  LDS: A, the tile with its halo (SF_T + up4(ny) rows of pitch swz_width(SF_T + up8(nx)), swizzled), and
// B, its rows filtered along x (as many rows of pitch SF_PITCH_B).  A row of B that lies outside the frame under "constant" is
// cval, as the border rule of the column pass sees the intermediate, not the frame.
__global__ void __launch_bounds__(256) k_smooth_fused(Frame a, TapsFused t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ny_t = t.ny, nx_t = t.nx, loy = ny_t / 2, lox = nx_t / 2;
    const int pitch_a = swz_width(SF_T + up8(nx_t)), rows = SF_T + up4(ny_t);
    float* A = lds;
    float* B = lds + rows * pitch_a;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * SF_T, y0 = tile_y * SF_T;
    const size_t fo = (size_t)blockIdx.y * a.ny * a.nx;
    const int tw = min(SF_T, a.nx - x0), th = min(SF_T, a.ny - y0);
    const int ha = th + ny_t - 1;
    stage<Swz>(A, pitch_a, a.in + fo, a.ny, a.nx, y0 - loy, ha, x0 - lox, tw + nx_t - 1, a.mode, a.cval, a.vec_in != 0, threadIdx.x);
    __syncthreads();
    const bool id_x = nx_t == 1 && t.wx[0] == 1.f, id_y = ny_t == 1 && t.wy[0] == 1.f;
    for (int idx = threadIdx.x; idx < ha * (SF_T / 8); idx += 256) {
        const int r = idx >> 3, lx = idx & 7;
        const float* row = A + r * pitch_a;
        float acc[8];
        const int yy = y0 - loy + r;
        if (a.mode == MODE_CONSTANT && (yy < 0 || yy >= a.ny)) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = a.cval;
        } else if (id_x) {
            load_x8(row, 8 * lx, acc);
        } else {
            window_conv<8>([&](int o, float(&v)[8]) { load_x8(row, 8 * lx + o, v); }, t.wx, nx_t, acc);
        }
        *reinterpret_cast<v4f*>(B + r * SF_PITCH_B + 8 * lx) = v4f{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<v4f*>(B + r * SF_PITCH_B + 8 * lx + 4) = v4f{acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, r0 = 4 * (threadIdx.x >> 4), ox = x0 + 4 * lx;
    if (ox >= a.nx || r0 >= th) return;
    v4f acc[4];
    const float* col = B + r0 * SF_PITCH_B + 4 * lx;
    if (id_y) load_y<4>(col, SF_PITCH_B, 0, acc);
    else window_conv<4>([&](int o, v4f(&v)[4]) { load_y<4>(col, SF_PITCH_B, o, v); }, t.wy, ny_t, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (r0 + j < th) {
            if (a.epi) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[j][e] = epilogue(a.epi, acc[j][e], A[Swz::at(loy + r0 + j, lox + 4 * lx + e, pitch_a)], a.eps);
            }
            store4(a.out + fo + (size_t)(y0 + r0 + j) * a.nx + ox, acc[j], a.nx - ox, a.vec_out != 0, true);
        }
    }
}

// ---------------------------------------------------------------------------------------------- local statistics
// grid (tiles_x * tiles_y, frames).  The one-frame user of b4d_window.hpp, which states the padding and the order of the sums: A,
// the tile with its halo as float32, and the float64 row sums of x and x * x, laid out by window_layout(1, 2, ..).  One sum per lane
// and LDS value: a lane that forms four adjacent sums from one read of each value was measured 1.3 - 1.8 x slower (a quarter of
// the lanes, each four times as long).
__global__ void __launch_bounds__(256) k_local_stats(Frame a, float* __restrict__ var_out, float* __restrict__ con_out, WindowTaps t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int sy = t.sy, sx = t.sx, loy = sy / 2, lox = sx / 2;
    const WindowLayout l = window_layout(1, 2, sy, sx, 0);
    float* A = lds;
    double* B = reinterpret_cast<double*>(lds + l.sums);
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * WIN_T, y0 = tile_y * WIN_T;
    const size_t fo = (size_t)blockIdx.y * a.ny * a.nx;
    const int tw = min(WIN_T, a.nx - x0), th = min(WIN_T, a.ny - y0);
    const int ha = th + sy - 1;
    stage<NoSwz>(A, l.pitch, a.in + fo, a.ny, a.nx, y0 - loy, ha, x0 - lox, tw + sx - 1, a.mode, a.cval, a.vec_in != 0, threadIdx.x);
    __syncthreads();
    window_row_pass<1, 256>(A, B, l, ha, tw, t);
    __syncthreads();
    const double W = window_weight(t);
    const int c = threadIdx.x & 31, ox = x0 + c;
    if (ox >= a.nx) return;
    for (int ly = threadIdx.x >> 5; ly < th; ly += 8) {
        // the column pass as b4d_window.hpp states it (window_col_sums<2, 1> gives the same bits); the loops are this kernel's own
        // because box 7 x 7 ran 0.7 % slower on the shared function, outside the parent's spread
        double s1 = 0.0, s2 = 0.0;
        const double* B1 = B;
        const double* B2 = B + l.sum_plane;
        if (t.box) {
            for (int j = 0; j < sy; ++j) {
                s1 += B1[(ly + j) * WIN_T + c];
                s2 += B2[(ly + j) * WIN_T + c];
            }
        } else {
            for (int j = 0; j < sy; ++j) {
                s1 = fma(t.wy[j], B1[(ly + j) * WIN_T + c], s1);
                s2 = fma(t.wy[j], B2[(ly + j) * WIN_T + c], s2);
            }
        }
        const double m = s1 / W;
        double v = s2 / W - m * m;
        if (v < 0.0) v = 0.0;   // (a NaN stays)
        const size_t po = fo + (size_t)(y0 + ly) * a.nx + ox;
        if (a.out) a.out[po] = (float)m;
        if (var_out) var_out[po] = (float)v;
        if (con_out) con_out[po] = m > 0.0 ? (float)(sqrt(v) / m) : __builtin_nanf("");
    }
}

// ---------------------------------------------------------------------------------------------- host side
static void round_taps(const double* w, int n, float* dst, int cap) {
    for (int k = 0; k < cap; ++k) dst[k] = k < n ? (float)w[k] : 0.f;
}
static size_t lds_row(int n) { return sizeof(float) * (SR_TY / 2) * (size_t)pair_width(SR_TX + up8(n)); }
static size_t lds_col(int n) { return sizeof(float) * SC_PITCH * (size_t)(SC_TY + up8(n)); }
static size_t lds_fused(int n_y, int n_x) { return sizeof(float) * (size_t)(SF_T + up4(n_y)) * (swz_width(SF_T + up8(n_x)) + SF_PITCH_B); }

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_separable_filter(const float* in, int batch, int ny, int nx, const double* taps_y, int n_y, const double* taps_x, int n_x,
                                    int mode, float cval, int epilogue, float eps, int flags, float* out, void* stream) {
    if (!in || !out || !taps_y || !taps_x) return fail(B4D_EINVAL, "b4d_separable_filter: null argument");
    if (const int rc = check_stack("b4d_separable_filter", "empty shape", true, batch, ny, nx, mode, true)) return rc;
    if (n_y < 1 || n_y > SM_MAX_TAPS || n_x < 1 || n_x > SM_MAX_TAPS)
        return fail(B4D_EINVAL, "b4d_separable_filter: tap counts must be in 1 .. " + std::to_string(SM_MAX_TAPS));
    if (epilogue < 0 || epilogue > 2) return fail(B4D_EINVAL, "b4d_separable_filter: epilogue must be 0 filtered, 1 subtract or 2 divide");
    const size_t fpix = (size_t)ny * nx, bytes = fpix * batch * sizeof(float);
    if (ranges_overlap(in, bytes, out, bytes)) return fail(B4D_EINVAL, "b4d_separable_filter: in and out must not overlap");
    hipStream_t st = (hipStream_t)stream;
    Frame a{};
    a.ny = ny;
    a.nx = nx;
    a.mode = mode;
    a.cval = cval;
    a.eps = eps;
    const int vec_in = vec_ok(in, nx, 16), vec_out = vec_ok(out, nx, 16);
    const bool id_y = n_y == 1 && (float)taps_y[0] == 1.f, id_x = n_x == 1 && (float)taps_x[0] == 1.f;
    const int fused_max = (flags & 2) ? SM_FUSED_CAP : SM_FUSED_TAPS;
    const bool fused = !(flags & 1) && n_y <= fused_max && n_x <= fused_max;
    if (fused) {
        TapsFused t{};
        t.ny = n_y;
        t.nx = n_x;
        round_taps(taps_y, n_y, t.wy, SM_FUSED_PAD);
        round_taps(taps_x, n_x, t.wx, SM_FUSED_PAD);
        a.tiles_x = (int)tiles(nx, SF_T);
        a.vec_in = vec_in;
        a.vec_out = vec_out;
        a.epi = epilogue;
        return for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
            a.in = in + fpix * b0;
            a.out = out + fpix * b0;
            return launch(k_smooth_fused, dim3(a.tiles_x * tiles(ny, SF_T), nb), dim3(256), lds_fused(n_y, n_x), st, a, t);
        });
    }
    // two passes, a group of frames at a time so that the intermediate of a group stays in the last-level cache; an identity axis
    // is skipped (with both, the row kernel copies with its one tap)
    Taps tx{}, ty{};
    tx.n = n_x;
    ty.n = n_y;
    round_taps(taps_x, n_x, tx.w, SM_MAX_TAPS + 1);
    round_taps(taps_y, n_y, ty.w, SM_MAX_TAPS + 1);
    const bool do_col = !id_y, do_row = !id_x || !do_col;
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)MAX_GRID_FRAMES, ((size_t)128 << 20) / (fpix * sizeof(float))));
    B4D_SCRATCH_LOCK();
    float* mid = nullptr;
    if (do_row && do_col) {
        void* p = nullptr;
        if (const int rc = get_scratch(fpix * std::min(group, batch) * sizeof(float), &p, st)) return rc;
        mid = static_cast<float*>(p);
    }
    return for_frame_chunks(batch, group, [&](int b0, int nb) {
        const float* pin = in + fpix * b0;
        float* pout = out + fpix * b0;
        if (do_row) {
            a.in = pin;
            a.out = do_col ? mid : pout;
            a.tiles_x = (int)tiles(nx, SR_TX);
            a.vec_in = vec_in;
            a.vec_out = do_col ? (nx % 4 == 0) : vec_out;
            a.epi = do_col ? -1 : epilogue;   // -1: intermediate (plain stores, no epilogue)
            if (const int rc = launch(k_smooth_row, dim3(a.tiles_x * tiles(ny, SR_TY), nb), dim3(256), lds_row(n_x), st, a, tx)) return rc;
        }
        if (do_col) {
            a.in = do_row ? mid : pin;
            a.out = pout;
            a.tiles_x = (int)tiles(nx, SC_TX);
            a.vec_in = do_row ? (nx % 4 == 0) : vec_in;
            a.vec_out = vec_out;
            a.epi = epilogue;
            if (const int rc = launch(k_smooth_col, dim3(a.tiles_x * tiles(ny, SC_TY), nb), dim3(256), lds_col(n_y), st, a, pin, vec_in, ty)) return rc;
        }
        return B4D_OK;
    });
}

extern "C" int b4d_local_stats(const float* in, int batch, int ny, int nx, int size_y, int size_x, const double* taps_y, const double* taps_x,
                               int mode, float cval, float* mean, float* variance, float* contrast, void* stream) {
    if (const int rc = check_stack("b4d_local_stats", "null input or empty shape", in, batch, ny, nx, mode, true)) return rc;
    if (const int rc = check_window("b4d_local_stats", size_y, size_x, taps_y, taps_x)) return rc;
    if (!mean && !variance && !contrast) return fail(B4D_EINVAL, "b4d_local_stats: mean, variance and contrast are all null");
    const size_t fpix = (size_t)ny * nx, bytes = fpix * batch * sizeof(float);
    if (ranges_overlap(in, bytes, mean, bytes) || ranges_overlap(in, bytes, variance, bytes) || ranges_overlap(in, bytes, contrast, bytes))
        return fail(B4D_EINVAL, "b4d_local_stats: an output overlaps the input");
    hipStream_t st = (hipStream_t)stream;
    const WindowTaps t = fill_window_taps(size_y, size_x, taps_y, taps_x);
    const size_t lds = window_layout(1, 2, size_y, size_x, 0).bytes;
    Frame a{};
    a.ny = ny;
    a.nx = nx;
    a.mode = mode;
    a.cval = cval;
    a.tiles_x = (int)tiles(nx, WIN_T);
    a.vec_in = vec_ok(in, nx, 16);
    return for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        a.in = in + fpix * b0;
        a.out = mean ? mean + fpix * b0 : nullptr;
        return launch(k_local_stats, dim3(a.tiles_x * tiles(ny, WIN_T), nb), dim3(256), lds, st, a,
                      variance ? variance + fpix * b0 : nullptr, contrast ? contrast + fpix * b0 : nullptr, t);
    });
}
