// b4d_warp.hip -- distortion correction: frames warped by a displacement field (barc4dip_amd/preprocessing/distortion.py;
// DESIGN.md section 12).
//
// out[t, y, x] = scipy.ndimage.map_coordinates(src[t], [y + dy, x + dx], order, mode, cval) for order 0 / 1 / 3 and the modes
// nearest / reflect / mirror / constant, in float32.  Three kernels, each one launch for the whole stack on the caller's stream:
//   k_prefilter_col  (order 3) cubic B-spline prefilter along y: a truncated symmetric FIR h[k] = sqrt(3) (sqrt(3) - 2)^|k|,
//                    |k| <= 14, on the mode-extended signal; lanes along x, each lane walks WP_RB output rows (coalesced, no LDS).
//                    "nearest" first pads the frame by 12 px with edge values and filters the padded frame with mirror
//                    extension, as scipy does (_prepad_for_spline_filter)
//   k_prefilter_row  (order 3) the same FIR along x, in place: one workgroup stages one coefficient row in LDS
//   k_warp           one lane per WP_PX neighbouring output pixels of a row; the field comes from dense per-pixel arrays or
//                    from the window grid of a displacement map, bilinear in the kernel (the per-pixel field never reaches HBM);
//                    1, 4 or 16 direct taps from the frame or the coefficients
// Precision rule: the integer tap and the fractional weight come from the float32 DISPLACEMENT (iy = y + floor(dy),
// wy = dy - floor(dy)), never from a float32 absolute coordinate (5e-4 px of resolution near 4096).
#include <cmath>
#include <string>

#include "b4d_common.hpp"
#include "b4d_tile.hpp"   // MODE_*

namespace b4d {

constexpr int WP_PAD = 12;          // "nearest", order 3: edge padding of the frame before the prefilter (scipy's npad)
constexpr int WP_R = 14;            // FIR half-length: |sqrt(3) - 2|^15 = 2.7e-9
constexpr int WP_RB = 8;            // output rows per lane of the column pass
constexpr int WP_PX = 4;            // output pixels per lane of the warp
constexpr int WP_THREADS = 256;
constexpr int WP_MAX_ROW = 16384;   // padded row length of the in-place row pass (64 KiB of LDS)
constexpr int WP_MAX_FOLD = 1 << 24;   // |floor(displacement)| is clamped here before the integer conversion

struct FirTaps {
    float h[WP_R + 1];
    constexpr FirTaps() : h() {
        double v = 1.7320508075688772;   // sqrt(3)
        for (int k = 0; k <= WP_R; ++k) {
            h[k] = (float)v;
            v *= -0.2679491924311228;    // sqrt(3) - 2
        }
    }
};
constexpr FirTaps kFir{};

// index i of a signal of n samples folded back into [0, n): edge clamp, half-sample ("reflect": -1 -> 0) or whole-sample
// ("mirror": -1 -> 1) symmetric extension.  border_index (b4d_tile.hpp) gives the same indices for these three modes; with its
// branches for "constant" and "wrap" k_prefilter_row takes 66 VGPRs instead of 37 and loses a wave per SIMD, so the fold stays.
__device__ __forceinline__ int wp_fold(int i, int n, int mode) {
    if ((unsigned)i < (unsigned)n) return i;
    if (mode == MODE_NEAREST) return i < 0 ? 0 : n - 1;
    if (mode == MODE_REFLECT) {
        const int p = 2 * n;
        i %= p;
        if (i < 0) i += p;
        return i >= n ? p - 1 - i : i;
    }
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// extension used by the prefilter (fm) and by the taps (tm) of a mode; "constant" takes the mirror route inside the frame,
// "nearest" filters its padded frame with mirror extension and clamps the taps
__device__ __forceinline__ int wp_filter_mode(int mode) { return mode == MODE_REFLECT ? MODE_REFLECT : MODE_MIRROR; }
__device__ __forceinline__ int wp_tap_mode(int mode) { return mode == MODE_CONSTANT ? MODE_MIRROR : mode; }

// ---- prefilter, pass 1: src (n, h, w) -> coef (n, hp, wp) filtered along y; padded row / column i reads src row clamp(i - pad)
__global__ void __launch_bounds__(WP_THREADS) k_prefilter_col(const float* __restrict__ src, int h, int w, int pad, int mode,
                                                              float* __restrict__ coef) {
    const int hp = h + 2 * pad, wp = w + 2 * pad;
    const int j = blockIdx.x * WP_THREADS + threadIdx.x, r0 = blockIdx.y * WP_RB;
    if (j >= wp) return;
    const int fm = wp_filter_mode(mode);
    const float* s = src + (size_t)blockIdx.z * h * w + min(max(j - pad, 0), w - 1);
    float v[WP_RB + 2 * WP_R];
#pragma unroll
    for (int m = 0; m < WP_RB + 2 * WP_R; ++m) {
        const int a = wp_fold(r0 - WP_R + m, hp, fm) - pad;
        v[m] = s[(size_t)min(max(a, 0), h - 1) * w];
    }
    float* c = coef + (size_t)blockIdx.z * hp * wp + j;
#pragma unroll
    for (int r = 0; r < WP_RB; ++r) {
        if (r0 + r >= hp) break;
        float acc = kFir.h[0] * v[r + WP_R];
#pragma unroll
        for (int k = 1; k <= WP_R; ++k) acc += kFir.h[k] * (v[r + WP_R - k] + v[r + WP_R + k]);
        c[(size_t)(r0 + r) * wp] = acc;
    }
}

// ---- prefilter, pass 2: coef rows filtered along x in place; grid (hp, n), dynamic LDS of wp floats
__global__ void __launch_bounds__(WP_THREADS) k_prefilter_row(float* __restrict__ coef, int hp, int wp, int mode) {
    extern __shared__ float wp_row[];
    float* c = coef + ((size_t)blockIdx.y * hp + blockIdx.x) * wp;
    for (int j = threadIdx.x; j < wp; j += WP_THREADS) wp_row[j] = c[j];
    __syncthreads();
    const int fm = wp_filter_mode(mode);
    for (int j = threadIdx.x; j < wp; j += WP_THREADS) {
        float acc = kFir.h[0] * wp_row[j];
#pragma unroll
        for (int k = 1; k <= WP_R; ++k) acc += kFir.h[k] * (wp_row[wp_fold(j - k, wp, fm)] + wp_row[wp_fold(j + k, wp, fm)]);
        c[j] = acc;
    }
}

struct WarpArgs {
    const float* src;        // frames (order 0 / 1) or spline coefficients (order 3), planes of sh x sw
    const float* fy;         // field: dense (h, w) or grid (gy, gx) planes
    const float* fx;
    float* out;              // (n, h, w)
    size_t fstride;          // elements between field planes; 0: one field for every frame
    int h, w, sh, sw, pad;
    int mode;
    float cval;
    int gy, gx;              // grid: gy x gx window centres at gy0 + i * gsy, gx0 + j * gsx
    double gy0, ginvy, gx0, ginvx;
};

// one grid axis of the bilinear field: taps i0, i1 and weight t at grid coordinate u, held constant beyond the end points
// (map_coordinates(order=1, mode="nearest") on the grid)
__device__ __forceinline__ void wp_grid_axis(double u, int n, int& i0, int& i1, float& t) {
    u = fmin(fmax(u, 0.0), (double)(n - 1));
    i0 = min((int)floor(u), max(n - 2, 0));
    i1 = min(i0 + 1, n - 1);
    t = (float)(u - (double)i0);
}

__device__ __forceinline__ float wp_lerp(float a, float b, float t) { return (1.0f - t) * a + t * b; }

// integer part (clamped) and fraction of a float32 displacement
__device__ __forceinline__ int wp_split(float d, float& t) {
    const float f = fminf(fmaxf(floorf(d), (float)-WP_MAX_FOLD), (float)WP_MAX_FOLD);
    t = d - f;
    return (int)f;
}

__device__ __forceinline__ void wp_cubic(float t, float (&wt)[4]) {
    const float s = 1.0f - t, t2 = t * t, t3 = t2 * t;
    wt[0] = s * s * s * (1.0f / 6.0f);
    wt[1] = (3.0f * t3 - 6.0f * t2 + 4.0f) * (1.0f / 6.0f);
    wt[2] = (-3.0f * t3 + 3.0f * t2 + 3.0f * t + 1.0f) * (1.0f / 6.0f);
    wt[3] = t3 * (1.0f / 6.0f);
}

template <int ORDER>
__device__ __forceinline__ float wp_sample(const float* __restrict__ P, const WarpArgs& a, int y, int x, float dy, float dx) {
    if (a.mode == MODE_CONSTANT && (dy < (float)-y || dy > (float)(a.h - 1 - y) || dx < (float)-x || dx > (float)(a.w - 1 - x)))
        return a.cval;
    const int tm = wp_tap_mode(a.mode);
    float ty, tx;
    const int iy = y + a.pad + wp_split(dy, ty), ix = x + a.pad + wp_split(dx, tx);
    if (ORDER == 0) {   // scipy: floor(c + 0.5), half-integers round up
        const int ry = wp_fold(iy + (ty >= 0.5f), a.sh, tm), rx = wp_fold(ix + (tx >= 0.5f), a.sw, tm);
        return P[(size_t)ry * a.sw + rx];
    } else if (ORDER == 1) {
        const int y0 = wp_fold(iy, a.sh, tm), y1 = wp_fold(iy + 1, a.sh, tm);
        const int x0 = wp_fold(ix, a.sw, tm), x1 = wp_fold(ix + 1, a.sw, tm);
        const float* r0 = P + (size_t)y0 * a.sw;
        const float* r1 = P + (size_t)y1 * a.sw;
        return wp_lerp(wp_lerp(r0[x0], r0[x1], tx), wp_lerp(r1[x0], r1[x1], tx), ty);
    } else {
        float wy[4], wx[4];
        wp_cubic(ty, wy);
        wp_cubic(tx, wx);
        int cx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cx[k] = wp_fold(ix - 1 + k, a.sw, tm);
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* r = P + (size_t)wp_fold(iy - 1 + k, a.sh, tm) * a.sw;
            acc += wy[k] * (wx[0] * r[cx[0]] + wx[1] * r[cx[1]] + wx[2] * r[cx[2]] + wx[3] * r[cx[3]]);
        }
        return acc;
    }
}

// grid (ceil(w / (64 WP_PX)), ceil(h / 4), n), block 256: wave k of the block takes row 4 blockIdx.y + k
template <int ORDER, bool GRID>
__global__ void __launch_bounds__(WP_THREADS) k_warp(WarpArgs a) {
    const int lane = threadIdx.x & 63, y = blockIdx.y * (WP_THREADS / 64) + (threadIdx.x >> 6);
    const int x0 = (blockIdx.x * 64 + lane) * WP_PX;
    if (y >= a.h || x0 >= a.w) return;
    const int t = blockIdx.z;
    const bool full = (a.w % WP_PX == 0);    // whole-vector loads and stores (x0 + WP_PX <= w then holds)
    const int nx = min(WP_PX, a.w - x0);
    float dy[WP_PX], dx[WP_PX];
    if (GRID) {
        const float* gfy = a.fy + a.fstride * t;
        const float* gfx = a.fx + a.fstride * t;
        int u0, u1;
        float tu;
        wp_grid_axis(((double)y - a.gy0) * a.ginvy, a.gy, u0, u1, tu);
#pragma unroll
        for (int k = 0; k < WP_PX; ++k) {
            int v0, v1;
            float tv;
            wp_grid_axis(((double)(x0 + k) - a.gx0) * a.ginvx, a.gx, v0, v1, tv);
            const int p00 = u0 * a.gx + v0, p01 = u0 * a.gx + v1, p10 = u1 * a.gx + v0, p11 = u1 * a.gx + v1;
            dy[k] = wp_lerp(wp_lerp(gfy[p00], gfy[p01], tv), wp_lerp(gfy[p10], gfy[p11], tv), tu);
            dx[k] = wp_lerp(wp_lerp(gfx[p00], gfx[p01], tv), wp_lerp(gfx[p10], gfx[p11], tv), tu);
        }
    } else {
        const size_t o = a.fstride * t + (size_t)y * a.w + x0;
        if (full) {
            const float4 vy = *reinterpret_cast<const float4*>(a.fy + o), vx = *reinterpret_cast<const float4*>(a.fx + o);
            dy[0] = vy.x, dy[1] = vy.y, dy[2] = vy.z, dy[3] = vy.w;
            dx[0] = vx.x, dx[1] = vx.y, dx[2] = vx.z, dx[3] = vx.w;
        } else {
#pragma unroll
            for (int k = 0; k < WP_PX; ++k) {
                dy[k] = k < nx ? a.fy[o + k] : 0.0f;
                dx[k] = k < nx ? a.fx[o + k] : 0.0f;
            }
        }
    }
    const float* P = a.src + (size_t)t * a.sh * a.sw;
    float v[WP_PX];
#pragma unroll
    for (int k = 0; k < WP_PX; ++k) v[k] = wp_sample<ORDER>(P, a, y, x0 + k, dy[k], dx[k]);
    float* o = a.out + ((size_t)t * a.h + y) * a.w + x0;
    if (full) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < WP_PX; ++k)
            if (k < nx) o[k] = v[k];
    }
}

template <int ORDER, bool GRID>
static int launch_warp(const WarpArgs& a, int n, hipStream_t st) {
    const dim3 grid((a.w + 64 * WP_PX - 1) / (64 * WP_PX), (a.h + WP_THREADS / 64 - 1) / (WP_THREADS / 64), n);
    hipLaunchKernelGGL((k_warp<ORDER, GRID>), grid, dim3(WP_THREADS), 0, st, a);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

template <bool GRID>
static int warp_dispatch(const WarpArgs& a, int n, int order, hipStream_t st) {
    if (order == 0) return launch_warp<0, GRID>(a, n, st);
    if (order == 1) return launch_warp<1, GRID>(a, n, st);
    return launch_warp<3, GRID>(a, n, st);
}

static int warp_check(const float* src, int n, int h, int w, int order, int mode, const float* dy, const float* dx,
                      int field_frames, const float* out) {
    if (!src || !dy || !dx || !out) return fail(B4D_EINVAL, "null argument");
    if (n < 1 || h < 1 || w < 1) return fail(B4D_EINVAL, "frame count and sides must be >= 1");
    if (order != 0 && order != 1 && order != 3) return fail(B4D_EINVAL, "order must be 0, 1 or 3");
    if (mode < MODE_NEAREST || mode > MODE_CONSTANT) return fail(B4D_EINVAL, "mode must be 0 (nearest) .. 3 (constant)");
    if (field_frames != 1 && field_frames != n) return fail(B4D_EINVAL, "field_frames must be 1 or the frame count");
    if (n > 65535 || h > 4 * 65535 || w > WP_MAX_FOLD) return fail(B4D_ESIZE, "warp: at most 65535 frames and 262140 rows");
    return B4D_OK;
}

static WarpArgs warp_args(const float* src, int h, int w, int order, int mode, float cval, const float* dy, const float* dx,
                          int field_frames, size_t plane, float* out) {
    WarpArgs a{};
    a.src = src;
    a.fy = dy;
    a.fx = dx;
    a.out = out;
    a.fstride = field_frames == 1 ? 0 : plane;
    a.h = h;
    a.w = w;
    a.pad = (order == 3 && mode == MODE_NEAREST) ? WP_PAD : 0;
    a.sh = h + 2 * a.pad;
    a.sw = w + 2 * a.pad;
    a.mode = mode;
    a.cval = cval;
    return a;
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_spline_prefilter(const float* src, int n, int h, int w, int mode, float* coef, void* stream) {
    if (!src || !coef) return fail(B4D_EINVAL, "null argument");
    if (n < 1 || h < 1 || w < 1) return fail(B4D_EINVAL, "frame count and sides must be >= 1");
    if (mode < MODE_NEAREST || mode > MODE_CONSTANT) return fail(B4D_EINVAL, "mode must be 0 (nearest) .. 3 (constant)");
    const int pad = mode == MODE_NEAREST ? WP_PAD : 0, hp = h + 2 * pad, wp = w + 2 * pad;
    if (n > 65535 || wp > WP_MAX_ROW || h > 4 * 65535)
        return fail(B4D_ESIZE, "spline prefilter: at most 65535 frames, 262140 rows and " + std::to_string(WP_MAX_ROW) +
                                   " padded columns");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_prefilter_col, dim3((wp + WP_THREADS - 1) / WP_THREADS, (hp + WP_RB - 1) / WP_RB, n), dim3(WP_THREADS),
                       0, st, src, h, w, pad, mode, coef);
    B4D_HIP(hipGetLastError());
    // dynamic LDS: one padded row, at most 4 WP_MAX_ROW = 65 536 bytes (the check above): 64 KiB is reached, never passed
    return launch(k_prefilter_row, dim3(hp, n), dim3(WP_THREADS), sizeof(float) * wp, st, coef, hp, wp, mode);
}

extern "C" int b4d_warp_dense(const float* src, int n, int h, int w, int order, int mode, float cval, const float* dy,
                              const float* dx, int field_frames, float* out, void* stream) {
    int rc = warp_check(src, n, h, w, order, mode, dy, dx, field_frames, out);
    if (rc) return rc;
    const WarpArgs a = warp_args(src, h, w, order, mode, cval, dy, dx, field_frames, (size_t)h * w, out);
    return warp_dispatch<false>(a, n, order, (hipStream_t)stream);
}

extern "C" int b4d_warp_grid(const float* src, int n, int h, int w, int order, int mode, float cval, const float* dy,
                             const float* dx, int field_frames, int gy, int gx, double y0, double step_y, double x0,
                             double step_x, float* out, void* stream) {
    int rc = warp_check(src, n, h, w, order, mode, dy, dx, field_frames, out);
    if (rc) return rc;
    if (gy < 1 || gx < 1) return fail(B4D_EINVAL, "the grid needs at least one point per axis");
    if (!(step_y != 0.0 && step_x != 0.0 && std::isfinite(step_y) && std::isfinite(step_x) && std::isfinite(y0) &&
          std::isfinite(x0)))
        return fail(B4D_EINVAL, "grid origin and steps must be finite, steps non-zero");
    WarpArgs a = warp_args(src, h, w, order, mode, cval, dy, dx, field_frames, (size_t)gy * gx, out);
    a.gy = gy;
    a.gx = gx;
    a.gy0 = y0;
    a.ginvy = 1.0 / step_y;
    a.gx0 = x0;
    a.ginvx = 1.0 / step_x;
    return warp_dispatch<true>(a, n, order, (hipStream_t)stream);
}
