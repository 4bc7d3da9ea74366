// b4d_perceptual.hip -- how close a frame is to a reference frame: structural similarity (SSIM, Wang et
// al. 2004) with the per-frame means reduced on the device, the sums behind MSE / PSNR / NRMSE / MAE, and the 2 x 2 mean pooling
// between the scales of MS-SSIM.  Frames are (batch, ny, nx) float32; the reference is one frame for the whole batch
// (ref_stride 0) or one per frame.
//
// b4d_ssim is the pair form of k_local_stats (b4d_smooth.hip): both tiles with their halos in LDS as float32, five float64 row
// sums (r, x, r r, x x, r x) per staged row, five float64 column sums per output pixel, every sum in ascending tap order.  The
// taps travel in the kernel arguments.  No atomics anywhere: a workgroup writes its partial sums to its own slot of the per-stream
// scratch buffer and a second launch adds the slots in a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_reduce.hpp"
#include "b4d_tile.hpp"

// The quotients below are written as the header documents them, product by product: nothing is contracted into an FMA that the
// text does not show (a contracted mu_r^2 + mu_x^2 would not be symmetric in r and x).  The explicit fma() calls stay.
#pragma clang fp contract(off)

namespace b4d {

// 32 x 32 outputs per workgroup, windows up to 63 per axis as far as the LDS holds them (lds_ssim)
constexpr int PS_T = 32, PS_MAX = 63, PS_LANES = 512;
constexpr size_t PS_LDS_LIMIT = 160 * 1024;
// pair errors: a lane takes groups of four consecutive pixels; a workgroup at most PE_GROUPS of them per lane
constexpr int PE_COLS = 8, PE_SUMS = 5, PE_GROUPS = 8, PE_MAX_SPLIT = 1024;

struct TapsPair {
    int sy, sx, box;
    double wy[PS_MAX + 1], wx[PS_MAX + 1];
};
struct SsimArgs {
    const float* ref;   // of frame b0
    const float* img;
    long long ref_stride;
    float* ssim_map;
    float* cs_map;
    double* part;       // (frames, tiles, 2) partial sums of this chunk's frames, or null
    int ny, nx, tiles_x, mode;
    float cval;
    int vec_ref, vec_img;
    double c1, c2, cov_norm;
    int crop_y, crop_x;
};

constexpr int ps_up4(int n) { return (n + 3) & ~3; }

// frame rows ys + [0, nrows) and columns xs + [0, ncols) -> lds (row pitch `pitch`) under the border rule, padded in two dimensions:
// outside on either axis is cval under "constant".  The walk of 256 lanes (lane index t) is that of the separable filters' stager
// (tile_walk): 16-byte loads for aligned groups of four inside a row, element by element for the others; the loads of a lane's
// four (row, group) pairs are issued before the first value goes to LDS.
__device__ __forceinline__ v4f load_group(const float* __restrict__ f, int ny, int nx, int yy, int xb, int mode, float cval, bool vec) {
    v4f q = v4f{cval, cval, cval, cval};
    if (yy >= 0) {
        const float* row = f + (size_t)yy * nx;
        if (vec && xb >= 0 && xb + 3 < nx) {
            q = *reinterpret_cast<const v4f*>(row + xb);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int xx = border_index(xb + e, nx, mode);
                if (xx >= 0) q[e] = row[xx];
            }
        }
    }
    return q;
}
__device__ __forceinline__ void stage_frame(float* __restrict__ lds, int pitch, const float* __restrict__ f, int ny, int nx, int ys, int nrows,
                                            int xs, int ncols, int mode, float cval, bool vec, int t) {
    const int xa = xs & ~3;
    const int ng = (xs + ncols - xa + 3) >> 2;
    TileWalk w = tile_walk(t, ng);
    while (w.j < nrows) {
        v4f q[4];
        int at[4], c0[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            at[u] = -1;
            if (w.j < nrows) {
                const int xb = xa + 4 * w.g;
                at[u] = w.j;
                c0[u] = xb - xs;
                q[u] = load_group(f, ny, nx, border_index(ys + w.j, ny, mode), xb, mode, cval, vec);
            }
            tile_step(w);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (at[u] >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = c0[u] + e;
                    if (c >= 0 && c < ncols) lds[at[u] * pitch + c] = q[u][e];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- SSIM
// grid (tiles_x * tiles_y, frames), 512 lanes.  LDS: R, X, both tiles with their halos as float32 (PS_T + sy - 1 rows of pitch
// up4(PS_T + sx - 1) each); B, five planes of float64 row sums (as many rows of PS_T: S_r, S_x, S_rr, S_xx, S_rx); sixteen doubles
// for the workgroup's sums.  Lanes 0 .. 255 stage the reference tile, lanes 256 .. 511 the image tile.  Row pass: one lane forms
// all five sums of a position, a tap costs two LDS reads for five FMAs.  Column pass: a lane forms the sums of two adjacent rows of
// its column from one read of the sy + 1 rows of B below them (a box window has taps of 1.0: fma(1.0, v, s) is s + v).
__global__ void __launch_bounds__(PS_LANES) k_ssim(SsimArgs a, TapsPair t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int sy = t.sy, sx = t.sx, loy = sy / 2, lox = sx / 2;
    const int pitch = ps_up4(PS_T + sx - 1), rows = PS_T + sy - 1;
    const int plane_a = (rows * pitch + 3) & ~3, plane_b = rows * PS_T;
    float* R = lds;
    float* X = lds + plane_a;
    double* B = reinterpret_cast<double*>(lds + 2 * plane_a);
    double* sh = B + 5 * plane_b;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * PS_T, y0 = tile_y * PS_T;
    const size_t fo = (size_t)blockIdx.y * a.ny * a.nx;
    const int tw = min(PS_T, a.nx - x0), th = min(PS_T, a.ny - y0);
    const int ha = th + sy - 1;
    if (threadIdx.x < 256)
        stage_frame(R, pitch, a.ref + (size_t)a.ref_stride * blockIdx.y, a.ny, a.nx, y0 - loy, ha, x0 - lox, tw + sx - 1, a.mode, a.cval,
                    a.vec_ref != 0, threadIdx.x);
    else
        stage_frame(X, pitch, a.img + fo, a.ny, a.nx, y0 - loy, ha, x0 - lox, tw + sx - 1, a.mode, a.cval, a.vec_img != 0, threadIdx.x - 256);
    __syncthreads();
    for (int idx = threadIdx.x; idx < ha * PS_T; idx += PS_LANES) {
        const int r = idx >> 5, c = idx & 31;
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (c < tw) {
            const float* pr = R + r * pitch + c;
            const float* px = X + r * pitch + c;
            if (t.box) {
#pragma unroll 4
                for (int k = 0; k < sx; ++k) {
                    const double u = (double)pr[k], v = (double)px[k];
                    s[0] += u;
                    s[1] += v;
                    s[2] = fma(u, u, s[2]);   // (the products of two float32 are exact in float64: s + u * u, rounded once)
                    s[3] = fma(v, v, s[3]);
                    s[4] = fma(u, v, s[4]);
                }
            } else {
#pragma unroll 4
                for (int k = 0; k < sx; ++k) {
                    const double u = (double)pr[k], v = (double)px[k], w = t.wx[k];
                    s[0] = fma(w, u, s[0]);
                    s[1] = fma(w, v, s[1]);
                    s[2] = fma(w, u * u, s[2]);
                    s[3] = fma(w, v * v, s[3]);
                    s[4] = fma(w, u * v, s[4]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) B[q * plane_b + idx] = s[q];
    }
    __syncthreads();
    // W: the window's weight, summed as S_r of a frame of ones is
    double W = (double)(sy * sx);
    if (!t.box) {
        double wx = 0.0;
        for (int k = 0; k < sx; ++k) wx = fma(t.wx[k], 1.0, wx);
        W = 0.0;
        for (int j = 0; j < sy; ++j) W = fma(t.wy[j], wx, W);
    }
    const double iw = 1.0 / W;   // the one division by W: the five window means are products with it
    const int c = threadIdx.x & 31, ox = x0 + c, ly = 2 * (threadIdx.x >> 5);
    double s[2][5] = {{0.0, 0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0}};
    if (ly < th && ox < a.nx) {
        const double* b = B + ly * PS_T + c;
#pragma unroll 2
        for (int j = 0; j <= sy; ++j) {   // row ly + j of B is tap j of output row ly and tap j - 1 of output row ly + 1
            double v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = b[q * plane_b + j * PS_T];
            if (j < sy) {
                const double w = t.wy[j];
#pragma unroll
                for (int q = 0; q < 5; ++q) s[0][q] = fma(w, v[q], s[0][q]);
            }
            if (j > 0) {
                const double w = t.wy[j - 1];
#pragma unroll
                for (int q = 0; q < 5; ++q) s[1][q] = fma(w, v[q], s[1][q]);
            }
        }
    }
    double acc[2] = {0.0, 0.0};   // this lane's ssim and cs inside the region, the upper row first
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int oy = y0 + ly + i;
        if (ly + i >= th || ox >= a.nx) continue;
        const double mr = s[i][0] * iw, mx = s[i][1] * iw;
        const double vr = a.cov_norm * (s[i][2] * iw - mr * mr);
        const double vx = a.cov_norm * (s[i][3] * iw - mx * mx);
        const double vrx = a.cov_norm * (s[i][4] * iw - mr * mx);
        const double cs = (2.0 * vrx + a.c2) / (vr + vx + a.c2);
        const double ss = ((2.0 * (mr * mx) + a.c1) / (mr * mr + mx * mx + a.c1)) * cs;
        const size_t po = fo + (size_t)oy * a.nx + ox;
        if (a.ssim_map) a.ssim_map[po] = (float)ss;
        if (a.cs_map) a.cs_map[po] = (float)cs;
        if (oy >= a.crop_y && oy < a.ny - a.crop_y && ox >= a.crop_x && ox < a.nx - a.crop_x) {
            acc[0] += ss;
            acc[1] += cs;
        }
    }
    if (a.part) {   // (uniform: the whole workgroup calls)
        block_sum(acc, sh, PS_LANES / 64);
        if (threadIdx.x == 0) {
            double* p = a.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
            p[0] = acc[0];
            p[1] = acc[1];
        }
    }
}

// grid (frames), 256 lanes: lane l adds the tiles l, l + 256, .. of its frame in ascending order from 0.0, the 256 lane sums go
// through block_tree_sum256, and the sum is divided by the region's pixel count.
__global__ void __launch_bounds__(256) k_ssim_fin(const double* __restrict__ part, int ntiles, double count, double* __restrict__ means) {
    __shared__ double sh[256];
    const double* p = part + (size_t)blockIdx.x * ntiles * 2;
    for (int k = 0; k < 2; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < ntiles; i += 256) s += p[2 * (size_t)i + k];
        s = block_tree_sum256(s, sh, true);
        if (threadIdx.x == 0) means[2 * (size_t)blockIdx.x + k] = s / count;
    }
}

// ---------------------------------------------------------------------------------------------- pair errors
// A NaN must reach the extrema: the merge takes the newcomer when it is smaller (larger) or a NaN, and a NaN that is held is never
// replaced, because every comparison with it is false.
__device__ __forceinline__ double nan_min(double m, double v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }

struct ErrAcc {
    double sum[PE_SUMS];   // (x - r)^2, |x - r|, r^2, r, x
    double dmax, rmin, rmax;
};
__device__ __forceinline__ void err_take(ErrAcc& e, float rf, float xf) {
    const double r = (double)rf, x = (double)xf, d = x - r, ad = fabs(d);
    e.sum[0] += d * d;
    e.sum[1] += ad;
    e.sum[2] += r * r;
    e.sum[3] += r;
    e.sum[4] += x;
    e.dmax = nan_max(e.dmax, ad);
    e.rmin = nan_min(e.rmin, r);
    e.rmax = nan_max(e.rmax, r);
}
// the extrema of a workgroup of 256 lanes into thread 0: down the wave as wave_sum goes (lane l with lane l + o, o = 32 .. 1), then
// the four waves in order.  sh: 12 doubles.
__device__ __forceinline__ void block_extrema(ErrAcc& e, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        e.dmax = nan_max(e.dmax, __shfl_down(e.dmax, o, 64));
        e.rmin = nan_min(e.rmin, __shfl_down(e.rmin, o, 64));
        e.rmax = nan_max(e.rmax, __shfl_down(e.rmax, o, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh[3 * wave] = e.dmax;
        sh[3 * wave + 1] = e.rmin;
        sh[3 * wave + 2] = e.rmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            e.dmax = nan_max(e.dmax, sh[3 * w]);
            e.rmin = nan_min(e.rmin, sh[3 * w + 1]);
            e.rmax = nan_max(e.rmax, sh[3 * w + 2]);
        }
    }
}

// grid (split, frames).  The frame's pixels in groups of four; workgroup s takes the groups [s per, (s + 1) per), lane l of it the
// groups l, l + 256, .. of that range in ascending order, the four pixels of a group in order: which pixel goes to which lane does
// not depend on the access width.  part: (frames, split, 8).
__global__ void __launch_bounds__(256) k_pair_errors(const float* __restrict__ ref, long long ref_stride, const float* __restrict__ img,
                                                     long long npix, long long per, int vec_ref, int vec_img, double* __restrict__ part) {
    __shared__ double sh[4 * PE_SUMS + 12];
    const float* r = ref + (size_t)ref_stride * blockIdx.y;
    const float* x = img + (size_t)npix * blockIdx.y;
    const long long groups = (npix + 3) >> 2;
    const long long g0 = per * blockIdx.x, g1 = min(groups, g0 + per);
    ErrAcc e;
#pragma unroll
    for (int k = 0; k < PE_SUMS; ++k) e.sum[k] = 0.0;
    e.dmax = 0.0;
    e.rmin = __builtin_inf();
    e.rmax = -__builtin_inf();
    for (long long g = g0 + threadIdx.x; g < g1; g += 256) {
        const long long p = 4 * g;
        if (p + 3 < npix) {
            v4f qr, qx;
            if (vec_ref) qr = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(r + p));
            else qr = v4f{r[p], r[p + 1], r[p + 2], r[p + 3]};
            if (vec_img) qx = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(x + p));
            else qx = v4f{x[p], x[p + 1], x[p + 2], x[p + 3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) err_take(e, qr[j], qx[j]);
        } else {
            for (long long q = p; q < npix; ++q) err_take(e, r[q], x[q]);
        }
    }
    block_sum(e.sum, sh, 4);
    block_extrema(e, sh + 4 * PE_SUMS);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * PE_COLS;
        o[0] = e.sum[0];
        o[1] = e.sum[1];
        o[2] = e.dmax;
        o[3] = e.sum[2];
        o[4] = e.sum[3];
        o[5] = e.rmin;
        o[6] = e.rmax;
        o[7] = e.sum[4];
    }
}
// grid (frames), 256 lanes: lane l merges the workgroup rows l, l + 256, .. in ascending order; the sums then go through
// block_tree_sum256, the extrema through LDS, merged by thread 0 in lane order.
__global__ void __launch_bounds__(256) k_pair_errors_fin(const double* __restrict__ part, int split, double* __restrict__ out) {
    __shared__ double sh[256];
    __shared__ double ex[3 * 256];
    const double* p = part + (size_t)blockIdx.x * split * PE_COLS;
    double v[PE_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inf(), -__builtin_inf(), 0.0};
    for (int s = threadIdx.x; s < split; s += 256) {
        const double* q = p + (size_t)s * PE_COLS;
        v[0] += q[0];
        v[1] += q[1];
        v[2] = nan_max(v[2], q[2]);
        v[3] += q[3];
        v[4] += q[4];
        v[5] = nan_min(v[5], q[5]);
        v[6] = nan_max(v[6], q[6]);
        v[7] += q[7];
    }
    ex[threadIdx.x] = v[2];
    ex[256 + threadIdx.x] = v[5];
    ex[512 + threadIdx.x] = v[6];
    const int sums[PE_SUMS] = {0, 1, 3, 4, 7};
#pragma unroll
    for (int k = 0; k < PE_SUMS; ++k) v[sums[k]] = block_tree_sum256(v[sums[k]], sh, true);
    if (threadIdx.x == 0) {
        for (int l = 1; l < 256; ++l) {
            v[2] = nan_max(v[2], ex[l]);
            v[5] = nan_min(v[5], ex[256 + l]);
            v[6] = nan_max(v[6], ex[512 + l]);
        }
        double* o = out + (size_t)blockIdx.x * PE_COLS;
#pragma unroll
        for (int k = 0; k < PE_COLS; ++k) o[k] = v[k];
    }
}

// ---------------------------------------------------------------------------------------------- 2 x 2 mean pooling
// grid (groups of 256 output pixels, frames)
__global__ void __launch_bounds__(256) k_pool2(const float* __restrict__ in, int ny, int nx, int oy, int ox, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)oy * ox) return;
    const int y = (int)(i / ox), x = (int)(i - (long long)y * ox);
    const float* p = in + (size_t)blockIdx.y * ny * nx + (size_t)(2 * y) * nx + 2 * x;
    const float top = p[0] + p[1], bottom = p[nx] + p[nx + 1];
    out[(size_t)blockIdx.y * oy * ox + i] = (top + bottom) * 0.25f;
}

// ---------------------------------------------------------------------------------------------- host side
// dynamic LDS of k_ssim: both staged tiles, the five planes of row sums, the workgroup's sums
static size_t lds_ssim(int sy, int sx) {
    const size_t rows = PS_T + sy - 1;
    return 2 * sizeof(float) * ((rows * ps_up4(PS_T + sx - 1) + 3) & ~(size_t)3) + 5 * sizeof(double) * rows * PS_T + 2 * (PS_LANES / 64) * sizeof(double);
}
static unsigned tiles(int n, int t) { return (unsigned)((n + t - 1) / t); }
// bytes of the reference: one frame, or batch frames ref_stride apart
static size_t ref_bytes(long long ref_stride, int batch, size_t fpix) { return ((size_t)ref_stride * (batch - 1) + fpix) * sizeof(float); }
static int check_ref(const char* fn, long long ref_stride, size_t fpix) {
    if (ref_stride != 0 && ref_stride < (long long)fpix) return fail(B4D_EINVAL, std::string(fn) + ": ref_stride must be 0 (one reference frame) or >= ny * nx");
    return B4D_OK;
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_ssim(const float* ref, long long ref_stride, const float* img, int batch, int ny, int nx, int size_y, int size_x,
                        const double* taps_y, const double* taps_x, int mode, float cval, double c1, double c2, double cov_norm, int crop_y,
                        int crop_x, float* ssim_map, float* cs_map, double* means, void* stream) {
    if (const int rc = check_stack("b4d_ssim", "null input or empty shape", ref && img, batch, ny, nx, mode, true)) return rc;
    const size_t fpix = (size_t)ny * nx, bytes = fpix * batch * sizeof(float);
    if (const int rc = check_ref("b4d_ssim", ref_stride, fpix)) return rc;
    if (size_y < 1 || size_y > PS_MAX || size_x < 1 || size_x > PS_MAX)
        return fail(B4D_EINVAL, "b4d_ssim: window sizes must be in 1 .. " + std::to_string(PS_MAX));
    if (lds_ssim(size_y, size_x) > PS_LDS_LIMIT)
        return fail(B4D_ESIZE, "b4d_ssim: a " + std::to_string(size_y) + " x " + std::to_string(size_x) + " window needs " +
                                   std::to_string(lds_ssim(size_y, size_x)) + " bytes of LDS, more than " + std::to_string(PS_LDS_LIMIT));
    if ((taps_y == nullptr) != (taps_x == nullptr)) return fail(B4D_EINVAL, "b4d_ssim: taps_y and taps_x must both be given or both be null");
    if (!ssim_map && !cs_map && !means) return fail(B4D_EINVAL, "b4d_ssim: ssim_map, cs_map and means are all null");
    if (!(c1 > 0.0) || !(c2 > 0.0) || !(cov_norm > 0.0)) return fail(B4D_EINVAL, "b4d_ssim: c1, c2 and cov_norm must be > 0");
    if (crop_y < 0 || crop_x < 0) return fail(B4D_EINVAL, "b4d_ssim: negative crop");
    const long long ry = (long long)ny - 2LL * crop_y, rx = (long long)nx - 2LL * crop_x;
    if (means && (ry < 1 || rx < 1)) return fail(B4D_EINVAL, "b4d_ssim: the crop leaves no pixel to average over");
    const size_t rbytes = ref_bytes(ref_stride, batch, fpix), mbytes = sizeof(double) * 2 * (size_t)batch;
    const void* ins[2] = {ref, img};
    const size_t in_bytes[2] = {rbytes, bytes};
    for (int k = 0; k < 2; ++k)
        if (ranges_overlap(ins[k], in_bytes[k], ssim_map, bytes) || ranges_overlap(ins[k], in_bytes[k], cs_map, bytes) ||
            ranges_overlap(ins[k], in_bytes[k], means, mbytes))
            return fail(B4D_EINVAL, "b4d_ssim: an output overlaps an input");
    hipStream_t st = (hipStream_t)stream;
    TapsPair t{};
    t.sy = size_y;
    t.sx = size_x;
    t.box = taps_y ? 0 : 1;
    for (int k = 0; k < size_y; ++k) t.wy[k] = taps_y ? taps_y[k] : 1.0;
    for (int k = 0; k < size_x; ++k) t.wx[k] = taps_x ? taps_x[k] : 1.0;
    SsimArgs a{};
    a.ref_stride = ref_stride;
    a.ny = ny;
    a.nx = nx;
    a.mode = mode;
    a.cval = cval;
    a.tiles_x = (int)tiles(nx, PS_T);
    a.vec_ref = vec_ok(ref, nx, 16) && ref_stride % 4 == 0;
    a.vec_img = vec_ok(img, nx, 16);
    a.c1 = c1;
    a.c2 = c2;
    a.cov_norm = cov_norm;
    a.crop_y = crop_y;
    a.crop_x = crop_x;
    const unsigned ntiles = a.tiles_x * tiles(ny, PS_T);
    B4D_SCRATCH_LOCK();
    double* part = nullptr;
    if (means) {
        void* p = nullptr;
        if (const int rc = get_scratch(sizeof(double) * 2 * (size_t)batch * ntiles, &p, st)) return rc;
        part = static_cast<double*>(p);
    }
    const int rc = for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        a.ref = ref + (size_t)ref_stride * b0;
        a.img = img + fpix * b0;
        a.ssim_map = ssim_map ? ssim_map + fpix * b0 : nullptr;
        a.cs_map = cs_map ? cs_map + fpix * b0 : nullptr;
        a.part = part ? part + (size_t)2 * ntiles * b0 : nullptr;
        return launch(k_ssim, dim3(ntiles, nb), dim3(PS_LANES), lds_ssim(size_y, size_x), st, a, t);
    });
    if (rc || !means) return rc;
    return launch(k_ssim_fin, dim3(batch), dim3(256), 0, st, part, (int)ntiles, (double)ry * (double)rx, means);
}

extern "C" int b4d_pair_errors(const float* ref, long long ref_stride, const float* img, int batch, int ny, int nx, double* out, void* stream) {
    if (const int rc = check_stack("b4d_pair_errors", "null argument or empty shape", ref && img && out, batch, ny, nx, MODE_NEAREST, true)) return rc;
    const size_t fpix = (size_t)ny * nx, bytes = fpix * batch * sizeof(float);
    if (const int rc = check_ref("b4d_pair_errors", ref_stride, fpix)) return rc;
    const size_t obytes = sizeof(double) * PE_COLS * (size_t)batch;
    if (ranges_overlap(ref, ref_bytes(ref_stride, batch, fpix), out, obytes) || ranges_overlap(img, bytes, out, obytes))
        return fail(B4D_EINVAL, "b4d_pair_errors: out overlaps an input");
    hipStream_t st = (hipStream_t)stream;
    // the split depends on the frame size alone: a frame is summed alike in every batch
    const long long groups = ((long long)fpix + 3) >> 2;
    const int split = (int)std::min<long long>(PE_MAX_SPLIT, (groups + 256LL * PE_GROUPS - 1) / (256LL * PE_GROUPS));
    const long long per = (groups + split - 1) / split;
    const int vec_ref = ptr_aligned(ref, 16) && ref_stride % 4 == 0, vec_img = ptr_aligned(img, 16) && fpix % 4 == 0;
    B4D_SCRATCH_LOCK();
    void* p = nullptr;
    if (const int rc = get_scratch(sizeof(double) * PE_COLS * (size_t)batch * split, &p, st)) return rc;
    double* part = static_cast<double*>(p);
    const int rc = for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        return launch(k_pair_errors, dim3(split, nb), dim3(256), 0, st, ref + (size_t)ref_stride * b0, ref_stride, img + fpix * b0, (long long)fpix,
                      per, vec_ref, vec_img, part + (size_t)PE_COLS * split * b0);
    });
    if (rc) return rc;
    return launch(k_pair_errors_fin, dim3(batch), dim3(256), 0, st, part, split, out);
}

extern "C" int b4d_pool2(const float* in, int batch, int ny, int nx, float* out, void* stream) {
    if (const int rc = check_stack("b4d_pool2", "null argument or empty shape", in && out, batch, ny, nx, MODE_NEAREST, true)) return rc;
    if (ny < 2 || nx < 2) return fail(B4D_EINVAL, "b4d_pool2: a frame needs at least 2 x 2 pixels");
    const int oy = ny / 2, ox = nx / 2;
    const size_t fpix = (size_t)ny * nx, opix = (size_t)oy * ox;
    if (ranges_overlap(in, fpix * batch * sizeof(float), out, opix * batch * sizeof(float))) return fail(B4D_EINVAL, "b4d_pool2: in and out must not overlap");
    hipStream_t st = (hipStream_t)stream;
    return for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        return launch(k_pool2, dim3((unsigned)((opix + 255) / 256), nb), dim3(256), 0, st, in + fpix * b0, ny, nx, oy, ox, out + opix * b0);
    });
}
