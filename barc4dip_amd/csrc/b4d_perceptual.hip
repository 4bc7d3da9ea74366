// b4d_perceptual.hip -- how close a frame is to a reference frame: structural similarity (SSIM, Wang et
// al. 2004) with the per-frame means reduced on the device, the sums behind MSE / PSNR / NRMSE / MAE, and the 2 x 2 mean pooling
// between the scales of MS-SSIM.  Frames are (batch, ny, nx) float32; the reference is one frame for the whole batch
// (ref_stride 0) or one per frame.
//
// b4d_ssim is the pair form of k_local_stats (b4d_smooth.hip), and both stand on b4d_window.hpp: the stager, the taps in the kernel
// arguments, the LDS layout, the row pass (five float64 sums r, x, r r, x x, r x per staged position) and the column pass (five
// window sums per output pixel), every sum in ascending tap order.  This unit keeps the 512 lanes, the quotients and the means.
// No atomics anywhere: a workgroup writes its partial sums to its own slot of the per-stream scratch buffer and a second launch
// adds the slots in a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_reduce.hpp"
#include "b4d_tile.hpp"
#include "b4d_window.hpp"

// The quotients below are written as the header documents them, product by product: nothing is contracted into an FMA that the
// text does not show (a contracted mu_r^2 + mu_x^2 would not be symmetric in r and x).  The pragma stands below the includes: the
// sums of b4d_window.hpp are compiled as in b4d_smooth.hip (explicit fma() calls, exact products), this unit's own code is not contracted.
#pragma clang fp contract(off)

namespace b4d {

// k_ssim: the 32 x 32 tiles and windows up to 63 per axis of b4d_window.hpp, as far as the LDS holds them; its own doubles behind
// the row sums are block_sum's (two sums, a slot per wave)
constexpr int PS_EXTRA = 2 * (WIN_PAIR_LANES / 64);
// pair errors: a lane takes groups of four consecutive pixels; a workgroup at most PE_GROUPS of them per lane
constexpr int PE_COLS = 8, PE_SUMS = 5, PE_GROUPS = 8, PE_MAX_SPLIT = 1024;

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

// ---------------------------------------------------------------------------------------------- SSIM
// grid (tiles_x * tiles_y, frames), 512 lanes.  The pair user of b4d_window.hpp, which states the padding and the order of the
// sums.  LDS by window_layout(2, 5, .., PS_EXTRA): R, X, both tiles with their halos as float32; five planes of float64 row sums (S_r,
// S_x, S_rr, S_xx, S_rx); sixteen doubles for the workgroup's sums.  Lanes 0 .. 255 stage the reference tile, lanes 256 .. 511 the
// image tile.  Row pass: one lane forms all five sums of a position, a tap costs two LDS reads for five FMAs.  Column pass: a lane
// forms the sums of two adjacent rows of its column from one read of the sy + 1 rows of the planes below them.
__global__ void __launch_bounds__(WIN_PAIR_LANES) k_ssim(SsimArgs a, WindowTaps t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int sy = t.sy, sx = t.sx, loy = sy / 2, lox = sx / 2;
    const WindowLayout l = window_layout(2, 5, sy, sx, PS_EXTRA);
    double* B = reinterpret_cast<double*>(lds + l.sums);
    double* sh = B + 5 * l.sum_plane;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * WIN_T, y0 = tile_y * WIN_T;
    const size_t fo = (size_t)blockIdx.y * a.ny * a.nx;
    const int tw = min(WIN_T, a.nx - x0), th = min(WIN_T, a.ny - y0);
    const int ha = th + sy - 1;
    if (threadIdx.x < 256)
        stage<NoSwz>(lds, l.pitch, a.ref + (size_t)a.ref_stride * blockIdx.y, a.ny, a.nx, y0 - loy, ha, x0 - lox, tw + sx - 1, a.mode, a.cval,
                     a.vec_ref != 0, threadIdx.x);
    else
        stage<NoSwz>(lds + l.plane, l.pitch, a.img + fo, a.ny, a.nx, y0 - loy, ha, x0 - lox, tw + sx - 1, a.mode, a.cval, a.vec_img != 0,
                     threadIdx.x - 256);
    __syncthreads();
    window_row_pass<2, WIN_PAIR_LANES>(lds, B, l, ha, tw, t);
    __syncthreads();
    const double iw = 1.0 / window_weight(t);   // the one division by W: the five window means are products with it
    const int c = threadIdx.x & 31, ox = x0 + c, ly = 2 * (threadIdx.x >> 5);
    WindowSums<5, 2> sums{};
    if (ly < th && ox < a.nx) sums = window_col_sums<5, 2>(B + ly * WIN_T + c, l.sum_plane, t);
    const auto& s = sums.s;
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
        block_sum(acc, sh, WIN_PAIR_LANES / 64);
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
    if (const int rc = check_window("b4d_ssim", size_y, size_x, taps_y, taps_x)) return rc;
    const size_t lds = window_layout(2, 5, size_y, size_x, PS_EXTRA).bytes;
    if (lds > WIN_LDS_LIMIT)
        return fail(B4D_ESIZE, "b4d_ssim: a " + std::to_string(size_y) + " x " + std::to_string(size_x) + " window needs " + std::to_string(lds) +
                                   " bytes of LDS, more than " + std::to_string(WIN_LDS_LIMIT));
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
    const WindowTaps t = fill_window_taps(size_y, size_x, taps_y, taps_x);
    SsimArgs a{};
    a.ref_stride = ref_stride;
    a.ny = ny;
    a.nx = nx;
    a.mode = mode;
    a.cval = cval;
    a.tiles_x = (int)tiles(nx, WIN_T);
    a.vec_ref = vec_ok(ref, nx, 16) && ref_stride % 4 == 0;
    a.vec_img = vec_ok(img, nx, 16);
    a.c1 = c1;
    a.c2 = c2;
    a.cov_norm = cov_norm;
    a.crop_y = crop_y;
    a.crop_x = crop_x;
    const unsigned ntiles = a.tiles_x * tiles(ny, WIN_T);
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
        return launch(k_ssim, dim3(ntiles, nb), dim3(WIN_PAIR_LANES), lds, st, a, t);
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
