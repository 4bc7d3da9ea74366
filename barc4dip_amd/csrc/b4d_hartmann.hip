// b4d_hartmann.hip -- spot centroids of a Hartmann / Shack-Hartmann frame over a lattice of rectangular cells (include/b4d.h
// "Hartmann sensor").  One entry point, one kernel:
//   b4d_spot_centroids  k_spot_centroids<VEC>  one workgroup per (frame, cell row, span of neighbouring cells)
// The workgroup stages the span -- the rows of the cell row by the columns of its cells -- in LDS with one read of the frame, then
// each of its four waves takes the cells w, w + 4, .. of the span and makes every pass over a cell from LDS.
// Summation order (part of the contract): lane l of the wave adds the pixels l, l + 64, l + 128, .. of the cell in row-major order,
// in float64, then the 64 partials go through wave_sum_all (b4d_reduce.hpp).  Nothing in it depends on the span, the frame or the
// batch, so a cell gives the same bits run to run, alone or anywhere in a stack.  No atomics, no inline assembly, plain stores.
#include <cfloat>
#include <climits>
#include <cmath>

#include "b4d_common.hpp"
#include "b4d_reduce.hpp"
#include "b4d_tile.hpp"

namespace b4d {
namespace {

constexpr int HT_THREADS = 256;
constexpr int HT_WAVES = HT_THREADS / 64;
constexpr int HT_MIN_SIDE = 2, HT_MAX_SIDE = 128;
constexpr int HT_STAGE_FLOATS = 16384;    // the staging limit: 64 KiB, one 128 x 128 cell
constexpr int HT_TARGET_FLOATS = 8192;    // what a span of small cells aims at: 32 KiB, five workgroups a CU
constexpr int HT_MAX_SPAN = 16;           // cells per span at most: a row of tiny cells still spreads over many workgroups
constexpr int HT_NQ = 14;

struct HtArgs {
    const float* frames;
    int ny, nx, gy, gx, nspan;
    const int32_t* ye;
    const int32_t* xe;
    int bg_mode;
    double bg_value, threshold;
    int method;
    double two_s2;
    int iterations;
    double saturation;
    double* out;
};

// f(v, r, c, p) for the pixels p = lane, lane + 64, .. < h * w of a cell (row r, column c; p = r * w + c) whose first pixel is at
// `cell` in a staged span of `stride` floats a row.  One division per lane: 64 = dq * w + dr, a step adds dq rows and dr columns.
template <class F>
__device__ __forceinline__ void walk_cell(const float* cell, int stride, int h, int w, int lane, F f) {
    const int n = h * w, dq = 64 / w, dr = 64 - dq * w;
    int r = lane / w, c = lane - r * w;
    for (int p = lane; p < n; p += 64) {
        f(cell[r * stride + c], r, c, p);
        c += dr;
        r += dq;
        if (c >= w) {
            c -= w;
            ++r;
        }
    }
}

// grid (spans, nb * gy): blockIdx.y = frame * gy + cell row.  VEC: nx % 4 == 0 and the stack on 16 bytes, so the first 16-byte
// boundary of every row of the span is the same xs & 3 columns in; the columns in front of it and behind the last whole group,
// and every column of an unaligned stack, are loaded one by one.
template <bool VEC>
__global__ void __launch_bounds__(HT_THREADS) k_spot_centroids(HtArgs a, int frame0) {
    extern __shared__ __align__(16) float tile[];
    const int fr = blockIdx.y / a.gy, ci = blockIdx.y - fr * a.gy;
    const int frame = frame0 + fr;
    const int y0 = a.ye[ci], h = a.ye[ci + 1] - y0;
    const int j0 = blockIdx.x * a.nspan, j1 = min(a.gx, j0 + a.nspan);
    const int xs = a.xe[j0], W = a.xe[j1] - xs;
    const float* src = a.frames + ((size_t)frame * a.ny + y0) * a.nx + xs;

    const int head = VEC ? min((4 - (xs & 3)) & 3, W) : W, body = (W - head) >> 2, tail = W - head - 4 * body;
    const int units = head + body + tail;
    for (int idx = threadIdx.x; idx < h * units; idx += HT_THREADS) {
        const int r = idx / units, u = idx - r * units;
        const float* row = src + (size_t)r * a.nx;
        float* dst = tile + r * W;
        if (u < body) {
            const int c = head + 4 * u;
            const float4 q = *reinterpret_cast<const float4*>(row + c);
            if (((r * W + c) & 3) == 0) {
                *reinterpret_cast<float4*>(dst + c) = q;
            } else {
                dst[c] = q.x;
                dst[c + 1] = q.y;
                dst[c + 2] = q.z;
                dst[c + 3] = q.w;
            }
        } else {
            const int k = u - body;
            const int c = k < head ? k : 4 * body + k;
            dst[c] = row[c];
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int j = j0 + wave; j < j1; j += HT_WAVES) {
        const int x0 = a.xe[j], w = a.xe[j + 1] - x0;
        const float* cell = tile + (x0 - xs);

        // pass 1: peak, minimum, counts, ring sum
        float pv = -INFINITY, mn = INFINITY;
        int pi = INT_MAX;
        unsigned n_nan = 0, n_sat = 0, rn = 0;
        double rs = 0.0;
        walk_cell(cell, W, h, w, lane, [&](float v, int r, int c, int p) __attribute__((always_inline)) {
            // without a branch: a NaN never wins argmax_merge or fminf and compares false
            const bool ok = v == v, edge = ok && (r == 0 || r == h - 1 || c == 0 || c == w - 1);
            n_nan += ok ? 0u : 1u;
            argmax_merge(pv, pi, v, p);
            mn = fminf(mn, v);
            n_sat += (double)v >= a.saturation ? 1u : 0u;
            rs += edge ? (double)v : 0.0;
            rn += edge ? 1u : 0u;
        });
        wave_argmax_all(pv, pi);
        mn = -__shfl(wave_max(-mn), 0, 64);
        n_nan = wave_sum_all(n_nan);
        n_sat = wave_sum_all(n_sat);
        rn = wave_sum_all(rn);
        rs = wave_sum_all(rs);
        const bool any = pi != INT_MAX;
        const double peak = any ? (double)pv : nan;
        const int pr = any ? pi / w : 0, pc = any ? pi - pr * w : 0;
        const double ring = rn ? rs / (double)rn : nan;
        const double b = a.bg_mode == 0 ? 0.0 : a.bg_mode == 1 ? a.bg_value : a.bg_mode == 2 ? (any ? (double)mn : nan) : ring;
        const double t = b + a.threshold * (peak - b);

        // pass 2: ring variance about its mean; flux and first moments about the cell's geometric centre
        const double yc = 0.5 * (double)(h - 1), xc = 0.5 * (double)(w - 1);
        double q = 0.0, F = 0.0, Sy = 0.0, Sx = 0.0;
        unsigned npix = 0;
        walk_cell(cell, W, h, w, lane, [&](float v, int r, int c, int) __attribute__((always_inline)) {
            if (v != v) return;
            if (r == 0 || r == h - 1 || c == 0 || c == w - 1) {
                const double d = (double)v - ring;
                q += d * d;
            }
            const double d = (double)v - t;
            if (d > 0.0) {
                ++npix;
                F += d;
                Sy += d * ((double)r - yc);
                Sx += d * ((double)c - xc);
            }
        });
        q = wave_sum_all(q);
        F = wave_sum_all(F);
        Sy = wave_sum_all(Sy);
        Sx = wave_sum_all(Sx);
        npix = wave_sum_all(npix);
        const double noise = rn >= 2 ? sqrt(q / (double)rn) : 0.0;
        const bool lit = F > 0.0;
        const double cyc = (double)y0 + yc, cxc = (double)x0 + xc;      // the cell centre in frame coordinates
        double cy = lit ? cyc + Sy / F : nan, cx = lit ? cxc + Sx / F : nan;
        double vyy = nan, vxx = nan, vyx = nan;
        if (lit) {
            // pass 3: second moments about the centre of gravity
            double Myy = 0.0, Mxx = 0.0, Myx = 0.0;
            walk_cell(cell, W, h, w, lane, [&](float v, int r, int c, int) __attribute__((always_inline)) {
                const double d = (double)v - t;
                if (d > 0.0) {      // false for a NaN pixel
                    const double ey = (double)(y0 + r) - cy, ex = (double)(x0 + c) - cx;
                    Myy += d * ey * ey;
                    Mxx += d * ex * ex;
                    Myx += d * ey * ex;
                }
            });
            vyy = wave_sum_all(Myy) / F;
            vxx = wave_sum_all(Mxx) / F;
            vyx = wave_sum_all(Myx) / F;
            if (a.method == 1) {
                for (int it = 0; it < a.iterations; ++it) {
                    double G = 0.0, Gy = 0.0, Gx = 0.0;
                    walk_cell(cell, W, h, w, lane, [&](float v, int r, int c, int) __attribute__((always_inline)) {
                        const double d = (double)v - t;
                        if (d > 0.0) {
                            const double ey = (double)(y0 + r) - cy, ex = (double)(x0 + c) - cx;
                            const double g = d * exp(-(ey * ey + ex * ex) / a.two_s2);
                            G += g;
                            Gy += g * ((double)r - yc);
                            Gx += g * ((double)c - xc);
                        }
                    });
                    G = wave_sum_all(G);
                    Gy = wave_sum_all(Gy);
                    Gx = wave_sum_all(Gx);
                    cy = cyc + Gy / G;
                    cx = cxc + Gx / G;
                }
            }
        }
        if (lane == 0) {
            double* o = a.out + (((size_t)frame * a.gy + ci) * a.gx + j) * HT_NQ;
            o[0] = cy;
            o[1] = cx;
            o[2] = lit ? F : 0.0;
            o[3] = peak;
            o[4] = any ? (double)(y0 + pr) : nan;
            o[5] = any ? (double)(x0 + pc) : nan;
            o[6] = b;
            o[7] = noise;
            o[8] = vyy;
            o[9] = vxx;
            o[10] = vyx;
            o[11] = lit ? (double)npix : 0.0;
            o[12] = (double)n_sat;
            o[13] = (double)n_nan;
        }
    }
}

// edges of one axis: n + 1 ascending values, every side in 2 .. 128, all inside [0, side]; *smax = the longest side
int check_edges(const int32_t* e, int n, int side, const char* name, int* smax) {
    const std::string f = std::string("b4d_spot_centroids: ") + name + " edges ";
    if (e[0] < 0 || e[n] > side) return fail(B4D_EINVAL, f + "leave the frame");
    *smax = 0;
    for (int i = 0; i < n; ++i) {
        const long long s = (long long)e[i + 1] - e[i];
        if (s < 1) return fail(B4D_EINVAL, f + "must ascend");
        if (s < HT_MIN_SIDE || s > HT_MAX_SIDE) return fail(B4D_ESIZE, f + "give a cell side outside 2 .. 128");
        *smax = std::max(*smax, (int)s);
    }
    return B4D_OK;
}

}  // namespace
}  // namespace b4d

using namespace b4d;

extern "C" int b4d_spot_centroids(const float* frames, int batch, int ny, int nx, const int32_t* y_edges, int gy, const int32_t* x_edges,
                                  int gx, int background_mode, double background_value, double threshold, int method, double sigma,
                                  int iterations, double saturation, double* out, void* stream) {
    if (!frames || !y_edges || !x_edges || !out) return fail(B4D_EINVAL, "b4d_spot_centroids: null pointer");
    if (batch < 1 || ny < 1 || nx < 1 || gy < 1 || gx < 1) return fail(B4D_EINVAL, "b4d_spot_centroids: batch, frame or lattice empty");
    if ((long long)ny * nx >= (1LL << 31)) return fail(B4D_ESIZE, "b4d_spot_centroids: 2^31 or more pixels per frame");
    if (gy > MAX_GRID_FRAMES) return fail(B4D_ESIZE, "b4d_spot_centroids: more than 65535 cell rows");
    if (background_mode < 0 || background_mode > 3)
        return fail(B4D_EINVAL, "b4d_spot_centroids: background_mode must be 0 none, 1 value, 2 minimum or 3 border");
    if (background_mode == 1 && !std::isfinite(background_value)) return fail(B4D_EINVAL, "b4d_spot_centroids: background_value must be finite");
    if (!(threshold >= 0.0 && threshold < 1.0)) return fail(B4D_EINVAL, "b4d_spot_centroids: threshold must be in [0, 1)");
    if (method != 0 && method != 1) return fail(B4D_EINVAL, "b4d_spot_centroids: method must be 0 (centre of gravity) or 1 (iteratively weighted)");
    if (method == 1 && (!(sigma > 0.0) || !std::isfinite(sigma) || iterations < 0))
        return fail(B4D_EINVAL, "b4d_spot_centroids: method 1 takes sigma > 0 and iterations >= 0");
    if (saturation != saturation) return fail(B4D_EINVAL, "b4d_spot_centroids: saturation is NaN");
    if (!ptr_aligned(frames, 4) || !ptr_aligned(out, 8)) return fail(B4D_EINVAL, "b4d_spot_centroids: frames on 4 bytes, out on 8");
    int hmax, wmax;
    if (const int rc = check_edges(y_edges, gy, ny, "y", &hmax)) return rc;
    if (const int rc = check_edges(x_edges, gx, nx, "x", &wmax)) return rc;

    // cells per span from the largest cell, then the widest span for the LDS size
    const int nspan = std::max(1, std::min({HT_MAX_SPAN, HT_TARGET_FLOATS / (hmax * wmax), gx}));
    const int spans = (gx + nspan - 1) / nspan;
    int wspan = 0;
    for (int s = 0; s < spans; ++s) wspan = std::max(wspan, (int)(x_edges[std::min(gx, (s + 1) * nspan)] - x_edges[s * nspan]));
    const size_t lds = (size_t)hmax * wspan * sizeof(float);
    if (lds > (size_t)HT_STAGE_FLOATS * sizeof(float)) return fail(B4D_ESIZE, "b4d_spot_centroids: a span beyond the staging limit");

    hipStream_t st = (hipStream_t)stream;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    if (const int rc = get_scratch(sizeof(int32_t) * ((size_t)gy + gx + 2), &scratch, st)) return rc;
    int32_t* d_edges = static_cast<int32_t*>(scratch);
    B4D_HIP(hipMemcpyAsync(d_edges, y_edges, sizeof(int32_t) * (gy + 1), hipMemcpyHostToDevice, st));
    B4D_HIP(hipMemcpyAsync(d_edges + gy + 1, x_edges, sizeof(int32_t) * (gx + 1), hipMemcpyHostToDevice, st));

    HtArgs a{};
    a.frames = frames;
    a.ny = ny;
    a.nx = nx;
    a.gy = gy;
    a.gx = gx;
    a.nspan = nspan;
    a.ye = d_edges;
    a.xe = d_edges + gy + 1;
    a.bg_mode = background_mode;
    a.bg_value = background_value;
    a.threshold = threshold;
    a.method = method;
    a.two_s2 = 2.0 * sigma * sigma;
    a.iterations = iterations;
    a.saturation = saturation;
    a.out = out;
    const bool vec = vec_ok(frames, nx, 16);
    return for_frame_chunks(batch, std::max(1, MAX_GRID_FRAMES / gy), [&](int b0, int nb) {
        return launch(vec ? k_spot_centroids<true> : k_spot_centroids<false>, dim3(spans, nb * gy), dim3(HT_THREADS), lds, st, a, b0);
    });
}
