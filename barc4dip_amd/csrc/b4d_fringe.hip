// b4d_fringe.hip -- fringe analysis of grating interferograms: windowed Fourier demodulation of frames
// at a few carriers, the elementwise comparison of sample and reference harmonics, the phase -> displacement map, and the node
// weights of the weighted unwrap.
//
// Harmonic map of carrier f = (fy, fx) on the window grid (origins y0 = Y sty, x0 = X stx, half-sample Hann taper h):
//   S_f[Y][X] = sum_j sum_i h_wy[j] h_wx[i] I[y0+j][x0+i] exp(-2 pi i (fy (y0+j) + fx (x0+i))) / (sum h_wy . sum h_wx)
// The phasor takes ABSOLUTE pixel coordinates and separates into e_y[y] e_x[x]: k_fr_tables writes h_wy, h_wx and, per carrier,
// e_y (H entries) and e_x (W entries), the argument f y reduced modulo 1 in float64 before it is rounded to float32.
// k_fr_demod then reads the frame once per band of windows: lanes along x own four neighbouring columns (one 16-byte load a
// row where the rows are 16-byte aligned) and sum them down the wy rows of the band with the weights h_wy[j] e_y[y]; the 1 + 2K
// column sums of the tile go to LDS, from where one wave per window takes the x sums with h_wx[i] e_x[x] and reduces them by
// shuffles.  A workgroup walks FR_BANDS consecutive bands of one x tile, so the rows that overlapping bands share are read
// twice in close succession (from the Infinity Cache at best: DESIGN.md section 17 has the measurement and the remedy).
// Every sum has a fixed order that depends on the geometry alone.
#include <cmath>
#include <string>

#include "b4d_common.hpp"
#include "b4d_reduce.hpp"

namespace b4d {

constexpr int FR_MAX_K = 4;
constexpr int FR_MAX_WINDOW = 256;
constexpr int FR_THREADS = 256;
constexpr int FR_COLS = 4;                          // columns per lane
constexpr int FR_TILE = FR_THREADS * FR_COLS;       // pixel columns of a tile
constexpr int FR_BANDS = 8;                         // bands of windows that one workgroup walks

struct FrCarriers {
    double fy[FR_MAX_K], fx[FR_MAX_K];
};

// float tables in the caller's workspace
struct FrTables {
    float* hy;        // (wy)
    float* hx;        // (wx)
    float2* ey;       // (K, H)   exp(-2 pi i fy y)
    float2* ex;       // (K, W)   exp(-2 pi i fx x)
};

static size_t fr_layout(char* base, int K, int H, int W, int wy, int wx, FrTables& t) {
    size_t o = 0;
    t.hy = (float*)(base + o), o += align256((size_t)wy * sizeof(float));
    t.hx = (float*)(base + o), o += align256((size_t)wx * sizeof(float));
    t.ey = (float2*)(base + o), o += align256((size_t)K * H * sizeof(float2));
    t.ex = (float2*)(base + o), o += align256((size_t)K * W * sizeof(float2));
    return o;
}

// exp(-2 pi i f c) with f c reduced to [-1/2, 1/2] turns in float64: the product of a double and an integer below 2^24 carries
// an error below 2^-29 turns even before the reduction would matter, and the reduced turn is rounded to float32 once
__device__ __forceinline__ float2 fr_phasor(double f, int c) {
    const double p = f * (double)c;
    const double r = p - rint(p);
    double s, co;
    sincospi(-2.0 * r, &s, &co);
    return make_float2((float)co, (float)s);
}

__device__ __forceinline__ float fr_hann(int j, int w) { return (float)(0.5 - 0.5 * cospi(2.0 * ((double)j + 0.5) / (double)w)); }

// grid ceil(max(H, W, wy, wx) / 256)
__global__ void __launch_bounds__(256) k_fr_tables(FrTables t, FrCarriers f, int K, int H, int W, int wy, int wx) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < wy) t.hy[e] = fr_hann(e, wy);
    if (e < wx) t.hx[e] = fr_hann(e, wx);
    for (int k = 0; k < K; ++k) {
        if (e < H) t.ey[(size_t)k * H + e] = fr_phasor(f.fy[k], e);
        if (e < W) t.ex[(size_t)k * W + e] = fr_phasor(f.fx[k], e);
    }
}

struct FrGeom {
    int H, W, wy, wx, sty, stx, gy, gx;
    int nxw;          // windows along x per tile
    int vec;          // rows are 16-byte aligned: one 16-byte load per lane and row
    float norm;       // 1 / (sum h_wy . sum h_wx)
};

// grid (x tiles, groups of FR_BANDS bands, frames); LDS: (1 + 2K) rows of FR_TILE column sums
template <int K>
__global__ void __launch_bounds__(FR_THREADS) k_fr_demod(const float* __restrict__ frames, FrTables t, FrGeom g,
                                                         float2* __restrict__ out) {
    constexpr int NC = 1 + 2 * K;
    __shared__ float col[NC][FR_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X0 = blockIdx.x * g.nxw;                                 // first window of the tile
    const int nxw = min(g.nxw, g.gx - X0);
    const int xa = g.vec ? (X0 * g.stx) & ~3 : X0 * g.stx;             // first pixel column of the tile
    const int span = (X0 + nxw - 1) * g.stx + g.wx - xa;               // <= FR_TILE (host)
    const int xl = FR_COLS * threadIdx.x;                              // this lane's first column in the tile
    const int x = xa + xl;
    const bool active = xl < span;
    const float* __restrict__ frame = frames + (size_t)blockIdx.z * g.H * g.W;
    float2* __restrict__ fo = out + (size_t)blockIdx.z * (K + 1) * g.gy * g.gx;
    const int Y1 = min(g.gy, ((int)blockIdx.y + 1) * FR_BANDS);
    for (int Y = blockIdx.y * FR_BANDS; Y < Y1; ++Y) {
        const int y0 = Y * g.sty;
        float a0[FR_COLS], ar[K][FR_COLS], ai[K][FR_COLS];
#pragma unroll
        for (int c = 0; c < FR_COLS; ++c) {
            a0[c] = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) ar[k][c] = ai[k][c] = 0.f;
        }
        if (active) {
#pragma unroll 4
            for (int j = 0; j < g.wy; ++j) {
                const float* __restrict__ row = frame + (size_t)(y0 + j) * g.W;
                float v[FR_COLS];
                if (g.vec && x + FR_COLS <= g.W) {
                    const float4 q = *reinterpret_cast<const float4*>(row + x);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int c = 0; c < FR_COLS; ++c) v[c] = x + c < g.W ? row[x + c] : 0.f;
                }
                const float h = t.hy[j];
#pragma unroll
                for (int c = 0; c < FR_COLS; ++c) {
                    v[c] *= h;
                    a0[c] += v[c];
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 e = t.ey[(size_t)k * g.H + y0 + j];
#pragma unroll
                    for (int c = 0; c < FR_COLS; ++c) {
                        ar[k][c] = fmaf(e.x, v[c], ar[k][c]);
                        ai[k][c] = fmaf(e.y, v[c], ai[k][c]);
                    }
                }
            }
        }
        *reinterpret_cast<float4*>(&col[0][xl]) = make_float4(a0[0], a0[1], a0[2], a0[3]);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            *reinterpret_cast<float4*>(&col[1 + 2 * k][xl]) = make_float4(ar[k][0], ar[k][1], ar[k][2], ar[k][3]);
            *reinterpret_cast<float4*>(&col[2 + 2 * k][xl]) = make_float4(ai[k][0], ai[k][1], ai[k][2], ai[k][3]);
        }
        __syncthreads();
        // x sums: wave w takes windows w, w + 4, ...; lane l the taps l, l + 64, ...; then the 64 partials by shuffles
        for (int Xw = wave; Xw < nxw; Xw += FR_THREADS / 64) {
            const int x0 = (X0 + Xw) * g.stx;
            float s0 = 0.f, sr[K], si[K];
#pragma unroll
            for (int k = 0; k < K; ++k) sr[k] = si[k] = 0.f;
            for (int i = lane; i < g.wx; i += 64) {
                const float h = t.hx[i];
                const int cl = x0 + i - xa;
                s0 = fmaf(h, col[0][cl], s0);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float2 e = t.ex[(size_t)k * g.W + x0 + i];
                    const float cr = h * col[1 + 2 * k][cl], ci = h * col[2 + 2 * k][cl];
                    sr[k] += e.x * cr - e.y * ci;
                    si[k] += e.x * ci + e.y * cr;
                }
            }
            s0 = wave_sum(s0);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                sr[k] = wave_sum(sr[k]);
                si[k] = wave_sum(si[k]);
            }
            if (lane == 0) {
                const size_t node = (size_t)Y * g.gx + X0 + Xw, plane = (size_t)g.gy * g.gx;
                fo[node] = make_float2(s0 * g.norm, 0.f);
#pragma unroll
                for (int k = 0; k < K; ++k) fo[(size_t)(k + 1) * plane + node] = make_float2(sr[k] * g.norm, si[k] * g.norm);
            }
        }
        __syncthreads();
    }
}

// ---- comparison of sample harmonics S with reference harmonics R (K + 1 planes each, plane 0 the window mean), per node:
//   phase_k = arg(S_k conj R_k) in (-pi, pi] (arg S_k without a reference), visibility_k = 2 |S_k| / S_0,
//   transmission = S_0 / R_0, dark_field_k = (|S_k| / S_0) / (|R_k| / R_0), peak = min_k visibility_k
// grid (ceil(plane / 256), n)
__global__ void __launch_bounds__(256) k_fr_compare(const float2* __restrict__ S, const float2* __restrict__ R, long long r_stride,
                                                    int K, int plane, float* __restrict__ phase, float* __restrict__ vis,
                                                    float* __restrict__ trans, float* __restrict__ dark, double* __restrict__ peak) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= plane) return;
    const size_t m = blockIdx.y;
    const float2* __restrict__ s = S + m * (size_t)(K + 1) * plane + e;
    const float2* __restrict__ r = R ? R + m * r_stride + e : nullptr;
    const float s0 = s[0].x;
    const float r0 = r ? r[0].x : 1.f;
    if (r) trans[m * plane + e] = s0 / r0;
    float pk = 0.f;
    for (int k = 0; k < K; ++k) {
        const float2 a = s[(size_t)(k + 1) * plane];
        float2 p = a;
        const float va = hypotf(a.x, a.y) / s0;
        if (r) {
            const float2 b = r[(size_t)(k + 1) * plane];
            p = make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
            dark[(m * K + k) * plane + e] = va / (hypotf(b.x, b.y) / r0);
        }
        float ph = atan2f(p.y, p.x);
        if (ph <= -(float)M_PI) ph = (float)M_PI;
        phase[(m * K + k) * plane + e] = ph;
        const float v = 2.f * va;
        vis[(m * K + k) * plane + e] = v;
        pk = (k == 0 || v < pk || v != v) ? v : pk;
    }
    peak[m * plane + e] = (double)pk;
}

// (dy, dx) = -Minv (phase_1, phase_2) / 2 pi in float64.  grid (ceil(plane / 256), n)
__global__ void __launch_bounds__(256) k_fr_shift(const float* __restrict__ p1, const float* __restrict__ p2, long long stride, int plane,
                                                  double m00, double m01, double m10, double m11, double* __restrict__ dy,
                                                  double* __restrict__ dx) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= plane) return;
    const size_t m = blockIdx.y;
    const double a = (double)p1[m * stride + e], b = (double)p2[m * stride + e];
    dy[m * plane + e] = -(m00 * a + m01 * b) * (0.5 * M_1_PI);
    dx[m * plane + e] = -(m10 * a + m11 * b) * (0.5 * M_1_PI);
}

// ---- node weights for the weighted unwrap.  A node is valid if S_0 >= min_level max(S_0 of its frame),
// the same for R_0 where there is a reference, and every visibility 2 |S_k| / S_0 (and 2 |R_k| / R_0) >= min_visibility; a
// threshold <= 0 switches its test off.  The tests are made in float64 on the float32 harmonics.  Weight of carrier k at a valid
// node: mode 0: 1; mode 1: |S_k|^2 / S_0, with a reference 1 / (S_0 / |S_k|^2 + R_0 / |R_k|^2) (inverse shot-noise phase variance);
// 0 where that is not finite and positive.
constexpr int FR_W_THREADS = 256;
constexpr int FR_W_MAXBLOCKS = 256;   // partial maxima per frame

__device__ __forceinline__ double fr_abs2(float2 a) { return (double)a.x * (double)a.x + (double)a.y * (double)a.y; }

static int fr_w_blocks(long long plane) {
    const long long b = (plane + FR_W_THREADS - 1) / FR_W_THREADS;
    return (int)(b < FR_W_MAXBLOCKS ? b : FR_W_MAXBLOCKS);
}

// stage 1 of the frame maximum of plane 0: workgroup b of frame m strides over the nodes and writes part[m nb + b].  A maximum
// does not depend on the order it is taken in; non-finite values never win a comparison (-inf for a frame without a finite one).
// grid (nb, frames of S, 2): z = 1 takes the reference, which has nr frames
__global__ void __launch_bounds__(FR_W_THREADS) k_fr_level_partials(const float2* __restrict__ S, const float2* __restrict__ R, int nr,
                                                                    long long frame_stride, int plane, int nb, float* __restrict__ part_s,
                                                                    float* __restrict__ part_r) {
    __shared__ float sh[FR_W_THREADS / 64];
    const int m = blockIdx.y, ref = blockIdx.z;
    if (ref && (!R || m >= nr)) return;
    const float2* __restrict__ h = (ref ? R : S) + (size_t)m * frame_stride;
    float best = -INFINITY;
    for (int e = blockIdx.x * FR_W_THREADS + threadIdx.x; e < plane; e += nb * FR_W_THREADS) {
        const float v = h[e].x;
        if (v > best && v < INFINITY) best = v;
    }
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FR_W_THREADS / 64; ++w) best = fmaxf(best, sh[w]);
        (ref ? part_r : part_s)[(size_t)m * nb + blockIdx.x] = best;
    }
}

// stage 2 (every workgroup of a frame takes the maximum of its nb partials in index order) and the weights.  grid (ceil(plane / 256), n)
__global__ void __launch_bounds__(FR_W_THREADS) k_fr_weights(const float2* __restrict__ S, const float2* __restrict__ R, long long r_stride,
                                                             int K, int plane, int nb, const float* __restrict__ part_s,
                                                             const float* __restrict__ part_r, double min_level, double min_vis, int mode,
                                                             float* __restrict__ w_out) {
    __shared__ float top[2];
    const size_t m = blockIdx.y;
    if (threadIdx.x < 2 && min_level > 0.0) {     // without a level test there are no partials
        const float* __restrict__ part = threadIdx.x == 0 ? part_s + m * nb : part_r + (r_stride ? m * nb : 0);
        float best = -INFINITY;
        if (threadIdx.x == 0 || R)
            for (int b = 0; b < nb; ++b) best = fmaxf(best, part[b]);
        top[threadIdx.x] = best;
    }
    __syncthreads();
    const int e = blockIdx.x * FR_W_THREADS + threadIdx.x;
    if (e >= plane) return;
    const float2* __restrict__ s = S + m * (size_t)(K + 1) * plane + e;
    const float2* __restrict__ r = R ? R + m * r_stride + e : nullptr;
    const double s0 = (double)s[0].x, r0 = r ? (double)r[0].x : 1.0;
    bool ok = true;
    if (min_level > 0.0) ok = s0 >= min_level * (double)top[0] && (!r || r0 >= min_level * (double)top[1]);
    if (min_vis > 0.0)
        for (int k = 0; k < K; ++k) {
            ok = ok && 2.0 * sqrt(fr_abs2(s[(size_t)(k + 1) * plane])) / s0 >= min_vis;
            if (r) ok = ok && 2.0 * sqrt(fr_abs2(r[(size_t)(k + 1) * plane])) / r0 >= min_vis;
        }
    for (int k = 0; k < K; ++k) {     // the validity is that of all carriers, the value that of carrier k
        double inv = s0 / fr_abs2(s[(size_t)(k + 1) * plane]);
        if (r) inv += r0 / fr_abs2(r[(size_t)(k + 1) * plane]);
        const float v = mode == 0 ? 1.f : (float)(1.0 / inv);
        w_out[(m * K + k) * plane + e] = (ok && v > 0.f && isfinite(v)) ? v : 0.f;
    }
}

// k_fr_shift from a wrapped map and its unwrapped copy: the float32 unwrapped phase carries half a spacing of up to tens of radians,
// so the phase is formed again in float64 as wrapped + 2 pi round((unwrapped - wrapped) / 2 pi); NaN where the unwrapped map is NaN.
__global__ void __launch_bounds__(256) k_fr_shift_levels(const float* __restrict__ w1, const float* __restrict__ w2,
                                                         const float* __restrict__ u1, const float* __restrict__ u2, long long stride,
                                                         int plane, double m00, double m01, double m10, double m11,
                                                         double* __restrict__ dy, double* __restrict__ dx) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= plane) return;
    const size_t m = blockIdx.y;
    const double wa = (double)w1[m * stride + e], wb = (double)w2[m * stride + e];
    const double a = wa + 2.0 * M_PI * rint(((double)u1[m * stride + e] - wa) * (0.5 * M_1_PI));
    const double b = wb + 2.0 * M_PI * rint(((double)u2[m * stride + e] - wb) * (0.5 * M_1_PI));
    dy[m * plane + e] = -(m00 * a + m01 * b) * (0.5 * M_1_PI);
    dx[m * plane + e] = -(m10 * a + m11 * b) * (0.5 * M_1_PI);
}

static int fr_check_shift(const void* p1, const void* p2, long long stride, int n, int gy, int gx, const double* minv, const void* dy,
                          const void* dx) {
    if (!p1 || !p2 || !minv || !dy || !dx) return fail(B4D_EINVAL, "null argument");
    if (n < 1 || gy < 1 || gx < 1) return fail(B4D_EINVAL, "fringe: map count and sides must be >= 1");
    if (n > 65535) return fail(B4D_ESIZE, "fringe: at most 65535 maps per call");
    const long long plane = (long long)gy * gx;
    if (plane > (1LL << 28)) return fail(B4D_ESIZE, "fringe: grids are limited to 2^28 nodes");
    if (stride < plane) return fail(B4D_EINVAL, "fringe: the map stride is at least gy * gx");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(minv[k])) return fail(B4D_EINVAL, "fringe: the inverse carrier matrix must be finite");
    return B4D_OK;
}

static int fr_check(int n, int K, int H, int W, int wy, int wx, int sty, int stx) {
    if (n < 1 || H < 1 || W < 1) return fail(B4D_EINVAL, "fringe: frame count and sides must be >= 1");
    if (n > 65535) return fail(B4D_ESIZE, "fringe: at most 65535 frames per call");
    if (K < 1 || K > FR_MAX_K) return fail(B4D_EINVAL, "fringe: 1 .. " + std::to_string(FR_MAX_K) + " carriers, got " + std::to_string(K));
    if (wy < 2 || wx < 2 || wy > FR_MAX_WINDOW || wx > FR_MAX_WINDOW)
        return fail(B4D_ESIZE, "fringe: the window is limited to 2 .. " + std::to_string(FR_MAX_WINDOW) + " px per axis, got (" +
                                   std::to_string(wy) + ", " + std::to_string(wx) + ")");
    if (sty < 1 || stx < 1) return fail(B4D_EINVAL, "fringe: the step must be >= 1 per axis");
    if (wy > H || wx > W) return fail(B4D_EINVAL, "fringe: the window does not fit in the frame");
    if ((long long)H * W > (1LL << 30) || H >= (1 << 24) || W >= (1 << 24)) return fail(B4D_ESIZE, "fringe: frames are limited to 2^30 pixels");
    return B4D_OK;
}

template <int K>
static void fr_launch(const float* frames, const FrTables& t, const FrGeom& g, int n, float2* out, hipStream_t st) {
    const dim3 grid((g.gx + g.nxw - 1) / g.nxw, (g.gy + FR_BANDS - 1) / FR_BANDS, n);
    hipLaunchKernelGGL(k_fr_demod<K>, grid, dim3(FR_THREADS), 0, st, frames, t, g, out);
}

}  // namespace b4d

using namespace b4d;

extern "C" size_t b4d_fringe_demodulate_workspace_bytes(int n_carriers, int H, int W, int wy, int wx) {
    if (n_carriers < 1 || n_carriers > FR_MAX_K || H < 1 || W < 1 || wy < 2 || wx < 2 || wy > FR_MAX_WINDOW || wx > FR_MAX_WINDOW) return 0;
    FrTables t;
    return fr_layout(nullptr, n_carriers, H, W, wy, wx, t);
}

extern "C" int b4d_fringe_demodulate(const float* frames, int n, int H, int W, const double* carriers, int n_carriers, int wy, int wx,
                                     int sty, int stx, void* workspace, void* out, void* stream) {
    if (!frames || !carriers || !workspace || !out) return fail(B4D_EINVAL, "null argument");
    const int K = n_carriers;
    if (const int rc = fr_check(n, K, H, W, wy, wx, sty, stx)) return rc;
    FrCarriers f{};
    for (int k = 0; k < K; ++k) {
        f.fy[k] = carriers[2 * k], f.fx[k] = carriers[2 * k + 1];
        if (!std::isfinite(f.fy[k]) || !std::isfinite(f.fx[k])) return fail(B4D_EINVAL, "fringe: carriers must be finite");
    }
    hipStream_t st = (hipStream_t)stream;
    FrTables t;
    fr_layout((char*)workspace, K, H, W, wy, wx, t);
    FrGeom g;
    g.H = H, g.W = W, g.wy = wy, g.wx = wx, g.sty = sty, g.stx = stx;
    g.gy = (H - wy) / sty + 1, g.gx = (W - wx) / stx + 1;
    g.vec = (W % 4 == 0) && ((uintptr_t)frames % 16 == 0);
    // windows per tile: the tile spans (nxw - 1) stx + wx columns plus up to 3 of alignment, balanced over the tiles of a row
    const int fit = (FR_TILE - 3 - wx) / stx + 1;
    const int tiles = (g.gx + fit - 1) / fit;
    g.nxw = (g.gx + tiles - 1) / tiles;
    double shy = 0.0, shx = 0.0;
    for (int j = 0; j < wy; ++j) shy += 0.5 - 0.5 * std::cos(2.0 * M_PI * (j + 0.5) / wy);
    for (int i = 0; i < wx; ++i) shx += 0.5 - 0.5 * std::cos(2.0 * M_PI * (i + 0.5) / wx);
    g.norm = (float)(1.0 / (shy * shx));
    const int longest = std::max(std::max(H, W), std::max(wy, wx));
    hipLaunchKernelGGL(k_fr_tables, dim3((longest + 255) / 256), dim3(256), 0, st, t, f, K, H, W, wy, wx);
    switch (K) {
        case 1: fr_launch<1>(frames, t, g, n, (float2*)out, st); break;
        case 2: fr_launch<2>(frames, t, g, n, (float2*)out, st); break;
        case 3: fr_launch<3>(frames, t, g, n, (float2*)out, st); break;
        default: fr_launch<4>(frames, t, g, n, (float2*)out, st); break;
    }
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_fringe_compare(const void* sample, const void* reference, long long reference_stride, int n, int n_carriers, int gy,
                                  int gx, float* phase, float* visibility, float* transmission, float* dark_field, double* peak,
                                  void* stream) {
    if (!sample || !phase || !visibility || !peak) return fail(B4D_EINVAL, "null argument");
    if (reference && (!transmission || !dark_field)) return fail(B4D_EINVAL, "fringe: a reference needs transmission and dark_field");
    if (n < 1 || gy < 1 || gx < 1) return fail(B4D_EINVAL, "fringe: map count and sides must be >= 1");
    if (n > 65535) return fail(B4D_ESIZE, "fringe: at most 65535 maps per call");
    if (n_carriers < 1 || n_carriers > FR_MAX_K) return fail(B4D_EINVAL, "fringe: 1 .. " + std::to_string(FR_MAX_K) + " carriers");
    const long long plane = (long long)gy * gx;
    if (plane > (1LL << 28)) return fail(B4D_ESIZE, "fringe: grids are limited to 2^28 nodes");
    if (reference && reference_stride != 0 && reference_stride != (n_carriers + 1) * plane)
        return fail(B4D_EINVAL, "fringe: reference_stride is 0 (shared reference) or (n_carriers + 1) * gy * gx (paired)");
    hipLaunchKernelGGL(k_fr_compare, dim3((unsigned)((plane + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, (const float2*)sample,
                       (const float2*)reference, reference_stride, n_carriers, (int)plane, phase, visibility, transmission, dark_field, peak);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" size_t b4d_fringe_weights_workspace_bytes(int n, int gy, int gx) {
    if (n < 1 || n > 65535 || gy < 1 || gx < 1 || (long long)gy * gx > (1LL << 28)) return 0;
    return 2 * align256((size_t)n * fr_w_blocks((long long)gy * gx) * sizeof(float));
}

extern "C" int b4d_fringe_weights(const void* sample, const void* reference, long long reference_stride, int n, int n_carriers, int gy,
                                  int gx, double min_level, double min_visibility, int mode, float* w_out, void* workspace,
                                  void* stream) {
    if (!sample || !w_out || !workspace) return fail(B4D_EINVAL, "null argument");
    if (n < 1 || gy < 1 || gx < 1) return fail(B4D_EINVAL, "fringe: map count and sides must be >= 1");
    if (n > 65535) return fail(B4D_ESIZE, "fringe: at most 65535 maps per call");
    if (n_carriers < 1 || n_carriers > FR_MAX_K) return fail(B4D_EINVAL, "fringe: 1 .. " + std::to_string(FR_MAX_K) + " carriers");
    const long long plane = (long long)gy * gx;
    if (plane > (1LL << 28)) return fail(B4D_ESIZE, "fringe: grids are limited to 2^28 nodes");
    if (!reference) reference_stride = 0;
    if (reference_stride != 0 && reference_stride != (n_carriers + 1) * plane)
        return fail(B4D_EINVAL, "fringe: reference_stride is 0 (shared reference) or (n_carriers + 1) * gy * gx (paired)");
    if (!(min_level >= 0.0 && min_level <= 1.0)) return fail(B4D_EINVAL, "fringe: min_level lies in 0 .. 1");
    if (!(min_visibility >= 0.0 && std::isfinite(min_visibility))) return fail(B4D_EINVAL, "fringe: min_visibility is finite and >= 0");
    if (mode != 0 && mode != 1) return fail(B4D_EINVAL, "fringe: weight mode is 0 (mask) or 1 (inverse phase variance)");
    hipStream_t st = (hipStream_t)stream;
    const int nb = fr_w_blocks(plane);
    float* part_s = (float*)workspace;
    float* part_r = (float*)((char*)workspace + align256((size_t)n * nb * sizeof(float)));
    if (min_level > 0.0)
        hipLaunchKernelGGL(k_fr_level_partials, dim3(nb, n, reference ? 2 : 1), dim3(FR_W_THREADS), 0, st, (const float2*)sample,
                           (const float2*)reference, reference_stride ? n : 1, (n_carriers + 1) * plane, (int)plane, nb, part_s, part_r);
    hipLaunchKernelGGL(k_fr_weights, dim3((unsigned)((plane + FR_W_THREADS - 1) / FR_W_THREADS), n), dim3(FR_W_THREADS), 0, st,
                       (const float2*)sample, (const float2*)reference, reference_stride, n_carriers, (int)plane, nb,
                       (const float*)part_s, (const float*)part_r, min_level, min_visibility, mode, w_out);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_fringe_shift(const float* phase1, const float* phase2, long long stride, int n, int gy, int gx, const double* minv,
                                double* dy, double* dx, void* stream) {
    if (const int rc = fr_check_shift(phase1, phase2, stride, n, gy, gx, minv, dy, dx)) return rc;
    const long long plane = (long long)gy * gx;
    hipLaunchKernelGGL(k_fr_shift, dim3((unsigned)((plane + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, phase1, phase2, stride,
                       (int)plane, minv[0], minv[1], minv[2], minv[3], dy, dx);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_fringe_shift_levels(const float* wrapped1, const float* wrapped2, const float* unwrapped1, const float* unwrapped2,
                                       long long stride, int n, int gy, int gx, const double* minv, double* dy, double* dx, void* stream) {
    if (!unwrapped1 || !unwrapped2) return fail(B4D_EINVAL, "null argument");
    if (const int rc = fr_check_shift(wrapped1, wrapped2, stride, n, gy, gx, minv, dy, dx)) return rc;
    const long long plane = (long long)gy * gx;
    hipLaunchKernelGGL(k_fr_shift_levels, dim3((unsigned)((plane + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, wrapped1, wrapped2,
                       unwrapped1, unwrapped2, stride, (int)plane, minv[0], minv[1], minv[2], minv[3], dy, dx);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
