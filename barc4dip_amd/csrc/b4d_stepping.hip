// b4d_stepping.hip -- phase-stepping analysis of grating scans (barc4dip_amd.signal.stepping): the per-pixel
// least-squares fit of a harmonic model along the T samples of a scan, the elementwise comparison of sample and reference
// coefficients, and one iteration of the step self-calibration (frame sums over the stack plus a one-workgroup update).
// Model: I_t = a0 + sum_k (c_k cos k phi_t + s_k sin k phi_t), K = 1 or 2 harmonics, M = 2K + 1 unknowns, coefficient order
// (a0, c_1, s_1, c_2, s_2).  The host forms the basis table B (T, M), its normal matrix G = B^T B and G^-1 in float64; they
// travel as kernel arguments (constants) and the fit kernel stages them in LDS.  All sums are float64 in an order fixed by the
// shape; there are no atomics and every store is a plain vector store.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "b4d_common.hpp"
#include "b4d_reduce.hpp"

// every fused multiply-add of this unit is written as fma(): a product and a sum that are written apart stay apart, so the 16-byte
// and the dword instantiation of a kernel give the same bits
#pragma clang fp contract(off)

namespace b4d {

constexpr int ST_MAX_T = 64;        // samples per pixel: the dropped-sample mask is one 64-bit word
constexpr int ST_MAX_M = 5;
constexpr int ST_THREADS = 256;
constexpr double ST_PIVOT_RTOL = 1e-10;

struct StTables {                   // 2960 bytes of kernel arguments
    double B[ST_MAX_T * ST_MAX_M];  // (T, M) row-major
    double G[ST_MAX_M * ST_MAX_M];  // (M, M)
    double Ginv[ST_MAX_M * ST_MAX_M];
};

typedef float st_f4 __attribute__((ext_vector_type(4)));

// a sample takes no part if it is not finite or reaches the saturation level (sat = +inf: no level)
__device__ __forceinline__ bool st_dropped(float x, double sat) { return !(fabsf(x) <= FLT_MAX) || (double)x >= sat; }

// the stack is read exactly once: streaming loads, as in the temporal accumulator
template <int PPL>
__device__ __forceinline__ void st_load(const float* p, float (&v)[PPL]) {
    if constexpr (PPL == 4) {
        const st_f4 q = __builtin_nontemporal_load(reinterpret_cast<const st_f4*>(p));
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = __builtin_nontemporal_load(p);
    }
}
template <int PPL>
__device__ __forceinline__ void st_store(float* p, const float (&v)[PPL]) {
    if constexpr (PPL == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        p[0] = v[0];
    }
}

// x of A x = b by Cholesky in place (the lower triangle of A becomes L); false if a pivot is not above ST_PIVOT_RTOL times the
// largest diagonal entry of A, and x is then meaningless
template <int M>
__device__ __forceinline__ bool st_cholesky_solve(double (&A)[M][M], const double (&b)[M], double (&x)[M]) {
    double dmax = A[0][0];
#pragma unroll
    for (int j = 1; j < M; ++j) dmax = fmax(dmax, A[j][j]);
    const double floor = ST_PIVOT_RTOL * dmax;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
        ok = ok && (d > floor);
        const double l = sqrt(d);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
            A[i][j] = s / l;
        }
    }
    double y[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= A[i][k] * y[k];
        y[i] = s / A[i][i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < M; ++k) s -= A[k][i] * x[k];
        x[i] = s / A[i][i];
    }
    return ok;
}

// The rare path of the fit: the normal matrix of the kept samples, G - sum over the dropped t of B_t B_t^T, solved by Cholesky.
// sB, sG: LDS tables.
template <int M>
__device__ __forceinline__ bool st_solve_masked(const double* sB, const double* sG, unsigned long long mask, const double (&b)[M],
                                                double (&x)[M]) {
    double A[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) A[i][k] = sG[i * M + k];
    while (mask) {
        const int t = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        double bt[M];
#pragma unroll
        for (int i = 0; i < M; ++i) bt[i] = sB[t * M + i];
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int k = 0; k <= i; ++k) A[i][k] -= bt[i] * bt[k];
    }
    return st_cholesky_solve<M>(A, b, x);
}

// ------------------------------------------------------------------------------------------------------------ the fit
// grid (ceil(npix / PPL / 256), n scans).  PPL = 4: a lane owns 4 adjacent pixels, one 16-byte load per frame and lane (npix a
// multiple of 4 and every base 16-byte aligned, so every frame of every scan starts on a 16-byte boundary).  PPL = 1: a lane owns
// one pixel, dword accesses, for every other pixel count and alignment (with npix mod 4 != 0 the frames of a scan start at
// different offsets within 16 bytes, so no partition of the pixels gives aligned 16-byte loads in every frame).  Either way the
// 64 lanes of a wave read whole lines of every frame.
template <int K, int PPL>
__global__ void __launch_bounds__(ST_THREADS) k_step_fit(const float* __restrict__ stack, int T, size_t npix, StTables tab, double sat,
                                                         int use_ginv, float* __restrict__ coeff, float* __restrict__ residual,
                                                         unsigned char* __restrict__ nsamp) {
    constexpr int M = 2 * K + 1;
    __shared__ double sB[ST_MAX_T * M], sG[M * M], sGi[M * M];
    for (int i = threadIdx.x; i < T * M; i += ST_THREADS) sB[i] = tab.B[i];
    if (threadIdx.x < M * M) {
        sG[threadIdx.x] = tab.G[threadIdx.x];
        sGi[threadIdx.x] = tab.Ginv[threadIdx.x];
    }
    __syncthreads();
    const size_t i0 = ((size_t)blockIdx.x * ST_THREADS + threadIdx.x) * PPL;
    if (i0 >= npix) return;
    const float* p = stack + (size_t)blockIdx.y * T * npix + i0;

    double b[PPL][M], q[PPL];
    unsigned long long mask[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        q[j] = 0.0, mask[j] = 0;
#pragma unroll
        for (int m = 0; m < M; ++m) b[j][m] = 0.0;
    }
    auto take = [&](const float (&v)[PPL], int t) {
        double bt[M];
#pragma unroll
        for (int m = 0; m < M; ++m) bt[m] = sB[t * M + m];
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const bool drop = st_dropped(v[j], sat);
            const double x = drop ? 0.0 : (double)v[j];
            mask[j] |= (unsigned long long)drop << t;
#pragma unroll
            for (int m = 0; m < M; ++m) b[j][m] = fma(bt[m], x, b[j][m]);
            q[j] = fma(x, x, q[j]);
        }
    };
    int t = 0;
    for (; t + 4 <= T; t += 4) {        // four frames in flight
        float v[4][PPL];
#pragma unroll
        for (int u = 0; u < 4; ++u) st_load<PPL>(p + (size_t)(t + u) * npix, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) take(v[u], t + u);
    }
    for (; t < T; ++t) {
        float v[PPL];
        st_load<PPL>(p + (size_t)t * npix, v);
        take(v, t);
    }

    float oc[M][PPL], ores[PPL];
    unsigned char on[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        double x[M];
        const int nk = T - __popcll(mask[j]);
        bool ok;
        if (mask[j] == 0 && use_ginv) {       // the common case: the shared inverse
            ok = true;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < M; ++m) s = fma(sGi[i * M + m], b[j][m], s);
                x[i] = s;
            }
        } else {
            ok = nk >= M;
            if (ok) ok = st_solve_masked<M>(sB, sG, mask[j], b[j], x);
        }
        double bx = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) bx = fma(b[j][m], x[m], bx);
        const float nanf_ = __builtin_nanf("");
#pragma unroll
        for (int m = 0; m < M; ++m) oc[m][j] = ok ? (float)x[m] : nanf_;
        ores[j] = ok ? (float)sqrt(fmax(q[j] - bx, 0.0) / (double)nk) : nanf_;
        on[j] = (unsigned char)nk;
    }
    const size_t o = (size_t)blockIdx.y * npix + i0;
#pragma unroll
    for (int m = 0; m < M; ++m) st_store<PPL>(coeff + ((size_t)blockIdx.y * M + m) * npix + i0, oc[m]);
    st_store<PPL>(residual + o, ores);
    if constexpr (PPL == 4) {
        *reinterpret_cast<uchar4*>(nsamp + o) = make_uchar4(on[0], on[1], on[2], on[3]);
    } else {
        nsamp[o] = on[0];
    }
}

// ------------------------------------------------------------------------------------------------------------ the comparison
__device__ __forceinline__ double st_wrap(double d) {       // (-2 pi, 2 pi) -> (-pi, pi]
    constexpr double PI = 3.141592653589793238462643383279502884;
    if (d > PI) d -= 2.0 * PI;
    else if (d <= -PI) d += 2.0 * PI;
    return d;
}

// One lane per pixel of one scan; grid (ceil(npix / 256), n).  REF: sample against reference coefficients (r_stride = 0: one
// shared reference scan, M * npix: paired); otherwise the amplitude, phase and visibility of the sample alone.
template <bool REF>
__global__ void __launch_bounds__(ST_THREADS) k_step_compare(const float* __restrict__ cs, const float* __restrict__ cr, size_t r_stride,
                                                             int K, size_t npix, float* __restrict__ phase, float* __restrict__ vis,
                                                             float* __restrict__ amp, float* __restrict__ trans,
                                                             float* __restrict__ vis_ref, float* __restrict__ dark,
                                                             unsigned char* __restrict__ valid) {
    const size_t i = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= npix) return;
    const int M = 2 * K + 1;
    const size_t n = blockIdx.y;
    const float* s = cs + n * M * npix + i;
    const double a0s = s[0];
    const bool oks = !isnan(s[0]);
    double a0r = 0.0;
    const float* r = nullptr;
    bool okr = true;
    if constexpr (REF) {
        r = cr + n * r_stride + i;
        a0r = r[0];
        okr = !isnan(r[0]);
        trans[n * npix + i] = (float)(a0s / a0r);
    }
    for (int k = 0; k < K; ++k) {
        const size_t o = (n * K + k) * npix + i;
        const double c = s[(2 * k + 1) * npix], sn = s[(2 * k + 2) * npix];
        const double a = hypot(c, sn), ph = atan2(-sn, c), v = a / a0s;
        vis[o] = (float)v;
        if (amp) amp[o] = (float)a;
        if constexpr (REF) {
            const double rc = r[(2 * k + 1) * npix], rs = r[(2 * k + 2) * npix];
            const double ar = hypot(rc, rs), vr = ar / a0r;
            phase[o] = (float)st_wrap(ph - atan2(-rs, rc));
            vis_ref[o] = (float)vr;
            dark[o] = (float)(v / vr);
            valid[o] = (unsigned char)(oks && okr && a0s > 0.0 && a0r > 0.0 && ar > 0.0);
        } else {
            phase[o] = (float)ph;
            if (valid) valid[o] = (unsigned char)oks;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ self-calibration
constexpr int ST_CAL_MAX_T = 32;
constexpr int ST_CAL_MAX_BLOCKS = 512;    // partials per column; 8 segments of 64 in the update
constexpr int ST_CAL_SEGMENTS = 8;

struct StCalTables {
    double B[ST_CAL_MAX_T * 3];   // (T, 3)
    double Ginv[9];
    double delta[ST_CAL_MAX_T];   // the step phases that B was formed from
};

// One pass over a scan with the current steps (K = 1): a lane keeps the T samples of its pixels in registers, fits (a0, c, s) with
// the shared inverse as k_step_fit does, and adds, over the pixels without a dropped sample, the products a0 I_t, c I_t, s I_t for
// every t (columns 3 t .. 3 t + 2) and the six entries of the 3 x 3 matrix of (a0, c, s) (columns 3 TMAX ..).  Lanes walk the
// pixels with the stride of the grid; the lane sums go through block_sum_columns, and workgroup g writes column k to
// part[k * gridDim.x + g].  TMAX = 8, 16 or 32 sizes the register arrays; PPL as in k_step_fit.
template <int TMAX, int PPL>
__global__ void __launch_bounds__(ST_THREADS) k_step_frames(const float* __restrict__ stack, int T, size_t npix, StCalTables tab, double sat,
                                                            double* __restrict__ part) {
    constexpr int NV = 3 * TMAX + 6;
    __shared__ double sh[(ST_THREADS / 64) * NV], sB[3 * TMAX], sGi[9];
    if (threadIdx.x < 3 * TMAX) sB[threadIdx.x] = threadIdx.x < 3 * T ? tab.B[threadIdx.x] : 0.0;
    if (threadIdx.x < 9) sGi[threadIdx.x] = tab.Ginv[threadIdx.x];
    __syncthreads();
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    const size_t stride = (size_t)gridDim.x * ST_THREADS * PPL;
    for (size_t i0 = ((size_t)blockIdx.x * ST_THREADS + threadIdx.x) * PPL; i0 < npix; i0 += stride) {
        float v[TMAX][PPL];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {       // frames T .. TMAX - 1 are zeros that meet zero rows of the table
            if (t < T) {
                st_load<PPL>(stack + (size_t)t * npix + i0, v[t]);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; ++j) v[t][j] = 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            double b0 = 0.0, b1 = 0.0, b2 = 0.0;
            bool any = false;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                const bool drop = st_dropped(v[t][j], sat);
                any = any || drop;
                v[t][j] = drop ? 0.0f : v[t][j];
                const double x = (double)v[t][j];
                b0 = fma(sB[3 * t], x, b0);
                b1 = fma(sB[3 * t + 1], x, b1);
                b2 = fma(sB[3 * t + 2], x, b2);
            }
            double a0 = fma(sGi[2], b2, fma(sGi[1], b1, sGi[0] * b0));
            double c = fma(sGi[5], b2, fma(sGi[4], b1, sGi[3] * b0));
            double s = fma(sGi[8], b2, fma(sGi[7], b1, sGi[6] * b0));
            if (any) a0 = c = s = 0.0;       // the pixel takes no part: its (cleaned) samples meet zeros
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                const double x = (double)v[t][j];
                acc[3 * t] = fma(a0, x, acc[3 * t]);
                acc[3 * t + 1] = fma(c, x, acc[3 * t + 1]);
                acc[3 * t + 2] = fma(s, x, acc[3 * t + 2]);
            }
            acc[3 * TMAX] = fma(a0, a0, acc[3 * TMAX]);
            acc[3 * TMAX + 1] = fma(a0, c, acc[3 * TMAX + 1]);
            acc[3 * TMAX + 2] = fma(a0, s, acc[3 * TMAX + 2]);
            acc[3 * TMAX + 3] = fma(c, c, acc[3 * TMAX + 3]);
            acc[3 * TMAX + 4] = fma(c, s, acc[3 * TMAX + 4]);
            acc[3 * TMAX + 5] = fma(s, s, acc[3 * TMAX + 5]);
            __builtin_amdgcn_sched_barrier(0);      // one pixel at a time: interleaving them only lengthens live ranges
        }
    }
    const double col = block_sum_columns<NV>(acc, sh, ST_THREADS / 64);
    if (threadIdx.x < NV) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = col;
}

// One workgroup of 1024: thread (segment s, column k) adds the partials of column k over its segment of ceil(nb / 8) consecutive
// workgroups in index order, thread k then adds the 8 segment sums in order.  Thread t < T solves
// N (g_t, u_t, v_t)^T = r_t by Cholesky (N: the 3 x 3 matrix of (a0, c, s), r_t: the three products of frame t), and
// delta_t <- atan2(v_t, u_t) - atan2(v_0, u_0), unwrapped towards the previous delta_t.
// out: [0] max |change|, [1 ..] delta (T), then g (T), then m = hypot(u, v) (T).  No valid pixel at all gives NaN throughout.
__global__ void __launch_bounds__(1024) k_step_update(const double* __restrict__ part, int nb, int T, int tmax, StCalTables tab,
                                                      double* __restrict__ out) {
    __shared__ double seg[ST_CAL_SEGMENTS][128], tot[128], ang[ST_CAL_MAX_T], dd[ST_CAL_MAX_T];
    const int k = threadIdx.x & 127, s = threadIdx.x >> 7, nv = 3 * tmax + 6;
    const int per = (nb + ST_CAL_SEGMENTS - 1) / ST_CAL_SEGMENTS;
    if (k < nv) {
        double a = 0.0;
        const int hi = min(nb, (s + 1) * per);
        const double* col = part + (size_t)k * nb;
        int g = s * per;
        for (; g + 8 <= hi; g += 8) {       // eight loads in flight, added in index order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = col[g + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += v[u];
        }
        for (; g < hi; ++g) a += col[g];
        seg[s][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < nv) {
        double a = 0.0;
        for (int g = 0; g < ST_CAL_SEGMENTS; ++g) a += seg[g][threadIdx.x];
        tot[threadIdx.x] = a;
    }
    __syncthreads();
    const int t = threadIdx.x;
    double g = 0.0, m = 0.0;
    if (t < T) {
        const double* nn = tot + 3 * tmax;
        double A[3][3] = {{nn[0], 0.0, 0.0}, {nn[1], nn[3], 0.0}, {nn[2], nn[4], nn[5]}};
        const double r[3] = {tot[3 * t], tot[3 * t + 1], tot[3 * t + 2]};
        double x[3];
        const bool ok = st_cholesky_solve<3>(A, r, x);
        const double nan_ = __builtin_nan("");
        g = ok ? x[0] : nan_;
        m = ok ? hypot(x[1], x[2]) : nan_;
        ang[t] = ok ? atan2(x[2], x[1]) : nan_;
    }
    __syncthreads();
    if (t < T) {
        constexpr double TWO_PI = 6.283185307179586476925286766559;
        const double prev = tab.delta[t], d = (ang[t] - ang[0]) - prev;
        const double nw = prev + (d - TWO_PI * ceil((d - 0.5 * TWO_PI) / TWO_PI));
        dd[t] = fabs(nw - prev);
        out[1 + t] = nw;
        out[1 + T + t] = g;
        out[1 + 2 * T + t] = m;
    }
    __syncthreads();
    if (t == 0) {
        double mx = 0.0;
        for (int u = 0; u < T; ++u) mx = (dd[u] > mx || isnan(dd[u])) ? dd[u] : mx;
        out[0] = mx;
    }
}


template <int TMAX>
static int st_launch_frames(bool vec, int nb, hipStream_t st, const float* stack, int T, size_t npix, const StCalTables& tab, double sat,
                            double* part) {
    if (vec) return launch(k_step_frames<TMAX, 4>, dim3(nb), dim3(ST_THREADS), 0, st, stack, T, npix, tab, sat, part);
    return launch(k_step_frames<TMAX, 1>, dim3(nb), dim3(ST_THREADS), 0, st, stack, T, npix, tab, sat, part);
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_stepping_fit(const float* stack, int n, int T, long long npix, int harmonics, const double* basis, const double* gram,
                                const double* gram_inv, double saturation, float* coeff, float* residual, unsigned char* n_samples,
                                void* stream) {
    if (!stack || !basis || !gram || !coeff || !residual || !n_samples) return fail(B4D_EINVAL, "stepping: null argument");
    if (harmonics != 1 && harmonics != 2) return fail(B4D_EINVAL, "stepping: harmonics must be 1 or 2");
    const int M = 2 * harmonics + 1;
    if (T < 3 || T > ST_MAX_T) return fail(B4D_ESIZE, "stepping: 3 .. 64 samples per pixel, got " + std::to_string(T));
    if (T < M) return fail(B4D_EINVAL, "stepping: fewer samples than unknowns");
    if (n < 1 || n > 65535 || npix < 1) return fail(B4D_EINVAL, "stepping: 1 .. 65535 scans of at least one pixel");
    if (std::isnan(saturation)) return fail(B4D_EINVAL, "stepping: saturation is NaN (+inf switches it off)");
    StTables tab{};
    for (int i = 0; i < T * M; ++i) {
        if (!std::isfinite(basis[i])) return fail(B4D_EINVAL, "stepping: the basis table must be finite");
        tab.B[i] = basis[i];
    }
    for (int i = 0; i < M * M; ++i) {
        tab.G[i] = gram[i];
        tab.Ginv[i] = gram_inv ? gram_inv[i] : 0.0;
    }
    const size_t np = (size_t)npix;
    const bool vec = (np & 3) == 0 && ptr_aligned(stack, 16) && ptr_aligned(coeff, 16) && ptr_aligned(residual, 16) && ptr_aligned(n_samples, 4);
    const size_t blocks = (np / (vec ? 4 : 1) + ST_THREADS - 1) / ST_THREADS;
    if (blocks > 0x7fffffffull) return fail(B4D_ESIZE, "stepping: scan too large");
    const dim3 grid((unsigned)blocks, (unsigned)n), block(ST_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const int ug = gram_inv != nullptr;
    if (harmonics == 1)
        return vec ? launch(k_step_fit<1, 4>, grid, block, 0, st, stack, T, np, tab, saturation, ug, coeff, residual, n_samples)
                   : launch(k_step_fit<1, 1>, grid, block, 0, st, stack, T, np, tab, saturation, ug, coeff, residual, n_samples);
    return vec ? launch(k_step_fit<2, 4>, grid, block, 0, st, stack, T, np, tab, saturation, ug, coeff, residual, n_samples)
               : launch(k_step_fit<2, 1>, grid, block, 0, st, stack, T, np, tab, saturation, ug, coeff, residual, n_samples);
}

extern "C" int b4d_stepping_compare(const float* sample, const float* reference, long long reference_stride, int n, int harmonics,
                                    long long npix, float* phase, float* visibility, float* amplitude, float* transmission,
                                    float* visibility_ref, float* dark_field, unsigned char* valid, void* stream) {
    if (!sample || !phase || !visibility) return fail(B4D_EINVAL, "stepping: null argument");
    if (harmonics != 1 && harmonics != 2) return fail(B4D_EINVAL, "stepping: harmonics must be 1 or 2");
    if (n < 1 || n > 65535 || npix < 1) return fail(B4D_EINVAL, "stepping: 1 .. 65535 scans of at least one pixel");
    const size_t np = (size_t)npix, blocks = (np + ST_THREADS - 1) / ST_THREADS;
    if (blocks > 0x7fffffffull) return fail(B4D_ESIZE, "stepping: scan too large");
    const dim3 grid((unsigned)blocks, (unsigned)n), block(ST_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (!reference) {
        if (!amplitude) return fail(B4D_EINVAL, "stepping: amplitude is required without a reference");
        if (transmission || visibility_ref || dark_field) return fail(B4D_EINVAL, "stepping: transmission, visibility_ref and dark_field need a reference");
        return launch(k_step_compare<false>, grid, block, 0, st, sample, reference, 0, harmonics, np, phase, visibility, amplitude, transmission,
                      visibility_ref, dark_field, valid);
    }
    if (!transmission || !visibility_ref || !dark_field || !valid) return fail(B4D_EINVAL, "stepping: null output");
    const long long full = (long long)(2 * harmonics + 1) * npix;
    if (reference_stride != 0 && reference_stride != full)
        return fail(B4D_EINVAL, "stepping: reference_stride is 0 (shared reference) or (2 harmonics + 1) * npix (paired)");
    return launch(k_step_compare<true>, grid, block, 0, st, sample, reference, (size_t)reference_stride, harmonics, np, phase, visibility,
                  amplitude, transmission, visibility_ref, dark_field, valid);
}

extern "C" int b4d_stepping_calibrate_step(const float* stack, int T, long long npix, const double* basis, const double* gram_inv,
                                           const double* delta, double saturation, double* out, void* stream) {
    B4D_SCRATCH_LOCK();
    if (!stack || !basis || !gram_inv || !delta || !out) return fail(B4D_EINVAL, "stepping: null argument");
    if (T < 5 || T > ST_CAL_MAX_T) return fail(T < 5 ? B4D_EINVAL : B4D_ESIZE, "stepping: calibration takes 5 .. 32 samples per pixel, got " + std::to_string(T));
    if (npix < 1) return fail(B4D_EINVAL, "stepping: empty scan");
    if (std::isnan(saturation)) return fail(B4D_EINVAL, "stepping: saturation is NaN (+inf switches it off)");
    StCalTables tab{};
    for (int i = 0; i < 3 * T; ++i) tab.B[i] = basis[i];
    for (int i = 0; i < 9; ++i) tab.Ginv[i] = gram_inv[i];
    for (int i = 0; i < T; ++i) tab.delta[i] = delta[i];
    for (int i = 0; i < 3 * T + 9 + T; ++i)
        if (!std::isfinite(i < 3 * T ? basis[i] : i < 3 * T + 9 ? gram_inv[i - 3 * T] : delta[i - 3 * T - 9]))
            return fail(B4D_EINVAL, "stepping: the tables must be finite");
    const size_t np = (size_t)npix;
    const bool vec = (np & 3) == 0 && ptr_aligned(stack, 16);
    const size_t want = (np / (vec ? 4 : 1) + ST_THREADS - 1) / ST_THREADS;
    const int nb = (int)std::min<size_t>(want, ST_CAL_MAX_BLOCKS);
    const int tmax = T <= 8 ? 8 : T <= 16 ? 16 : 32;
    void* ws = nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = get_scratch(sizeof(double) * (3 * ST_CAL_MAX_T + 6) * ST_CAL_MAX_BLOCKS, &ws, st)) return rc;
    double* part = static_cast<double*>(ws);
    int rc;
    if (tmax == 8) rc = st_launch_frames<8>(vec, nb, st, stack, T, np, tab, saturation, part);
    else if (tmax == 16) rc = st_launch_frames<16>(vec, nb, st, stack, T, np, tab, saturation, part);
    else rc = st_launch_frames<32>(vec, nb, st, stack, T, np, tab, saturation, part);
    if (rc) return rc;
    return launch(k_step_update, dim3(1), dim3(1024), 0, st, part, nb, T, tmax, tab, out);
}
