// b4d_poly2.hip -- the low-order (6-term quadratic) fit of a wavefront map and its residual and the
// weighted variant (section 14): float64 moments per map, the 6 x 6 Gram matrix by a Cholesky factorisation with a drop rule.
#include <cmath>
#include <string>

#include "b4d_common.hpp"
#include "b4d_reduce.hpp"
#include "b4d_wf.hpp"

namespace b4d {

// ---- low-order fit: moments sum m_k w of the six monomials m = (1, u, v, u^2, u v, v^2) in float64, u = (j - cx) / xh along x,
// v = (i - cy) / yh along y; lane 0 multiplies by the inverse Gram matrix of the grid (host, float64).  One workgroup per map.
struct WfFit {
    double ginv[36];
    double cx, cy, ixh, iyh;
};
constexpr int WF_FIT_THREADS = 1024;

__global__ void __launch_bounds__(WF_FIT_THREADS) k_wf_poly2_moments(const float* __restrict__ w, int ny, int nx, WfFit f,
                                                                     double* __restrict__ coeff) {
    __shared__ double sh[WF_FIT_THREADS / 64][6];
    const int npix = ny * nx;
    const float* __restrict__ p = w + (size_t)blockIdx.x * npix;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < npix; e += WF_FIT_THREADS) {
        const int i = e / nx, j = e % nx;
        const double u = ((double)j - f.cx) * f.ixh, v = ((double)i - f.cy) * f.iyh, x = (double)p[e];
        s[0] += x;
        s[1] += u * x;
        s[2] += v * x;
        s[3] += u * u * x;
        s[4] += u * v * x;
        s[5] += v * v * x;
    }
    block_sum(s, &sh[0][0], WF_FIT_THREADS / 64);
    if (threadIdx.x == 0)
        for (int a = 0; a < 6; ++a) {
            double c = 0.0;
            for (int b = 0; b < 6; ++b) c += f.ginv[6 * a + b] * s[b];
            coeff[6 * (size_t)blockIdx.x + a] = c;
        }
}

// residual = scale (w - sum of the terms selected by mask) in float32 (may alias w), rms = population standard deviation of
// the residual in float64
__global__ void __launch_bounds__(WF_FIT_THREADS) k_wf_poly2_residual(const float* w, int ny, int nx, WfFit f,
                                                                      const double* __restrict__ coeff, unsigned mask, double scale,
                                                                      float* residual, double* __restrict__ rms) {
    __shared__ double sh[WF_FIT_THREADS / 64][2];
    const int npix = ny * nx;
    const float* p = w + (size_t)blockIdx.x * npix;
    float* q = residual + (size_t)blockIdx.x * npix;
    double c[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = ((mask >> k) & 1u) ? coeff[6 * (size_t)blockIdx.x + k] : 0.0;
    double s[2] = {0.0, 0.0};
    for (int e = threadIdx.x; e < npix; e += WF_FIT_THREADS) {
        const int i = e / nx, j = e % nx;
        const double u = ((double)j - f.cx) * f.ixh, v = ((double)i - f.cy) * f.iyh;
        const double fit = c[0] + u * (c[1] + c[3] * u + c[4] * v) + v * (c[2] + c[5] * v);
        const float out = (float)(scale * ((double)p[e] - fit));
        q[e] = out;
        s[0] += (double)out;
        s[1] += (double)out * (double)out;
    }
    block_sum(s, &sh[0][0], WF_FIT_THREADS / 64);
    if (threadIdx.x == 0) {
        const double mean = s[0] / npix;
        rms[blockIdx.x] = sqrt(fmax(0.0, s[1] / npix - mean * mean));
    }
}

// Cholesky factor of the Gram matrix G of the six monomials and the solve with it, float64, for the host (unweighted fit: G
// depends on the grid alone, the host keeps its inverse) and for one lane of the device (weighted fit: G from the weighted
// moments of the map).  Monomials are taken in order; one whose remainder after the kept ones is below 1e-12 of itself is
// dropped, and its coefficient is 0.
struct WfChol {       // the device keeps it in LDS: the loops index it with run-time subscripts
    double L[6][6];
    double y[6];
    bool kept[6];
};

__host__ __device__ inline void wf_gram_factor(const double (&G)[6][6], WfChol& f) {
    for (int a = 0; a < 6; ++a) {
        double d = G[a][a];
        for (int b = 0; b < a; ++b) {
            f.L[a][b] = 0.0;
            if (!f.kept[b]) continue;
            double s = G[a][b];
            for (int c = 0; c < b; ++c)
                if (f.kept[c]) s -= f.L[a][c] * f.L[b][c];
            f.L[a][b] = s / f.L[b][b];
            d -= f.L[a][b] * f.L[a][b];
        }
        f.kept[a] = d > 1e-12 * G[a][a] && G[a][a] > 0.0;
        f.L[a][a] = f.kept[a] ? sqrt(d) : 0.0;
    }
}

// x = G^-1 rhs on the kept set (G^-1 = L^-T L^-1: L y = rhs, L^T x = y), 0 for a dropped monomial
__host__ __device__ inline void wf_gram_solve(WfChol& f, const double (&rhs)[6], double (&x)[6]) {
    double* y = f.y;
    for (int a = 0; a < 6; ++a) {
        x[a] = 0.0;
        if (!f.kept[a]) continue;
        double s = rhs[a];
        for (int c = 0; c < a; ++c)
            if (f.kept[c]) s -= f.L[a][c] * y[c];
        y[a] = s / f.L[a][a];
    }
    for (int a = 5; a >= 0; --a) {
        if (!f.kept[a]) continue;
        double s = y[a];
        for (int c = a + 1; c < 6; ++c)
            if (f.kept[c]) s -= f.L[c][a] * x[c];
        x[a] = s / f.L[a][a];
    }
}

// normalised coordinates of the fit: u = (j - cx) / max(cx, 1), v likewise
static void wf_fit_coords(int ny, int nx, WfFit& f) {
    f.cx = 0.5 * (nx - 1);
    f.cy = 0.5 * (ny - 1);
    f.ixh = 1.0 / (nx > 1 ? f.cx : 1.0);
    f.iyh = 1.0 / (ny > 1 ? f.cy : 1.0);
}

// Inverse Gram matrix of the six monomials on the (ny, nx) grid, float64.  The sums separate: sum u^a v^b = (sum_j u^a)(sum_i v^b).
// A monomial that the grid cannot tell from the ones before it (a side of 1 or 2 nodes) is left out: its coefficient is 0.
static void wf_gram_inverse(int ny, int nx, WfFit& f) {
    wf_fit_coords(ny, nx, f);
    double su[5] = {0, 0, 0, 0, 0}, sv[5] = {0, 0, 0, 0, 0};
    for (int j = 0; j < nx; ++j) {
        const double u = (j - f.cx) * f.ixh;
        double p = 1.0;
        for (int a = 0; a < 5; ++a, p *= u) su[a] += p;
    }
    for (int i = 0; i < ny; ++i) {
        const double v = (i - f.cy) * f.iyh;
        double p = 1.0;
        for (int a = 0; a < 5; ++a, p *= v) sv[a] += p;
    }
    static const int pu[6] = {0, 1, 0, 2, 1, 0}, pv[6] = {0, 0, 1, 0, 1, 2};
    double G[6][6];
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) G[a][b] = su[pu[a] + pu[b]] * sv[pv[a] + pv[b]];
    WfChol ch;
    wf_gram_factor(G, ch);
    for (int k = 0; k < 36; ++k) f.ginv[k] = 0.0;
    for (int b = 0; b < 6; ++b) {     // column b of the inverse: the solve of the unit vector e_b
        if (!ch.kept[b]) continue;
        double rhs[6] = {}, x[6];
        rhs[b] = 1.0;
        wf_gram_solve(ch, rhs, x);
        for (int a = 0; a < 6; ++a) f.ginv[6 * a + b] = x[a];
    }
}

// ---- weighted fit: the 15 weighted monomial moments sum w u^a v^b (a + b <= 4) and the six weighted right-hand moments of a map
// in float64, one workgroup per map; lane 0 forms the Gram matrix and solves it with the factorisation and drop rule of the unweighted fit.
// A node counts only if its weight is finite and positive, so a NaN in the map at a weight-0 node is never read into a sum.
constexpr int WF_WFIT_THREADS = 1024;
__host__ __device__ constexpr int wf_midx(int a, int b) { return 5 * a - a * (a - 1) / 2 + b; }   // (a, b), a + b <= 4 -> 0 .. 14

__device__ __forceinline__ float wf_fit_weight(const float* __restrict__ w, int e) {
    const float a = w[e];
    return (a > 0.f && isfinite(a)) ? a : 0.f;
}

__global__ void __launch_bounds__(WF_WFIT_THREADS) k_wf_poly2_wmoments(const float* __restrict__ phi, const float* __restrict__ w,
                                                                      long long w_stride, int ny, int nx, WfFit f,
                                                                      double* __restrict__ coeff) {
    __shared__ double sh[WF_WFIT_THREADS / 64][21];
    __shared__ struct {
        double G[6][6], rhs[6], c[6];
        WfChol ch;
    } fit;
    const int npix = ny * nx;
    const float* __restrict__ p = phi + (size_t)blockIdx.x * npix;
    const float* __restrict__ mw = w + (long long)blockIdx.x * w_stride;
    double s[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) s[k] = 0.0;
    for (int e = threadIdx.x; e < npix; e += WF_WFIT_THREADS) {
        const float wf = wf_fit_weight(mw, e);
        if (!(wf > 0.f)) continue;
        const int i = e / nx, j = e % nx;
        const double u = ((double)j - f.cx) * f.ixh, v = ((double)i - f.cy) * f.iyh, wd = (double)wf, x = wd * (double)p[e];
        double up[5], vp[5];
        up[0] = vp[0] = 1.0;
#pragma unroll
        for (int a = 1; a < 5; ++a) up[a] = up[a - 1] * u, vp[a] = vp[a - 1] * v;
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; a + b < 5; ++b) s[wf_midx(a, b)] += wd * up[a] * vp[b];
        s[15] += x;
        s[16] += u * x;
        s[17] += v * x;
        s[18] += u * u * x;
        s[19] += u * v * x;
        s[20] += v * v * x;
    }
    {   // lane k adds column k of the wave sums (thread 0 would hold 21 x 16 loads at once), thread 0 collects them
        const double t = block_sum_columns(s, &sh[0][0], WF_WFIT_THREADS / 64);
        if (threadIdx.x < 21) sh[0][threadIdx.x] = t;
        __syncthreads();
        if (threadIdx.x == 0)
#pragma unroll
            for (int k = 0; k < 21; ++k) s[k] = sh[0][k];
    }
    if (threadIdx.x == 0) {
        constexpr int pu[6] = {0, 1, 0, 2, 1, 0}, pv[6] = {0, 0, 1, 0, 1, 2};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            fit.rhs[a] = s[15 + a];
#pragma unroll
            for (int b = 0; b < 6; ++b) fit.G[a][b] = s[wf_midx(pu[a] + pu[b], pv[a] + pv[b])];
        }
        wf_gram_factor(fit.G, fit.ch);
        wf_gram_solve(fit.ch, fit.rhs, fit.c);
        for (int a = 0; a < 6; ++a) coeff[6 * (size_t)blockIdx.x + a] = fit.c[a];
    }
}

// residual as k_wf_poly2_residual; rms = weighted population standard deviation sqrt(sum w r^2 / sum w - (sum w r / sum w)^2) over
// the nodes of positive weight (NaN if there is none); weight-0 nodes get NaN when nan_invalid, else the same subtraction
__global__ void __launch_bounds__(WF_FIT_THREADS) k_wf_poly2_wresidual(const float* phi, const float* __restrict__ w, long long w_stride,
                                                                       int ny, int nx, WfFit f, const double* __restrict__ coeff,
                                                                       unsigned mask, double scale, int nan_invalid, float* residual,
                                                                       double* __restrict__ rms) {
    __shared__ double sh[WF_FIT_THREADS / 64][3];
    const int npix = ny * nx;
    const float* p = phi + (size_t)blockIdx.x * npix;
    const float* __restrict__ mw = w + (long long)blockIdx.x * w_stride;
    float* q = residual + (size_t)blockIdx.x * npix;
    double c[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = ((mask >> k) & 1u) ? coeff[6 * (size_t)blockIdx.x + k] : 0.0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < npix; e += WF_FIT_THREADS) {
        const float wf = wf_fit_weight(mw, e);
        if (!(wf > 0.f) && nan_invalid) {
            q[e] = __builtin_nanf("");
            continue;
        }
        const int i = e / nx, j = e % nx;
        const double u = ((double)j - f.cx) * f.ixh, v = ((double)i - f.cy) * f.iyh;
        const double fit = c[0] + u * (c[1] + c[3] * u + c[4] * v) + v * (c[2] + c[5] * v);
        const float out = (float)(scale * ((double)p[e] - fit));
        q[e] = out;
        if (wf > 0.f) {
            s[0] += (double)wf;
            s[1] += (double)wf * (double)out;
            s[2] += (double)wf * (double)out * (double)out;
        }
    }
    block_sum(s, &sh[0][0], WF_FIT_THREADS / 64);
    if (threadIdx.x == 0) {
        const double mean = s[0] > 0.0 ? s[1] / s[0] : 0.0;
        rms[blockIdx.x] = s[0] > 0.0 ? sqrt(fmax(0.0, s[2] / s[0] - mean * mean)) : __builtin_nan("");
    }
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_poly2_fit(const float* w, int n, int ny, int nx, unsigned remove_mask, double scale, double* coeff, float* residual,
                             double* rms, void* stream) {
    if (!w || !coeff) return fail(B4D_EINVAL, "null argument");
    if ((residual == nullptr) != (rms == nullptr)) return fail(B4D_EINVAL, "residual and rms go together (both or neither)");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    if (remove_mask > 63u) return fail(B4D_EINVAL, "remove_mask has six bits");
    if (!std::isfinite(scale)) return fail(B4D_EINVAL, "scale must be finite");
    hipStream_t st = (hipStream_t)stream;
    WfFit f;
    wf_gram_inverse(ny, nx, f);
    hipLaunchKernelGGL(k_wf_poly2_moments, dim3(n), dim3(WF_FIT_THREADS), 0, st, w, ny, nx, f, coeff);
    if (residual)
        hipLaunchKernelGGL(k_wf_poly2_residual, dim3(n), dim3(WF_FIT_THREADS), 0, st, w, ny, nx, f, (const double*)coeff, remove_mask,
                           scale, residual, rms);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_poly2_fit_weighted(const float* w_map, const float* weights, long long weight_stride, int n, int ny, int nx,
                                      unsigned remove_mask, double scale, int nan_invalid, double* coeff, float* residual, double* rms,
                                      void* stream) {
    if (!w_map || !weights || !coeff) return fail(B4D_EINVAL, "null argument");
    if ((residual == nullptr) != (rms == nullptr)) return fail(B4D_EINVAL, "residual and rms go together (both or neither)");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    if (weight_stride != 0 && weight_stride != (long long)ny * nx)
        return fail(B4D_EINVAL, "weight_stride is 0 (shared weights) or ny * nx (per map)");
    if (remove_mask > 63u) return fail(B4D_EINVAL, "remove_mask has six bits");
    if (!std::isfinite(scale)) return fail(B4D_EINVAL, "scale must be finite");
    hipStream_t st = (hipStream_t)stream;
    WfFit f;
    wf_fit_coords(ny, nx, f);
    for (double& v : f.ginv) v = 0.0;
    hipLaunchKernelGGL(k_wf_poly2_wmoments, dim3(n), dim3(WF_WFIT_THREADS), 0, st, w_map, weights, weight_stride, ny, nx, f, coeff);
    if (residual)
        hipLaunchKernelGGL(k_wf_poly2_wresidual, dim3(n), dim3(WF_FIT_THREADS), 0, st, w_map, weights, weight_stride, ny, nx, f,
                           (const double*)coeff, remove_mask, scale, nan_invalid, residual, rms);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
