// b4d_integrate.hip -- wavefront reconstruction: least-squares integration of a slope field on a regular grid and the
// low-order (6-term quadratic) fit of the result.
//
// Southwell geometry: the slope on the edge between two neighbouring nodes is the mean of the two node slopes; phi is the
// zero-mean minimiser of the squared edge residuals.  The normal equations are a 5-point Neumann Laplacian, which the
// orthonormal DCT-II diagonalises exactly:
//   r      = divergence of the edge slopes (k_wf_rhs, one elementwise launch)
//   A1     = r   . Cx^T
//   P      = (Cy . A1) / Lambda, P[0][0] = 0          Lambda[k][l] = 4 sin^2(pi k / 2 ny) / hy^2 + 4 sin^2(pi l / 2 nx) / hx^2
//   A2     = P   . Cx
//   phi    = Cy^T . A2
// Four launches of one real matrix-product kernel on v_mfma_f32_32x32x2_f32 for the whole batch, the basis as the shared
// operand.  Basis, its transpose and the eigenvalue terms are computed in float64 on the host, rounded once and cached per
// side and device.
#include <cmath>
#include <list>
#include <mutex>
#include <string>
#include <vector>

#include "b4d_common.hpp"

namespace b4d {

constexpr int WF_MAX_SIDE = 2048;
constexpr int WF_TILE = 128;   // output tile of a workgroup (4 waves in 2 x 2, each 2 x 2 MFMA tiles of 32 x 32)
constexpr int WF_BK = 16;
constexpr int WF_LD = 130;     // LDS row stride: 130 % 32 == 2 keeps the staging writes (k fastest) off each other's banks

typedef float wf_f32x16 __attribute__((ext_vector_type(16)));

// ---- right-hand side.  With gbar the edge means, r[i][j] = (gbar_y[i-1][j] - gbar_y[i][j]) / hy + (gbar_x[i][j-1] - gbar_x[i][j]) / hx,
// terms with an index outside the grid absent: interior (g[i-1] - g[i+1]) / 2, first node -(g[0] + g[1]) / 2, last node
// (g[n-2] + g[n-1]) / 2, a single node 0.  grid (ceil(ny nx / 256), batch)
__device__ __forceinline__ float wf_div1(const float* __restrict__ g, int i, int n, long long stride) {
    if (n == 1) return 0.f;
    if (i == 0) return -0.5f * (g[0] + g[stride]);
    if (i == n - 1) return 0.5f * (g[-stride] + g[0]);
    return 0.5f * (g[-stride] - g[stride]);
}

__global__ void __launch_bounds__(256) k_wf_rhs(const float* __restrict__ gy, const float* __restrict__ gx, int ny, int nx,
                                                float ihy, float ihx, float* __restrict__ r) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ny * nx) return;
    const size_t fo = (size_t)blockIdx.y * ny * nx;
    const int i = e / nx, j = e % nx;
    r[fo + e] = wf_div1(gy + fo + e, i, ny, nx) * ihy + wf_div1(gx + fo + e, j, nx, 1) * ihx;
}

// ---- real matrix product C[z] = A[z] . B[z] on the matrix cores, row-major operands, batch on blockIdx.z (a stride of 0
// shares an operand).  K and the M / N edges are padded with zeros in LDS.  Fragment maps of v_mfma_f32_32x32x2_f32:
// A: lane l holds A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; C/D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// DIV: the store divides by the float32 rounding of the float64 eigenvalue Lambda[m][n] = ly[m] ihy2 + lx[n] ihx2 and zeroes (0, 0).
struct WfGemm {
    const float* A;
    const float* B;
    float* C;
    int M, N, K;
    long long sA, sB, sC;
    const double* ly;
    const double* lx;
    double ihy2, ihx2;
};

template <bool DIV>
__global__ void __launch_bounds__(256) k_wf_gemm(WfGemm g) {
    __shared__ float As[WF_BK][WF_LD];  // [k][m]
    __shared__ float Bs[WF_BK][WF_LD];  // [k][n]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int m0 = blockIdx.y * WF_TILE, n0 = blockIdx.x * WF_TILE;
    const float* __restrict__ A = g.A + (long long)blockIdx.z * g.sA;
    const float* __restrict__ B = g.B + (long long)blockIdx.z * g.sB;
    float* __restrict__ Cm = g.C + (long long)blockIdx.z * g.sC;
    wf_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int k0 = 0; k0 < g.K; k0 += WF_BK) {
#pragma unroll
        for (int r = 0; r < WF_TILE * WF_BK / 256; ++r) {
            const int e = threadIdx.x + 256 * r;
            {
                const int kk = e & (WF_BK - 1), mm = e / WF_BK;
                const int m = m0 + mm, k = k0 + kk;
                As[kk][mm] = (m < g.M && k < g.K) ? A[(long long)m * g.K + k] : 0.f;
            }
            {
                const int nn = e & (WF_TILE - 1), kk = e / WF_TILE;
                const int n = n0 + nn, k = k0 + kk;
                Bs[kk][nn] = (n < g.N && k < g.K) ? B[(long long)k * g.N + n] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < WF_BK; kk += 2) {
            const float a0 = As[kk + lk][64 * wr + li], a1 = As[kk + lk][64 * wr + 32 + li];
            const float b0 = Bs[kk + lk][64 * wc + li], b1 = Bs[kk + lk][64 * wc + 32 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 64 * wc + 32 * j + li;
        if (n >= g.N) continue;
        double lxn = 0.0;
        if (DIV) lxn = g.lx[n] * g.ihx2;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + 64 * wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m >= g.M) continue;
                float v = acc[i][j][r];
                if (DIV) v = (m == 0 && n == 0) ? 0.f : v / (float)(g.ly[m] * g.ihy2 + lxn);
                Cm[(long long)m * g.N + n] = v;
            }
    }
}

// ---- low-order fit: moments sum m_k w of the six monomials m = (1, u, v, u^2, u v, v^2) in float64, u = (j - cx) / xh along x,
// v = (i - cy) / yh along y; lane 0 multiplies by the inverse Gram matrix of the grid (host, float64).  One workgroup per map.
struct WfFit {
    double ginv[36];
    double cx, cy, ixh, iyh;
};
constexpr int WF_FIT_THREADS = 1024;

template <int NV>
__device__ __forceinline__ void wf_block_sum(double (&v)[NV], double (*sh)[NV]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
        if (lane == 0) sh[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = 0.0;
            for (int w = 0; w < WF_FIT_THREADS / 64; ++w) s += sh[w][k];
            v[k] = s;
        }
}

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
    wf_block_sum<6>(s, sh);
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
    wf_block_sum<2>(s, sh);
    if (threadIdx.x == 0) {
        const double mean = s[0] / npix;
        rms[blockIdx.x] = sqrt(fmax(0.0, s[1] / npix - mean * mean));
    }
}

// ---- DCT-II basis C[k][j] = s_k sqrt(2/n) cos(pi (2j+1) k / 2n) (s_0 = 1/sqrt 2), its transpose and the eigenvalue terms
// 4 sin^2(pi k / 2n) of one side, float64 on the host, cached per (device, side).  The cache is bounded by bytes: the oldest
// sides are released first (hipFree waits for the device, so no launch still reads them).
struct WfBasis {
    int device, n;
    float *C, *CT;
    double* lam;
    size_t bytes;
};
constexpr size_t WF_CACHE_BYTES = (size_t)192 << 20;

static std::mutex& wf_mutex() {
    static std::mutex m;
    return m;
}
static std::list<WfBasis>& wf_cache() {
    static std::list<WfBasis> c;
    return c;
}

// caller holds wf_mutex(); `keep` sides are not evicted
static int wf_basis(int n, int keep, const WfBasis** out) {
    int dev = 0;
    B4D_HIP(hipGetDevice(&dev));
    auto& cache = wf_cache();
    for (auto it = cache.begin(); it != cache.end(); ++it)
        if (it->device == dev && it->n == n) {
            cache.splice(cache.end(), cache, it);   // most recently used last
            *out = &cache.back();
            return B4D_OK;
        }
    const size_t nn = (size_t)n * n;
    std::vector<float> hc(nn), ht(nn);
    std::vector<double> hl(n);
    const double norm = std::sqrt(2.0 / n);
    for (int k = 0; k < n; ++k) {
        const double sk = k == 0 ? norm * M_SQRT1_2 : norm;
        for (int j = 0; j < n; ++j) {
            const long long q = ((long long)(2 * j + 1) * k) % (4LL * n);   // the angle pi q / 2n, reduced in integers
            const float c = (float)(sk * std::cos(M_PI * (double)q / (2.0 * n)));
            hc[(size_t)k * n + j] = c;
            ht[(size_t)j * n + k] = c;
        }
        const double s = std::sin(M_PI * (double)k / (2.0 * n));
        hl[k] = 4.0 * s * s;
    }
    WfBasis b{dev, n, nullptr, nullptr, nullptr, 2 * nn * sizeof(float) + n * sizeof(double)};
    size_t total = b.bytes;
    for (const auto& e : cache) total += e.bytes;
    for (auto it = cache.begin(); it != cache.end() && total > WF_CACHE_BYTES;) {
        if (it->device == dev && it->n == keep) {
            ++it;
            continue;
        }
        int cur = dev;
        if (it->device != cur) (void)hipSetDevice(it->device);
        (void)hipFree(it->C);
        (void)hipFree(it->CT);
        (void)hipFree(it->lam);
        if (it->device != cur) (void)hipSetDevice(cur);
        total -= it->bytes;
        it = cache.erase(it);
    }
    B4D_HIP(hipMalloc((void**)&b.C, nn * sizeof(float)));
    if (hipMalloc((void**)&b.CT, nn * sizeof(float)) != hipSuccess || hipMalloc((void**)&b.lam, n * sizeof(double)) != hipSuccess) {
        (void)hipFree(b.C);
        (void)hipFree(b.CT);
        return fail(B4D_ENOMEM, "integrate: no device memory for the DCT basis of side " + std::to_string(n));
    }
    hipError_t e = hipMemcpy(b.C, hc.data(), nn * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b.CT, ht.data(), nn * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b.lam, hl.data(), n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(b.C);
        (void)hipFree(b.CT);
        (void)hipFree(b.lam);
        return fail(B4D_EHIP, std::string("integrate: basis upload: ") + hipGetErrorString(e));
    }
    cache.push_back(b);
    *out = &cache.back();
    return B4D_OK;
}

static int wf_check_grid(int n, int ny, int nx) {
    if (n < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "map count and sides must be >= 1");
    if (ny > WF_MAX_SIDE || nx > WF_MAX_SIDE)
        return fail(B4D_ESIZE, "wavefront grids are limited to " + std::to_string(WF_MAX_SIDE) + " nodes per side, got (" +
                                   std::to_string(ny) + ", " + std::to_string(nx) + ")");
    if (n > 65535) return fail(B4D_ESIZE, "at most 65535 maps per call");
    return B4D_OK;
}

// Inverse Gram matrix of the six monomials on the (ny, nx) grid, float64.  The sums separate: sum u^a v^b = (sum_j u^a)(sum_i v^b).
// A monomial that the grid cannot tell from the ones before it (a side of 1 or 2 nodes) is left out: its coefficient is 0.
static void wf_gram_inverse(int ny, int nx, WfFit& f) {
    f.cx = 0.5 * (nx - 1);
    f.cy = 0.5 * (ny - 1);
    f.ixh = 1.0 / (nx > 1 ? f.cx : 1.0);
    f.iyh = 1.0 / (ny > 1 ? f.cy : 1.0);
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
    // Cholesky of the kept monomials, in order; a monomial whose remainder after the kept ones is below 1e-12 of itself is dropped
    bool kept[6];
    double L[6][6] = {};
    for (int a = 0; a < 6; ++a) {
        double d = G[a][a];
        for (int b = 0; b < a; ++b) {
            if (!kept[b]) continue;
            double s = G[a][b];
            for (int c = 0; c < b; ++c)
                if (kept[c]) s -= L[a][c] * L[b][c];
            L[a][b] = s / L[b][b];
            d -= L[a][b] * L[a][b];
        }
        kept[a] = d > 1e-12 * G[a][a] && G[a][a] > 0.0;
        L[a][a] = kept[a] ? std::sqrt(d) : 0.0;
    }
    // G^-1 = L^-T L^-1 on the kept set: solve L y = e_b, L^T x = y for every kept column
    for (int k = 0; k < 36; ++k) f.ginv[k] = 0.0;
    for (int b = 0; b < 6; ++b) {
        if (!kept[b]) continue;
        double y[6] = {}, x[6] = {};
        for (int a = 0; a < 6; ++a) {
            if (!kept[a]) continue;
            double s = a == b ? 1.0 : 0.0;
            for (int c = 0; c < a; ++c)
                if (kept[c]) s -= L[a][c] * y[c];
            y[a] = s / L[a][a];
        }
        for (int a = 5; a >= 0; --a) {
            if (!kept[a]) continue;
            double s = y[a];
            for (int c = a + 1; c < 6; ++c)
                if (kept[c]) s -= L[c][a] * x[c];
            x[a] = s / L[a][a];
        }
        for (int a = 0; a < 6; ++a) f.ginv[6 * a + b] = x[a];
    }
}

}  // namespace b4d

using namespace b4d;

extern "C" size_t b4d_integrate_workspace_bytes(int n, int ny, int nx) {
    if (n < 1 || ny < 1 || nx < 1 || ny > WF_MAX_SIDE || nx > WF_MAX_SIDE) return 0;
    return (size_t)n * ny * nx * sizeof(float);
}

extern "C" int b4d_integrate_gradient(const float* gy, const float* gx, int n, int ny, int nx, double hy, double hx, void* workspace,
                                      float* out, void* stream) {
    if (!gy || !gx || !workspace || !out) return fail(B4D_EINVAL, "null argument");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    if (!(hy > 0.0 && hx > 0.0 && std::isfinite(hy) && std::isfinite(hx)))
        return fail(B4D_EINVAL, "grid spacings must be finite and > 0");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const long long plane = (long long)ny * nx;
    std::lock_guard<std::mutex> lk(wf_mutex());     // basis pointers stay valid until the launches below are queued
    const WfBasis *by = nullptr, *bx = nullptr;
    if (const int rc = wf_basis(ny, ny, &by)) return rc;
    if (const int rc = wf_basis(nx, ny, &bx)) return rc;
    hipLaunchKernelGGL(k_wf_rhs, dim3((unsigned)((plane + 255) / 256), n), dim3(256), 0, st, gy, gx, ny, nx, (float)(1.0 / hy),
                       (float)(1.0 / hx), out);
    const dim3 grid((nx + WF_TILE - 1) / WF_TILE, (ny + WF_TILE - 1) / WF_TILE, n);
    const double ihy2 = 1.0 / (hy * hy), ihx2 = 1.0 / (hx * hx);
    const WfGemm p1{out, bx->CT, ws, ny, nx, nx, plane, 0, plane, nullptr, nullptr, 0.0, 0.0};          // A1 = r . Cx^T
    const WfGemm p2{by->C, ws, out, ny, nx, ny, 0, plane, plane, by->lam, bx->lam, ihy2, ihx2};         // P = (Cy . A1) / Lambda
    const WfGemm p3{out, bx->C, ws, ny, nx, nx, plane, 0, plane, nullptr, nullptr, 0.0, 0.0};           // A2 = P . Cx
    const WfGemm p4{by->CT, ws, out, ny, nx, ny, 0, plane, plane, nullptr, nullptr, 0.0, 0.0};          // phi = Cy^T . A2
    hipLaunchKernelGGL(k_wf_gemm<false>, grid, dim3(256), 0, st, p1);
    hipLaunchKernelGGL(k_wf_gemm<true>, grid, dim3(256), 0, st, p2);
    hipLaunchKernelGGL(k_wf_gemm<false>, grid, dim3(256), 0, st, p3);
    hipLaunchKernelGGL(k_wf_gemm<false>, grid, dim3(256), 0, st, p4);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

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
