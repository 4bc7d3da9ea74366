// b4d_integrate.hip -- wavefront reconstruction: least-squares integration of a slope field on a regular grid and the
// low-order (6-term quadratic) fit of the result; the weighted variants (section 14) and the phase unwraps
// that share their solvers (sections 17 and 18).
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
#include "b4d_reduce.hpp"

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
    const int* skip;   // per batch entry, may be null: a non-zero entry leaves its C untouched (maps that the weighted solver has frozen)
};

template <bool DIV>
__global__ void __launch_bounds__(256) k_wf_gemm(WfGemm g) {
    __shared__ float As[WF_BK][WF_LD];  // [k][m]
    __shared__ float Bs[WF_BK][WF_LD];  // [k][n]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int m0 = blockIdx.y * WF_TILE, n0 = blockIdx.x * WF_TILE;
    if (g.skip && g.skip[blockIdx.z]) return;
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

// ---- weighted / masked integration: preconditioned conjugate gradients on the weighted normal equations
// A phi = b, started from 0, the unweighted DCT solve above as preconditioner.  Vectors are float32; every dot product is
// accumulated in float64 per workgroup, written to the workspace and summed in index order by whoever needs it; alpha, beta and
// the per-map state live on the device.  grid (nb, maps), nb = wf_pcg_blocks(plane) workgroups stride over a map.
constexpr int WF_PCG_THREADS = 256;
constexpr int WF_PCG_MAXBLOCKS = 256;   // partials per map and dot product
constexpr int WF_PCG_CHECK = 4;         // the host reads the per-map flags every this many iterations

struct WfPcgState {   // per map; iteration k reads slot k & 1 and writes the other, so no workgroup reads what another writes
    double rz;        // r . z of the current search direction
    double rr;        // |r|^2 of the recurrence residual
    int iters;
    int frozen;
};

struct WfPcg {
    float *weff, *cy, *cx, *r, *p, *qz, *t;   // (n, ny, nx) each: node weights, edge coefficients wy/hy^2 and wx/hx^2, PCG vectors
    double *bb, *part_a, *part_b, *part_c;    // (n), 3 x (n, nb): |b|^2; partials of |b|^2 then p.q; of r.r; of r.z
    WfPcgState* state;                        // (2, n)
    int *badpq, *flags;                       // (n): p.q was not finite and positive; frozen, for the host
    int n, ny, nx, nb;
    double tol2;                              // rtol^2
};

static int wf_pcg_blocks(long long plane) {
    const long long b = (plane + WF_PCG_THREADS - 1) / WF_PCG_THREADS;
    return (int)(b < WF_PCG_MAXBLOCKS ? b : WF_PCG_MAXBLOCKS);
}

static size_t wf_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// carves the caller's workspace; returns the bytes used (base == nullptr: size only)
static size_t wf_pcg_layout(char* base, int n, int ny, int nx, WfPcg& g) {
    const size_t plane = (size_t)ny * nx, fv = wf_align256((size_t)n * plane * sizeof(float));
    const int nb = wf_pcg_blocks((long long)plane);
    const size_t dv = wf_align256((size_t)n * nb * sizeof(double)), sv = wf_align256((size_t)n * sizeof(double));
    size_t o = 0;
    float** fp[7] = {&g.weff, &g.cy, &g.cx, &g.r, &g.p, &g.qz, &g.t};
    for (auto f : fp) {
        *f = (float*)(base + o);
        o += fv;
    }
    g.bb = (double*)(base + o), o += sv;
    double** dp[3] = {&g.part_a, &g.part_b, &g.part_c};
    for (auto d : dp) {
        *d = (double*)(base + o);
        o += dv;
    }
    g.state = (WfPcgState*)(base + o), o += wf_align256(2 * (size_t)n * sizeof(WfPcgState));
    g.badpq = (int*)(base + o), o += wf_align256((size_t)n * sizeof(int));
    g.flags = (int*)(base + o), o += wf_align256((size_t)n * sizeof(int));
    g.n = n, g.ny = ny, g.nx = nx, g.nb = nb;
    return o;
}

// sum of the nb partials of one map, in index order (every lane the same chain, so every workgroup gets the same bits)
__device__ __forceinline__ double wf_sum_partials(const double* __restrict__ part, int map, int nb) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(size_t)map * nb + b];
    return s;
}

// effective weight of a node: 0 unless the weight is finite and positive and both slopes are finite
__device__ __forceinline__ float wf_weff(const float* __restrict__ w, const float* __restrict__ gy, const float* __restrict__ gx, int e) {
    const float a = w[e];
    return (a > 0.f && isfinite(a) && isfinite(gy[e]) && isfinite(gx[e])) ? a : 0.f;
}

// harmonic mean 2ab / (a + b) of two node weights, 0 if either is 0
__device__ __forceinline__ float wf_hmean(float a, float b) { return (a > 0.f && b > 0.f) ? 2.f * a * (b / (a + b)) : 0.f; }

// once per call: effective weights, edge coefficients, b, x = 0, partials of |b|^2.  Slopes of weight-0 nodes only pass through
// isfinite: their edges have coefficient 0 and are selected away, not multiplied.  w_stride 0 shares the weights across maps.
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_wsetup(const float* __restrict__ gy, const float* __restrict__ gx,
                                                              const float* __restrict__ w, long long w_stride, float ihy, float ihx,
                                                              WfPcg g, float* __restrict__ x) {
    __shared__ double sh[WF_PCG_THREADS / 64][1];
    const int map = blockIdx.y, ny = g.ny, nx = g.nx, plane = ny * nx;
    const size_t fo = (size_t)map * plane;
    const float* __restrict__ my = gy + fo;
    const float* __restrict__ mx = gx + fo;
    const float* __restrict__ mw = w + (long long)map * w_stride;
    double s[1] = {0.0};
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS) {
        const int i = e / nx, j = e % nx;
        const float w0 = wf_weff(mw, my, mx, e);
        const float hd = i + 1 < ny ? wf_hmean(w0, wf_weff(mw, my, mx, e + nx)) : 0.f;
        const float hu = i > 0 ? wf_hmean(w0, wf_weff(mw, my, mx, e - nx)) : 0.f;
        const float hr = j + 1 < nx ? wf_hmean(w0, wf_weff(mw, my, mx, e + 1)) : 0.f;
        const float hl = j > 0 ? wf_hmean(w0, wf_weff(mw, my, mx, e - 1)) : 0.f;
        float by = 0.f, bx = 0.f;
        if (hu > 0.f) by += hu * (0.5f * (my[e - nx] + my[e]));
        if (hd > 0.f) by -= hd * (0.5f * (my[e] + my[e + nx]));
        if (hl > 0.f) bx += hl * (0.5f * (mx[e - 1] + mx[e]));
        if (hr > 0.f) bx -= hr * (0.5f * (mx[e] + mx[e + 1]));
        const float b = by * ihy + bx * ihx;
        g.weff[fo + e] = w0;
        g.cy[fo + e] = hd * ihy * ihy;
        g.cx[fo + e] = hr * ihx * ihx;
        g.r[fo + e] = b;
        x[fo + e] = 0.f;
        s[0] += (double)b * (double)b;
    }
    block_sum(s, &sh[0][0], WF_PCG_THREADS / 64);
    if (threadIdx.x == 0) g.part_a[(size_t)map * g.nb + blockIdx.x] = s[0];
}

// q = A p (weighted 5-point operator; the last row of cy and the last column of cx are 0), partials of p . q
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_wapply(WfPcg g, int slot) {
    __shared__ double sh[WF_PCG_THREADS / 64][1];
    const int map = blockIdx.y;
    if (g.state[(size_t)slot * g.n + map].frozen) return;
    const int ny = g.ny, nx = g.nx, plane = ny * nx;
    const size_t fo = (size_t)map * plane;
    const float* __restrict__ p = g.p + fo;
    const float* __restrict__ cy = g.cy + fo;
    const float* __restrict__ cx = g.cx + fo;
    double s[1] = {0.0};
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS) {
        const int i = e / nx, j = e % nx;
        const float pc = p[e];
        float a = 0.f;
        if (i > 0) a += cy[e - nx] * (pc - p[e - nx]);
        if (i + 1 < ny) a += cy[e] * (pc - p[e + nx]);
        if (j > 0) a += cx[e - 1] * (pc - p[e - 1]);
        if (j + 1 < nx) a += cx[e] * (pc - p[e + 1]);
        g.qz[fo + e] = a;
        s[0] += (double)pc * (double)a;
    }
    block_sum(s, &sh[0][0], WF_PCG_THREADS / 64);
    if (threadIdx.x == 0) g.part_a[(size_t)map * g.nb + blockIdx.x] = s[0];
}

// alpha = r.z / p.q in float64; x += alpha p, r -= alpha q, partials of r . r.  A p.q that is not finite and positive stops the map.
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_wupdate(WfPcg g, int slot, float* __restrict__ x) {
    __shared__ double sh[WF_PCG_THREADS / 64][1];
    const int map = blockIdx.y;
    const WfPcgState st = g.state[(size_t)slot * g.n + map];
    if (st.frozen) return;
    const double pq = wf_sum_partials(g.part_a, map, g.nb);
    if (!(pq > 0.0 && isfinite(pq))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) g.badpq[map] = 1;
        return;
    }
    const float alpha = (float)(st.rz / pq);
    const int plane = g.ny * g.nx;
    const size_t fo = (size_t)map * plane;
    double s[1] = {0.0};
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS) {
        x[fo + e] = fmaf(alpha, g.p[fo + e], x[fo + e]);
        const float r = fmaf(-alpha, g.qz[fo + e], g.r[fo + e]);
        g.r[fo + e] = r;
        s[0] += (double)r * (double)r;
    }
    block_sum(s, &sh[0][0], WF_PCG_THREADS / 64);
    if (threadIdx.x == 0) g.part_b[(size_t)map * g.nb + blockIdx.x] = s[0];
}

// partials of r . z (z = M r sits in qz after the four products)
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_wdot(WfPcg g, int slot, int first) {
    __shared__ double sh[WF_PCG_THREADS / 64][1];
    const int map = blockIdx.y;
    if (!first && (g.state[(size_t)slot * g.n + map].frozen || g.badpq[map])) return;
    const int plane = g.ny * g.nx;
    const size_t fo = (size_t)map * plane;
    double s[1] = {0.0};
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS)
        s[0] += (double)g.r[fo + e] * (double)g.qz[fo + e];
    block_sum(s, &sh[0][0], WF_PCG_THREADS / 64);
    if (threadIdx.x == 0) g.part_c[(size_t)map * g.nb + blockIdx.x] = s[0];
}

// state of the next iteration and p = z + beta p.  first: state from |b|^2 and r.z, p = z.  A map is frozen when b = 0 (or not
// finite), when p.q was bad, or when |r| <= rtol |b|; a frozen map is not touched again, so no 0/0 is ever formed for it.
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_wdirection(WfPcg g, int slot, int first) {
    const int map = blockIdx.y;
    WfPcgState st;
    double beta = 0.0;
    if (first) {
        const double bb = wf_sum_partials(g.part_a, map, g.nb);
        st.rr = bb;
        st.iters = 0;
        st.frozen = !(bb > 0.0 && isfinite(bb));
        st.rz = st.frozen ? 0.0 : wf_sum_partials(g.part_c, map, g.nb);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            g.bb[map] = bb;
            g.badpq[map] = 0;
        }
    } else {
        st = g.state[(size_t)slot * g.n + map];
        if (!st.frozen) {
            if (g.badpq[map]) {
                st.frozen = 1;
            } else {
                st.rr = wf_sum_partials(g.part_b, map, g.nb);
                st.iters += 1;
                if (st.rr <= g.tol2 * g.bb[map] || !isfinite(st.rr)) {
                    st.frozen = 1;
                } else {
                    const double rz = wf_sum_partials(g.part_c, map, g.nb);
                    beta = st.rz > 0.0 ? rz / st.rz : 0.0;
                    st.rz = rz;
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        g.state[(size_t)(first ? 0 : slot ^ 1) * g.n + map] = st;
        g.flags[map] = st.frozen;
    }
    if (st.frozen) return;
    const float bt = (float)beta;
    const int plane = g.ny * g.nx;
    const size_t fo = (size_t)map * plane;
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS)
        g.p[fo + e] = first ? g.qz[fo + e] : fmaf(bt, g.p[fo + e], g.qz[fo + e]);
}

// iterations, final |r| / |b| (0 for b = 0), and NaN at the weight-0 nodes when asked
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_wfinish(WfPcg g, int slot, int nan_invalid, float* __restrict__ x,
                                                               int* __restrict__ iterations, double* __restrict__ residual) {
    const int map = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const WfPcgState st = g.state[(size_t)slot * g.n + map];
        const double bb = g.bb[map];
        iterations[map] = st.iters;
        residual[map] = (bb > 0.0 && isfinite(bb)) ? sqrt(st.rr / bb) : 0.0;
    }
    if (!nan_invalid) return;
    const int plane = g.ny * g.nx;
    const size_t fo = (size_t)map * plane;
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS)
        if (!(g.weff[fo + e] > 0.f)) x[fo + e] = __builtin_nanf("");
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

// z = M rhs: the four products of the DCT Poisson solve; `out` may be `rhs` itself, `scratch` is distinct from both; maps with a
// non-zero skip[] entry (may be null) are left out
static void wf_poisson(const WfBasis* by, const WfBasis* bx, const float* rhs, float* scratch, float* out, int n, int ny, int nx,
                       double hy, double hx, const int* skip, hipStream_t st) {
    const long long plane = (long long)ny * nx;
    const dim3 grid((nx + WF_TILE - 1) / WF_TILE, (ny + WF_TILE - 1) / WF_TILE, n);
    const double ihy2 = 1.0 / (hy * hy), ihx2 = 1.0 / (hx * hx);
    const WfGemm p1{rhs, bx->CT, scratch, ny, nx, nx, plane, 0, plane, nullptr, nullptr, 0.0, 0.0, skip};        // A1 = r . Cx^T
    const WfGemm p2{by->C, scratch, out, ny, nx, ny, 0, plane, plane, by->lam, bx->lam, ihy2, ihx2, skip};       // P = (Cy . A1) / Lambda
    const WfGemm p3{out, bx->C, scratch, ny, nx, nx, plane, 0, plane, nullptr, nullptr, 0.0, 0.0, skip};         // A2 = P . Cx
    const WfGemm p4{by->CT, scratch, out, ny, nx, ny, 0, plane, plane, nullptr, nullptr, 0.0, 0.0, skip};        // phi = Cy^T . A2
    hipLaunchKernelGGL(k_wf_gemm<false>, grid, dim3(256), 0, st, p1);
    hipLaunchKernelGGL(k_wf_gemm<true>, grid, dim3(256), 0, st, p2);
    hipLaunchKernelGGL(k_wf_gemm<false>, grid, dim3(256), 0, st, p3);
    hipLaunchKernelGGL(k_wf_gemm<false>, grid, dim3(256), 0, st, p4);
}

// ---- phase unwrapping: the wrapped differences of neighbouring nodes are the EDGE slopes of the same
// 5-point Neumann problem (no Southwell means), so the right-hand side is their divergence and wf_poisson solves it; the
// congruence step then moves every node by the whole number of turns that brings it closest to the solution.
__device__ __forceinline__ float wf_wrap(float a) { return a - 6.283185307179586f * rintf(a * 0.15915494309189535f); }

// r[i][j] = W(ph[i][j] - ph[i-1][j]) - W(ph[i+1][j] - ph[i][j]) + W(ph[i][j] - ph[i][j-1]) - W(ph[i][j+1] - ph[i][j]), terms with
// a node outside the grid absent.  grid (ceil(ny nx / 256), batch)
__global__ void __launch_bounds__(256) k_wf_unwrap_rhs(const float* __restrict__ ph, int ny, int nx, float* __restrict__ r) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ny * nx) return;
    const size_t fo = (size_t)blockIdx.y * ny * nx;
    const int i = e / nx, j = e % nx;
    const float* __restrict__ p = ph + fo + e;
    const float c = p[0];
    float s = 0.f;
    if (i > 0) s += wf_wrap(c - p[-nx]);
    if (i + 1 < ny) s -= wf_wrap(p[nx] - c);
    if (j > 0) s += wf_wrap(c - p[-1]);
    if (j + 1 < nx) s -= wf_wrap(p[1] - c);
    r[fo + e] = s;
}

// out = ph + 2 pi round((p + (ph[c] - p[c]) - ph) / 2 pi) with c the node (ny / 2, nx / 2); a node that keeps its level keeps its bits
__global__ void __launch_bounds__(256) k_wf_unwrap_congruence(const float* __restrict__ ph, const float* __restrict__ p, int ny, int nx,
                                                              float* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ny * nx) return;
    const size_t fo = (size_t)blockIdx.y * ny * nx;
    const size_t c = fo + (size_t)(ny / 2) * nx + nx / 2;
    const float shift = ph[c] - p[c];
    const float v = ph[fo + e];
    const float k = rintf((p[fo + e] + shift - v) * 0.15915494309189535f);
    out[fo + e] = k == 0.f ? v : (float)((double)v + 6.283185307179586 * (double)k);
}

// ---- the PCG loop of section 14, shared by the weighted integration and the weighted unwrap.  A setup kernel has written weff, cy,
// cx, r = b, x = 0 and the partials of |b|^2 into part_a; x is the solution, started at 0.  Ends with k_wf_wfinish.  The caller
// holds wf_mutex() (the basis pointers stay valid until the launches are queued).
static int wf_pcg_solve(const WfPcg& g, const WfBasis* by, const WfBasis* bx, double hy, double hx, int max_iter, int nan_invalid,
                        float* x, int* iterations, double* residual, hipStream_t st) {
    const int n = g.n, ny = g.ny, nx = g.nx;
    const dim3 grid(g.nb, n), block(WF_PCG_THREADS);
    wf_poisson(by, bx, g.r, g.t, g.qz, n, ny, nx, hy, hx, nullptr, st);
    hipLaunchKernelGGL(k_wf_wdot, grid, block, 0, st, g, 0, 1);
    hipLaunchKernelGGL(k_wf_wdirection, grid, block, 0, st, g, 0, 1);
    std::vector<int> flags(n);
    int done = 0;
    while (done < max_iter) {
        const int slot = done & 1;
        hipLaunchKernelGGL(k_wf_wapply, grid, block, 0, st, g, slot);
        hipLaunchKernelGGL(k_wf_wupdate, grid, block, 0, st, g, slot, x);
        wf_poisson(by, bx, g.r, g.t, g.qz, n, ny, nx, hy, hx, g.flags, st);      // frozen maps cost no products
        hipLaunchKernelGGL(k_wf_wdot, grid, block, 0, st, g, slot, 0);
        hipLaunchKernelGGL(k_wf_wdirection, grid, block, 0, st, g, slot, 0);
        ++done;
        if (done % WF_PCG_CHECK == 0 && done < max_iter) {   // every map frozen: stop early (one small copy and a wait)
            B4D_HIP(hipMemcpyAsync(flags.data(), g.flags, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
            B4D_HIP(hipStreamSynchronize(st));
            bool all = true;
            for (int m = 0; m < n && all; ++m) all = flags[m] != 0;
            if (all) break;
        }
    }
    hipLaunchKernelGGL(k_wf_wfinish, grid, block, 0, st, g, done & 1, nan_invalid, x, iterations, residual);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

// ---- weighted / masked unwrapping: the weighted normal equations of section 14 with the wrapped differences
// as edge slopes (unit spacings), then the congruence step against a seed node chosen among the valid ones.
// effective weight of a node: 0 unless the weight is finite and positive and the phase is finite
__device__ __forceinline__ float wf_unwrap_weff(const float* __restrict__ w, const float* __restrict__ ph, int e) {
    const float a = w[e];
    return (a > 0.f && isfinite(a) && isfinite(ph[e])) ? a : 0.f;
}

// once per call, as k_wf_wsetup: effective weights, edge coefficients, b = weighted divergence of the wrapped differences, x = 0,
// partials of |b|^2.  A difference is formed only across an edge of positive coefficient, so the phase of a weight-0 node (NaN
// included) passes through isfinite alone.
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_unwrap_wsetup(const float* __restrict__ phase, const float* __restrict__ w,
                                                                     long long w_stride, WfPcg g, float* __restrict__ x) {
    __shared__ double sh[WF_PCG_THREADS / 64][1];
    const int map = blockIdx.y, ny = g.ny, nx = g.nx, plane = ny * nx;
    const size_t fo = (size_t)map * plane;
    const float* __restrict__ ph = phase + fo;
    const float* __restrict__ mw = w + (long long)map * w_stride;
    double s[1] = {0.0};
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS) {
        const int i = e / nx, j = e % nx;
        const float w0 = wf_unwrap_weff(mw, ph, e);
        const float hd = i + 1 < ny ? wf_hmean(w0, wf_unwrap_weff(mw, ph, e + nx)) : 0.f;
        const float hu = i > 0 ? wf_hmean(w0, wf_unwrap_weff(mw, ph, e - nx)) : 0.f;
        const float hr = j + 1 < nx ? wf_hmean(w0, wf_unwrap_weff(mw, ph, e + 1)) : 0.f;
        const float hl = j > 0 ? wf_hmean(w0, wf_unwrap_weff(mw, ph, e - 1)) : 0.f;
        float by = 0.f, bx = 0.f;
        if (hu > 0.f) by += hu * wf_wrap(ph[e] - ph[e - nx]);
        if (hd > 0.f) by -= hd * wf_wrap(ph[e + nx] - ph[e]);
        if (hl > 0.f) bx += hl * wf_wrap(ph[e] - ph[e - 1]);
        if (hr > 0.f) bx -= hr * wf_wrap(ph[e + 1] - ph[e]);
        const float b = by + bx;
        g.weff[fo + e] = w0;
        g.cy[fo + e] = hd;
        g.cx[fo + e] = hr;
        g.r[fo + e] = b;
        x[fo + e] = 0.f;
        s[0] += (double)b * (double)b;
    }
    block_sum(s, &sh[0][0], WF_PCG_THREADS / 64);
    if (threadIdx.x == 0) g.part_a[(size_t)map * g.nb + blockIdx.x] = s[0];
}

// seed node of a map: the valid node of largest weight, ties to the smallest (i - ny/2)^2 + (j - nx/2)^2, then to the smallest
// index.  The three keys order the nodes totally, so the winner does not depend on the order of the comparisons; they are made
// in a fixed order all the same (lane stride, then a tree over the workgroup in LDS).  One workgroup per map; seed = -1 and
// shift = 0 for a map without a valid node, else shift = phase[seed] - p[seed].
struct WfSeed {
    float w;
    int d, e;
};
__device__ __forceinline__ bool wf_seed_better(const WfSeed& a, const WfSeed& b) {   // a before b
    if (a.w != b.w) return a.w > b.w;
    if (a.d != b.d) return a.d < b.d;
    return a.e < b.e;
}

__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_unwrap_seed(const float* __restrict__ phase, WfPcg g, const float* __restrict__ p,
                                                                   int* __restrict__ seed, float* __restrict__ shift) {
    __shared__ WfSeed sh[WF_PCG_THREADS];
    const int map = blockIdx.x, ny = g.ny, nx = g.nx, plane = ny * nx;
    const size_t fo = (size_t)map * plane;
    WfSeed best{0.f, 0x7fffffff, 0x7fffffff};
    for (int e = threadIdx.x; e < plane; e += WF_PCG_THREADS) {
        const int di = e / nx - ny / 2, dj = e % nx - nx / 2;
        const WfSeed c{g.weff[fo + e], di * di + dj * dj, e};
        if (c.w > 0.f && wf_seed_better(c, best)) best = c;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int o = WF_PCG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && wf_seed_better(sh[threadIdx.x + o], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool any = sh[0].w > 0.f;
        seed[map] = any ? sh[0].e : -1;
        shift[map] = any ? phase[fo + sh[0].e] - p[fo + sh[0].e] : 0.f;
    }
}

// in place on the solution p (= out): out = ph + 2 pi round((p + shift - ph) / 2 pi) at the valid nodes, a node that keeps its
// level keeps its bits; weight-0 nodes get NaN or the levelled p + shift; a map without a valid node is NaN throughout
__global__ void __launch_bounds__(WF_PCG_THREADS) k_wf_unwrap_wcongruence(const float* __restrict__ phase, WfPcg g,
                                                                          const int* __restrict__ seed, const float* __restrict__ shift,
                                                                          int nan_invalid, float* __restrict__ out) {
    const int map = blockIdx.y, plane = g.ny * g.nx;
    const size_t fo = (size_t)map * plane;
    const bool none = seed[map] < 0;
    const float sf = shift[map];
    for (int e = blockIdx.x * WF_PCG_THREADS + threadIdx.x; e < plane; e += g.nb * WF_PCG_THREADS) {
        const float p = out[fo + e] + sf;
        float r;
        if (g.weff[fo + e] > 0.f) {
            const float v = phase[fo + e];
            const float k = rintf((p - v) * 0.15915494309189535f);
            r = k == 0.f ? v : (float)((double)v + 6.283185307179586 * (double)k);
        } else {
            r = (nan_invalid || none) ? __builtin_nanf("") : p;
        }
        out[fo + e] = r;
    }
}

}  // namespace b4d

using namespace b4d;

extern "C" size_t b4d_phase_unwrap_workspace_bytes(int n, int ny, int nx) {
    if (n < 1 || n > 65535 || ny < 1 || nx < 1 || ny > WF_MAX_SIDE || nx > WF_MAX_SIDE) return 0;
    return 2 * wf_align256((size_t)n * ny * nx * sizeof(float));
}

extern "C" int b4d_phase_unwrap(const float* phase, int n, int ny, int nx, void* workspace, float* out, void* stream) {
    if (!phase || !workspace || !out) return fail(B4D_EINVAL, "null argument");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long plane = (long long)ny * nx;
    float* p = (float*)workspace;
    float* scratch = (float*)((char*)workspace + wf_align256((size_t)n * plane * sizeof(float)));
    std::lock_guard<std::mutex> lk(wf_mutex());     // basis pointers stay valid until the launches below are queued
    const WfBasis *by = nullptr, *bx = nullptr;
    if (const int rc = wf_basis(ny, ny, &by)) return rc;
    if (const int rc = wf_basis(nx, ny, &bx)) return rc;
    const dim3 grid((unsigned)((plane + 255) / 256), n);
    hipLaunchKernelGGL(k_wf_unwrap_rhs, grid, dim3(256), 0, st, phase, ny, nx, p);
    wf_poisson(by, bx, p, scratch, p, n, ny, nx, 1.0, 1.0, nullptr, st);
    hipLaunchKernelGGL(k_wf_unwrap_congruence, grid, dim3(256), 0, st, phase, (const float*)p, ny, nx, out);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

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
    wf_poisson(by, bx, out, ws, out, n, ny, nx, hy, hx, nullptr, st);
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

extern "C" size_t b4d_integrate_weighted_workspace_bytes(int n, int ny, int nx) {
    if (n < 1 || n > 65535 || ny < 1 || nx < 1 || ny > WF_MAX_SIDE || nx > WF_MAX_SIDE) return 0;
    WfPcg g;
    return wf_pcg_layout(nullptr, n, ny, nx, g);
}

extern "C" int b4d_integrate_gradient_weighted(const float* gy, const float* gx, const float* w, long long w_stride, int n, int ny,
                                               int nx, double hy, double hx, double rtol, int max_iter, int nan_invalid,
                                               void* workspace, float* out, int* iterations, double* residual, void* stream) {
    if (!gy || !gx || !w || !workspace || !out || !iterations || !residual) return fail(B4D_EINVAL, "null argument");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    if (!(hy > 0.0 && hx > 0.0 && std::isfinite(hy) && std::isfinite(hx)))
        return fail(B4D_EINVAL, "grid spacings must be finite and > 0");
    const long long plane = (long long)ny * nx;
    if (w_stride != 0 && w_stride != plane) return fail(B4D_EINVAL, "w_stride is 0 (shared weights) or ny * nx (per map)");
    if (!(rtol >= 0.0 && std::isfinite(rtol))) return fail(B4D_EINVAL, "rtol must be finite and >= 0");
    if (max_iter < 0) return fail(B4D_EINVAL, "max_iter must be >= 0");
    hipStream_t st = (hipStream_t)stream;
    WfPcg g;
    wf_pcg_layout((char*)workspace, n, ny, nx, g);
    g.tol2 = rtol * rtol;
    std::lock_guard<std::mutex> lk(wf_mutex());     // basis pointers stay valid until the launches below are queued
    const WfBasis *by = nullptr, *bx = nullptr;
    if (const int rc = wf_basis(ny, ny, &by)) return rc;
    if (const int rc = wf_basis(nx, ny, &bx)) return rc;
    hipLaunchKernelGGL(k_wf_wsetup, dim3(g.nb, n), dim3(WF_PCG_THREADS), 0, st, gy, gx, w, w_stride, (float)(1.0 / hy),
                       (float)(1.0 / hx), g, out);
    return wf_pcg_solve(g, by, bx, hy, hx, max_iter, nan_invalid, out, iterations, residual, st);
}

extern "C" size_t b4d_phase_unwrap_weighted_workspace_bytes(int n, int ny, int nx) {
    if (n < 1 || n > 65535 || ny < 1 || nx < 1 || ny > WF_MAX_SIDE || nx > WF_MAX_SIDE) return 0;
    WfPcg g;
    return wf_pcg_layout(nullptr, n, ny, nx, g) + 2 * wf_align256((size_t)n * sizeof(int));
}

extern "C" int b4d_phase_unwrap_weighted(const float* phase, const float* w, long long w_stride, int n, int ny, int nx, double rtol,
                                         int max_iter, int nan_invalid, void* workspace, float* out, int* iterations, double* residual,
                                         void* stream) {
    if (!phase || !w || !workspace || !out || !iterations || !residual) return fail(B4D_EINVAL, "null argument");
    if (phase == out) return fail(B4D_EINVAL, "unwrap: out must not be the input");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    const long long plane = (long long)ny * nx;
    if (w_stride != 0 && w_stride != plane) return fail(B4D_EINVAL, "w_stride is 0 (shared weights) or ny * nx (per map)");
    if (!(rtol >= 0.0 && std::isfinite(rtol))) return fail(B4D_EINVAL, "rtol must be finite and >= 0");
    if (max_iter < 0) return fail(B4D_EINVAL, "max_iter must be >= 0");
    hipStream_t st = (hipStream_t)stream;
    WfPcg g;
    char* tail = (char*)workspace + wf_pcg_layout((char*)workspace, n, ny, nx, g);
    int* seed = (int*)tail;
    float* shift = (float*)(tail + wf_align256((size_t)n * sizeof(int)));
    g.tol2 = rtol * rtol;
    std::lock_guard<std::mutex> lk(wf_mutex());     // basis pointers stay valid until the launches below are queued
    const WfBasis *by = nullptr, *bx = nullptr;
    if (const int rc = wf_basis(ny, ny, &by)) return rc;
    if (const int rc = wf_basis(nx, ny, &bx)) return rc;
    const dim3 grid(g.nb, n), block(WF_PCG_THREADS);
    hipLaunchKernelGGL(k_wf_unwrap_wsetup, grid, block, 0, st, phase, w, w_stride, g, out);
    if (const int rc = wf_pcg_solve(g, by, bx, 1.0, 1.0, max_iter, 0, out, iterations, residual, st)) return rc;
    hipLaunchKernelGGL(k_wf_unwrap_seed, dim3(n), block, 0, st, phase, g, (const float*)out, seed, shift);
    hipLaunchKernelGGL(k_wf_unwrap_wcongruence, grid, block, 0, st, phase, g, (const int*)seed, (const float*)shift, nan_invalid, out);
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
