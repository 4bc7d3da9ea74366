// b4d_integrate.hip -- wavefront reconstruction: least-squares integration of a slope field on a regular grid (DESIGN.md
// section 13): the product kernel, the DCT basis cache and the Poisson solve; the weighted variant by preconditioned conjugate
// gradients (section 14) and the two phase unwraps that share these solvers (sections 17 and 18); the fit: b4d_poly2.hip.
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
#include "b4d_mfma.hpp"
#include "b4d_reduce.hpp"
#include "b4d_wf.hpp"

namespace b4d {

constexpr int WF_TILE = 128;   // output tile of a workgroup (4 waves in 2 x 2, each 2 x 2 MFMA tiles of 32 x 32)
constexpr int WF_BK = 16;
constexpr int WF_LD = 130;     // LDS row stride: 130 % 32 == 2 keeps the staging writes (k fastest) off each other's banks

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
// shares an operand).  K and the M / N edges are padded with zeros in LDS; multiply and lane maps: b4d_mfma.hpp.
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
    const WaveTile t = wave_tile(threadIdx.x);
    const int m0 = blockIdx.y * WF_TILE, n0 = blockIdx.x * WF_TILE;
    if (g.skip && g.skip[blockIdx.z]) return;
    const float* __restrict__ A = g.A + (long long)blockIdx.z * g.sA;
    const float* __restrict__ B = g.B + (long long)blockIdx.z * g.sB;
    float* __restrict__ Cm = g.C + (long long)blockIdx.z * g.sC;
    f32x16 acc[2][2];
    zero(acc);
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
        mma_slab<WF_BK>(As, Bs, t, acc);
        __syncthreads();
    }
    double lxn[2] = {0.0, 0.0};   // the x term of Lambda for the lane's two columns (32 apart), once per column
#pragma unroll
    for (int j = 0; DIV && j < 2; ++j) {
        const int n = n0 + 64 * t.wc + 32 * j + t.li;
        if (n < g.N) lxn[j] = g.lx[n] * g.ihx2;
    }
    for_each(acc, t, m0, n0, [&](int m, int n, float v) {
        if (m >= g.M || n >= g.N) return;
        if (DIV) v = (m == 0 && n == 0) ? 0.f : v / (float)(g.ly[m] * g.ihy2 + (((n - n0) & 32) ? lxn[1] : lxn[0]));
        Cm[(long long)m * g.N + n] = v;
    });
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

// carves the caller's workspace; returns the bytes used (base == nullptr: size only)
static size_t wf_pcg_layout(char* base, int n, int ny, int nx, WfPcg& g) {
    const size_t plane = (size_t)ny * nx, fv = align256((size_t)n * plane * sizeof(float));
    const int nb = wf_pcg_blocks((long long)plane);
    const size_t dv = align256((size_t)n * nb * sizeof(double)), sv = align256((size_t)n * sizeof(double));
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
    g.state = (WfPcgState*)(base + o), o += align256(2 * (size_t)n * sizeof(WfPcgState));
    g.badpq = (int*)(base + o), o += align256((size_t)n * sizeof(int));
    g.flags = (int*)(base + o), o += align256((size_t)n * sizeof(int));
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
    return 2 * align256((size_t)n * ny * nx * sizeof(float));
}

extern "C" int b4d_phase_unwrap(const float* phase, int n, int ny, int nx, void* workspace, float* out, void* stream) {
    if (!phase || !workspace || !out) return fail(B4D_EINVAL, "null argument");
    if (const int rc = wf_check_grid(n, ny, nx)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long plane = (long long)ny * nx;
    float* p = (float*)workspace;
    float* scratch = (float*)((char*)workspace + align256((size_t)n * plane * sizeof(float)));
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
    return wf_pcg_layout(nullptr, n, ny, nx, g) + 2 * align256((size_t)n * sizeof(int));
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
    float* shift = (float*)(tail + align256((size_t)n * sizeof(int)));
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
