// b4d_modal.hip -- modal fits of wavefront maps: Zernike modes (Noll order, unit rms over the unit disc) and products of
// Legendre polynomials (unit rms over the square), weighted least squares in float64.
//
//   k_modal_gram    grid (chunks, maps): a workgroup walks a contiguous chunk of nodes in tiles of 64, evaluates the J modes of
//                   every node by recurrence, stages sqrt(w) * mode and sqrt(w) * phi in LDS and accumulates the upper tile
//                   triangle of [A phi]^T W [A phi] with v_mfma_f64_16x16x4_f64; partial sums go to the workspace
//   k_modal_finish  one workgroup per map: partials summed in chunk order, Cholesky with the drop rule of the 6-term fit on the
//                   augmented matrix (its last row is the forward solve), back substitution, all in LDS
//   k_modal_apply   grid (blocks, maps): out = scale (phi - sum of the removed modes) or the bare synthesis, float64 per node,
//                   stored as float32; per-workgroup sums for the rms, which k_modal_rms adds in block order
//
// The chunking depends on (ny, nx, n_modes) alone, every sum has a fixed order and there are no floating-point atomics, so a map
// gives the same bits alone and inside any batch.
//
// Both bases run one table-driven evaluator: an outer factor f_m of the node (Zernike: (u + i v)^m by one complex multiply per
// order; Legendre: P_m(v) by Bonnet) times an inner three-term recurrence p_{k+1} = (A x + B) p_k - C p_{k-1} in x (Zernike:
// the Jacobi polynomials P_k^(m,0)(1 - 2 rho^2), so that R_n^m = (-1)^k rho^m P_k^(m,0); Legendre: P_k(u)).  No trigonometry, no
// division by rho.  The table (recurrence coefficients, norms, output columns) is built on the host in float64 and cached per
// device and basis.
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "b4d_common.hpp"
#include "b4d_reduce.hpp"

namespace b4d {

constexpr int MD_MAX_SIDE = 2048;
constexpr int MD_MAX_MODES = 66;                               // radial order 10 / total degree 10: the one cap
constexpr int MD_ORDERS = 11;                                  // outer orders 0 .. 10
constexpr int MD_COLS = 16 * ((MD_MAX_MODES + 1 + 15) / 16);   // modes + right-hand side, padded to MFMA tiles: 80
constexpr int MD_TILES = MD_COLS / 16;
constexpr int MD_PAIRS = MD_TILES * (MD_TILES + 1) / 2;
constexpr int MD_SLOTS = (MD_PAIRS + 3) / 4;                   // tile pairs per wave
constexpr int MD_NODES = 64;                                   // nodes per staged tile
constexpr int MD_LDN = MD_NODES + 2;   // LDS stride of a column: 66 % 32 == 2 spreads the 16 columns x 2 nodes of a half-wave read
constexpr int MD_THREADS = 256;
constexpr int MD_FIN_THREADS = 1024;   // finish kernel: four groups of 256
constexpr int MD_MAX_CHUNKS = 256;
constexpr int MD_MIN_TILES = 8;        // tiles per chunk at least
constexpr int MD_GL = MD_MAX_MODES + 15;   // LDS row stride of the finish kernel (odd: columns walk all banks)

typedef double md_f64x4 __attribute__((ext_vector_type(4)));

struct MdEntry {       // inner step k of outer order m
    double A, B, C;    // p_{k+1} = (A x + B) p_k - C p_{k-1}
    double nc, ns;     // mode[jc] = nc p_k Re f_m, mode[js] = ns p_k Im f_m
    int jc, js;        // 0-based columns, -1 for none
};
struct MdTable {
    MdEntry e[MD_ORDERS][MD_ORDERS];
    double oa[MD_ORDERS], oc[MD_ORDERS];   // Legendre outer step: f_{m+1} = oa[m] v f_m - oc[m] f_{m-1}
};
struct MdGeom {
    double cy, cx, sy, sx;
    int ny, nx, J, norders;
    int cnt[MD_ORDERS];    // inner steps of order m that reach a column < J
};

static void md_build_table(int basis, MdTable& t) {
    for (int m = 0; m < MD_ORDERS; ++m) {
        t.oa[m] = (2.0 * m + 1.0) / (m + 1.0);
        t.oc[m] = (double)m / (m + 1.0);
        for (int k = 0; k < MD_ORDERS; ++k) t.e[m][k] = MdEntry{0.0, 0.0, 0.0, 0.0, 0.0, -1, -1};
    }
    if (basis == 0) {
        for (int m = 0; m < MD_ORDERS; ++m)
            for (int k = 0; m + 2 * k < MD_ORDERS; ++k) {
                MdEntry& e = t.e[m][k];
                const int n = m + 2 * k, j0 = n * (n + 1) / 2;      // 0-based column of the first mode of radial order n
                const double sign = (k & 1) ? -1.0 : 1.0;
                if (m == 0) {
                    e.jc = j0;
                    e.nc = sign * std::sqrt(n + 1.0);
                } else {          // Noll: the pair sits at 1-based j0 + m, j0 + m + 1; the even number takes the cosine
                    const int a = j0 + m - 1, b = j0 + m;
                    e.jc = ((a + 1) % 2 == 0) ? a : b;
                    e.js = ((a + 1) % 2 == 0) ? b : a;
                    e.nc = e.ns = sign * std::sqrt(2.0 * (n + 1.0));
                }
                const int q = k + 1;      // Jacobi step to P_q^(m,0)
                const double al = m;
                if (q == 1) {
                    e.A = 0.5 * (al + 2.0);
                    e.B = 0.5 * al;
                    e.C = 0.0;
                } else {
                    const double s = 2.0 * q + al, den = 2.0 * q * (q + al) * (s - 2.0);
                    e.A = (s - 1.0) * s * (s - 2.0) / den;
                    e.B = (s - 1.0) * al * al / den;
                    e.C = 2.0 * (q + al - 1.0) * (q - 1.0) * s / den;
                }
            }
    } else {
        for (int b = 0; b < MD_ORDERS; ++b)
            for (int a = 0; a + b < MD_ORDERS; ++a) {
                MdEntry& e = t.e[b][a];
                const int d = a + b;
                e.jc = d * (d + 1) / 2 + b;
                e.nc = std::sqrt(2.0 * a + 1.0) * std::sqrt(2.0 * b + 1.0);
                e.A = (2.0 * a + 1.0) / (a + 1.0);
                e.B = 0.0;
                e.C = (double)a / (a + 1.0);
            }
    }
}

// device copies of the two tables, one per (device, basis); never released (6 KB each).  Caller holds md_mutex().
struct MdCached {
    int device, basis;
    MdTable* dev;
};
static std::mutex& md_mutex() {
    static std::mutex m;
    return m;
}
static int md_table(int basis, const MdTable** out) {
    static std::vector<MdCached> cache;
    int dev = 0;
    B4D_HIP(hipGetDevice(&dev));
    for (const auto& c : cache)
        if (c.device == dev && c.basis == basis) {
            *out = c.dev;
            return B4D_OK;
        }
    MdTable host;
    md_build_table(basis, host);
    MdTable* d = nullptr;
    B4D_HIP(hipMalloc((void**)&d, sizeof(MdTable)));
    const hipError_t e = hipMemcpy(d, &host, sizeof(MdTable), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(B4D_EHIP, std::string("modal: table upload: ") + hipGetErrorString(e));
    }
    cache.push_back(MdCached{dev, basis, d});
    *out = d;
    return B4D_OK;
}

static void md_geom(int basis, int ny, int nx, int J, double cy, double cx, double sy, double sx, MdGeom& g) {
    MdTable t;
    md_build_table(basis, t);
    g = MdGeom{cy, cx, sy, sx, ny, nx, J, 0, {}};
    for (int m = 0; m < MD_ORDERS; ++m) {
        g.cnt[m] = 0;
        for (int k = 0; k < MD_ORDERS; ++k) {
            const MdEntry& e = t.e[m][k];
            if ((e.jc >= 0 && e.jc < J) || (e.js >= 0 && e.js < J)) g.cnt[m] = k + 1;
        }
        if (g.cnt[m] > 0) g.norders = m + 1;
    }
}

// chunking of the Gram pass: a function of the grid alone
struct MdChunks {
    int tiles, per, chunks, blocks;    // 64-node tiles of a map, tiles per chunk, chunks; workgroups of the apply pass
};
__host__ __device__ inline MdChunks md_chunks(int ny, int nx) {
    MdChunks c;
    const long long nodes = (long long)ny * nx;
    c.tiles = (int)((nodes + MD_NODES - 1) / MD_NODES);
    c.per = (c.tiles + MD_MAX_CHUNKS - 1) / MD_MAX_CHUNKS;
    if (c.per < MD_MIN_TILES) c.per = MD_MIN_TILES;
    c.chunks = (c.tiles + c.per - 1) / c.per;
    const long long b = (nodes + MD_THREADS - 1) / MD_THREADS;
    c.blocks = (int)(b < MD_MAX_CHUNKS ? b : MD_MAX_CHUNKS);
    return c;
}
__host__ __device__ inline int md_tiles(int J) { return (J + 1 + 15) / 16; }
__host__ __device__ inline int md_pairs(int J) { return md_tiles(J) * (md_tiles(J) + 1) / 2; }

// node e -> (u, v)
__device__ __forceinline__ void md_coords(const MdGeom& g, int e, double& u, double& v) {
    const int i = e / g.nx, j = e - i * g.nx;
    u = ((double)j - g.cx) * g.sx;
    v = ((double)i - g.cy) * g.sy;
}
// the weight of a node from its raw weight a and map value x: 0 unless the weight is finite and positive, the node lies on the
// unit disc (Zernike) and the map value is finite; `value` is x for a node of positive weight and 0 otherwise, so that a
// rejected map value is selected away and enters no arithmetic
template <int BASIS>
__device__ __forceinline__ float md_weight(float a, float x, double u, double v, float& value) {
    const bool ok = a > 0.f && isfinite(a) && (BASIS != 0 || u * u + v * v <= 1.0 + 1e-9) && isfinite(x);
    value = ok ? x : 0.f;
    return ok ? a : 0.f;
}

// The evaluator: calls emit(column, value) for every mode below g.J of the orders m with (m & mask) == part.
template <int BASIS, class F>
__device__ __forceinline__ void md_modes(const MdTable* __restrict__ t, const MdGeom& g, double u, double v, int mask, int part, F emit) {
    const double x = BASIS == 0 ? 1.0 - 2.0 * (u * u + v * v) : u;
    double fr = 1.0, fi = 0.0, fprev = 0.0;
    for (int m = 0; m < g.norders; ++m) {
        if ((m & mask) == part) {
            double p = 1.0, pp = 0.0;
            const int cnt = g.cnt[m];
            for (int k = 0; k < cnt; ++k) {
                const MdEntry& e = t->e[m][k];
                if (e.jc >= 0 && e.jc < g.J) emit(e.jc, e.nc * p * fr);
                if (BASIS == 0 && e.js >= 0 && e.js < g.J) emit(e.js, e.ns * p * fi);
                const double pn = (e.A * x + e.B) * p - e.C * pp;
                pp = p;
                p = pn;
            }
        }
        if (BASIS == 0) {
            const double nr = fr * u - fi * v;
            fi = fr * v + fi * u;
            fr = nr;
        } else {
            const double fn = t->oa[m] * v * fr - t->oc[m] * fprev;
            fprev = fr;
            fr = fn;
        }
    }
}

// pair p of the upper tile triangle, row-major: (0,0), (0,1), .., (0,T-1), (1,1), ..
__device__ __forceinline__ void md_pair(int p, int T, int& ta, int& tb) {
    ta = 0;
    while (p >= T - ta) {
        p -= T - ta;
        ++ta;
    }
    tb = ta + p;
}

template <int BASIS>
__global__ void __launch_bounds__(MD_THREADS) k_modal_gram(const float* __restrict__ maps, const float* __restrict__ weights,
                                                           long long w_stride, const MdTable* __restrict__ table, MdGeom g,
                                                           double* __restrict__ partials) {
    __shared__ double S[MD_COLS * MD_LDN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nodes = g.ny * g.nx;
    const MdChunks ch = md_chunks(g.ny, g.nx);
    const int T = md_tiles(g.J), npairs = md_pairs(g.J);
    const float* __restrict__ phi = maps + (size_t)blockIdx.y * nodes;
    const float* __restrict__ w = weights ? weights + (long long)blockIdx.y * w_stride : nullptr;

    for (int k = tid; k < MD_COLS * MD_LDN; k += MD_THREADS) S[k] = 0.0;    // columns above J stay zero

    int ta[MD_SLOTS], tb[MD_SLOTS];
    md_f64x4 acc[MD_SLOTS];
#pragma unroll
    for (int q = 0; q < MD_SLOTS; ++q) {
        acc[q] = md_f64x4{0.0, 0.0, 0.0, 0.0};
        ta[q] = tb[q] = 0;
        if (wave + 4 * q < npairs) md_pair(wave + 4 * q, T, ta[q], tb[q]);
    }
    const int t0 = blockIdx.x * ch.per, t1 = min(t0 + ch.per, ch.tiles);
    const int rowoff = (lane & 15) * MD_LDN + (lane >> 4);
    for (int tile = t0; tile < t1; ++tile) {
        __syncthreads();     // the previous tile is consumed (and the zero fill is done)
        {
            const int e = tile * MD_NODES + lane;
            float araw = 0.f, xraw = 0.f;
            if (e < nodes) {
                araw = w ? w[e] : 1.f;
                xraw = phi[e];
            }
            double u = 0.0, v = 0.0, sw = 0.0, val = 0.0;
            if (e < nodes) {
                md_coords(g, e, u, v);
                float x;
                const float a = md_weight<BASIS>(araw, xraw, u, v, x);
                sw = sqrt((double)a);
                val = (double)x;
            }
            // a weight-0 node stores zeros whatever its modes evaluate to (far outside the disc they may overflow)
            if (wave == 0) S[g.J * MD_LDN + lane] = sw > 0.0 ? sw * val : 0.0;
            md_modes<BASIS>(table, g, u, v, 3, wave, [&](int col, double m) { S[col * MD_LDN + lane] = sw > 0.0 ? sw * m : 0.0; });
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < MD_NODES / 4; ++s) {
#pragma unroll
            for (int q = 0; q < MD_SLOTS; ++q)
                if (wave + 4 * q < npairs) {
                    const double a = S[16 * ta[q] * MD_LDN + rowoff + 4 * s];
                    const double b = S[16 * tb[q] * MD_LDN + rowoff + 4 * s];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
                }
        }
    }
    // partials[map][chunk][pair][reg][lane]: element (row 16 ta + (lane >> 4) + 4 reg, column 16 tb + (lane & 15))
    double* __restrict__ out = partials + ((size_t)blockIdx.y * ch.chunks + blockIdx.x) * ((size_t)npairs * 256);
#pragma unroll
    for (int q = 0; q < MD_SLOTS; ++q)
        if (wave + 4 * q < npairs)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(wave + 4 * q) * 256 + 64 * r + lane] = acc[q][r];
}

__global__ void __launch_bounds__(MD_FIN_THREADS) k_modal_finish(const double* __restrict__ partials, int ny, int nx, int J,
                                                                 double* __restrict__ coeff, unsigned char* __restrict__ kept) {
    __shared__ double G[(MD_MAX_MODES + 1) * MD_GL];
    __shared__ double red[4][256];
    __shared__ double diag[MD_MAX_MODES], tmp[MD_MAX_MODES + 1], y[MD_MAX_MODES], x[MD_MAX_MODES];
    __shared__ int keep[MD_MAX_MODES];
    const int tid = threadIdx.x;
    const MdChunks ch = md_chunks(ny, nx);
    const int T = md_tiles(J), npairs = md_pairs(J);
    const size_t per = (size_t)npairs * 256;
    const double* __restrict__ p = partials + (size_t)blockIdx.x * ch.chunks * per;
    {   // four thread groups add a quarter of the chunks each, in chunk order, one accumulator per tile pair so that many
        // loads are in flight; the quarters are then added in order
        const int grp = tid >> 8, t = tid & 255;
        const int cq = (ch.chunks + 3) / 4, c0 = grp * cq, c1 = min(c0 + cq, ch.chunks);
        double a[MD_PAIRS];
#pragma unroll
        for (int q = 0; q < MD_PAIRS; ++q) a[q] = 0.0;
        for (int c = c0; c < c1; ++c)
#pragma unroll
            for (int q = 0; q < MD_PAIRS; ++q)
                if (q < npairs) a[q] += p[(size_t)c * per + 256 * q + t];
#pragma unroll
        for (int q = 0; q < MD_PAIRS; ++q) {
            if (q >= npairs) continue;      // uniform
            red[grp][t] = a[q];
            __syncthreads();
            if (grp == 0) {
                const double s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
                int ta, tb;
                md_pair(q, T, ta, tb);
                const int r = t >> 6, l = t & 63;
                const int row = 16 * ta + (l >> 4) + 4 * r, col = 16 * tb + (l & 15);
                if (row <= col && col <= J) {
                    G[row * MD_GL + col] = s;
                    G[col * MD_GL + row] = s;
                }
            }
            __syncthreads();
        }
    }
    if (tid < J) diag[tid] = G[tid * MD_GL + tid];
    __syncthreads();
    // left-looking Cholesky of the augmented matrix in the lower triangle, modes in order; a dropped column is zero
    for (int b = 0; b < J; ++b) {
        const int a = tid;
        double s = 0.0;
        if (a >= b && a <= J) {
            s = G[a * MD_GL + b];
            for (int c = 0; c < b; ++c) s -= G[a * MD_GL + c] * G[b * MD_GL + c];
            tmp[a] = s;
        }
        __syncthreads();
        const double d = tmp[b];
        const bool k = d > 1e-12 * diag[b] && diag[b] > 0.0;
        if (a >= b && a <= J) {
            const double root = sqrt(d);
            G[a * MD_GL + b] = k ? (a == b ? root : s / root) : 0.0;
        }
        if (a == b) keep[b] = k;
        __syncthreads();
    }
    if (tid < J) y[tid] = G[J * MD_GL + tid];
    __syncthreads();
    for (int a = J - 1; a >= 0; --a) {
        if (tid == 0) x[a] = keep[a] ? y[a] / G[a * MD_GL + a] : 0.0;
        __syncthreads();
        if (tid < a) y[tid] -= G[a * MD_GL + tid] * x[a];
        __syncthreads();
    }
    if (tid < J) {
        coeff[(size_t)blockIdx.x * J + tid] = x[tid];
        kept[(size_t)blockIdx.x * J + tid] = keep[tid] ? 1 : 0;
    }
}

// out = scale (phi - sum_j c_j mode_j) over the modes flagged in `remove` (all when null), or the synthesis sum_j c_j mode_j
// when there is no map; valid (may be null) = 1 at the nodes of positive weight, the one place where that rule is decided for
// the caller; sums[map][block] = (sum w, sum w r, sum w r^2) over the nodes of positive weight, r the stored float32
template <int BASIS>
__global__ void __launch_bounds__(MD_THREADS) k_modal_apply(const float* maps, const float* __restrict__ weights, long long w_stride,
                                                            const MdTable* __restrict__ table, MdGeom g,
                                                            const double* __restrict__ coeff, const unsigned char* __restrict__ remove,
                                                            double scale, int nan_invalid, float* out, double* __restrict__ sums,
                                                            unsigned char* __restrict__ valid) {
    __shared__ double c[MD_MAX_MODES];
    __shared__ double sh[MD_THREADS / 64][3];
    const int tid = threadIdx.x;
    const int nodes = g.ny * g.nx;
    const float* phi = maps ? maps + (size_t)blockIdx.y * nodes : nullptr;
    const float* __restrict__ w = weights ? weights + (long long)blockIdx.y * w_stride : nullptr;
    float* q = out + (size_t)blockIdx.y * nodes;
    if (tid < g.J) c[tid] = (!remove || remove[tid]) ? coeff[(size_t)blockIdx.y * g.J + tid] : 0.0;
    __syncthreads();
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = blockIdx.x * MD_THREADS + tid; e < nodes; e += gridDim.x * MD_THREADS) {
        double u, v;
        md_coords(g, e, u, v);
        float val = 0.f, wf = 1.f;
        if (phi) {
            wf = md_weight<BASIS>(w ? w[e] : 1.f, phi[e], u, v, val);
            if (valid) valid[(size_t)blockIdx.y * nodes + e] = wf > 0.f ? 1 : 0;
            if (!(wf > 0.f)) {
                if (nan_invalid) {
                    q[e] = __builtin_nanf("");
                    continue;
                }
                val = phi[e];
            }
        }
        double fit = 0.0;
        md_modes<BASIS>(table, g, u, v, 0, 0, [&](int col, double m) { fit += c[col] * m; });
        const float r = phi ? (float)(scale * ((double)val - fit)) : (float)fit;
        q[e] = r;
        if (phi && wf > 0.f) {
            s[0] += (double)wf;
            s[1] += (double)wf * (double)r;
            s[2] += (double)wf * (double)r * (double)r;
        }
    }
    if (!sums) return;
    const double t = block_sum_columns(s, &sh[0][0], MD_THREADS / 64);
    if (tid < 3) sums[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + tid] = t;
}

// rms = sqrt(sum w r^2 / sum w - (sum w r / sum w)^2), NaN without a valid node; one thread per map adds the blocks in order
__global__ void k_modal_rms(const double* __restrict__ sums, int n, int blocks, double* __restrict__ rms) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < blocks; ++b)
        for (int k = 0; k < 3; ++k) s[k] += sums[((size_t)m * blocks + b) * 3 + k];
    const double mean = s[0] > 0.0 ? s[1] / s[0] : 0.0;
    rms[m] = s[0] > 0.0 ? sqrt(fmax(0.0, s[2] / s[0] - mean * mean)) : __builtin_nan("");
}

static int md_check(int n, int ny, int nx, int basis, int n_modes, double cy, double cx, double sy, double sx) {
    if (n < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "map count and sides must be >= 1");
    if (ny > MD_MAX_SIDE || nx > MD_MAX_SIDE)
        return fail(B4D_ESIZE, "wavefront grids are limited to " + std::to_string(MD_MAX_SIDE) + " nodes per side, got (" +
                                   std::to_string(ny) + ", " + std::to_string(nx) + ")");
    if (n > 65535) return fail(B4D_ESIZE, "at most 65535 maps per call");
    if (basis != 0 && basis != 1) return fail(B4D_EINVAL, "basis is 0 (Zernike) or 1 (Legendre)");
    if (n_modes < 1) return fail(B4D_EINVAL, "n_modes must be >= 1");
    if (n_modes > MD_MAX_MODES) return fail(B4D_ESIZE, "at most " + std::to_string(MD_MAX_MODES) + " modes");
    if (!(std::isfinite(cy) && std::isfinite(cx) && std::isfinite(sy) && std::isfinite(sx)))
        return fail(B4D_EINVAL, "centre and coordinate scales must be finite");
    return B4D_OK;
}

// workspace: Gram partials [n][chunks][pairs][256] float64, then the rms partials [n][blocks][3] float64
static size_t md_gram_bytes(int n, int ny, int nx, int J) {
    return (size_t)n * md_chunks(ny, nx).chunks * md_pairs(J) * 256 * sizeof(double);
}

}  // namespace b4d

using namespace b4d;

extern "C" size_t b4d_modal_workspace_bytes(int n, int ny, int nx, int n_modes) {
    if (n < 1 || n > 65535 || ny < 1 || nx < 1 || ny > MD_MAX_SIDE || nx > MD_MAX_SIDE || n_modes < 1 || n_modes > MD_MAX_MODES)
        return 0;
    return md_gram_bytes(n, ny, nx, n_modes) + (size_t)n * md_chunks(ny, nx).blocks * 3 * sizeof(double);
}

extern "C" int b4d_modal_fit(const float* maps, const float* weights, long long weight_stride, int n, int ny, int nx, int basis,
                             int n_modes, double cy, double cx, double sy, double sx, void* workspace, double* coeff,
                             unsigned char* kept, void* stream) {
    if (!maps || !workspace || !coeff || !kept) return fail(B4D_EINVAL, "null argument");
    if (const int rc = md_check(n, ny, nx, basis, n_modes, cy, cx, sy, sx)) return rc;
    if (weight_stride != 0 && weight_stride != (long long)ny * nx)
        return fail(B4D_EINVAL, "weight_stride is 0 (shared weights) or ny * nx (per map)");
    hipStream_t st = (hipStream_t)stream;
    MdGeom g;
    md_geom(basis, ny, nx, n_modes, cy, cx, sy, sx, g);
    const MdTable* t = nullptr;
    {
        std::lock_guard<std::mutex> lk(md_mutex());
        if (const int rc = md_table(basis, &t)) return rc;
    }
    const MdChunks ch = md_chunks(ny, nx);
    const dim3 grid(ch.chunks, n), block(MD_THREADS);
    double* part = (double*)workspace;
    if (basis == 0)
        hipLaunchKernelGGL(k_modal_gram<0>, grid, block, 0, st, maps, weights, weight_stride, t, g, part);
    else
        hipLaunchKernelGGL(k_modal_gram<1>, grid, block, 0, st, maps, weights, weight_stride, t, g, part);
    hipLaunchKernelGGL(k_modal_finish, dim3(n), dim3(MD_FIN_THREADS), 0, st, (const double*)part, ny, nx, n_modes, coeff, kept);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_modal_residual(const float* maps, const float* weights, long long weight_stride, int n, int ny, int nx, int basis,
                                  int n_modes, double cy, double cx, double sy, double sx, const double* coeff,
                                  const unsigned char* remove, double scale, int nan_invalid, void* workspace, float* out, double* rms,
                                  unsigned char* valid, void* stream) {
    if (!maps || !workspace || !coeff || !out || !rms) return fail(B4D_EINVAL, "null argument");
    if (const int rc = md_check(n, ny, nx, basis, n_modes, cy, cx, sy, sx)) return rc;
    if (weight_stride != 0 && weight_stride != (long long)ny * nx)
        return fail(B4D_EINVAL, "weight_stride is 0 (shared weights) or ny * nx (per map)");
    if (!std::isfinite(scale)) return fail(B4D_EINVAL, "scale must be finite");
    hipStream_t st = (hipStream_t)stream;
    MdGeom g;
    md_geom(basis, ny, nx, n_modes, cy, cx, sy, sx, g);
    const MdTable* t = nullptr;
    {
        std::lock_guard<std::mutex> lk(md_mutex());
        if (const int rc = md_table(basis, &t)) return rc;
    }
    const MdChunks ch = md_chunks(ny, nx);
    double* sums = (double*)((char*)workspace + md_gram_bytes(n, ny, nx, n_modes));
    const dim3 grid(ch.blocks, n), block(MD_THREADS);
    if (basis == 0)
        hipLaunchKernelGGL(k_modal_apply<0>, grid, block, 0, st, maps, weights, weight_stride, t, g, coeff, remove, scale, nan_invalid,
                           out, sums, valid);
    else
        hipLaunchKernelGGL(k_modal_apply<1>, grid, block, 0, st, maps, weights, weight_stride, t, g, coeff, remove, scale, nan_invalid,
                           out, sums, valid);
    hipLaunchKernelGGL(k_modal_rms, dim3((n + 255) / 256), dim3(256), 0, st, (const double*)sums, n, ch.blocks, rms);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

extern "C" int b4d_modal_eval(const double* coeff, int n, int ny, int nx, int basis, int n_modes, double cy, double cx, double sy,
                              double sx, float* out, void* stream) {
    if (!coeff || !out) return fail(B4D_EINVAL, "null argument");
    if (const int rc = md_check(n, ny, nx, basis, n_modes, cy, cx, sy, sx)) return rc;
    hipStream_t st = (hipStream_t)stream;
    MdGeom g;
    md_geom(basis, ny, nx, n_modes, cy, cx, sy, sx, g);
    const MdTable* t = nullptr;
    {
        std::lock_guard<std::mutex> lk(md_mutex());
        if (const int rc = md_table(basis, &t)) return rc;
    }
    const dim3 grid(md_chunks(ny, nx).blocks, n), block(MD_THREADS);
    if (basis == 0)
        hipLaunchKernelGGL(k_modal_apply<0>, grid, block, 0, st, (const float*)nullptr, (const float*)nullptr, 0LL, t, g, coeff,
                           (const unsigned char*)nullptr, 1.0, 0, out, (double*)nullptr,
                           (unsigned char*)nullptr);
    else
        hipLaunchKernelGGL(k_modal_apply<1>, grid, block, 0, st, (const float*)nullptr, (const float*)nullptr, 0LL, t, g, coeff,
                           (const unsigned char*)nullptr, 1.0, 0, out, (double*)nullptr,
                           (unsigned char*)nullptr);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
