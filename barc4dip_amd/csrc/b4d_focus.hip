// b4d_focus.hip -- focal-spot and caustic prediction from measured wavefront maps (b4d_focal_spot).
//
// One figure-error map fans out into nz planes of a zero-padded canvas (Py, Px) of a general-length plan.  Per chunk of (map, plane)
// pairs:
//   k_focus_pupil   writes the WHOLE complex canvas (zeros included: no memset pass) straight into the plan's input buffer, 16 bytes
//                   per lane.  The phase of a node is evaluated in float64, in turns, from the integer node indices, reduced to
//                   [-1/2, 1/2] and handed to sincospi.
//   general_dft2    the plan's 2-D complex DFT in natural order (no shift pass).
//   k_focus_spot    reads the natural-order spectrum ONCE: |F|^2 / (sum A)^2 with the fftshift in its index arithmetic; optional
//                   float32 crop around the DC bin; per band of 32 spectrum rows the float64 row sums, q-weighted row sums, column
//                   partial sums and the band's peak.
//   k_focus_fin     adds the band partials in a fixed order: the two marginals, the moments (all from the marginals but sum I p q,
//                   from the q-weighted row sums) and the peak with its first index in shifted row-major order; two workgroups
//                   per pair, one for the columns and one for the rows.
// No float atomics; every sum has one order that depends on (Py, Px) alone, so results are the same bits from run to run and for
// any chunking of the (map, plane) batch.
#define B4D_UNIT_PASSES 0   // this unit launches none of the power-of-two passes
#include "b4d_fft2d.hpp"

#include <climits>

namespace b4d {

constexpr int FOCUS_BAND = 32;   // spectrum rows per workgroup of k_focus_spot
constexpr int FOCUS_PRM = 8;     // doubles per (map, plane) pair: phase polynomial in turns, 1 / lambda, 1 / (sum A)^2
constexpr int FOCUS_ZPACK = 64;  // plane positions per upload launch (they travel as kernel arguments: no host buffer outlives the call)

struct FocusZPack {
    double z[FOCUS_ZPACK];
};

__global__ void __launch_bounds__(64) k_focus_put(FocusZPack p, int count, double* __restrict__ dst) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < FOCUS_ZPACK; ++i)   // static indices: the argument block stays in scalar registers
        if ((int)threadIdx.x == i) v = p.z[i];
    if ((int)threadIdx.x < count) dst[threadIdx.x] = v;
}

__device__ __forceinline__ bool focus_valid(float e, float a) { return isfinite(e) && isfinite(a) && a > 0.f; }

// fixed-order sum over the 256 lanes of a workgroup; the result is valid in lane 0
// (not block_sum of b4d_reduce.hpp: an LDS tree over all 256 lanes, another order of additions)
__device__ __forceinline__ double focus_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// per-map sum A and sum A^2 over the valid nodes, float64.  grid (n), block 256
__global__ void __launch_bounds__(256) k_focus_sums(const float* __restrict__ err, const float* __restrict__ amp, long long amp_stride,
                                                    int npix, double* __restrict__ asum) {
    __shared__ double sh[256];
    const size_t t = blockIdx.x;
    const float* e = err + t * (size_t)npix;
    const float* a = amp ? amp + t * amp_stride : nullptr;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < npix; i += 256) {
        const float ev = e[i], av = a ? a[i] : 1.f;
        if (focus_valid(ev, av)) {
            s1 += (double)av;
            s2 += (double)av * (double)av;
        }
    }
    s1 = focus_block_sum(s1, sh);
    s2 = focus_block_sum(s2, sh);
    if (threadIdx.x == 0) {
        asum[2 * t] = s1;
        asum[2 * t + 1] = s2;
    }
}

// phase / (2 pi) = e / lambda + k0 + u (ku + kuu u + kuv v) + v (kv + kvv v); the chirp 1 / (2 lambda z) joins the u^2 and v^2 terms
__global__ void __launch_bounds__(256) k_focus_prm(const double* __restrict__ coeff, const double* __restrict__ z,
                                                   const double* __restrict__ asum, int npairs, int nz, double wavelength,
                                                   double* __restrict__ prm) {
    const int gp = blockIdx.x * 256 + threadIdx.x;
    if (gp >= npairs) return;
    const int t = gp / nz, k = gp - t * nz;
    const double* c = coeff + 6 * (size_t)t;
    const double il = 1.0 / wavelength, hz = 1.0 / (2.0 * wavelength * z[k]), sa = asum[2 * t];
    double* p = prm + (size_t)gp * FOCUS_PRM;
    p[0] = c[0] * il;
    p[1] = c[1] * il;
    p[2] = c[2] * il;
    p[3] = c[3] * il + hz;
    p[4] = c[4] * il;
    p[5] = c[5] * il + hz;
    p[6] = il;
    p[7] = sa > 0.0 ? 1.0 / (sa * sa) : __longlong_as_double(0x7ff8000000000000LL);
}

struct PupilArgs {
    const float* err;
    const float* amp;
    long long amp_stride;
    const double* prm;
    float2* out;   // (pairs of the chunk, Py, Px)
    int ny, nx, Py, Px, nz, p0, lsh;
    double hy, hx;
};

__device__ __forceinline__ float2 focus_node(const PupilArgs& a, const float* e, const float* am, const double* p, int i, int j, double v,
                                             double vterm) {
    const size_t o = (size_t)i * a.nx + j;
    const float ev = e[o], av = am ? am[o] : 1.f;
    if (!focus_valid(ev, av)) return make_float2(0.f, 0.f);
    const double u = ((double)j - 0.5 * (double)(a.nx - 1)) * a.hx;
    double s = (double)ev * p[6] + p[0] + u * (p[1] + p[3] * u + p[4] * v) + vterm;
    s -= rint(s);
    double sn, cs;
    sincospi(2.0 * s, &sn, &cs);
    return make_float2(av * (float)cs, av * (float)sn);
}

// grid (ceil(Py / rows per workgroup), pairs), block 256 = (256 >> lsh) rows x (1 << lsh) lanes of two complex words
__global__ void __launch_bounds__(256) k_focus_pupil(PupilArgs a) {
    const int lx = 1 << a.lsh, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> a.lsh;
    const int row = blockIdx.x * (256 >> a.lsh) + ty;
    if (row >= a.Py) return;
    const int gp = a.p0 + blockIdx.y, t = gp / a.nz;
    const double* p = a.prm + (size_t)gp * FOCUS_PRM;
    const float* e = a.err + (size_t)t * a.ny * a.nx;
    const float* am = a.amp ? a.amp + (size_t)t * a.amp_stride : nullptr;
    float2* orow = a.out + ((size_t)blockIdx.y * a.Py + row) * a.Px;
    const bool inrow = row < a.ny, even = (a.Px & 1) == 0;
    const double v = ((double)row - 0.5 * (double)(a.ny - 1)) * a.hy;
    const double vterm = v * (p[2] + p[5] * v);
    for (int c = 2 * tx; c < a.Px; c += 2 * lx) {
        float2 w0 = make_float2(0.f, 0.f), w1 = w0;
        if (inrow && c < a.nx) {
            w0 = focus_node(a, e, am, p, row, c, v, vterm);
            if (c + 1 < a.nx) w1 = focus_node(a, e, am, p, row, c + 1, v, vterm);
        }
        if (even) {
            *reinterpret_cast<float4*>(orow + c) = make_float4(w0.x, w0.y, w1.x, w1.y);
        } else {
            orow[c] = w0;
            if (c + 1 < a.Px) orow[c + 1] = w1;
        }
    }
}

struct SpotArgs {
    const float2* F;      // natural-order spectra of the chunk
    const double* prm;
    float* inten;         // null or (all pairs, cy, cx)
    double* rowsum;       // (chunk, Py)
    double* rowq;         // (chunk, Py)
    double* colpart;      // (chunk, nbands, Px)
    double* peakv;        // (chunk, nbands)
    int* peaki;
    int Py, Px, p0, cy, cx, nbands;
};

// grid (nbands, pairs), block 256 = (256 >> LSH) rows x (1 << LSH) lanes; a lane owns the column pairs 2 (tx + m lx), m < NM.
// The lane split is a template argument so that the row loop has a compile-time trip count: it is unrolled four rows deep, because
// the row reduction is a chain of six dependent cross-lane steps that would otherwise bound the loop.
template <int LSH, int NM>
__global__ void __launch_bounds__(256) k_focus_spot(SpotArgs a) {
    static_assert(LSH >= 3 && LSH <= 8 && (LSH == 8 || NM == 1), "lanes along x: 8 .. 256; several column pairs per lane only at 256");
    __shared__ double rpart[FOCUS_BAND][4][2];
    __shared__ double cbuf[512];
    __shared__ double pv[4];
    __shared__ int pi[4];
    const int Py = a.Py, Px = a.Px;
    constexpr int lx = 1 << LSH, rpp = 256 >> LSH;
    const int tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> LSH;
    const int pair = blockIdx.y, gp = a.p0 + pair, r0 = blockIdx.x * FOCUS_BAND;
    const int hx2 = (Px + 1) / 2, hy2 = (Py + 1) / 2;
    const bool even = (Px & 1) == 0;
    const double inv = a.prm[(size_t)gp * FOCUS_PRM + 7];
    const float2* F = a.F + (size_t)pair * Py * Px;
    float* crop = a.inten ? a.inten + (size_t)gp * a.cy * a.cx : nullptr;
    double cs[NM][2];
#pragma unroll
    for (int m = 0; m < NM; ++m) cs[m][0] = cs[m][1] = 0.0;
    double bv = -1.0;
    int bi = INT_MAX;
    constexpr int gw = lx < 64 ? lx : 64;   // lanes of one wave that share a row
    constexpr int trips = FOCUS_BAND / rpp;
#pragma unroll 4
    for (int it = 0; it < trips; ++it) {
        const int rr = ty + it * rpp;
        const int r = r0 + rr;
        const int p = r < hy2 ? r : r - Py, sr = p + Py / 2;
        const int yy = p + a.cy / 2;
        const bool rowcrop = crop && yy >= 0 && yy < a.cy;
        double rs = 0.0, rq = 0.0;
        if (r < Py) {
            const float2* Fr = F + (size_t)r * Px;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const int c = 2 * (tx + lx * m);
                if (c >= Px) continue;
                const bool two = c + 1 < Px;
                float2 f0, f1 = make_float2(0.f, 0.f);
                if (even) {
                    const float4 q4 = *reinterpret_cast<const float4*>(Fr + c);
                    f0 = make_float2(q4.x, q4.y);
                    f1 = make_float2(q4.z, q4.w);
                } else {
                    f0 = Fr[c];
                    if (two) f1 = Fr[c + 1];
                }
                const int q0 = c < hx2 ? c : c - Px, q1 = c + 1 < hx2 ? c + 1 : c + 1 - Px;
                const double i0 = ((double)f0.x * (double)f0.x + (double)f0.y * (double)f0.y) * inv;
                const double i1 = two ? ((double)f1.x * (double)f1.x + (double)f1.y * (double)f1.y) * inv : 0.0;
                cs[m][0] += i0;
                cs[m][1] += i1;
                rs += i0;
                rs += i1;
                rq = fma(i0, (double)q0, rq);
                rq = fma(i1, (double)q1, rq);
                argmax_merge(bv, bi, i0, sr * Px + q0 + Px / 2);
                if (two) argmax_merge(bv, bi, i1, sr * Px + q1 + Px / 2);
                if (rowcrop) {
                    const int x0 = q0 + a.cx / 2, x1 = q1 + a.cx / 2;
                    if (x0 >= 0 && x0 < a.cx) crop[(size_t)yy * a.cx + x0] = (float)i0;
                    if (two && x1 >= 0 && x1 < a.cx) crop[(size_t)yy * a.cx + x1] = (float)i1;
                }
            }
        }
        // (not wave_sum_all of b4d_reduce.hpp: groups of gw <= 64 lanes, one row each)
#pragma unroll
        for (int o = gw >> 1; o > 0; o >>= 1) {
            rs += __shfl_xor(rs, o, 64);
            rq += __shfl_xor(rq, o, 64);
        }
        if ((tx & (gw - 1)) == 0) {
            rpart[rr][tx >> 6][0] = rs;
            rpart[rr][tx >> 6][1] = rq;
        }
    }
    // column partial sums of the band
    double* cp = a.colpart + ((size_t)pair * a.nbands + blockIdx.x) * Px;
    if (rpp == 1) {
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int c = 2 * (tx + lx * m);
            if (c < Px) cp[c] = cs[m][0];
            if (c + 1 < Px) cp[c + 1] = cs[m][1];
        }
    } else {   // several rows ride side by side in the workgroup (NM == 1): add them in row order
        cbuf[ty * 2 * lx + 2 * tx] = cs[0][0];
        cbuf[ty * 2 * lx + 2 * tx + 1] = cs[0][1];
    }
    wave_argmax_all(bv, bi);
    if ((threadIdx.x & 63) == 0) {
        pv[threadIdx.x >> 6] = bv;
        pi[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (rpp > 1 && (int)threadIdx.x < 2 * lx && (int)threadIdx.x < Px) {
        double s = 0.0;
        for (int y = 0; y < rpp; ++y) s += cbuf[y * 2 * lx + threadIdx.x];
        cp[threadIdx.x] = s;
    }
    if ((int)threadIdx.x < FOCUS_BAND && r0 + (int)threadIdx.x < Py) {
        const int ns = lx > 64 ? lx >> 6 : 1;
        double s = 0.0, q = 0.0;
        for (int w = 0; w < ns; ++w) {
            s += rpart[threadIdx.x][w][0];
            q += rpart[threadIdx.x][w][1];
        }
        a.rowsum[(size_t)pair * Py + r0 + threadIdx.x] = s;
        a.rowq[(size_t)pair * Py + r0 + threadIdx.x] = q;
    }
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) argmax_merge(bv, bi, pv[w], pi[w]);
        a.peakv[(size_t)pair * a.nbands + blockIdx.x] = bv;
        a.peaki[(size_t)pair * a.nbands + blockIdx.x] = bi;
    }
}

struct FinArgs {
    const double* rowsum;
    const double* rowq;
    const double* colpart;
    const double* peakv;
    const int* peaki;
    const double* asum;
    double* stats;    // (all pairs, 10)
    double* marg_x;   // null or (all pairs, Px)
    double* marg_y;   // null or (all pairs, Py)
    int Py, Px, p0, nz, nbands;
};

// grid (pairs, 2), block 256: workgroup 0 of a pair adds the column partials (marginal along x, total, q moments), workgroup 1
// takes the rows (marginal along y, p moments, sum I p q) and the peak; they write disjoint slots of the pair's statistics
__global__ void __launch_bounds__(256) k_focus_fin(FinArgs a) {
    __shared__ double sh[256];
    __shared__ double pv[4];
    __shared__ int pi[4];
    const int Py = a.Py, Px = a.Px, pair = blockIdx.x, gp = a.p0 + pair;
    const int hx2 = (Px + 1) / 2, hy2 = (Py + 1) / 2;
    double* s = a.stats + (size_t)gp * 10;
    if (blockIdx.y == 0) {
        double tot = 0.0, sq = 0.0, sqq = 0.0;
        for (int c = threadIdx.x; c < Px; c += 256) {
            const double* cp = a.colpart + (size_t)pair * a.nbands * Px + c;
            double v = 0.0;
#pragma unroll 8
            for (int b = 0; b < a.nbands; ++b) v += cp[(size_t)b * Px];
            const int q = c < hx2 ? c : c - Px;
            if (a.marg_x) a.marg_x[(size_t)gp * Px + q + Px / 2] = v;
            tot += v;
            sq = fma(v, (double)q, sq);
            sqq = fma(v, (double)q * (double)q, sqq);
        }
        tot = focus_block_sum(tot, sh);
        sq = focus_block_sum(sq, sh);
        sqq = focus_block_sum(sqq, sh);
        if (threadIdx.x == 0) {
            s[0] = tot;
            s[4] = sq;
            s[6] = sqq;
            s[8] = a.asum[2 * (gp / a.nz)];
            s[9] = a.asum[2 * (gp / a.nz) + 1];
        }
        return;
    }
    double sp = 0.0, spp = 0.0, spq = 0.0;
    for (int r = threadIdx.x; r < Py; r += 256) {
        const double v = a.rowsum[(size_t)pair * Py + r], vq = a.rowq[(size_t)pair * Py + r];
        const int p = r < hy2 ? r : r - Py;
        if (a.marg_y) a.marg_y[(size_t)gp * Py + p + Py / 2] = v;
        sp = fma(v, (double)p, sp);
        spp = fma(v, (double)p * (double)p, spp);
        spq = fma(vq, (double)p, spq);
    }
    double bv = -1.0;
    int bi = INT_MAX;
    for (int b = threadIdx.x; b < a.nbands; b += 256) argmax_merge(bv, bi, a.peakv[(size_t)pair * a.nbands + b], a.peaki[(size_t)pair * a.nbands + b]);
    wave_argmax_all(bv, bi);
    if ((threadIdx.x & 63) == 0) {
        pv[threadIdx.x >> 6] = bv;
        pi[threadIdx.x >> 6] = bi;
    }
    sp = focus_block_sum(sp, sh);
    spp = focus_block_sum(spp, sh);
    spq = focus_block_sum(spq, sh);
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) argmax_merge(bv, bi, pv[w], pi[w]);
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const bool found = bi != INT_MAX;
        s[1] = found ? bv : nan;
        s[2] = found ? (double)bi : nan;
        s[3] = sp;
        s[5] = spp;
        s[7] = spq;
    }
}

// workspace layout (byte offsets, 256-byte aligned parts)
struct FocusWs {
    size_t z, asum, prm, rowsum, rowq, colpart, peakv, peaki, total;
    int nbands;
};
static FocusWs focus_layout(const b4d_plan* pl, int n, int nz) {
    FocusWs w{};
    const size_t Py = pl->ny, Px = pl->nx, ch = pl->chunk;
    w.nbands = (int)((Py + FOCUS_BAND - 1) / FOCUS_BAND);
    size_t o = 0;
    w.z = o, o += align256(sizeof(double) * (size_t)nz);
    w.asum = o, o += align256(sizeof(double) * 2 * (size_t)n);
    w.prm = o, o += align256(sizeof(double) * FOCUS_PRM * (size_t)n * nz);
    w.rowsum = o, o += align256(sizeof(double) * ch * Py);
    w.rowq = o, o += align256(sizeof(double) * ch * Py);
    w.colpart = o, o += align256(sizeof(double) * ch * w.nbands * Px);
    w.peakv = o, o += align256(sizeof(double) * ch * w.nbands);
    w.peaki = o, o += align256(sizeof(int) * ch * w.nbands);
    w.total = o;
    return w;
}

}  // namespace b4d

extern "C" {

size_t b4d_focal_spot_workspace_bytes(const b4d_plan* pl, int n, int nz) {
    if (!pl || !pl->general || n < 1 || nz < 1 || (long long)n * nz > INT_MAX / 16 || pl->ny > 4096 || pl->nx > 4096) return 0;
    return focus_layout(pl, n, nz).total;
}

int b4d_focal_spot(b4d_plan* pl, const float* err, const float* amp, long long amp_stride, int n, int ny, int nx, const double* coeff,
                   double hy, double hx, double wavelength, const double* z, int nz, int cy, int cx, float* intensity, double* stats,
                   double* marg_x, double* marg_y, void* workspace, void* stream) {
    if (!pl) return fail(B4D_EINVAL, "focal_spot: plan is null");
    B4D_PLAN_LOCK(pl);
    if (!pl->general) return fail(B4D_EINVAL, "focal_spot needs a plan from b4d_plan_create_general");
    const int Py = pl->ny, Px = pl->nx;
    if (Py > 4096 || Px > 4096) return fail(B4D_ESIZE, "focal_spot: canvases are limited to 4096 per side");
    if (!err || !coeff || !z || !stats || !workspace) return fail(B4D_EINVAL, "focal_spot: null err, coeff, z, stats or workspace");
    if (n < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "focal_spot: n, ny, nx must be >= 1");
    if (nz < 1) return fail(B4D_EINVAL, "focal_spot: nz must be >= 1");
    if ((long long)n * nz > INT_MAX / 16) return fail(B4D_EINVAL, "focal_spot: too many (map, plane) pairs");
    if (ny > Py || nx > Px)
        return fail(B4D_EINVAL, "focal_spot: the map (" + std::to_string(ny) + ", " + std::to_string(nx) + ") does not fit the canvas (" +
                                    std::to_string(Py) + ", " + std::to_string(Px) + ")");
    if (amp && amp_stride != 0 && amp_stride < (long long)ny * nx) return fail(B4D_EINVAL, "focal_spot: amp_stride must be 0 or >= ny * nx");
    if (intensity && (cy < 1 || cx < 1 || cy > Py || cx > Px)) return fail(B4D_EINVAL, "focal_spot: the crop must lie within the canvas");
    if (!(std::isfinite(hy) && std::isfinite(hx) && hy > 0.0 && hx > 0.0)) return fail(B4D_EINVAL, "focal_spot: spacings must be finite and > 0");
    if (!(std::isfinite(wavelength) && wavelength > 0.0)) return fail(B4D_EINVAL, "focal_spot: wavelength must be finite and > 0");
    for (int k = 0; k < nz; ++k)
        if (!std::isfinite(z[k]) || z[k] == 0.0) return fail(B4D_EINVAL, "focal_spot: plane positions must be finite and non-zero");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FocusWs w = focus_layout(pl, n, nz);
    char* ws = static_cast<char*>(workspace);
    double* zd = reinterpret_cast<double*>(ws + w.z);
    double* asum = reinterpret_cast<double*>(ws + w.asum);
    double* prm = reinterpret_cast<double*>(ws + w.prm);
    const int npairs = n * nz;

    for (int k0 = 0; k0 < nz; k0 += FOCUS_ZPACK) {
        FocusZPack pk{};
        const int cnt = std::min(FOCUS_ZPACK, nz - k0);
        for (int i = 0; i < cnt; ++i) pk.z[i] = z[k0 + i];
        hipLaunchKernelGGL(k_focus_put, dim3(1), dim3(64), 0, st, pk, cnt, zd + k0);
    }
    hipLaunchKernelGGL(k_focus_sums, dim3(n), dim3(256), 0, st, err, amp, amp ? amp_stride : 0LL, ny * nx, asum);
    hipLaunchKernelGGL(k_focus_prm, dim3((npairs + 255) / 256), dim3(256), 0, st, coeff, zd, asum, npairs, nz, wavelength, prm);
    B4D_HIP(hipGetLastError());

    // lanes along x: a power of two in [8, 256] covering Px / 2 column pairs (or 256 lanes walking NM pairs each)
    const int pairs_x = (Px + 1) / 2;
    int lsh = 3;
    while ((1 << lsh) < pairs_x && lsh < 8) ++lsh;
    const int lx = 1 << lsh, rpp = 256 >> lsh, nm = (pairs_x + lx - 1) / lx;

    for (int p0 = 0; p0 < npairs; p0 += pl->chunk) {
        const int nb = std::min(pl->chunk, npairs - p0);
        PupilArgs pa{err, amp, amp ? amp_stride : 0LL, prm, pl->gbuf3, ny, nx, Py, Px, nz, p0, lsh, hy, hx};
        hipLaunchKernelGGL(k_focus_pupil, dim3((Py + rpp - 1) / rpp, nb), dim3(256), 0, st, pa);
        B4D_HIP(hipGetLastError());
        int rc = general_dft2(pl, pl->gbuf3, false, nb, 0, pl->gbuf1, pl->gbuf2, st);
        if (rc) return rc;
        SpotArgs sa{pl->gbuf2, prm, intensity, reinterpret_cast<double*>(ws + w.rowsum), reinterpret_cast<double*>(ws + w.rowq),
                    reinterpret_cast<double*>(ws + w.colpart), reinterpret_cast<double*>(ws + w.peakv), reinterpret_cast<int*>(ws + w.peaki),
                    Py, Px, p0, cy, cx, w.nbands};
        const dim3 sg(w.nbands, nb);
#define B4D_SPOT(L, M) hipLaunchKernelGGL((k_focus_spot<L, M>), sg, dim3(256), 0, st, sa)
        switch (lsh) {
            case 3: B4D_SPOT(3, 1); break;
            case 4: B4D_SPOT(4, 1); break;
            case 5: B4D_SPOT(5, 1); break;
            case 6: B4D_SPOT(6, 1); break;
            case 7: B4D_SPOT(7, 1); break;
            default:
                if (nm <= 1) B4D_SPOT(8, 1);
                else if (nm <= 2) B4D_SPOT(8, 2);
                else if (nm <= 4) B4D_SPOT(8, 4);
                else B4D_SPOT(8, 8);
        }
#undef B4D_SPOT
        B4D_HIP(hipGetLastError());
        FinArgs fa{sa.rowsum, sa.rowq, sa.colpart, sa.peakv, sa.peaki, asum, stats, marg_x, marg_y, Py, Px, p0, nz, w.nbands};
        hipLaunchKernelGGL(k_focus_fin, dim3(nb, 2), dim3(256), 0, st, fa);
        B4D_HIP(hipGetLastError());
    }
    return B4D_OK;
}

}  // extern "C"
