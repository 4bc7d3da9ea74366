// b4d_scan.hip -- speckle scanning (speckle-vector tracking, "UMPA") at detector resolution: the same N diffuser positions
// recorded without and with the sample, compared at every pixel with a window of a few pixels and a local search
// (barc4dip_amd/signal/scanning.py; the definition is in include/b4d.h).
//
// Pixel p, shift u, weights w[n][j][i] = g[n] h_wy[j] h_wx[i] normalised to sum 1.  Every moment is a separable h_wy x h_wx
// filter of a plane that is summed over the positions n first:
//   Rm, VR        from  sum_n g (R_n - c)      and  sum_n g (R_n - c)^2       at p        (k_scan_moments, set 0)
//   Sm(u), VS(u)  from  sum_n g (S_n - c)      and  sum_n g (S_n - c)^2       at p + u    (k_scan_moments, set 1 + m)
//   C(u)          from  X_u[q] = sum_n g (R_n[q] - r0)(S_n[q + u] - s0)       at p        (k_scan_match)
// so a product R_n[q] S_n[q + u] is formed once and serves every window that covers q, and the u-independent sums are windowed
// once per frame (they land in the per-stream scratch buffer as mean and variance planes, which do not depend on the shift
// constant).  c, r0, s0 are one pixel of the workgroup's tile at the first weighted position: power sums of shifted values keep
// 1 % contrast on 30 000 counts from cancelling (b4d_speckle.hip).  A value that is not finite counts as 0 in every sum and
// turns the mean of each window that covers it into NaN, which is how k_scan_match learns of it: every pixel that the
// definition does not name keeps the bits it has with a 0 in that place.
//
// k_scan_match: one workgroup of 512 lanes per T x T output tile (T = 32 for windows up to 15, 16 beyond) and scan.  The halo
// tile (T + w - 1 per axis, at most 46 x 46) is spread over the lanes, at most SS_P pixels each.  For a block of SS_GS shifts a
// lane keeps SS_P x SS_GS float64 accumulators; per position the sample tile with the window + search halo is staged in LDS once
// and each lane reads its reference pixels from memory.  Then, shift by shift, the accumulated plane goes through LDS and the
// two filter passes in a fixed order, and each lane updates the running best of its output pixels.  A second sweep over the
// shifts that some pixel of the tile needs as an axis neighbour of its peak gives the values of the parabola step: the same
// instruction sequence per (pixel, shift), hence the same bits as in the first sweep.  No atomics; a scan gives the same bits
// alone and inside any batch.
#include <algorithm>
#include <cmath>
#include <string>

#include "b4d_common.hpp"

namespace b4d {

constexpr int SS_MAX_WIN = 31;
constexpr int SS_MAX_SEARCH = 16;
constexpr int SS_MAX_N = 4096;
constexpr int SS_THREADS = 512;
constexpr int SS_GS = 6;                                // shifts per register block (8 spills: 256 VGPRs at 512 lanes)
constexpr int SS_HALO = 46;                             // halo tile side: 32 + 15 - 1 = 16 + 31 - 1
constexpr int SS_P = 5;                                 // halo pixels per lane: 46 * 46 <= 5 * 512
constexpr int SS_NO = 2;                                // output pixels per lane: 32 * 32 / 512
constexpr int SS_SIDE = SS_HALO + 2 * SS_MAX_SEARCH;    // sample tile side
constexpr int SS_MAXK = (2 * SS_MAX_SEARCH + 1) * (2 * SS_MAX_SEARCH + 1);
constexpr int SM_T = 32;                                // k_scan_moments: centres per tile side
constexpr int SM_SIDE = SM_T + SS_MAX_WIN - 1;          // 62
constexpr int SM_THREADS = 256;
constexpr int SM_P = 16;                                // 62 * 62 <= 16 * 256
constexpr int SM_NO = 4;                                // 32 * 32 / 256
constexpr double SS_TINY = 1e-12;                       // a variance <= SS_TINY mean^2 has no contrast

struct ScanArgs {
    const float* ref;     // (N, H, W)
    const float* smp;     // (M, N, H, W)
    const double* g;      // (N,)
    double* mom;          // (1 + M, 2, H, W): mean and variance of the window centred on each pixel; set 0 is the reference
    double* out;          // (M, 6, H, W)
    int M, N, H, W;
    int wy, wx, sy, sx;
    int taper, subpixel;
    int T, tiles_x;
};

__device__ inline float ss_clean(float v) { return isfinite(v) ? v : 0.0f; }
__device__ inline int ss_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// filter taps of both axes, normalised to sum 1 (f[0..wy) and f[32..32 + wx)); sum of g and the first weighted position
__device__ inline void ss_setup(const ScanArgs& a, double* f, double& gsum, int& n0) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int ax = tid >> 5, k = tid & 31, w = ax ? a.wx : a.wy;
        if (k < w) {
            double s = 0.0, mine = 0.0;
            for (int j = 0; j < w; ++j) {
                const double h = a.taper ? 0.5 - 0.5 * cos(2.0 * M_PI * (j + 0.5) / w) : 1.0;
                s += h;
                if (j == k) mine = h;
            }
            f[ax * 32 + k] = mine / s;
        }
    }
    gsum = 0.0;
    n0 = -1;
    for (int n = 0; n < a.N; ++n) {
        const double gn = a.g[n];
        if (gn > 0.0) {
            gsum += gn;
            if (n0 < 0) n0 = n;
        }
    }
}

// out[o] = sum_j fy[j] sum_i fx[i] X[y + j][x + i] for the lane's pixels (y, x) = divmod(tid + THREADS o, T) of the T x T tile; X is
// (T + wy - 1) x HX.  Rows first, then columns, each in tap order.  Syncs before reading X; X may be rewritten on return, tmp
// only after the next barrier.
template <int NO, int THREADS>
__device__ inline void ss_filter(const double* X, double* tmp, const double* f, int HX, int T, int wy, int wx, double (&out)[NO]) {
    const int tid = threadIdx.x, HY = T + wy - 1;
    __syncthreads();
    for (int idx = tid; idx < HY * T; idx += THREADS) {
        const int y = idx / T, x = idx - y * T;
        const double* p = X + y * HX + x;
        double t = 0.0;
        for (int i = 0; i < wx; ++i) t = fma(f[32 + i], p[i], t);
        tmp[idx] = t;
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        const int id = tid + o * THREADS;
        double t = 0.0;
        if (id < T * T) {
            const double* p = tmp + id;
            for (int j = 0; j < wy; ++j) t = fma(f[j], p[j * T], t);
        }
        out[o] = t;
    }
}

// grid (tiles, 1 + M): mean and variance (NaN where a value is not finite) of the window centred on every pixel that has one
__global__ void __launch_bounds__(SM_THREADS) k_scan_moments(ScanArgs a) {
    __shared__ double X[SM_SIDE * SM_SIDE];
    __shared__ double tmp[SM_SIDE * SM_T];
    __shared__ double f[64];
    const int tid = threadIdx.x, T = SM_T;
    const int ty0 = (int)(blockIdx.x / a.tiles_x) * T, tx0 = (int)(blockIdx.x % a.tiles_x) * T;
    const int hy = a.wy / 2, hx = a.wx / 2;
    const int HY = T + a.wy - 1, HX = T + a.wx - 1, HP = HY * HX;
    const size_t fpix = (size_t)a.H * a.W;
    const float* F = blockIdx.y == 0 ? a.ref : a.smp + (size_t)(blockIdx.y - 1) * a.N * fpix;
    double gsum;
    int n0;
    ss_setup(a, f, gsum, n0);
    const bool usable = n0 >= 0 && isfinite(gsum);

    // the lane's pixels of the input tile; coordinates clamped into the frame (a clamped pixel feeds no window that is written)
    unsigned off[SM_P];
    const int np = (HP + SM_THREADS - 1) / SM_THREADS;
#pragma unroll
    for (int p = 0; p < SM_P; ++p) {
        const int q = min(tid + p * SM_THREADS, HP - 1);
        const int qy = q / HX, qx = q - qy * HX;
        off[p] = (unsigned)ss_clamp(ty0 - hy + qy, a.H - 1) * (unsigned)a.W + (unsigned)ss_clamp(tx0 - hx + qx, a.W - 1);
    }
    double s1[SM_P], s2[SM_P];
    unsigned badmask = 0;
#pragma unroll
    for (int p = 0; p < SM_P; ++p) s1[p] = s2[p] = 0.0;
    double c0 = 0.0;
    if (usable) {
        c0 = ss_clean(F[(size_t)n0 * fpix + (size_t)ss_clamp(ty0 - hy, a.H - 1) * a.W + ss_clamp(tx0 - hx, a.W - 1)]);
        for (int n = n0; n < a.N; ++n) {
            const double gn = a.g[n];
            if (!(gn > 0.0)) continue;   // a position of weight 0 is never read
            const double wn = gn / gsum;
            const float* Fn = F + (size_t)n * fpix;
#pragma unroll
            for (int p = 0; p < SM_P; ++p) {
                if (p < np) {
                    const float v = Fn[off[p]];
                    if (!isfinite(v)) badmask |= 1u << p;
                    const double d = (double)ss_clean(v) - c0;
                    s1[p] = fma(wn, d, s1[p]);
                    s2[p] = fma(wn * d, d, s2[p]);
                }
            }
        }
    }
    const int anybad = __syncthreads_or(badmask != 0);

    double m1[SM_NO], m2[SM_NO], mb[SM_NO];
#pragma unroll
    for (int p = 0; p < SM_P; ++p)
        if (tid + p * SM_THREADS < HP) X[tid + p * SM_THREADS] = s1[p];
    ss_filter<SM_NO, SM_THREADS>(X, tmp, f, HX, T, a.wy, a.wx, m1);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < SM_P; ++p)
        if (tid + p * SM_THREADS < HP) X[tid + p * SM_THREADS] = s2[p];
    ss_filter<SM_NO, SM_THREADS>(X, tmp, f, HX, T, a.wy, a.wx, m2);
#pragma unroll
    for (int o = 0; o < SM_NO; ++o) mb[o] = 0.0;
    if (anybad) {   // the taps are positive: the filtered indicator is above 0 exactly where a window covers a bad value
        __syncthreads();
#pragma unroll
        for (int p = 0; p < SM_P; ++p)
            if (tid + p * SM_THREADS < HP) X[tid + p * SM_THREADS] = (badmask >> p) & 1u ? 1.0 : 0.0;
        ss_filter<SM_NO, SM_THREADS>(X, tmp, f, HX, T, a.wy, a.wx, mb);
    }
    double* mean = a.mom + (size_t)blockIdx.y * 2 * fpix;
    double* var = mean + fpix;
#pragma unroll
    for (int o = 0; o < SM_NO; ++o) {
        const int id = tid + o * SM_THREADS;
        const int cy = ty0 + id / T, cx = tx0 + id % T;
        if (cy < hy || cy > a.H - 1 - hy || cx < hx || cx > a.W - 1 - hx) continue;
        const bool ok = usable && !(mb[o] > 0.0);
        mean[(size_t)cy * a.W + cx] = ok ? c0 + m1[o] : NAN;
        var[(size_t)cy * a.W + cx] = ok ? m2[o] - m1[o] * m1[o] : NAN;
    }
}

// one position's products of the lane's halo pixels with a block of shifts; FULL: all SS_GS shifts of the block are in use
template <bool FULL>
__device__ __forceinline__ void ss_products(double (&acc)[SS_P][SS_GS], const float* Rn, const unsigned (&roff)[SS_P], const float* Sl,
                                            const int (&qbase)[SS_P], const int (&koff)[SS_GS], int np, int kn, double wn, double r0,
                                            double s0) {
#pragma unroll
    for (int p = 0; p < SS_P; ++p) {
        if (p < np) {
            const double r = wn * ((double)ss_clean(Rn[roff[p]]) - r0);
            const float* sp = Sl + qbase[p];
#pragma unroll
            for (int k = 0; k < SS_GS; ++k)
                if (FULL || k < kn) acc[p][k] = fma(r, (double)sp[koff[k]] - s0, acc[p][k]);
        }
    }
}

// grid (tiles, M)
__global__ void __launch_bounds__(SS_THREADS) k_scan_match(ScanArgs a) {
    __shared__ float Sl[SS_SIDE * SS_SIDE];
    __shared__ double X[SS_HALO * SS_HALO];
    __shared__ double tmp[SS_HALO * 32];
    __shared__ double f[64];
    __shared__ unsigned short klist[SS_MAXK];
    __shared__ unsigned char need[SS_MAXK];
    __shared__ int nneed;
    const int tid = threadIdx.x, T = a.T, m = blockIdx.y;
    const int ty0 = (int)(blockIdx.x / a.tiles_x) * T, tx0 = (int)(blockIdx.x % a.tiles_x) * T;
    const int hy = a.wy / 2, hx = a.wx / 2, my = hy + a.sy, mx = hx + a.sx;
    const int HY = T + a.wy - 1, HX = T + a.wx - 1, HP = HY * HX;
    const int SH = HY + 2 * a.sy, SW = HX + 2 * a.sx;
    const int KX = 2 * a.sx + 1, K = (2 * a.sy + 1) * KX;
    const size_t fpix = (size_t)a.H * a.W;
    const float* S = a.smp + (size_t)m * a.N * fpix;
    const double* meanR = a.mom;
    const double* varR = a.mom + fpix;
    const double* meanS = a.mom + (size_t)(1 + m) * 2 * fpix;
    const double* varS = meanS + fpix;
    double* out = a.out + (size_t)m * 6 * fpix;

    // ---- the lane's output pixels
    bool live[SS_NO], bad[SS_NO];
    unsigned pix[SS_NO];
    double Rm[SS_NO], VR[SS_NO], best[SS_NO], bestC[SS_NO], bestS[SS_NO], nb[SS_NO][4];
    int bidx[SS_NO];
    bool anylive = false;
#pragma unroll
    for (int o = 0; o < SS_NO; ++o) {
        const int id = tid + o * SS_THREADS;
        const int py = ty0 + id / T, px = tx0 + id % T;
        const bool inframe = id < T * T && py < a.H && px < a.W;
        live[o] = inframe && py >= my && py < a.H - my && px >= mx && px < a.W - mx;
        pix[o] = inframe ? (unsigned)py * (unsigned)a.W + (unsigned)px : 0u;
        Rm[o] = live[o] ? meanR[pix[o]] : NAN;
        VR[o] = live[o] ? varR[pix[o]] : NAN;
        bad[o] = !(Rm[o] == Rm[o]);
        best[o] = -INFINITY;
        bestC[o] = bestS[o] = NAN;
        bidx[o] = -1;
        nb[o][0] = nb[o][1] = nb[o][2] = nb[o][3] = NAN;
        anylive |= live[o];
        if (inframe && !live[o]) {
            for (int pl = 0; pl < 5; ++pl) out[pl * fpix + pix[o]] = NAN;
            out[5 * fpix + pix[o]] = 0.0;
        }
    }
    if (!__syncthreads_or(anylive)) return;   // a tile in the margin

    double gsum;
    int n0;
    ss_setup(a, f, gsum, n0);   // a scan without a weighted position has NaN moments: every pixel is bad
    if (n0 < 0) n0 = 0;
    const int oy0 = ty0 - hy, ox0 = tx0 - hx;   // frame coordinates of the halo tile's first pixel
    const size_t corner = (size_t)n0 * fpix + (size_t)ss_clamp(oy0, a.H - 1) * a.W + ss_clamp(ox0, a.W - 1);
    const double r0 = ss_clean(a.ref[corner]), s0 = ss_clean(S[corner]);

    // ---- the lane's halo pixels: offset in the frame (clamped; a clamped pixel feeds no live output) and in the sample tile
    unsigned roff[SS_P];
    int qbase[SS_P];
    const int np = (HP + SS_THREADS - 1) / SS_THREADS;
#pragma unroll
    for (int p = 0; p < SS_P; ++p) {
        const int q = min(tid + p * SS_THREADS, HP - 1);
        const int qy = q / HX, qx = q - qy * HX;
        roff[p] = (unsigned)ss_clamp(oy0 + qy, a.H - 1) * (unsigned)a.W + (unsigned)ss_clamp(ox0 + qx, a.W - 1);
        qbase[p] = (qy + a.sy) * SW + qx + a.sx;
    }

    int count = K;
    for (int pass = 0; pass < (a.subpixel ? 2 : 1); ++pass) {
        if (pass == 1) {
            // the shifts that some pixel of the tile needs as an axis neighbour of its peak, in ascending order
            __syncthreads();
            for (int k = tid; k < K; k += SS_THREADS) need[k] = 0;
            __syncthreads();
#pragma unroll
            for (int o = 0; o < SS_NO; ++o) {
                if (!live[o] || bad[o] || bidx[o] < 0) continue;
                const int uy = bidx[o] / KX, ux = bidx[o] - uy * KX;
                if (ux > 0 && ux < KX - 1) need[bidx[o] - 1] = need[bidx[o] + 1] = 1;
                if (uy > 0 && uy < 2 * a.sy) need[bidx[o] - KX] = need[bidx[o] + KX] = 1;
            }
            __syncthreads();
            if (tid == 0) {
                int c = 0;
                for (int k = 0; k < K; ++k)
                    if (need[k]) klist[c++] = (unsigned short)k;
                nneed = c;
            }
            __syncthreads();
            count = nneed;
        }
        for (int c0 = 0; c0 < count; c0 += SS_GS) {
            const int kn = min(SS_GS, count - c0);
            int kk[SS_GS], koff[SS_GS];
#pragma unroll
            for (int k = 0; k < SS_GS; ++k) {
                const int c = min(c0 + k, count - 1);
                kk[k] = pass ? (int)klist[c] : c;
                koff[k] = (kk[k] / KX - a.sy) * SW + (kk[k] % KX - a.sx);
            }
            double acc[SS_P][SS_GS];
#pragma unroll
            for (int p = 0; p < SS_P; ++p)
#pragma unroll
                for (int k = 0; k < SS_GS; ++k) acc[p][k] = 0.0;

            for (int n = n0; n < a.N; ++n) {
                const double gn = a.g[n];
                if (!(gn > 0.0)) continue;
                const double wn = gn / gsum;
                const float* Sn = S + (size_t)n * fpix;
                const float* Rn = a.ref + (size_t)n * fpix;
                __syncthreads();
                for (int i = tid; i < SH * SW; i += SS_THREADS) {
                    const int y = i / SW, x = i - y * SW;
                    Sl[i] = ss_clean(Sn[(size_t)ss_clamp(oy0 - a.sy + y, a.H - 1) * a.W + ss_clamp(ox0 - a.sx + x, a.W - 1)]);
                }
                __syncthreads();
                if (kn == SS_GS)
                    ss_products<true>(acc, Rn, roff, Sl, qbase, koff, np, kn, wn, r0, s0);
                else
                    ss_products<false>(acc, Rn, roff, Sl, qbase, koff, np, kn, wn, r0, s0);
            }

#pragma unroll
            for (int k = 0; k < SS_GS; ++k) {
                if (k >= kn) break;
                __syncthreads();
#pragma unroll
                for (int p = 0; p < SS_P; ++p)
                    if (tid + p * SS_THREADS < HP) X[tid + p * SS_THREADS] = acc[p][k];
                double c[SS_NO];
                ss_filter<SS_NO, SS_THREADS>(X, tmp, f, HX, T, a.wy, a.wx, c);
                const int uy = kk[k] / KX - a.sy, ux = kk[k] % KX - a.sx;
#pragma unroll
                for (int o = 0; o < SS_NO; ++o) {
                    if (!live[o] || bad[o]) continue;
                    if (pass == 1) {
                        const int d = kk[k] - bidx[o];
                        if (bidx[o] < 0 || (d != -1 && d != 1 && d != -KX && d != KX)) continue;
                    }
                    const size_t at = (size_t)pix[o] + (size_t)((long long)uy * a.W + ux);
                    const double Sm = meanS[at], VS = varS[at];
                    if (!(Sm == Sm)) {
                        bad[o] = true;
                        continue;
                    }
                    const double C = c[o] - (Rm[o] - r0) * (Sm - s0);
                    const bool defined = VR[o] > SS_TINY * Rm[o] * Rm[o] && VS > SS_TINY * Sm * Sm;
                    const double rho = defined ? C / sqrt(VR[o] * VS) : NAN;
                    if (pass == 0) {
                        if (rho > best[o]) {
                            best[o] = rho;
                            bestC[o] = C;
                            bestS[o] = Sm;
                            bidx[o] = kk[k];
                        }
                    } else {
                        const int d = kk[k] - bidx[o];
                        // with KX == 1 a row neighbour has d = +-1 too: the column neighbours do not exist then
                        if (d == -KX) nb[o][0] = rho;
                        if (d == KX) nb[o][1] = rho;
                        if (KX > 1 && d == -1) nb[o][2] = rho;
                        if (KX > 1 && d == 1) nb[o][3] = rho;
                    }
                }
            }
        }
    }

#pragma unroll
    for (int o = 0; o < SS_NO; ++o) {
        if (!live[o]) continue;
        double v[6] = {NAN, NAN, NAN, NAN, NAN, 0.0};
        if (!bad[o] && bidx[o] >= 0) {
            const int iy = bidx[o] / KX, ix = bidx[o] - iy * KX;
            const bool ey = iy == 0 || iy == 2 * a.sy, ex = ix == 0 || ix == KX - 1;
            double d[2] = {0.0, 0.0};
            for (int ax = 0; ax < 2; ++ax) {
                if (ax ? ex : ey) continue;
                const double lo = nb[o][2 * ax], hi = nb[o][2 * ax + 1], den = lo - 2.0 * best[o] + hi;
                if (den < 0.0) d[ax] = fmin(0.5, fmax(-0.5, 0.5 * (lo - hi) / den));   // a NaN neighbour compares false
            }
            const double tr = bestS[o] / Rm[o];
            v[0] = (iy - a.sy) + d[0];
            v[1] = (ix - a.sx) + d[1];
            v[2] = best[o];
            v[3] = tr;
            v[4] = bestC[o] / (VR[o] * tr);
            v[5] = (ey || ex) ? 3.0 : 1.0;
        }
        for (int pl = 0; pl < 6; ++pl) out[pl * fpix + pix[o]] = v[pl];
    }
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_speckle_scan(const float* ref, const float* samples, int m, int n, int h, int w, int win_y, int win_x,
                                int search_y, int search_x, const double* weights, int taper, int subpixel, double* out,
                                void* stream) {
    if (!ref || !samples || !weights || !out) return fail(B4D_EINVAL, "null argument");
    if (m < 1 || n < 1 || h < 1 || w < 1) return fail(B4D_EINVAL, "counts and frame sides must be >= 1");
    if (win_y < 1 || win_x < 1 || search_y < 0 || search_x < 0) return fail(B4D_EINVAL, "window must be >= 1 and search >= 0");
    if (win_y > SS_MAX_WIN || win_x > SS_MAX_WIN || search_y > SS_MAX_SEARCH || search_x > SS_MAX_SEARCH || n > SS_MAX_N)
        return fail(B4D_ESIZE, "speckle scan: window <= " + std::to_string(SS_MAX_WIN) + ", search <= " +
                                   std::to_string(SS_MAX_SEARCH) + " px per axis, positions <= " + std::to_string(SS_MAX_N));
    if (win_y % 2 == 0 || win_x % 2 == 0) return fail(B4D_EINVAL, "the window sides must be odd");
    if (taper < 0 || taper > 1 || subpixel < 0 || subpixel > 1) return fail(B4D_EINVAL, "taper and subpixel must be 0 or 1");
    if (h < win_y + 2 * search_y || w < win_x + 2 * search_x)
        return fail(B4D_EINVAL, "the window plus twice the search does not fit in the frame");
    if ((long long)h * w > 0x7fffffffLL) return fail(B4D_EINVAL, "more than 2^31 - 1 pixels per frame");
    if (m > 65534) return fail(B4D_EINVAL, "more than 65534 scans");
    hipStream_t st = (hipStream_t)stream;
    ScanArgs a{};
    a.ref = ref;
    a.smp = samples;
    a.g = weights;
    a.out = out;
    a.M = m;
    a.N = n;
    a.H = h;
    a.W = w;
    a.wy = win_y;
    a.wx = win_x;
    a.sy = search_y;
    a.sx = search_x;
    a.taper = taper;
    a.subpixel = subpixel;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    const int rc = get_scratch(sizeof(double) * 2 * (size_t)(1 + m) * h * w, &scratch, st);
    if (rc) return rc;
    a.mom = static_cast<double*>(scratch);
    a.T = SM_T;
    a.tiles_x = (w + SM_T - 1) / SM_T;
    const long long mtiles = (long long)a.tiles_x * ((h + SM_T - 1) / SM_T);
    a.T = std::max(win_y, win_x) <= 15 ? 32 : 16;
    const int tx = (w + a.T - 1) / a.T;
    const long long tiles = (long long)tx * ((h + a.T - 1) / a.T);
    if (tiles > 0x7fffffffLL) return fail(B4D_EINVAL, "too many tiles");
    hipLaunchKernelGGL(k_scan_moments, dim3((unsigned)mtiles, 1 + m), dim3(SM_THREADS), 0, st, a);
    B4D_HIP(hipGetLastError());
    a.tiles_x = tx;
    hipLaunchKernelGGL(k_scan_match, dim3((unsigned)tiles, m), dim3(SS_THREADS), 0, st, a);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
