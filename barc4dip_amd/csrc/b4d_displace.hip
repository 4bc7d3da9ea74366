// b4d_displace.hip -- dense NCC displacement maps: the local shift of every window of a regular grid of a reference frame,
// searched +-(Sy, Sx) px in an image frame (barc4dip_amd/signal/displacement.py).
//
// Window (y0, x0) of pair z is exactly template_matching(ref[y0:y0+wy, x0:x0+wx], img[y0-Sy:y0+wy+Sy, x0-Sx:x0+wx+Sx],
// slices_yx=(slice(Sy, Sy+wy), slice(Sx, Sx+wx))): zero-mean NCC over the (2Sy+1) x (2Sx+1) local shifts, first-index arg-max,
// snr = |peak| / (median |map| + eps), 3x3 Taylor step.  Direct space, one workgroup per (window, pair), one launch:
//   1. float64 shifted power sums of the template and of the search box -> z-scoring constants
//   2. the box (z-scored for "opencv", centred for "skimage": no float32 cancellation on large offsets) goes to LDS in bands of
//      output rows; per-position window sums of I and I^2 in float64 (sliding column sums, then row sums) -> denominators
//   3. numerator: a lane owns RX neighbouring x-shifts of one output row; the template value of (p, q) is wave-uniform and
//      comes from a register row by v_readlane (no LDS traffic), one 16-byte LDS read of the box feeds 4 x RX FMAs;
//      float32 along a template row, float64 across rows
//   4. arg-max, exact median of |map| (b4d::radix_select, (2S+1)^2 is odd: one element), Taylor step (b4d_peak.hpp)
#include <algorithm>
#include <cfloat>
#include <string>

#include "b4d_common.hpp"
#include "b4d_peak.hpp"
#include "b4d_select.hpp"

namespace b4d {

constexpr int DM_MAX_WIN = 128;     // wy, wx: the template row lives in two VGPRs of a wave (q = lane, 64 + lane)
constexpr int DM_MAX_SEARCH = 32;   // Sy, Sx: the map of (2S+1)^2 <= 4225 values stays in LDS
constexpr int DM_THREADS = 256;
constexpr size_t DM_LDS_TARGET = 64 << 10;    // bands of output rows keep a workgroup under this (two or more per CU) ...
constexpr size_t DM_LDS_MAX = 160 << 10;      // ... unless one output row alone needs more (static __shared__ arrays included)

struct DispArgs {
    const float* ref;        // (nref, h, w)
    const float* img;        // (nimg, h, w)
    const int* pair_ref;     // (npairs,) device
    const int* pair_img;
    int h, w;
    int wy, wx, step_y, step_x, sy, sx;
    int gy, gx;              // windows per column / row of the grid
    int zscore, subpixel;
    double eps;
    int pitch;               // LDS row pitch of the box band (floats, multiple of 4)
    int band;                // output rows per band
    int nch;                 // RX-wide x-chunks per output row
    int wxp;                 // wx rounded up to RX (template row padded with zeros)
    int m_off, b_off;        // LDS byte offsets: [0, m_off) window-sum columns (2 x bw doubles), map, box band
    double* out;             // (npairs, gy, gx, 4) {dy, dx, peak, snr}
    int* peak_ij;            // (npairs, gy, gx, 2) or null
};

__device__ __forceinline__ float dm_readlane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int RX>
__device__ __forceinline__ void dm_load(float (&v)[RX], const float* p) {
#pragma unroll
    for (int k = 0; k < RX; k += 4) {
        const float4 t = *reinterpret_cast<const float4*>(p + k);
        v[k] = t.x;
        v[k + 1] = t.y;
        v[k + 2] = t.z;
        v[k + 3] = t.w;
    }
}

// grid (gx, gy, npairs), block 64..256, dynamic LDS (see b4d_displacement_map)
template <int RX>
__global__ void __launch_bounds__(DM_THREADS) k_displace(DispArgs a) {
    extern __shared__ __align__(16) unsigned char dm_lds[];
    const int bw = a.wx + 2 * a.sx, bh = a.wy + 2 * a.sy;
    const int mh = 2 * a.sy + 1, mw = 2 * a.sx + 1, nm = mh * mw, nt = a.wy * a.wx, P = a.pitch;
    double* V1 = reinterpret_cast<double*>(dm_lds);
    double* V2 = V1 + bw;
    float* M = reinterpret_cast<float*>(dm_lds + a.m_off);
    float* B = reinterpret_cast<float*>(dm_lds + a.b_off);
    __shared__ double red[4 * (DM_THREADS / 64)];
    __shared__ float sv[DM_THREADS / 64];
    __shared__ int si[DM_THREADS / 64];
    __shared__ unsigned sh[4];
    __shared__ float nb9[9];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    const int y0 = a.sy + (int)blockIdx.y * a.step_y, x0 = a.sx + (int)blockIdx.x * a.step_x;
    const size_t fpix = (size_t)a.h * a.w;
    const float* T = a.ref + (size_t)a.pair_ref[blockIdx.z] * fpix + (size_t)y0 * a.w + x0;
    const float* I = a.img + (size_t)a.pair_img[blockIdx.z] * fpix + (size_t)(y0 - a.sy) * a.w + (x0 - a.sx);

    // ---- 1. mean / std of template and box: power sums shifted by their first pixel (no cancellation), float64
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    {
        const double t0 = T[0], b0 = I[0];
        for (int k = tid; k < nt; k += nthr) {
            const double d = (double)T[(size_t)(k / a.wx) * a.w + k % a.wx] - t0;
            s[0] += d;
            s[1] += d * d;
        }
        for (int k = tid; k < bh * bw; k += nthr) {
            const double d = (double)I[(size_t)(k / bw) * a.w + k % bw] - b0;
            s[2] += d;
            s[3] += d * d;
        }
        block_sum_all(s, red, nthr >> 6);
        __syncthreads();   // red is written again below
        const double tm = s[0] / nt, bm = s[2] / (bh * bw);
        const double tsd = sqrt(fmax(s[1] / nt - tm * tm, 0.0)), bsd = sqrt(fmax(s[3] / (bh * bw) - bm * bm, 0.0));
        s[0] = t0 + tm;
        s[1] = 1.0 / (tsd + a.eps);
        s[2] = b0 + bm;
        s[3] = a.zscore ? 1.0 / (bsd + a.eps) : 1.0;
    }
    // z = (x - f32(mean)) * f32(1 / (std + eps)): tracking.py:308-311 up to the scale's rounding, which the NCC does not see
    const float tmf = (float)s[0], tinv = (float)s[1], bmf = (float)s[2], binv = (float)s[3];
    auto tz = [&](float v) { return __fmul_rn(__fsub_rn(v, tmf), tinv); };
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < nt; k += nthr) {
        const float z = tz(T[(size_t)(k / a.wx) * a.w + k % a.wx]);
        q[0] += z;
        q[1] += (double)z * z;
    }
    block_sum_all(q, red, nthr >> 6);
    __syncthreads();
    const double tssd = fmax(q[1] - q[0] * q[0] / nt, 0.0);   // sum (tz - mean tz)^2
    // the numerator's template is tz - f32(mean tz): mean tz is ~ulp(mean) / std, 3e-6 for 30 000 counts at 1 % contrast, and
    // would otherwise enter as (window sum of the box) x (mean tz) -- the oracle's num = xc - s1 * tmean removes it exactly
    const float tzm = (float)(q[0] / nt);
    auto tc = [&](float v) { return __fsub_rn(tz(v), tzm); };

    // ---- 2./3. bands of output rows
    for (int ib0 = 0; ib0 < mh; ib0 += a.band) {
        const int ib1 = min(ib0 + a.band, mh), nr = ib1 - ib0 + a.wy - 1;
        const int nload = (a.band + a.wy - 1) * P + 2 * RX;   // the whole band buffer: zeros past the data (read with t = 0)
        __syncthreads();
        for (int k = tid; k < nload; k += nthr) {
            const int r = k / P, c = k - r * P;
            float v = 0.0f;
            if (r < nr && c < bw) v = __fmul_rn(__fsub_rn(I[(size_t)(ib0 + r) * a.w + c], bmf), binv);
            B[k] = v;
        }
        __syncthreads();
        // denominators: column sums over wy rows (sliding down the band), then sums of wx columns; float64 on float32 values
        for (int i = ib0; i < ib1; ++i) {
            const int r = i - ib0;
            for (int c = tid; c < bw; c += nthr) {
                if (r == 0) {
                    double s1 = 0.0, s2 = 0.0;
                    for (int p = 0; p < a.wy; ++p) {
                        const double v = B[p * P + c];
                        s1 += v;
                        s2 += v * v;
                    }
                    V1[c] = s1;
                    V2[c] = s2;
                } else {
                    const double vi = B[(r + a.wy - 1) * P + c], vo = B[(r - 1) * P + c];
                    V1[c] += vi - vo;
                    V2[c] += vi * vi - vo * vo;
                }
            }
            __syncthreads();
            for (int j = tid; j < mw; j += nthr) {
                double s1 = 0.0, s2 = 0.0;
                for (int c = 0; c < a.wx; ++c) {
                    s1 += V1[j + c];
                    s2 += V2[j + c];
                }
                const double d2 = (s2 - s1 * s1 / nt) * tssd;
                const double den = d2 > 0.0 ? sqrt(d2) : 0.0;
                M[i * mw + j] = den > (double)FLT_EPSILON ? (float)den : 0.0f;   // 0: the oracle's masked response
            }
            __syncthreads();
        }
        // numerator: every lane runs every round (clamped task) so that the whole wave takes part in each v_readlane
        const int ntask = (ib1 - ib0) * a.nch;
        for (int tb = 0; tb < ntask; tb += nthr) {
            const int t = min(tb + tid, ntask - 1);
            const int i = ib0 + t / a.nch, j0 = (t % a.nch) * RX;
            double tot[RX];   // float32 FMAs along one template row (<= 128 terms), float64 across rows
#pragma unroll
            for (int r = 0; r < RX; ++r) tot[r] = 0.0;
            const float* brow = B + (i - ib0) * P + j0;
            for (int p = 0; p < a.wy; ++p) {
                float acc[RX];
#pragma unroll
                for (int r = 0; r < RX; ++r) acc[r] = 0.0f;
                const float* trow = T + (size_t)p * a.w;
                const float tv0 = lane < a.wx ? tc(trow[lane]) : 0.0f;
                const float tv1 = lane + 64 < a.wx ? tc(trow[lane + 64]) : 0.0f;
                const float* bp = brow + p * P;
                for (int half = 0; half < 2; ++half) {
                    const int qa = 64 * half, qe = min(a.wxp, qa + 64);
                    if (qa >= qe) break;
                    const float tv = half ? tv1 : tv0;
                    float lo[RX], hi[RX];
                    dm_load<RX>(lo, bp + qa);
                    for (int qb = qa; qb < qe; qb += RX) {
                        dm_load<RX>(hi, bp + qb + RX);
#pragma unroll
                        for (int u = 0; u < RX; ++u) {
                            const float tq = dm_readlane(tv, (qb + u) & 63);
#pragma unroll
                            for (int r = 0; r < RX; ++r) acc[r] = fmaf(tq, u + r < RX ? lo[u + r] : hi[u + r - RX], acc[r]);
                        }
#pragma unroll
                        for (int r = 0; r < RX; ++r) lo[r] = hi[r];
                    }
                }
#pragma unroll
                for (int r = 0; r < RX; ++r) tot[r] += (double)acc[r];
            }
            if (tb + tid < ntask) {
#pragma unroll
                for (int r = 0; r < RX; ++r) {
                    const int j = j0 + r;
                    if (j < mw) {
                        const float d = M[i * mw + j];
                        M[i * mw + j] = d != 0.0f ? (float)(tot[r] / (double)d) : 0.0f;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- 4. first-occurrence arg-max, Taylor neighbourhood, median of |map|, finish
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = tid; k < nm; k += nthr) argmax_merge(bv, bi, M[k], k);
    block_argmax(bv, bi, sv, si, nthr >> 6);
    if (bi == 0x7fffffff) bi = 0;   // all-NaN map: np.argmax would name the first NaN
    const int mi = bi / mw, mj = bi % mw;
    if (tid < 9) {
        const int yy = mi + tid / 3 - 1, xx = mj + tid % 3 - 1;
        nb9[tid] = (yy >= 0 && yy < mh && xx >= 0 && xx < mw) ? M[yy * mw + xx] : 0.0f;
    }
    __syncthreads();
    for (int k = tid; k < nm; k += nthr) M[k] = fabsf(M[k]);
    __syncthreads();
    unsigned nl, ne;
    const float med = keys::from_key(radix_select<1>(M, (unsigned)nm, (unsigned)nm / 2, reinterpret_cast<unsigned*>(B), sh, nl, ne));
    if (tid != 0) return;
    const size_t win = ((size_t)blockIdx.z * a.gy + blockIdx.y) * a.gx + blockIdx.x;
    auto c = [&](int di, int dj) { return nb9[(di + 1) * 3 + dj + 1]; };
    peak_finish(c, mi, mj, mh, mw, a.sy, a.sx, bv, med, a.subpixel, a.eps, a.out + win * 4);
    if (a.peak_ij) {
        a.peak_ij[win * 2] = mi;
        a.peak_ij[win * 2 + 1] = mj;
    }
}

// output rows per band and dynamic LDS bytes for a workgroup whose kernel already holds `static_lds` bytes of __shared__ arrays:
// as many rows as fit the target, one band when the whole box fits, else as many as fit the CU's LDS
static int plan_bands(DispArgs& a, int rx, size_t static_lds, size_t* lds) {
    const int mh = 2 * a.sy + 1;
    auto band_for = [&](size_t budget) {
        const long rows = ((long)budget - (long)static_lds - a.b_off - (long)sizeof(float) * 2 * rx) / ((long)sizeof(float) * a.pitch);
        return (int)std::min<long>(mh, rows - (a.wy - 1));
    };
    a.band = band_for(DM_LDS_TARGET);
    if (a.band < 1) a.band = band_for(DM_LDS_MAX);
    if (a.band < 1) return fail(B4D_ESIZE, "displacement map: window and search exceed the LDS of a CU");
    // the box band doubles as the median's 2048-bin histogram once the map is done
    const size_t bbytes = std::max<size_t>(sizeof(float) * ((size_t)(a.band + a.wy - 1) * a.pitch + 2 * rx), sizeof(unsigned) * 2048);
    *lds = a.b_off + bbytes;
    if (*lds + static_lds > DM_LDS_MAX) return fail(B4D_ESIZE, "displacement map: window and search exceed the LDS of a CU");
    return B4D_OK;
}

template <int RX>
static int launch_displace(DispArgs a, int npairs, hipStream_t st) {
    const void* kern = reinterpret_cast<const void*>(&k_displace<RX>);
    hipFuncAttributes attr{};
    B4D_HIP(hipFuncGetAttributes(&attr, kern));
    size_t lds = 0;
    int rc = plan_bands(a, RX, attr.sharedSizeBytes, &lds);
    if (rc) return rc;
    const int ntask = (2 * a.sy + 1) * a.nch;
    const int threads = std::min(DM_THREADS, std::max(64, (ntask + 63) / 64 * 64));
    return launch(k_displace<RX>, dim3(a.gx, a.gy, npairs), dim3(threads), lds, st, a);
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_displacement_map(const float* ref, int nref, const float* img, int nimg, const int32_t* pair_ref,
                                    const int32_t* pair_img, int npairs, int h, int w, int win_y, int win_x, int step_y,
                                    int step_x, int search_y, int search_x, int zscore_image, int subpixel, double eps,
                                    double* out, int32_t* peak_ij, void* stream) {
    if (!ref || !img || !pair_ref || !pair_img || !out) return fail(B4D_EINVAL, "null argument");
    if (nref < 1 || nimg < 1 || npairs < 1 || h < 1 || w < 1) return fail(B4D_EINVAL, "counts and frame sides must be >= 1");
    if (win_y < 1 || win_x < 1 || step_y < 1 || step_x < 1 || search_y < 1 || search_x < 1)
        return fail(B4D_EINVAL, "window, step and search must be >= 1");
    if (win_y > DM_MAX_WIN || win_x > DM_MAX_WIN || search_y > DM_MAX_SEARCH || search_x > DM_MAX_SEARCH)
        return fail(B4D_ESIZE, "displacement map: window <= " + std::to_string(DM_MAX_WIN) + " and search <= " +
                                   std::to_string(DM_MAX_SEARCH) + " px per axis");
    if (h < win_y + 2 * search_y || w < win_x + 2 * search_x)
        return fail(B4D_EINVAL, "the window plus its search margin does not fit in the frame");
    const int gy = (h - win_y - 2 * search_y) / step_y + 1, gx = (w - win_x - 2 * search_x) / step_x + 1;
    if (gy > 65535 || npairs > 65535) return fail(B4D_EINVAL, "more than 65535 window rows or pairs");
    for (int i = 0; i < npairs; ++i)
        if (pair_ref[i] < 0 || pair_ref[i] >= nref || pair_img[i] < 0 || pair_img[i] >= nimg)
            return fail(B4D_EINVAL, "pair " + std::to_string(i) + ": index out of range");
    hipStream_t st = (hipStream_t)stream;
    const int RX = (2 * search_x + 1 >= 16) ? 8 : 4;
    DispArgs a{};
    a.ref = ref;
    a.img = img;
    a.h = h;
    a.w = w;
    a.wy = win_y;
    a.wx = win_x;
    a.step_y = step_y;
    a.step_x = step_x;
    a.sy = search_y;
    a.sx = search_x;
    a.gy = gy;
    a.gx = gx;
    a.zscore = zscore_image ? 1 : 0;
    a.subpixel = subpixel == 2 ? 2 : (subpixel ? 1 : 0);
    a.eps = eps;
    a.nch = (2 * search_x + 1 + RX - 1) / RX;
    a.wxp = (win_x + RX - 1) / RX * RX;
    const int bw = win_x + 2 * search_x, nm = (2 * search_y + 1) * (2 * search_x + 1);
    a.pitch = (bw + 3) / 4 * 4;
    a.m_off = (int)(sizeof(double) * 2 * bw + 15) / 16 * 16;
    a.b_off = a.m_off + (int)sizeof(float) * ((nm + 3) / 4 * 4);
    a.out = out;
    a.peak_ij = peak_ij;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    int rc = get_scratch(sizeof(int32_t) * 2 * (size_t)npairs, &scratch, st);
    if (rc) return rc;
    int32_t* d_pairs = static_cast<int32_t*>(scratch);
    B4D_HIP(hipMemcpyAsync(d_pairs, pair_ref, sizeof(int32_t) * npairs, hipMemcpyHostToDevice, st));
    B4D_HIP(hipMemcpyAsync(d_pairs + npairs, pair_img, sizeof(int32_t) * npairs, hipMemcpyHostToDevice, st));
    a.pair_ref = d_pairs;
    a.pair_img = d_pairs + npairs;
    return RX == 8 ? launch_displace<8>(a, npairs, st) : launch_displace<4>(a, npairs, st);
}
