// b4d_speckle.hip -- transmission and dark-field maps of speckle tracking: the weighted moments of every window of a reference
// frame and of the image window that its tracked displacement points at (barc4dip_amd/signal/speckle.py).
//
// Window (y0, x0) of pair z on the grid of b4d_displacement_map, displacement (dy, dx):
//   r[j][i] = ref[y0+j][x0+i]      s[j][i] = img at (y0+j+dy, x0+i+dx), nearest (order 0) or bilinear in float64 (order 1)
// With the weights h[j][i] = h_wy[j] h_wx[i] / (sum h_wy sum h_wx) (flat, or the half-sample Hann of the fringe code) the means
// Rm, Sm, the variances VR, VS and the covariance C come from float64 power sums of (r - r[0][0]) and (s - s[0][0]): shifted by
// the window's first pixel, so that 1 % contrast on 30 000 counts loses nothing to cancellation (step 1 of k_displace).
// One workgroup per (window, pair), one launch; every window has its own sub-pixel offset, so nothing is shared between
// neighbours.  64 to 256 lanes by window area (SC_PER_LANE).  A lane walks the window in row-major order with the block's
// stride: the reference reads are contiguous win_x-runs, the sample reads the same runs displaced by one offset, the two x-taps
// of a lane adjacent.  The summation order depends on the window shape alone.
#include <algorithm>
#include <cmath>
#include <string>

#include "b4d_common.hpp"
#include "b4d_reduce.hpp"

namespace b4d {

constexpr int SC_MAX_WIN = 128;      // the limits of b4d_displacement_map, so that every field it produces is accepted
constexpr int SC_MAX_MARGIN = 32;
constexpr int SC_THREADS = 256;
constexpr int SC_NSUM = 6;           // sum h, h dr, h dr^2, h ds, h ds^2, h dr ds
// window pixels per lane before the workgroup grows: 31 x 31 runs on one wave, 63 x 63 on two, 79 x 79 and larger on four.
// Measured at 4 ... 128: fewer, longer-running waves keep more windows in flight per CU and reduce less
constexpr int SC_PER_LANE = 32;

struct SpeckleArgs {
    const float* ref;        // (nref, h, w)
    const float* img;        // (nimg, h, w)
    const int* pair_ref;     // (npairs,) device
    const int* pair_img;
    int h, w;
    int wy, wx, step_y, step_x, my, mx;
    int gy, gx;
    const double* dy;        // node (Y, X) of pair z at z * field_stride + (Y * gx + X) * node_stride
    const double* dx;
    long long field_stride;
    int node_stride;
    int order, taper;
    double* out;             // (npairs, gy, gx, 6)
};

// integer tap t and the weights of the taps t and t + 1 along one axis; w0 is never 0 (a fraction that rounds to 1 moves the tap)
__device__ inline void sc_taps(double d, int order, double& t, double& w0, double& w1) {
    t = floor(order == 0 ? d + 0.5 : d);
    w1 = order == 0 ? 0.0 : d - t;
    w0 = 1.0 - w1;
    if (w0 == 0.0) {
        t += 1.0;
        w0 = 1.0;
        w1 = 0.0;
    }
}

// grid (gx, gy, npairs), block 64..256
__global__ void __launch_bounds__(SC_THREADS) k_speckle_contrast(SpeckleArgs a) {
    __shared__ double hy[SC_MAX_WIN], hx[SC_MAX_WIN];
    __shared__ double red[SC_NSUM * (SC_THREADS / 64)];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int y0 = a.my + (int)blockIdx.y * a.step_y, x0 = a.mx + (int)blockIdx.x * a.step_x;
    const size_t node = (size_t)blockIdx.y * a.gx + blockIdx.x;
    double* o = a.out + ((size_t)blockIdx.z * a.gy * a.gx + node) * 6;
    const size_t fo = (size_t)blockIdx.z * (size_t)a.field_stride + node * (size_t)a.node_stride;
    const double dy = a.dy[fo], dx = a.dx[fo];

    // ---- taps of non-zero weight must lie in the frame; tested in float64 before any integer or address is formed
    double ty, tx, wy0, wy1, wx0, wx1;
    sc_taps(dy, a.order, ty, wy0, wy1);
    sc_taps(dx, a.order, tx, wx0, wx1);
    const double yhi = ty + (wy1 != 0.0 ? 1.0 : 0.0), xhi = tx + (wx1 != 0.0 ? 1.0 : 0.0);
    const bool inside = isfinite(dy) && isfinite(dx) && y0 + ty >= 0.0 && y0 + a.wy - 1 + yhi <= (double)(a.h - 1) &&
                        x0 + tx >= 0.0 && x0 + a.wx - 1 + xhi <= (double)(a.w - 1);
    if (!inside) {   // the same for every lane of the workgroup
        if (tid < 6) o[tid] = NAN;
        return;
    }
    const int iy = (int)ty, ix = (int)tx;
    const size_t fpix = (size_t)a.h * a.w;
    const float* R = a.ref + (size_t)a.pair_ref[blockIdx.z] * fpix + (size_t)y0 * a.w + x0;
    const float* S = a.img + (size_t)a.pair_img[blockIdx.z] * fpix + (size_t)(y0 + iy) * a.w + (x0 + ix);

    for (int k = tid; k < a.wy; k += nthr) hy[k] = a.taper ? 0.5 - 0.5 * cos(2.0 * M_PI * (k + 0.5) / a.wy) : 1.0;
    for (int k = tid; k < a.wx; k += nthr) hx[k] = a.taper ? 0.5 - 0.5 * cos(2.0 * M_PI * (k + 0.5) / a.wx) : 1.0;

    // a tap of weight 0 is not read (wave-uniform branches): at +margin on the last window its address is outside the frame
    auto row = [&](const float* p) {
        double v = wx0 * (double)p[0];
        if (wx1 != 0.0) v += wx1 * (double)p[1];
        return v;
    };
    auto sample = [&](int j, int i) {
        const float* p = S + (size_t)j * a.w + i;
        double v = wy0 * row(p);
        if (wy1 != 0.0) v += wy1 * row(p + a.w);
        return v;
    };
    const double r0 = R[0], s0 = sample(0, 0);
    __syncthreads();

    double s[SC_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int nt = a.wy * a.wx, qj = nthr / a.wx, qi = nthr % a.wx;
    int j = tid / a.wx, i = tid % a.wx;
    for (int k = tid; k < nt; k += nthr) {
        const double hw = hy[j] * hx[i];
        const double dr = (double)R[(size_t)j * a.w + i] - r0, ds = sample(j, i) - s0;
        s[0] += hw;
        s[1] += hw * dr;
        s[2] += hw * dr * dr;
        s[3] += hw * ds;
        s[4] += hw * ds * ds;
        s[5] += hw * dr * ds;
        j += qj;
        i += qi;
        if (i >= a.wx) {
            i -= a.wx;
            ++j;
        }
    }
    block_sum_all(s, red, blockDim.x >> 6);   // (<= 4 waves) fixed order, result in every lane
    if (tid != 0) return;

    const double mr = s[1] / s[0], ms = s[3] / s[0];
    const double Rm = r0 + mr, Sm = s0 + ms;
    const double VR = s[2] / s[0] - mr * mr, VS = s[4] / s[0] - ms * ms, Cv = s[5] / s[0] - mr * ms;
    // a denominator, or a variance under a square root, that is not above 0 gives NaN (a NaN operand compares false)
    const double T = Rm > 0.0 ? Sm / Rm : NAN;
    const double vr = (VR > 0.0 && Rm > 0.0) ? sqrt(VR) / Rm : NAN;
    const double vs = (VS > 0.0 && Sm > 0.0) ? sqrt(VS) / Sm : NAN;
    o[0] = T;
    o[1] = vr > 0.0 ? vs / vr : NAN;
    o[2] = VR * T > 0.0 ? Cv / (VR * T) : NAN;
    o[3] = (VR > 0.0 && VS > 0.0) ? Cv / sqrt(VS * VR) : NAN;
    o[4] = vr;
    o[5] = vs;
}

}  // namespace b4d

using namespace b4d;

extern "C" int b4d_speckle_contrast(const float* ref, int nref, const float* img, int nimg, const int32_t* pair_ref,
                                    const int32_t* pair_img, int npairs, int h, int w, int win_y, int win_x, int step_y,
                                    int step_x, int margin_y, int margin_x, const double* dy, const double* dx,
                                    long long field_stride, int order, int taper, double* out, void* stream) {
    if (!ref || !img || !pair_ref || !pair_img || !dy || !dx || !out) return fail(B4D_EINVAL, "null argument");
    if (nref < 1 || nimg < 1 || npairs < 1 || h < 1 || w < 1) return fail(B4D_EINVAL, "counts and frame sides must be >= 1");
    if (win_y < 1 || win_x < 1 || step_y < 1 || step_x < 1 || margin_y < 0 || margin_x < 0)
        return fail(B4D_EINVAL, "window and step must be >= 1, margin >= 0");
    if (order < 0 || order > 1 || taper < 0 || taper > 1) return fail(B4D_EINVAL, "order and taper must be 0 or 1");
    if (win_y > SC_MAX_WIN || win_x > SC_MAX_WIN || margin_y > SC_MAX_MARGIN || margin_x > SC_MAX_MARGIN)
        return fail(B4D_ESIZE, "speckle contrast: window <= " + std::to_string(SC_MAX_WIN) + " and margin <= " +
                                   std::to_string(SC_MAX_MARGIN) + " px per axis");
    if (h < win_y + 2 * margin_y || w < win_x + 2 * margin_x)
        return fail(B4D_EINVAL, "the window plus its margin does not fit in the frame");
    const int gy = (h - win_y - 2 * margin_y) / step_y + 1, gx = (w - win_x - 2 * margin_x) / step_x + 1;
    if (gy > 65535 || npairs > 65535) return fail(B4D_EINVAL, "more than 65535 window rows or pairs");
    const long long nodes = (long long)gy * gx;
    if (field_stride < nodes || field_stride % nodes != 0 || field_stride / nodes > 0x7fffffff)
        return fail(B4D_EINVAL, "field_stride must be a positive multiple of gy * gx (the multiple is the stride between nodes)");
    for (int i = 0; i < npairs; ++i)
        if (pair_ref[i] < 0 || pair_ref[i] >= nref || pair_img[i] < 0 || pair_img[i] >= nimg)
            return fail(B4D_EINVAL, "pair " + std::to_string(i) + ": index out of range");
    hipStream_t st = (hipStream_t)stream;
    SpeckleArgs a{};
    a.ref = ref;
    a.img = img;
    a.h = h;
    a.w = w;
    a.wy = win_y;
    a.wx = win_x;
    a.step_y = step_y;
    a.step_x = step_x;
    a.my = margin_y;
    a.mx = margin_x;
    a.gy = gy;
    a.gx = gx;
    a.dy = dy;
    a.dx = dx;
    a.field_stride = field_stride;
    a.node_stride = (int)(field_stride / nodes);
    a.order = order;
    a.taper = taper;
    a.out = out;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    int rc = get_scratch(sizeof(int32_t) * 2 * (size_t)npairs, &scratch, st);
    if (rc) return rc;
    int32_t* d_pairs = static_cast<int32_t*>(scratch);
    B4D_HIP(hipMemcpyAsync(d_pairs, pair_ref, sizeof(int32_t) * npairs, hipMemcpyHostToDevice, st));
    B4D_HIP(hipMemcpyAsync(d_pairs + npairs, pair_img, sizeof(int32_t) * npairs, hipMemcpyHostToDevice, st));
    a.pair_ref = d_pairs;
    a.pair_img = d_pairs + npairs;
    const int lanes = (win_y * win_x + SC_PER_LANE - 1) / SC_PER_LANE;
    const int threads = std::min(SC_THREADS, std::max(64, (lanes + 63) / 64 * 64));
    hipLaunchKernelGGL(k_speckle_contrast, dim3(gx, gy, npairs), dim3(threads), 0, st, a);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
