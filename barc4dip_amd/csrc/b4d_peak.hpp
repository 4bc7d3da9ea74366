// b4d_peak.hpp -- peak quality and 3x3 Taylor step of a correlation map, shared by the trackers
// (b4d_track.hip: phase correlation and template matching; b4d_displace.hip: displacement maps).
#pragma once
#include <hip/hip_runtime.h>

#include "b4d_reduce.hpp"   // argmax_merge, block_argmax

namespace b4d {

// One lane: peak, snr = |peak| / (median + eps) and the sub-pixel shift of the arg-max (mi, mj) of an mny x mnx map,
// op for op like tracking.py:314-375 (float32 scalars, no contraction).  c(di, dj) returns the map value at
// (mi + di, mj + dj); it is only called for interior peaks.  Shifts are counted from (oy, ox).
// subpixel: 0 none, 1 the reference's Taylor step, 2 the Newton step.  o[0..3] = {dy, dx, peak, snr}.
template <class MapAt>
__device__ inline void peak_finish(MapAt c, int mi, int mj, int mny, int mnx, int oy, int ox, float bv, float med, int subpixel,
                                   double eps, double* o) {
    const double peak = (double)bv;
    const double snr = fabs(peak) / ((double)med + eps);
    double dy = (double)(mi - oy), dx = (double)(mj - ox);
    if (subpixel && mi > 0 && mi < mny - 1 && mj > 0 && mj < mnx - 1) {
        const float c00 = c(0, 0);
        const float gy = __fdiv_rn(__fsub_rn(c(1, 0), c(-1, 0)), 2.0f);
        const float hyy = __fsub_rn(__fadd_rn(c(1, 0), c(-1, 0)), __fmul_rn(2.0f, c00));
        const float gx = __fdiv_rn(__fsub_rn(c(0, 1), c(0, -1)), 2.0f);
        const float hxx = __fsub_rn(__fadd_rn(c(0, 1), c(0, -1)), __fmul_rn(2.0f, c00));
        const float hxy = __fdiv_rn(__fadd_rn(__fsub_rn(__fsub_rn(c(1, 1), c(1, -1)), c(-1, 1)), c(-1, -1)), 4.0f);
        const float det = __fsub_rn(__fmul_rn(hxx, hyy), __fmul_rn(hxy, hxy));
        if (det != 0.0f) {
            const float inv = __fdiv_rn(1.0f, det);
            // NOTE the reference's swapped corrections (tracking.py:372-373), reproduced on purpose for subpixel == 1;
            // subpixel == 2 ("newton", displacement maps only) puts each correction on its own axis
            const float di = __fmul_rn(-__fsub_rn(__fmul_rn(hyy, gx), __fmul_rn(hxy, gy)), inv);
            const float dj = __fmul_rn(-__fsub_rn(__fmul_rn(hxx, gy), __fmul_rn(hxy, gx)), inv);
            dy += (double)(subpixel == 2 ? dj : di);
            dx += (double)(subpixel == 2 ? di : dj);
        }
    }
    o[0] = dy;
    o[1] = dx;
    o[2] = peak;
    o[3] = snr;
}

}  // namespace b4d
