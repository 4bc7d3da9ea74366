// b4d_wf.hpp -- the grid limits shared by the wavefront units (b4d_integrate.hip, b4d_poly2.hip).
#pragma once
#include "b4d_common.hpp"

namespace b4d {

constexpr int WF_MAX_SIDE = 2048;

inline int wf_check_grid(int n, int ny, int nx) {
    if (n < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "map count and sides must be >= 1");
    if (ny > WF_MAX_SIDE || nx > WF_MAX_SIDE)
        return fail(B4D_ESIZE, "wavefront grids are limited to " + std::to_string(WF_MAX_SIDE) + " nodes per side, got (" +
                                   std::to_string(ny) + ", " + std::to_string(nx) + ")");
    if (n > 65535) return fail(B4D_ESIZE, "at most 65535 maps per call");
    return B4D_OK;
}

}  // namespace b4d
