// b4d_window.hpp -- the windowed-moments core of k_local_stats (b4d_smooth.hip, moments {x, x x} of one frame) and k_ssim
// (b4d_perceptual.hip, moments {r, x, r r, x x, r x} of a frame pair); DESIGN.md section 31.  The contract of include/b4d.h that
// both entry points state stands here once:
//   - a WIN_T x WIN_T tile of outputs per workgroup; every staged frame tile with its halo in LDS as float32, padded in two
//     dimensions under the border rule ("constant": cval everywhere outside), SciPy's placement (the window starts size / 2 before
//     the pixel);
//   - the moments of a sample are formed in float64 (the product of two float32 is exact there) and summed in float64 along x
//     (row pass, into planes of WIN_T columns), then along y (column pass), every sum from 0.0 in ascending tap order; a box window
//     adds (s + m), a weighted one multiplies by the tap in one rounding (fma(w, m, s));
//   - W, the window's weight, is summed as the first moment of a frame of ones is; what is divided by it is the kernel's business.
// What each kernel keeps: its lane count, its epilogue and stores, its entry point.  Everything above the HIP section is
// __host__ __device__ over plain pointers and free of HIP types, so a plain C++ program can run it (tests/test_window_core_host.py).
// Both units include this header above any fp-contract pragma of their own, so it is compiled with contraction on in both:
// every fused multiply-add here is an explicit fma(), and every product that is added unfused (s + m) is exact.
#pragma once
#include <cmath>
#include <cstddef>

#include "b4d_tile.hpp"

namespace b4d {

// tile edge; largest window per axis; lanes of k_ssim (k_local_stats: the stager's 256); what one workgroup may take of a CU's LDS
constexpr int WIN_T = 32, WIN_MAX = 63, WIN_PAIR_LANES = 512;
constexpr size_t WIN_LDS_LIMIT = 160 * 1024;

struct WindowTaps {   // they travel in the kernel arguments
    int sy, sx, box;
    double wy[WIN_MAX + 1], wx[WIN_MAX + 1];
};
// null taps: a box window (taps of 1.0, never multiplied)
inline WindowTaps fill_window_taps(int size_y, int size_x, const double* taps_y, const double* taps_x) {
    WindowTaps t{};
    t.sy = size_y;
    t.sx = size_x;
    t.box = taps_y ? 0 : 1;
    for (int k = 0; k < size_y; ++k) t.wy[k] = taps_y ? taps_y[k] : 1.0;
    for (int k = 0; k < size_x; ++k) t.wx[k] = taps_x ? taps_x[k] : 1.0;
    return t;
}
B4D_HD double window_weight(const WindowTaps& t) {
    if (t.box) return (double)(t.sy * t.sx);
    double wx = 0.0, W = 0.0;
    for (int k = 0; k < t.sx; ++k) wx = fma(t.wx[k], 1.0, wx);
    for (int j = 0; j < t.sy; ++j) W = fma(t.wy[j], wx, W);
    return W;
}

// sums of a position: {x, x x} from one staged plane, {r, x, r r, x x, r x} from two
constexpr int window_sums(int planes) { return planes == 1 ? 2 : 5; }

// Dynamic LDS of a kernel on this core, from its start: `planes` float32 planes of `rows` rows of `pitch` floats, `plane` floats
// apart (a multiple of four: every plane starts on 16 bytes); from float offset `sums` on, float64: `sums_n` planes of row sums,
// `sum_plane` doubles apart (rows x WIN_T), then `extra` doubles of the kernel's own.
struct WindowLayout {
    int pitch, rows, plane, sums, sum_plane;
    size_t bytes;
};
B4D_HD WindowLayout window_layout(int planes, int sums_n, int sy, int sx, int extra) {
    WindowLayout l{};
    l.pitch = up4(WIN_T + sx - 1);
    l.rows = WIN_T + sy - 1;
    l.plane = up4(l.rows * l.pitch);
    l.sums = planes * l.plane;
    l.sum_plane = l.rows * WIN_T;
    l.bytes = sizeof(float) * (size_t)l.sums + sizeof(double) * ((size_t)sums_n * l.sum_plane + extra);
    return l;
}

// unroll counts of the tap loops: 4 along x and 2 along y where a lane carries five or ten sums (k_ssim: more costs registers, DESIGN.md
// section 31), 8 where it carries two (what the compiler picks unasked)
#if defined(__clang__)
#define B4D_WIN_PRAGMA(x) _Pragma(#x)
#define B4D_WIN_UNROLL(n) B4D_WIN_PRAGMA(clang loop unroll_count(n))
#else
#define B4D_WIN_UNROLL(n)
#endif

// ---- row pass.  p: the position's first sample in the first plane (the second plane `plane` floats behind); s: NS sums, from 0.0.
template <int NP, bool BOX>
B4D_HD void window_row_taps(const float* p, int plane, int sx, const double* wx, double* s) {
    constexpr int NS = window_sums(NP);
    B4D_WIN_UNROLL(NP == 1 ? 8 : 4)
    for (int k = 0; k < sx; ++k) {
        double m[NS];
        const double u = (double)p[k];
        if constexpr (NP == 1) {
            m[0] = u;
            m[1] = u * u;
        } else {
            const double v = (double)p[plane + k];
            m[0] = u;
            m[1] = v;
            m[2] = u * u;
            m[3] = v * v;
            m[4] = u * v;
        }
        B4D_HD_UNROLL
        for (int q = 0; q < NS; ++q) s[q] = BOX ? s[q] + m[q] : fma(wx[k], m[q], s[q]);
    }
}
template <int NP>
B4D_HD void window_row_sums(const float* p, int plane, const WindowTaps& t, double* s) {
    if (t.box) window_row_taps<NP, true>(p, plane, t.sx, t.wx, s);
    else window_row_taps<NP, false>(p, plane, t.sx, t.wx, s);
}

// ---- column pass (k_ssim; k_local_stats keeps loops of its own that do the same).  b: row ly, column c of
// the first plane of row sums (the planes `plane` doubles apart); s[i] of the result: the NS window sums of output row ly + i.
// The ROWS outputs share their reads: row ly + j of a plane is tap j - i of output ly + i.
template <int NS, int ROWS>
struct WindowSums {
    double s[ROWS][NS];
};
template <int NS, int ROWS, bool BOX>
B4D_HD WindowSums<NS, ROWS> window_col_taps(const double* b, int plane, int sy, const double* wy) {
    WindowSums<NS, ROWS> r{};
    B4D_WIN_UNROLL(ROWS == 1 ? 8 : 2)
    for (int j = 0; j < sy + ROWS - 1; ++j) {
        double v[NS];
        B4D_HD_UNROLL
        for (int q = 0; q < NS; ++q) v[q] = b[q * plane + j * WIN_T];
        B4D_HD_UNROLL
        for (int i = 0; i < ROWS; ++i) {
            if (j >= i && j - i < sy) {
                B4D_HD_UNROLL
                for (int q = 0; q < NS; ++q) r.s[i][q] = BOX ? r.s[i][q] + v[q] : fma(wy[j - i], v[q], r.s[i][q]);
            }
        }
    }
    return r;
}
template <int NS, int ROWS>
B4D_HD WindowSums<NS, ROWS> window_col_sums(const double* b, int plane, const WindowTaps& t) {
    if (t.box) return window_col_taps<NS, ROWS, true>(b, plane, t.sy, t.wy);
    return window_col_taps<NS, ROWS, false>(b, plane, t.sy, t.wy);
}

}  // namespace b4d

#if defined(__HIPCC__)
namespace b4d {

struct NoSwz {   // where sample (row j, column c) of a staged tile lives in LDS: plain rows (b4d_smooth.hip has two more layouts)
    __device__ static __forceinline__ int at(int j, int c, int pitch) { return j * pitch + c; }
};

// frame rows ys + [0, nrows) and columns xs + [0, ncols) -> lds[S::at(j, c, pitch)], under the border rule; 16-byte loads for
// aligned groups of four inside a row (vec: nx % 4 == 0 and an aligned base), element by element for the others.  Lane t of 256
// walks the (row, group) pairs 256 apart without a division per pair (tile_walk), four pairs at a time: their loads are all
// issued before the first value goes to LDS.
template <class S>
__device__ __forceinline__ void stage(float* __restrict__ lds, int pitch, const float* __restrict__ f, int ny, int nx, int ys, int nrows, int xs,
                                      int ncols, int mode, float cval, bool vec, int t) {
    const int xa = xs & ~3;
    const int ng = (xs + ncols - xa + 3) >> 2;
    TileWalk w = tile_walk(t, ng);
    while (w.j < nrows) {
        v4f q[4];
        int at[4], c0[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            at[u] = -1;
            q[u] = v4f{cval, cval, cval, cval};
            if (w.j < nrows) {
                const int yy = border_index(ys + w.j, ny, mode);
                const int xb = xa + 4 * w.g;
                at[u] = w.j;
                c0[u] = xb - xs;
                if (yy >= 0) {
                    const float* row = f + (size_t)yy * nx;
                    if (vec && xb >= 0 && xb + 3 < nx) {
                        q[u] = *reinterpret_cast<const v4f*>(row + xb);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int xx = border_index(xb + e, nx, mode);
                            if (xx >= 0) q[u][e] = row[xx];
                        }
                    }
                }
            }
            tile_step(w);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (at[u] >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = c0[u] + e;
                    if (c >= 0 && c < ncols) lds[S::at(at[u], c, pitch)] = q[u][e];
                }
            }
        }
    }
}

// the row pass of a workgroup of LANES lanes: the sums of the `ha` staged rows, positions c < tw (0.0 beyond), into the planes at B
template <int NP, int LANES>
__device__ __forceinline__ void window_row_pass(const float* A, double* B, const WindowLayout& l, int ha, int tw, const WindowTaps& t) {
    constexpr int NS = window_sums(NP);
    for (int idx = threadIdx.x; idx < ha * WIN_T; idx += LANES) {
        const int r = (unsigned)idx / WIN_T, c = (unsigned)idx % WIN_T;
        double s[NS] = {};
        if (c < tw) window_row_sums<NP>(A + r * l.pitch + c, l.plane, t, s);
#pragma unroll
        for (int q = 0; q < NS; ++q) B[q * l.sum_plane + idx] = s[q];
    }
}

// what an entry point `fn` checks of its window arguments: the range, and both tap arrays or neither
inline int check_window(const char* fn, int size_y, int size_x, const double* taps_y, const double* taps_x) {
    if (size_y < 1 || size_y > WIN_MAX || size_x < 1 || size_x > WIN_MAX)
        return fail(B4D_EINVAL, std::string(fn) + ": window sizes must be in 1 .. " + std::to_string(WIN_MAX));
    if ((taps_y == nullptr) != (taps_x == nullptr)) return fail(B4D_EINVAL, std::string(fn) + ": taps_y and taps_x must both be given or both be null");
    return B4D_OK;
}

}  // namespace b4d
#endif
