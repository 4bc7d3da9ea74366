// b4d_tile.hpp -- what a tiled kernel over a (batch, ny, nx) float32 stack needs (b4d_rankfilt.hip, b4d_smooth.hip,
// b4d_perceptual.hip; the mode codes also b4d_warp.hip): the border rule, the division-free walk of a workgroup over a tile's
// groups, the four-wide stores, and the argument check, alignment predicate, tile count and frame-chunk loop of the entry points
// (the rank filters keep their own stager, and why; the other one is `stage` of b4d_window.hpp).  The border
// rule and the walk are __host__ __device__ and free of HIP types, so a plain C++ program can include this header and run them
// (tests/test_rank_filter_host.py, tests/test_tile_walk_host.py); everything below them needs hipcc.
#pragma once
#include "b4d_keys.hpp"   // B4D_HD

namespace b4d {

constexpr int up4(int n) { return (n + 3) & ~3; }

// source index of position i on an axis of n samples under scipy.ndimage's border modes, for any overhang (repeated
// reflection / wrap); -1 = outside (mode "constant").  The codes of every entry point that takes a mode: b4d_warp_* knows 0 .. 3.
enum { MODE_NEAREST = 0, MODE_REFLECT = 1, MODE_MIRROR = 2, MODE_CONSTANT = 3, MODE_WRAP = 4 };
B4D_HD int border_index(int i, int n, int mode) {
    if (i >= 0 && i < n) return i;
    if (mode == MODE_CONSTANT) return -1;
    if (mode == MODE_NEAREST || n == 1) return i < 0 ? 0 : n - 1;
    if (mode == MODE_WRAP) {
        i %= n;
        return i < 0 ? i + n : i;
    }
    const int p = mode == MODE_REFLECT ? 2 * n : 2 * n - 2;   // reflect: d c b a | a b c d | d c b a; mirror: d c b | a b c d | c b a
    i %= p;
    if (i < 0) i += p;
    if (i < n) return i;
    return mode == MODE_REFLECT ? p - 1 - i : p - i;
}

// The walk of 256 lanes over the (row j, group g) pairs of a tile with ng groups of four columns a row: lane t takes the pairs
// t, t + 256, t + 512, .. of the row-major order.  One division per lane, none per pair: 256 = dq * ng + dr, so a step adds dq rows
// and dr groups and carries once.  Its one user is `stage` of b4d_window.hpp (separable filters, local statistics, SSIM); it is host
// code, so that a program can run it for every lane and tile shape.
struct TileWalk {
    int j, g, ng, dq, dr;
};
B4D_HD TileWalk tile_walk(int t, int ng) {
    const int j = t / ng, dq = 256 / ng;
    return TileWalk{j, t - j * ng, ng, dq, 256 - dq * ng};
}
B4D_HD void tile_step(TileWalk& w) {
    w.g += w.dr;
    w.j += w.dq;
    if (w.g >= w.ng) {
        w.g -= w.ng;
        ++w.j;
    }
}

}  // namespace b4d

#if defined(__HIPCC__)
#include <algorithm>
#include <string>

#include "b4d_common.hpp"

namespace b4d {

typedef float v4f __attribute__((ext_vector_type(4)));

// four values to out[0 .. 4) of a row that ends `left` elements from out; 16 bytes where vec (final: streaming store)
__device__ __forceinline__ void store4(float* __restrict__ out, v4f v, int left, bool vec, bool final) {
    if (vec && left >= 4) {
        if (final) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(out));
        else *reinterpret_cast<v4f*>(out) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < left) out[e] = v[e];
    }
}
// four byte flags likewise; one 32-bit store where vec
__device__ __forceinline__ void store4(unsigned char* __restrict__ out, const unsigned char (&v)[4], int left, bool vec) {
    if (vec && left >= 4) {
        *reinterpret_cast<uint32_t*>(out) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < left) out[e] = v[e];
    }
}

// ---- host side of an entry point over a frame stack
// The errors they share, under the entry point's name fn: `what` (its own wording) for a null pointer or an empty shape, the mode,
// and, where the kernels index a frame with 32 bits (max_pixels), the frame size.
inline int check_stack(const char* fn, const char* what, bool ptrs, int batch, int ny, int nx, int mode, bool max_pixels) {
    const std::string f = std::string(fn) + ": ";
    if (!ptrs || batch < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, f + what);
    if (mode < MODE_NEAREST || mode > MODE_WRAP) return fail(B4D_EINVAL, f + "mode must be 0 nearest, 1 reflect, 2 mirror, 3 constant or 4 wrap");
    if (max_pixels && (long long)ny * nx >= (1LL << 31)) return fail(B4D_ESIZE, f + "2^31 or more pixels per frame");
    return B4D_OK;
}
// whether rows of nx elements behind p take accesses of four elements, `bytes` wide (every row then starts on a multiple of it)
inline bool vec_ok(const void* p, int nx, size_t bytes) { return p && nx % 4 == 0 && ptr_aligned(p, bytes); }
// tiles of edge t along an axis of n
static unsigned tiles(int n, int t) { return (unsigned)((n + t - 1) / t); }
// f(b0, nb) for every chunk of at most `chunk` frames (a grid dimension holds 65535); stops at the first error
constexpr int MAX_GRID_FRAMES = 65535;
template <class F>
int for_frame_chunks(int batch, int chunk, F f) {
    for (int b0 = 0; b0 < batch; b0 += chunk)
        if (const int rc = f(b0, std::min(chunk, batch - b0))) return rc;
    return B4D_OK;
}

}  // namespace b4d
#endif
