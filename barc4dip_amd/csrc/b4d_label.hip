// b4d_label.hip -- connected-component labelling and per-region measurements (include/b4d.h "Regions").
//   b4d_label_regions      k_label_tile     one workgroup labels a LB_TY x LB_TX tile in LDS by union-find, writes frame-wide links
//                          k_label_seams    one lane per seam pixel unites across tile edges (tile-corner diagonals included)
//                          k_label_flatten  every pixel -> its root; roots counted per scan block
//                          k_label_scan     exclusive scan of the block counts per frame, n_regions
//                          k_label_assign   roots take their number (as a code), k_label_final: every pixel reads its root's
//   b4d_region_properties  k_rp_init, k_rp_boxes (integer atomicMin / atomicMax from the pixels on a region's outline),
//                          k_rp_small (one wave per region), k_rp_big (one 512-lane workgroup per region whose box exceeds RP_WAVE_AREA)
//   b4d_relabel            k_relabel
// Separate launches order the passes; no workgroup waits for another.  The union-find itself, its termination argument and the
// numbering rule are in b4d_label.hpp.  Integer atomics only; every float64 sum is a fixed-order reduction (b4d_reduce.hpp's
// butterfly, then the waves in order), so every column has the same bits run to run, for a frame alone and in any batch.
#include <cfloat>
#include <climits>
#include <cmath>

#include "b4d_common.hpp"
#include "b4d_label.hpp"
#include "b4d_reduce.hpp"
#include "b4d_tile.hpp"

namespace b4d {
namespace {

// links in LDS (one workgroup) and in device memory (any workgroup of the launch): relaxed atomic loads, so that a link is read
// again wherever the algorithm asks for it, and integer atomicMin
struct LdsMem {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int fetch_min(int i, int v) { return atomicMin(p + i, v); }
    __device__ __forceinline__ void store(int i, int v) { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct GlobalMem {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) { return atomicMin(p + i, v); }
    __device__ __forceinline__ void store(int i, int v) { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct LbArgs {
    const float* frames;
    const float* thresholds;
    const uint8_t* mask;
    int32_t* labels;
    int32_t* n_regions;
    int ny, nx, conn, nblk;
    int* err;
    int* partial;   // (batch, nblk): roots per scan block, then their exclusive scan
};

constexpr int LB_ROWS_PER_PASS = LB_THREADS / LB_TX, LB_PASSES = LB_TY / LB_ROWS_PER_PASS;
static_assert(LB_TX == 64 && LB_THREADS % LB_TX == 0 && LB_TY % LB_ROWS_PER_PASS == 0, "a wave takes one tile row");
constexpr int LB_CHUNKS = LB_SCAN / LB_THREADS;    // 64-pixel chunks per wave of a scan block

// grid (tiles_x, tiles_y, frames)
__global__ void __launch_bounds__(LB_THREADS) k_label_tile(LbArgs a, int frame0) {
    __shared__ int lab[LB_TY * LB_TX];
    const int frame = frame0 + blockIdx.z, y0 = blockIdx.y * LB_TY, x0 = blockIdx.x * LB_TX;
    const int th = min(LB_TY, a.ny - y0), tw = min(LB_TX, a.nx - x0);
    const size_t base = (size_t)frame * a.ny * a.nx;
    const float thr = a.mask ? 0.f : a.thresholds[frame];
    const int lx = threadIdx.x & (LB_TX - 1), lr = threadIdx.x / LB_TX;
#pragma unroll
    for (int k = 0; k < LB_PASSES; ++k) {
        const int ly = lr + k * LB_ROWS_PER_PASS, l = ly * LB_TX + lx;
        bool fg = false;
        if (ly < th && lx < tw) {
            const size_t g = base + (size_t)(y0 + ly) * a.nx + x0 + lx;
            fg = a.mask ? a.mask[g] != 0 : a.frames[g] > thr;     // strict: false for a NaN
        }
        lab[l] = fg ? l : LB_BACKGROUND;
    }
    __syncthreads();
    LdsMem m{lab};
    int tripped = 0;
    for (int k = 0; k < LB_PASSES; ++k) {
        const int ly = lr + k * LB_ROWS_PER_PASS;
        if (ly < th && lx < tw) lb_tile_pixel(m, ly, lx, tw, LB_TX, a.conn, (unsigned)(LB_TY * LB_TX), tripped);
    }
    __syncthreads();
    for (int k = 0; k < LB_PASSES; ++k) {
        const int ly = lr + k * LB_ROWS_PER_PASS, l = ly * LB_TX + lx;
        if (ly < th && lx < tw) {
            int g = LB_BACKGROUND;
            if (m.load(l) >= 0) {
                const int r = uf_find(m, l, (unsigned)(LB_TY * LB_TX), tripped);
                g = (y0 + r / LB_TX) * a.nx + x0 + (r & (LB_TX - 1));
            }
            a.labels[base + (size_t)(y0 + ly) * a.nx + x0 + lx] = g;
        }
    }
    if (tripped) atomicOr(a.err, 1);
}

// grid (ceil(seam pixels / LB_THREADS), frames): the first rows of the tile rows 1.., then the first columns of the tile columns 1..
__global__ void __launch_bounds__(LB_THREADS) k_label_seams(LbArgs a, int frame0, int hs, int vs) {
    const int frame = frame0 + blockIdx.y;
    const long long idx = (long long)blockIdx.x * LB_THREADS + threadIdx.x, nrow = (long long)hs * a.nx;
    if (idx >= nrow + (long long)vs * a.ny) return;
    GlobalMem m{a.labels + (size_t)frame * a.ny * a.nx};
    int tripped = 0, y, x;
    const bool row_seam = idx < nrow;
    if (row_seam) {
        y = ((int)(idx / a.nx) + 1) * LB_TY;
        x = (int)(idx % a.nx);
    } else {
        const long long j = idx - nrow;
        x = ((int)(j / a.ny) + 1) * LB_TX;
        y = (int)(j % a.ny);
    }
    lb_seam_pixel(m, y, x, a.ny, a.nx, a.conn, row_seam, (unsigned)(a.ny * a.nx), tripped);
    if (tripped) atomicOr(a.err, 1);
}

// pixel of (scan block, wave, chunk, lane): a wave takes LB_CHUNKS whole 64-pixel chunks in raster order
__device__ __forceinline__ int scan_pixel(int c) {
    return blockIdx.x * LB_SCAN + (threadIdx.x >> 6) * (LB_CHUNKS * 64) + c * 64 + (threadIdx.x & 63);
}

// grid (nblk, frames)
__global__ void __launch_bounds__(LB_THREADS) k_label_flatten(LbArgs a, int frame0) {
    __shared__ int cnt[LB_THREADS / 64];
    const int frame = frame0 + blockIdx.y, npix = a.ny * a.nx;
    GlobalMem m{a.labels + (size_t)frame * npix};
    int tripped = 0, roots = 0;
    for (int c = 0; c < LB_CHUNKS; ++c) {
        const int p = scan_pixel(c);
        bool root = false;
        if (p < npix && m.load(p) >= 0) {
            const int r = uf_find(m, p, (unsigned)npix, tripped);
            root = r == p;
            if (!root) m.store(p, r);
        }
        roots += __popcll(__ballot(root));
    }
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = roots;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < LB_THREADS / 64; ++w) s += cnt[w];
        a.partial[(size_t)frame * a.nblk + blockIdx.x] = s;
    }
    if (tripped) atomicOr(a.err, 1);
}

// grid (frames): the block counts of a frame -> their exclusive scan, in place; n_regions
__global__ void __launch_bounds__(LB_THREADS) k_label_scan(LbArgs a, int frame0) {
    __shared__ unsigned tot[LB_THREADS / 64];
    const int frame = frame0 + blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* part = a.partial + (size_t)frame * a.nblk;
    unsigned carry = 0;
    for (int b0 = 0; b0 < a.nblk; b0 += LB_THREADS) {
        const int b = b0 + threadIdx.x;
        const unsigned v = b < a.nblk ? (unsigned)part[b] : 0u;
        const unsigned inc = wave_scan_inclusive(v, lane);
        if (lane == 63) tot[wave] = inc;
        __syncthreads();
        unsigned before = carry, all = 0;
        for (int w = 0; w < LB_THREADS / 64; ++w) {
            before += w < wave ? tot[w] : 0u;
            all += tot[w];
        }
        if (b < a.nblk) part[b] = (int)(before + inc - v);
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.n_regions[frame] = *a.err ? B4D_ELOOP : (int)carry;
}

// grid (nblk, frames): root number = roots before the block + before the wave + before the chunk + below the lane, + 1
__global__ void __launch_bounds__(LB_THREADS) k_label_assign(LbArgs a, int frame0) {
    __shared__ int cnt[LB_THREADS / 64];
    const int frame = frame0 + blockIdx.y, npix = a.ny * a.nx, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* lab = a.labels + (size_t)frame * npix;
    int rank[LB_CHUNKS], roots = 0;
#pragma unroll
    for (int c = 0; c < LB_CHUNKS; ++c) {
        const int p = scan_pixel(c);
        const bool root = p < npix && lab[p] == p;
        const unsigned long long ball = __ballot(root);
        rank[c] = root ? roots + __popcll(ball & ((1ull << lane) - 1ull)) : -1;
        roots += __popcll(ball);
    }
    if (lane == 0) cnt[wave] = roots;
    __syncthreads();
    int before = a.partial[(size_t)frame * a.nblk + blockIdx.x];
    for (int w = 0; w < wave; ++w) before += cnt[w];
#pragma unroll
    for (int c = 0; c < LB_CHUNKS; ++c)
        if (rank[c] >= 0) lab[scan_pixel(c)] = lb_code(before + rank[c] + 1);
}

// grid (nblk, frames): a pixel's own word is a link to its root, a code (it is a root) or LB_BACKGROUND
__global__ void __launch_bounds__(LB_THREADS) k_label_final(LbArgs a, int frame0) {
    const int frame = frame0 + blockIdx.y, npix = a.ny * a.nx;
    int32_t* lab = a.labels + (size_t)frame * npix;
    GlobalMem m{lab};
    for (int c = 0; c < LB_CHUNKS; ++c) {
        const int p = scan_pixel(c);
        if (p < npix) lab[p] = lb_final(m, lab[p]);
    }
}

// ------------------------------------------------------------------------------------------------------------ region properties
struct RpArgs {
    const float* frames;
    const int32_t* labels;
    const int32_t* off;   // DEVICE copy of the offsets (batch + 1)
    int batch, ny, nx, n_total;
    double background, saturation;
    int* box;             // (n_total, 4): first row, last row, first column, last column
    int* big;             // regions left to k_rp_big, in no particular order
    int* nbig;
    double* out;
};

__global__ void k_rp_init(RpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *a.nbig = 0;
    if (i < a.n_total) {
        a.box[4 * i] = INT_MAX;
        a.box[4 * i + 1] = INT_MIN;
        a.box[4 * i + 2] = INT_MAX;
        a.box[4 * i + 3] = INT_MIN;
    }
}

// grid (ceil(npix / 256), frames).  A region's first row is reached at a pixel whose upper neighbour is not of the region, and so on:
// only the pixels on the outline of a region touch its four words.  Inside a wave the outline pixels that share the label of the
// first of them are joined by a butterfly first and that lane sends their four values; the others send their own.  (Sent one by
// one, the outline of a percolating cluster is millions of atomics on one address: 18 ms a frame at 2048^2.)
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__global__ void __launch_bounds__(256) k_rp_boxes(RpArgs a, int frame0) {
    const int frame = frame0 + blockIdx.y, npix = a.ny * a.nx, lane = threadIdx.x & 63;
    const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;
    const int p = pl < npix ? (int)pl : 0, y = p / a.nx, x = p - y * a.nx;
    const int32_t* lab = a.labels + (size_t)frame * npix;
    const int o = a.off[frame], n = a.off[frame + 1] - o, l = pl < npix ? lab[p] : 0;
    const bool in = l >= 1 && l <= n;
    const bool up = in && (y == 0 || lab[p - a.nx] != l), down = in && (y == a.ny - 1 || lab[p + a.nx] != l);
    const bool left = in && (x == 0 || lab[p - 1] != l), right = in && (x == a.nx - 1 || lab[p + 1] != l);
    const bool any = up || down || left || right;
    const unsigned long long todo = __ballot(any);
    if (!todo) return;                                    // the whole wave
    const int lead = __ffsll((long long)todo) - 1;
    const bool mine = any && l == __shfl(l, lead, 64);
    const int y0 = wave_min_int(mine && up ? y : INT_MAX), y1 = -wave_min_int(mine && down ? -y : INT_MAX);
    const int x0 = wave_min_int(mine && left ? x : INT_MAX), x1 = -wave_min_int(mine && right ? -x : INT_MAX);
    if (!any) return;
    int* b = a.box + 4 * (size_t)(o + l - 1);
    if (lane == lead) {
        if (y0 != INT_MAX) atomicMin(b, y0);
        if (y1 != -INT_MAX) atomicMax(b + 1, y1);
        if (x0 != INT_MAX) atomicMin(b + 2, x0);
        if (x1 != -INT_MAX) atomicMax(b + 3, x1);
    } else if (!mine) {
        if (up) atomicMin(b, y);
        if (down) atomicMax(b + 1, y);
        if (left) atomicMin(b + 2, x);
        if (right) atomicMax(b + 3, x);
    }
}

// first pass over a box: counts, integer coordinate sums, value sums about the box corner, minimum, first maximum
struct RpAcc {
    int n, n_nan, n_sat, mi;
    long long sr, sc;
    double sum, flux, fy, fx;
    float mn, mx;
    __device__ __forceinline__ void merge(const RpAcc& o) {   // o holds pixels later in the order than this
        n += o.n;
        n_nan += o.n_nan;
        n_sat += o.n_sat;
        sr += o.sr;
        sc += o.sc;
        sum += o.sum;
        flux += o.flux;
        fy += o.fy;
        fx += o.fx;
        mn = fminf(mn, o.mn);
        argmax_merge(mx, mi, o.mx, o.mi);
    }
    __device__ __forceinline__ RpAcc across(int o) const {
        RpAcc r;
        r.n = __shfl_xor(n, o, 64);
        r.n_nan = __shfl_xor(n_nan, o, 64);
        r.n_sat = __shfl_xor(n_sat, o, 64);
        r.mi = __shfl_xor(mi, o, 64);
        r.sr = __shfl_xor(sr, o, 64);
        r.sc = __shfl_xor(sc, o, 64);
        r.sum = __shfl_xor(sum, o, 64);
        r.flux = __shfl_xor(flux, o, 64);
        r.fy = __shfl_xor(fy, o, 64);
        r.fx = __shfl_xor(fx, o, 64);
        r.mn = __shfl_xor(mn, o, 64);
        r.mx = __shfl_xor(mx, o, 64);
        return r;
    }
};
struct RpMom {   // second pass: moments about the weighted centroid
    double yy, xx, yx;
    __device__ __forceinline__ void merge(const RpMom& o) {
        yy += o.yy;
        xx += o.xx;
        yx += o.yx;
    }
    __device__ __forceinline__ RpMom across(int o) const {
        return RpMom{__shfl_xor(yy, o, 64), __shfl_xor(xx, o, 64), __shfl_xor(yx, o, 64)};
    }
};

// Every lane returns the merged value: the butterfly of b4d_reduce.hpp's "all" forms inside a wave (both partners merge the same
// two values: sums, fminf and the arg-max rule are symmetric), then, for a workgroup, the waves in order from wave 0.
template <int NT, class A>
__device__ __forceinline__ A rp_reduce(A v, A* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v.merge(v.across(o));
    if (NT > 64) {
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        v = sh[0];
        for (int w = 1; w < NT / 64; ++w) v.merge(sh[w]);
        __syncthreads();
    }
    return v;
}

// The pixels p = tid, tid + NT, .. of an h x w box in row-major order (p = r * w + c), RP_UNROLL at a time: x = load(r, c) for
// each of them first, so that their loads are in flight together, then use(x, r, c, p) in the order of p.
constexpr int RP_UNROLL = 4;
template <int NT, class Load, class Use>
__device__ __forceinline__ void walk_box(int h, int w, int tid, Load load, Use use) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const int dq = NT / w, dr = NT - dq * w;
    int r = tid / w, c = tid - r * w;
    for (unsigned p = tid; p < n; p += NT * RP_UNROLL) {
        int rr[RP_UNROLL], cc[RP_UNROLL];
        decltype(load(0, 0)) x[RP_UNROLL];
#pragma unroll
        for (int u = 0; u < RP_UNROLL; ++u) {
            rr[u] = r;
            cc[u] = c;
            if (p + (unsigned)(u * NT) < n) x[u] = load(r, c);
            c += dr;
            r += dq;
            if (c >= w) {
                c -= w;
                ++r;
            }
        }
#pragma unroll
        for (int u = 0; u < RP_UNROLL; ++u)
            if (p + (unsigned)(u * NT) < n) use(x[u], rr[u], cc[u], (int)(p + (unsigned)(u * NT)));
    }
}

struct RpPixel {
    int label;
    float v;
};

constexpr int RP_BIG_THREADS = 512;
union RpShared {
    RpAcc acc[RP_BIG_THREADS / 64];
    RpMom mom[RP_BIG_THREADS / 64];
};

// One region by NT lanes (tid = 0 .. NT - 1): lane p takes the box pixels p, p + NT, .. in row-major order, in that order.
template <int NT>
__device__ __forceinline__ void rp_measure(const RpArgs& a, int idx, int frame, int tid, RpShared* sh) {
    const int* b = a.box + 4 * (size_t)idx;
    const int y0 = b[0], x0 = b[2], h = b[1] - y0 + 1, w = b[3] - x0 + 1, L = idx - a.off[frame] + 1;
    const size_t first = ((size_t)frame * a.ny + y0) * a.nx + x0;
    const int32_t* lab = a.labels + first;
    const float* frm = a.frames ? a.frames + first : nullptr;
    const bool sat_on = a.saturation < INFINITY;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    RpAcc s{};
    s.mi = INT_MAX;
    s.mn = INFINITY;
    s.mx = -INFINITY;
    // the value is loaded with the label, member or not: the two loads do not wait for each other
    const auto load = [&](int r, int c) __attribute__((always_inline)) {
        const size_t g = (size_t)r * a.nx + c;
        return RpPixel{lab[g], frm ? frm[g] : 0.f};
    };
    walk_box<NT>(h, w, tid, load, [&](RpPixel x, int r, int c, int p) __attribute__((always_inline)) {
        if (x.label != L) return;
        ++s.n;
        s.sr += r;
        s.sc += c;
        if (!frm) return;
        const float v = x.v;
        if (v != v) {
            ++s.n_nan;
            return;
        }
        const double d = (double)v, wgt = fmax(d - a.background, 0.0);
        s.n_sat += sat_on && d >= a.saturation ? 1 : 0;
        s.sum += d;
        s.flux += wgt;
        s.fy += wgt * (double)r;
        s.fx += wgt * (double)c;
        s.mn = fminf(s.mn, v);
        argmax_merge(s.mx, s.mi, v, p);
    });
    s = rp_reduce<NT>(s, sh->acc);

    const bool valued = frm && s.n > s.n_nan, lit = valued && s.flux > 0.0;
    const double wr = lit ? s.fy / s.flux : nan, wc = lit ? s.fx / s.flux : nan;
    RpMom q{0.0, 0.0, 0.0};
    if (lit) {
        walk_box<NT>(h, w, tid, load, [&](RpPixel x, int r, int c, int) __attribute__((always_inline)) {
            if (x.label != L) return;
            const double wgt = fmax((double)x.v - a.background, 0.0);
            if (!(wgt > 0.0)) return;     // nothing to add, and false for a NaN
            const double ey = (double)r - wr, ex = (double)c - wc;
            q.yy += wgt * ey * ey;
            q.xx += wgt * ex * ex;
            q.yx += wgt * ey * ex;
        });
        q = rp_reduce<NT>(q, sh->mom);
    }
    if (tid == 0) {
        double* o = a.out + (size_t)idx * RP_NQ;
        const int pr = valued ? s.mi / w : 0, pc = valued ? s.mi - pr * w : 0;
        o[0] = (double)s.n;
        o[1] = (double)y0;
        o[2] = (double)(y0 + h);
        o[3] = (double)x0;
        o[4] = (double)(x0 + w);
        o[5] = (double)y0 + (double)s.sr / (double)s.n;
        o[6] = (double)x0 + (double)s.sc / (double)s.n;
        o[7] = frm ? s.sum : nan;
        o[8] = valued ? (double)s.mn : nan;
        o[9] = valued ? (double)s.mx : nan;
        o[10] = valued ? (double)(y0 + pr) : -1.0;
        o[11] = valued ? (double)(x0 + pc) : -1.0;
        o[12] = frm ? s.flux : nan;
        o[13] = lit ? (double)y0 + wr : nan;
        o[14] = lit ? (double)x0 + wc : nan;
        o[15] = lit ? q.yy / s.flux : nan;
        o[16] = lit ? q.xx / s.flux : nan;
        o[17] = lit ? q.yx / s.flux : nan;
        o[18] = (double)s.n_nan;
        o[19] = (double)s.n_sat;
    }
}

// the frame of row idx of the table: the last f with off[f] <= idx
__device__ __forceinline__ int rp_frame_of(const int32_t* off, int batch, int idx) {
    int lo = 0, hi = batch - 1;
    while (lo < hi) {               // at most 31 rounds: the interval halves
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// a label without a pixel: area 0, an empty box at the origin, no centroid and no value
__device__ __forceinline__ void rp_empty_row(const RpArgs& a, int idx) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* o = a.out + (size_t)idx * RP_NQ;
    for (int k = 0; k < RP_NQ; ++k) o[k] = 0.0;
    o[5] = o[6] = o[8] = o[9] = o[13] = o[14] = o[15] = o[16] = o[17] = nan;
    o[10] = o[11] = -1.0;
    if (!a.frames) o[7] = o[12] = nan;
}

// grid (ceil(n_total / 4)): one wave per region
__global__ void __launch_bounds__(256) k_rp_small(RpArgs a) {
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= a.n_total) return;
    const int* b = a.box + 4 * (size_t)idx;
    if (b[0] > b[1]) {
        if (lane == 0) rp_empty_row(a, idx);
        return;
    }
    if ((long long)(b[1] - b[0] + 1) * (b[3] - b[2] + 1) > RP_WAVE_AREA) {
        if (lane == 0) a.big[atomicAdd(a.nbig, 1)] = idx;
        return;
    }
    rp_measure<64>(a, idx, rp_frame_of(a.off, a.batch, idx), lane, nullptr);
}

// any grid: workgroup g takes the entries g, g + gridDim.x, .. of the list
__global__ void __launch_bounds__(RP_BIG_THREADS) k_rp_big(RpArgs a) {
    __shared__ RpShared sh;
    const int n = *a.nbig;
    for (int s = blockIdx.x; s < n; s += gridDim.x) {
        const int idx = a.big[s];
        rp_measure<RP_BIG_THREADS>(a, idx, rp_frame_of(a.off, a.batch, idx), threadIdx.x, &sh);
    }
}

// grid (ceil(npix / 256), frames)
__global__ void __launch_bounds__(256) k_relabel(const int32_t* labels, const int32_t* off, const int32_t* map, int32_t* out, int npix,
                                                 int frame0) {
    const int frame = frame0 + blockIdx.y;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const size_t g = (size_t)frame * npix + p;
    const int o = off[frame], n = off[frame + 1] - o, l = labels[g];
    out[g] = l >= 1 && l <= n ? map[o + l - 1] : 0;
}

// HOST offsets: off[0] == 0, ascending; returns their end in *n_total
int check_offsets(const char* fn, const int32_t* off, int batch, int* n_total) {
    if (off[0] != 0) return fail(B4D_EINVAL, std::string(fn) + ": offsets[0] must be 0");
    for (int t = 0; t < batch; ++t)
        if (off[t + 1] < off[t]) return fail(B4D_EINVAL, std::string(fn) + ": offsets must ascend");
    *n_total = off[batch];
    return B4D_OK;
}

}  // namespace
}  // namespace b4d

using namespace b4d;

extern "C" int b4d_label_regions(const float* frames, const float* thresholds, const unsigned char* mask, int batch, int ny, int nx,
                                 int connectivity, int32_t* labels, int32_t* n_regions, void* stream) {
    if ((frames != nullptr) == (mask != nullptr)) return fail(B4D_EINVAL, "b4d_label_regions: exactly one of frames and mask");
    if ((frames && !thresholds) || !labels || !n_regions) return fail(B4D_EINVAL, "b4d_label_regions: null pointer");
    if (batch < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "b4d_label_regions: batch or frame empty");
    if (connectivity != 1 && connectivity != 2) return fail(B4D_EINVAL, "b4d_label_regions: connectivity must be 1 or 2");
    if ((long long)ny * nx >= (1LL << 31) - LB_SCAN) return fail(B4D_ESIZE, "b4d_label_regions: 2^31 - 2048 or more pixels per frame");
    if (!ptr_aligned(frames, 4) || !ptr_aligned(thresholds, 4) || !ptr_aligned(labels, 4) || !ptr_aligned(n_regions, 4))
        return fail(B4D_EINVAL, "b4d_label_regions: frames, thresholds, labels and n_regions on 4 bytes");
    const int npix = ny * nx, nblk = (int)(((long long)npix + LB_SCAN - 1) / LB_SCAN);
    const unsigned tx = tiles(nx, LB_TX), ty = tiles(ny, LB_TY);
    if (ty > 65535u) return fail(B4D_ESIZE, "b4d_label_regions: more than 65535 tile rows");

    hipStream_t st = (hipStream_t)stream;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    if (const int rc = get_scratch(256 + sizeof(int) * (size_t)batch * nblk, &scratch, st)) return rc;
    LbArgs a{};
    a.frames = frames;
    a.thresholds = thresholds;
    a.mask = mask;
    a.labels = labels;
    a.n_regions = n_regions;
    a.ny = ny;
    a.nx = nx;
    a.conn = connectivity;
    a.nblk = nblk;
    a.err = static_cast<int*>(scratch);
    a.partial = a.err + 64;
    B4D_HIP(hipMemsetAsync(a.err, 0, sizeof(int), st));

    const int hs = (ny - 1) / LB_TY, vs = (nx - 1) / LB_TX;
    const long long seam = (long long)hs * nx + (long long)vs * ny;
    const dim3 blk(LB_THREADS);
    return for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        if (const int rc = launch(k_label_tile, dim3(tx, ty, nb), blk, 0, st, a, b0)) return rc;
        if (seam)
            if (const int rc = launch(k_label_seams, dim3((unsigned)((seam + LB_THREADS - 1) / LB_THREADS), nb), blk, 0, st, a, b0, hs, vs))
                return rc;
        if (const int rc = launch(k_label_flatten, dim3(nblk, nb), blk, 0, st, a, b0)) return rc;
        if (const int rc = launch(k_label_scan, dim3(nb), blk, 0, st, a, b0)) return rc;
        if (const int rc = launch(k_label_assign, dim3(nblk, nb), blk, 0, st, a, b0)) return rc;
        return launch(k_label_final, dim3(nblk, nb), blk, 0, st, a, b0);
    });
}

extern "C" int b4d_region_properties(const float* frames, const int32_t* labels, int batch, int ny, int nx, const int32_t* offsets,
                                     double background, double saturation, double* out, void* stream) {
    if (!labels || !offsets) return fail(B4D_EINVAL, "b4d_region_properties: null pointer");
    if (batch < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "b4d_region_properties: batch or frame empty");
    if ((long long)ny * nx >= (1LL << 31)) return fail(B4D_ESIZE, "b4d_region_properties: 2^31 or more pixels per frame");
    if (!std::isfinite(background)) return fail(B4D_EINVAL, "b4d_region_properties: background must be finite");
    if (saturation != saturation) return fail(B4D_EINVAL, "b4d_region_properties: saturation is NaN");
    if (!ptr_aligned(frames, 4) || !ptr_aligned(labels, 4) || !ptr_aligned(out, 8))
        return fail(B4D_EINVAL, "b4d_region_properties: frames and labels on 4 bytes, out on 8");
    int n_total = 0;
    if (const int rc = check_offsets("b4d_region_properties", offsets, batch, &n_total)) return rc;
    if (n_total == 0) return B4D_OK;
    if (!out) return fail(B4D_EINVAL, "b4d_region_properties: null pointer");

    hipStream_t st = (hipStream_t)stream;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    const size_t off_bytes = align256(sizeof(int32_t) * ((size_t)batch + 1));
    if (const int rc = get_scratch(off_bytes + 256 + sizeof(int) * 5 * (size_t)n_total, &scratch, st)) return rc;
    char* base = static_cast<char*>(scratch);
    B4D_HIP(hipMemcpyAsync(base, offsets, sizeof(int32_t) * ((size_t)batch + 1), hipMemcpyHostToDevice, st));
    RpArgs a{};
    a.frames = frames;
    a.labels = labels;
    a.off = reinterpret_cast<const int32_t*>(base);
    a.batch = batch;
    a.ny = ny;
    a.nx = nx;
    a.n_total = n_total;
    a.background = background;
    a.saturation = saturation;
    a.nbig = reinterpret_cast<int*>(base + off_bytes);
    a.box = a.nbig + 64;
    a.big = a.box + 4 * (size_t)n_total;
    a.out = out;

    const unsigned pix_blocks = (unsigned)(((long long)ny * nx + 255) / 256);
    if (const int rc = launch(k_rp_init, dim3((n_total + 255) / 256), dim3(256), 0, st, a)) return rc;
    if (const int rc = for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
            return launch(k_rp_boxes, dim3(pix_blocks, nb), dim3(256), 0, st, a, b0);
        }))
        return rc;
    if (const int rc = launch(k_rp_small, dim3((n_total + 3) / 4), dim3(256), 0, st, a)) return rc;
    return launch(k_rp_big, dim3(std::min(n_total, 2048)), dim3(RP_BIG_THREADS), 0, st, a);
}

extern "C" int b4d_relabel(const int32_t* labels, int batch, int ny, int nx, const int32_t* offsets, const int32_t* map, int32_t* out,
                           void* stream) {
    if (!labels || !offsets || !out) return fail(B4D_EINVAL, "b4d_relabel: null pointer");
    if (batch < 1 || ny < 1 || nx < 1) return fail(B4D_EINVAL, "b4d_relabel: batch or frame empty");
    if ((long long)ny * nx >= (1LL << 31)) return fail(B4D_ESIZE, "b4d_relabel: 2^31 or more pixels per frame");
    if (!ptr_aligned(labels, 4) || !ptr_aligned(map, 4) || !ptr_aligned(out, 4)) return fail(B4D_EINVAL, "b4d_relabel: pointers on 4 bytes");
    int n_total = 0;
    if (const int rc = check_offsets("b4d_relabel", offsets, batch, &n_total)) return rc;
    if (n_total > 0 && !map) return fail(B4D_EINVAL, "b4d_relabel: null pointer");

    hipStream_t st = (hipStream_t)stream;
    B4D_SCRATCH_LOCK();
    void* scratch = nullptr;
    if (const int rc = get_scratch(sizeof(int32_t) * ((size_t)batch + 1), &scratch, st)) return rc;
    B4D_HIP(hipMemcpyAsync(scratch, offsets, sizeof(int32_t) * ((size_t)batch + 1), hipMemcpyHostToDevice, st));
    const unsigned pix_blocks = (unsigned)(((long long)ny * nx + 255) / 256);
    return for_frame_chunks(batch, MAX_GRID_FRAMES, [&](int b0, int nb) {
        return launch(k_relabel, dim3(pix_blocks, nb), dim3(256), 0, st, labels, static_cast<const int32_t*>(scratch), map, out, ny * nx, b0);
    });
}
