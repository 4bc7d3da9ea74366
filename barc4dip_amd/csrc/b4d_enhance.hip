// b4d_enhance.hip -- contrast-limited adaptive histogram equalisation (CLAHE), global histogram equalisation and tile histograms
// of float32 frames (include/b4d.h "Histogram equalisation").  Three entry points, three kernels:
//   b4d_tile_histogram  k_tile_hist  one workgroup per (tile, bin slice): integer LDS atomics on replicated copies, plain stores out
//   b4d_equalize_lut    k_lut        one workgroup per tile: clip total, redistribution, block scan, 16-bit table
//   b4d_lut_apply       k_apply      quantise, gather four table entries, interpolate, epilogue
// Every count is an integer and every float32 operation is rounded on its own (no contraction in this unit), so a frame gives the
// same bits alone and inside any batch.  No float atomics, no inline assembly, no environment settings.
#include "b4d_common.hpp"
#include "b4d_reduce.hpp"

// Plain operators below, never the __f*_rn wrappers: those are inlined from a header compiled ahead of this pragma and fuse.
#pragma clang fp contract(off)

namespace b4d {
namespace {

constexpr int MAX_LEVELS = 65536;
constexpr int MAX_TILES = 4096;
constexpr int MAX_BATCH = 65535;         // frames are a grid dimension
constexpr int MAX_TILE_AREA = 1 << 24;   // the cumulative counts stay exact in float32
constexpr int SLICE_BINS = 32768;        // bins one workgroup counts: 128 KiB of the CU's 160 KiB of LDS
constexpr int HIST_THREADS = 512;
constexpr int APPLY_THREADS = 256;
constexpr int APPLY_ROWS = 16;           // rows per workgroup of k_apply: the column terms of a lane serve that many pixels each

// tiles of one axis: `side` pixels extended by pad = (tiles - side % tiles) % tiles reflected ones, tile = (side + pad) / tiles
struct Axis {
    int side, tiles, tile;
};
__host__ __device__ inline int reflect_src(int e, int side) { return e < side ? e : 2 * (side - 1) - e; }

// bin of a non-NaN pixel: clamp(floor((x - lo) * s), 0, L - 1), clamped as a float so that +-Inf and products beyond the int
// range take the end bins (a NaN product, 0 * Inf, takes bin 0)
__device__ __forceinline__ int quantise(float x, float lo, float s, float top) {
    const float f = floorf((x - lo) * s);
    return !(f > 0.0f) ? 0 : (f >= top ? (int)top : (int)f);
}

// ----------------------------------------------------------------------------------------------------------- tile histograms
// grid (slices, tiles, batch).  hist: rep copies of `sbins` words; lane l counts into copy l % rep.  A row of the tile is split
// into units: float4 groups of the in-frame columns from the first 16-byte boundary on, then single pixels (the columns in front
// of that boundary, behind the last whole group, and the reflected ones).  lpr lanes (a power of two) share a row.
__global__ void __launch_bounds__(HIST_THREADS) k_tile_hist(const float* __restrict__ in, const float4* __restrict__ qp, Axis ay, Axis ax,
                                                            int L, int sbins, int rep, int lpr_log2, int base_mod4,
                                                            unsigned* __restrict__ counts, unsigned* __restrict__ n_valid) {
    extern __shared__ __align__(16) unsigned hist[];
    __shared__ unsigned s_valid;
    const int slice = blockIdx.x, tile = blockIdx.y, frame = blockIdx.z;
    const int tyi = tile / ax.tiles, txi = tile - tyi * ax.tiles;
    const int b0 = slice * sbins, nb = min(L - b0, sbins);
    for (int i = threadIdx.x; i < rep * sbins; i += HIST_THREADS) hist[i] = 0;
    if (threadIdx.x == 0) s_valid = 0;
    __syncthreads();

    const float4 q = qp[frame];
    const float lo = q.x, s = q.y, top = (float)(L - 1);
    const float* img = in + (size_t)frame * ay.side * ax.side;
    const int frame_mod4 = (int)((base_mod4 + (size_t)frame * ay.side * ax.side) & 3);
    unsigned* my = hist + (threadIdx.x % rep) * sbins;
    unsigned valid = 0;
    auto visit = [&](float x) {
        if (x != x) return;
        ++valid;
        const unsigned b = (unsigned)(quantise(x, lo, s, top) - b0);
        if (b < (unsigned)nb) atomicAdd(&my[b], 1u);
    };

    const int c0 = txi * ax.tile, c1 = c0 + ax.tile;            // extended columns of the tile
    const int cin = max(min(c1, ax.side) - c0, 0);               // in-frame columns
    const int lpr = 1 << lpr_log2, sub = threadIdx.x & (lpr - 1);
    for (int r = threadIdx.x >> lpr_log2; r < ay.tile; r += HIST_THREADS >> lpr_log2) {
        const int sy = reflect_src(tyi * ay.tile + r, ay.side);
        const float* row = img + (size_t)sy * ax.side;
        const int mis = (int)((frame_mod4 + (size_t)sy * ax.side + c0) & 3);      // elements past a 16-byte boundary
        const int head = min((4 - mis) & 3, cin), body = (cin - head) >> 2, tail = cin - head - 4 * body;
        const int units = body + head + tail + (ax.tile - cin);
        for (int u = sub; u < units; u += lpr) {
            if (u < body) {
                const float4 a = *reinterpret_cast<const float4*>(row + c0 + head + 4 * u);
                visit(a.x); visit(a.y); visit(a.z); visit(a.w);
            } else {
                const int j = u - body;
                int c;
                if (j < head) c = c0 + j;
                else if (j < head + tail) c = c0 + head + 4 * body + (j - head);
                else c = reflect_src(c0 + cin + (j - head - tail), ax.side);
                visit(row[c]);
            }
        }
    }
    valid = wave_sum(valid);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_valid, valid);
    __syncthreads();
    unsigned* out = counts + ((size_t)frame * gridDim.y + tile) * L + b0;
    for (int i = threadIdx.x; i < nb; i += HIST_THREADS) {
        unsigned t = hist[i];
        for (int k = 1; k < rep; ++k) t += hist[k * sbins + i];
        out[i] = t;
    }
    if (slice == 0 && threadIdx.x == 0) n_valid[(size_t)frame * gridDim.y + tile] = s_valid;
}

// ----------------------------------------------------------------------------------------------------------- tables
// Exclusive prefix of v over the workgroup (thread order) plus carry; carry (the same in every thread) grows by the workgroup's
// total.  sh: one word per wave.  Two barriers; the whole workgroup calls.
__device__ __forceinline__ unsigned block_scan_exclusive(unsigned v, unsigned* sh, unsigned& carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned incl = wave_scan_inclusive(v, lane);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    unsigned before = carry, total = 0;
    for (int w = 0; w < nw; ++w) {
        const unsigned t = sh[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();
    carry += total;
    return before + incl - v;
}
// sum (IS_MIN: minimum) of v over the workgroup, in every thread.  sh: one word per wave.  Two barriers.
template <bool IS_MIN>
__device__ __forceinline__ unsigned block_fold(unsigned v, unsigned* sh) {
    v = IS_MIN ? wave_min_all(v) : wave_sum_all(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned t = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = IS_MIN ? min(t, sh[w]) : t + sh[w];
    __syncthreads();
    return t;
}

// grid (tiles, batch).  mode 0: the CLAHE table of every tile; mode 1: the equalize_hist table (one tile per frame), and
// unchanged[frame] = 1 where every valid pixel falls into one bin (or none is valid).  Thread t takes the bins 4 t .. 4 t + 3 of
// every run of 4 * blockDim.x bins.
__global__ void __launch_bounds__(1024) k_lut(const unsigned* __restrict__ counts, const unsigned* __restrict__ n_valid, int L,
                                              double clip_limit, int mode, unsigned short* __restrict__ lut, int* __restrict__ unchanged) {
    __shared__ unsigned sh[16];
    const size_t t = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned* h = counts + t * L;
    unsigned short* out = lut + t * L;
    const unsigned n = n_valid[t];
    const int run = 4 * blockDim.x;
    if (mode == 1 && threadIdx.x == 0) unchanged[blockIdx.y] = 0;
    if (n == 0) {      // identity table
        for (int i = threadIdx.x; i < L; i += blockDim.x) out[i] = (unsigned short)i;
        if (mode == 1 && threadIdx.x == 0) unchanged[blockIdx.y] = 1;
        return;
    }
    unsigned clip = 0, add_all = 0, residual = 0, step = 1, first = 0;
    float scale;
    if (mode == 0) {
        if (clip_limit > 0.0) {
            const double c = clip_limit * (double)n / (double)L;
            clip = c >= (double)n ? n : max((unsigned)c, 1u);
            unsigned excess = 0;
            for (int i = threadIdx.x; i < L; i += blockDim.x) {
                const unsigned v = h[i];
                excess += v > clip ? v - clip : 0u;
            }
            excess = block_fold<false>(excess, sh);
            add_all = excess / (unsigned)L;
            residual = excess - add_all * (unsigned)L;
            if (residual > 0) step = max((unsigned)L / residual, 1u);
        }
        scale = (float)(L - 1) / (float)n;
    } else {
        unsigned i0 = 0xffffffffu;
        for (int i = threadIdx.x; i < L; i += blockDim.x)
            if (h[i] != 0) i0 = min(i0, (unsigned)i);
        first = block_fold<true>(i0, sh);
        const unsigned h0 = h[first];
        if (h0 == n) {
            for (int i = threadIdx.x; i < L; i += blockDim.x) out[i] = (unsigned short)i;
            if (threadIdx.x == 0) unchanged[blockIdx.y] = 1;
            return;
        }
        scale = (float)(L - 1) / (float)(n - h0);
    }
    const float top = (float)(L - 1);
    unsigned carry = 0;
    for (int base = 0; base < L; base += run) {
        unsigned v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned i = base + 4 * threadIdx.x + k;
            unsigned c = 0;
            if (i < (unsigned)L) {
                c = h[i];
                if (mode == 0) {
                    if (clip > 0) c = min(c, clip) + add_all + ((residual > 0 && i % step == 0 && i / step < residual) ? 1u : 0u);
                } else if (i <= first) {
                    c = 0;
                }
            }
            v[k] = c;
            sum += c;
        }
        unsigned cum = block_scan_exclusive(sum, sh, carry);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned i = base + 4 * threadIdx.x + k;
            cum += v[k];
            if (i < (unsigned)L) out[i] = (unsigned short)fminf(fmaxf(rintf((float)cum * scale), 0.0f), top);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- apply
struct Term {      // one pixel's interpolation terms along an axis: the two tiles and their weights
    int t0, t1;
    float a, a1;
};
__device__ __forceinline__ Term axis_term(int p, float inv, int tiles) {
    const float f = (float)p * inv - 0.5f;
    const float fl = floorf(f);
    const int t = (int)fl;
    Term r;
    r.a = f - fl;
    r.a1 = 1.0f - r.a;
    r.t0 = max(t, 0);
    r.t1 = min(t + 1, tiles - 1);
    return r;
}

// grid (ceil(nx / (4 * APPLY_THREADS)), ceil(ny / APPLY_ROWS), batch).  A lane keeps four consecutive columns over APPLY_ROWS
// rows: the column terms are formed once per lane, the row terms once per row.  VEC: 16-byte loads and stores (nx % 4 == 0, both
// pointers on 16 bytes).  flags bit 0: float epilogue res * inv + lo (else rint and clamp); bit 1: lut[bin] without interpolation.
template <bool VEC>
__global__ void __launch_bounds__(APPLY_THREADS) k_apply(const float* __restrict__ in, const float4* __restrict__ qp, int ny, int nx, int tiles_y,
                                                         int tiles_x, float inv_h, float inv_w, int L, const unsigned short* __restrict__ lut,
                                                         const int* __restrict__ unchanged, int flags, float* __restrict__ out) {
    const int frame = blockIdx.z;
    const int x0 = 4 * (blockIdx.x * APPLY_THREADS + threadIdx.x);
    if (x0 >= nx) return;
    const int y0 = blockIdx.y * APPLY_ROWS, y1 = min(y0 + APPLY_ROWS, ny);
    const float4 q = qp[frame];
    const float lo = q.x, s = q.y, inv = q.z, top = (float)(L - 1);
    const bool direct = (flags & 2) != 0, scaled = (flags & 1) != 0;
    const bool copy = s == 0.0f || (direct && unchanged && unchanged[frame]);
    const int ncol = min(4, nx - x0);
    Term cx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = axis_term(x0 + k, inv_w, tiles_x);
    const unsigned short* flut = lut + (size_t)frame * tiles_y * tiles_x * L;
    for (int y = y0; y < y1; ++y) {
        const size_t off = ((size_t)frame * ny + y) * nx + x0;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(in + off);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < ncol) v[k] = in[off + k];
        }
        if (!copy) {
            const Term ry = axis_term(y, inv_h, tiles_y);
            const unsigned short* r0 = flut + (size_t)ry.t0 * tiles_x * L;
            const unsigned short* r1 = flut + (size_t)ry.t1 * tiles_x * L;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = v[k];
                if (x != x || k >= ncol) continue;
                const int bin = quantise(x, lo, s, top);
                float res;
                if (direct) {
                    res = (float)flut[bin];
                } else {
                    const size_t o0 = (size_t)cx[k].t0 * L + bin, o1 = (size_t)cx[k].t1 * L + bin;
                    const float v11 = (float)r0[o0], v12 = (float)r0[o1], v21 = (float)r1[o0], v22 = (float)r1[o1];
                    const float up = v11 * cx[k].a1 + v12 * cx[k].a;
                    const float dn = v21 * cx[k].a1 + v22 * cx[k].a;
                    res = up * ry.a1 + dn * ry.a;
                }
                v[k] = scaled ? res * inv + lo : fminf(fmaxf(rintf(res), 0.0f), top);
            }
        }
        if (VEC) {
            *reinterpret_cast<float4*>(out + off) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < ncol) out[off + k] = v[k];
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- host side
int check_axis(int side, int tiles, Axis* a, const char* name) {
    if (side < 1) return fail(B4D_EINVAL, std::string("enhance: empty ") + name + " axis");
    if (tiles < 1) return fail(B4D_EINVAL, std::string("enhance: tiles along ") + name + " must be >= 1");
    const int pad = (tiles - side % tiles) % tiles;
    if (pad > side - 1)
        return fail(B4D_EINVAL, std::string("enhance: the ") + name + " axis would be extended by more reflected pixels than it has less one");
    a->side = side;
    a->tiles = tiles;
    a->tile = (side + pad) / tiles;
    return B4D_OK;
}

int check_geometry(int batch, int ny, int nx, int tiles_y, int tiles_x, int levels, Axis* ay, Axis* ax) {
    if (batch < 1) return fail(B4D_EINVAL, "enhance: batch < 1");
    if (batch > MAX_BATCH) return fail(B4D_ESIZE, "enhance: more than 65535 frames in one call");
    if (levels < 2 || levels > MAX_LEVELS) return fail(B4D_ESIZE, "enhance: levels must be 2 .. 65536");
    if (ny >= 1 && nx >= 1 && (long long)ny * nx >= (1ll << 31)) return fail(B4D_ESIZE, "enhance: ny * nx >= 2^31");
    if (const int rc = check_axis(ny, tiles_y, ay, "y")) return rc;
    if (const int rc = check_axis(nx, tiles_x, ax, "x")) return rc;
    if ((long long)tiles_y * tiles_x > MAX_TILES) return fail(B4D_ESIZE, "enhance: more than 4096 tiles");
    if ((long long)ay->tile * ax->tile > MAX_TILE_AREA) return fail(B4D_ESIZE, "enhance: a tile of more than 2^24 pixels");
    return B4D_OK;
}

}  // namespace
}  // namespace b4d

using namespace b4d;

extern "C" int b4d_tile_histogram(const float* in, int batch, int ny, int nx, int tiles_x, int tiles_y, int levels, const float* qparams,
                                  unsigned* counts, unsigned* n_valid, void* stream) {
    if (!in || !qparams || !counts || !n_valid) return fail(B4D_EINVAL, "b4d_tile_histogram: null pointer");
    Axis ay, ax;
    if (const int rc = check_geometry(batch, ny, nx, tiles_y, tiles_x, levels, &ay, &ax)) return rc;
    if (!ptr_aligned(in, 4) || !ptr_aligned(qparams, 16)) return fail(B4D_EINVAL, "b4d_tile_histogram: in on 4 bytes, qparams on 16");
    const int slices = (levels + SLICE_BINS - 1) / SLICE_BINS;
    const int sbins = slices > 1 ? SLICE_BINS : levels;
    const int rep = slices > 1 ? 1 : std::max(1, std::min(16, 8192 / levels));
    int lpr_log2 = 0;      // lanes per tile row: the power of two at or above the float4 groups of a row plus its ragged ends
    while ((1 << lpr_log2) < ax.tile / 4 + 3 && lpr_log2 < 6) ++lpr_log2;
    const int base_mod4 = (int)((reinterpret_cast<uintptr_t>(in) >> 2) & 3);
    return launch(k_tile_hist, dim3(slices, tiles_y * tiles_x, batch), dim3(HIST_THREADS), (size_t)rep * sbins * sizeof(unsigned),
                  (hipStream_t)stream, in, reinterpret_cast<const float4*>(qparams), ay, ax, levels, sbins, rep, lpr_log2, base_mod4, counts,
                  n_valid);
}

extern "C" int b4d_equalize_lut(const unsigned* counts, const unsigned* n_valid, int batch, int tiles, int levels, double clip_limit, int mode,
                                unsigned short* lut, int* unchanged, void* stream) {
    if (!counts || !n_valid || !lut) return fail(B4D_EINVAL, "b4d_equalize_lut: null pointer");
    if (batch < 1 || tiles < 1) return fail(B4D_EINVAL, "b4d_equalize_lut: batch < 1 or tiles < 1");
    if (levels < 2 || levels > MAX_LEVELS) return fail(B4D_ESIZE, "b4d_equalize_lut: levels must be 2 .. 65536");
    if (tiles > MAX_TILES || batch > MAX_BATCH) return fail(B4D_ESIZE, "b4d_equalize_lut: more than 4096 tiles or 65535 frames");
    if (mode != 0 && mode != 1) return fail(B4D_EINVAL, "b4d_equalize_lut: mode must be 0 (CLAHE) or 1 (equalize_hist)");
    if (!(clip_limit >= 0.0)) return fail(B4D_EINVAL, "b4d_equalize_lut: clip_limit must be >= 0");
    if (mode == 1 && (tiles != 1 || !unchanged)) return fail(B4D_EINVAL, "b4d_equalize_lut: mode 1 takes one tile per frame and `unchanged`");
    const int threads = levels <= 1024 ? 256 : 1024;
    return launch(k_lut, dim3(tiles, batch), dim3(threads), 0, (hipStream_t)stream, counts, n_valid, levels, clip_limit, mode, lut, unchanged);
}

extern "C" int b4d_lut_apply(const float* in, int batch, int ny, int nx, int tiles_x, int tiles_y, int levels, const float* qparams,
                             const unsigned short* lut, const int* unchanged, int flags, float* out, void* stream) {
    if (!in || !qparams || !lut || !out) return fail(B4D_EINVAL, "b4d_lut_apply: null pointer");
    Axis ay, ax;
    if (const int rc = check_geometry(batch, ny, nx, tiles_y, tiles_x, levels, &ay, &ax)) return rc;
    if (flags & ~3) return fail(B4D_EINVAL, "b4d_lut_apply: flags out of range");
    if ((flags & 2) && tiles_y * tiles_x != 1) return fail(B4D_EINVAL, "b4d_lut_apply: flags bit 1 (no interpolation) takes one tile per frame");
    if (!ptr_aligned(in, 4) || !ptr_aligned(out, 4) || !ptr_aligned(qparams, 16)) return fail(B4D_EINVAL, "b4d_lut_apply: in / out on 4 bytes, qparams on 16");
    const size_t bytes = (size_t)batch * ny * nx * sizeof(float);
    if (ranges_overlap(in, bytes, out, bytes)) return fail(B4D_EINVAL, "b4d_lut_apply: in and out overlap");
    const float inv_h = 1.0f / (float)ay.tile, inv_w = 1.0f / (float)ax.tile;
    const dim3 grid((nx + 4 * APPLY_THREADS - 1) / (4 * APPLY_THREADS), (ny + APPLY_ROWS - 1) / APPLY_ROWS, batch);
    const bool vec = nx % 4 == 0 && ptr_aligned(in, 16) && ptr_aligned(out, 16);
    return launch(vec ? k_apply<true> : k_apply<false>, grid, dim3(APPLY_THREADS), 0, (hipStream_t)stream, in,
                  reinterpret_cast<const float4*>(qparams), ny, nx, tiles_y, tiles_x, inv_h, inv_w, levels, lut, unchanged, flags, out);
}
