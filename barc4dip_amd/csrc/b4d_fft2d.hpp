// b4d_fft2d.hpp -- batched 2-D real FFT pipeline kernels (row R2C, fused column, row C2R), the plan
// object and the launch dispatchers.  Included by the translation units that launch them
// (b4d_kernels.hip: fft2d / psd2d / autocorr2d; b4d_track.hip: xcorr2d / phase correlation).
//
// Data flow for a batch of real (ny, nx) frames ("rows first"):
//
//   K1 row_r2c   two real rows are packed as one complex row (z = a + i b), one FFT of length nx,
//                Hermitian split -> half spectra of both rows, kx = 0..nx/2-1, written in a
//                column-tile-major layout: tile ct holds CT adjacent kx for all ny rows contiguously
//                ([ct][y][c]), so that K2 streams whole tiles.  The (real) Nyquist bin kx = nx/2 of every
//                row goes to a small side array (batch, ny) handled by k_nyq.
//   K2 col       one workgroup owns a tile (CT = 16 columns x ny rows, 256 KiB at 2048^2) entirely in
//                registers: forward FFT along y, |F|^2 (PSD written shifted, with its Hermitian mirror),
//                inverse FFT along y of the power spectrum, written back in place.  Fusing forward and
//                inverse column passes removes one full read+write of the spectrum (SURVEY.md §8d counts
//                4 passes); two REAL power columns share one complex inverse transform.
//   k_nyq        the same for the single Nyquist column of each frame (1/1024 of the work).
//   K3 row_c2r   rebuilds the two-row packing from the half spectra, one inverse FFT of length nx,
//                shift + normalise -> two autocorrelation rows.
//
//
// "ysplit" route (PSD + autocorrelation of 2048-row frames; option "ysplit" of b4d_set_option): the row passes
// do one radix-2 stage of the column transform each, at no extra byte or launch.  With h = ny/2, w = exp(-2 pi i / ny):
//   K1 row_r2c   transform p packs rows p and p + h; their half spectra A, B leave as A + B (even ky) and (A - B) w^p (odd ky),
//                layout [frame][parity][ct][p][c] with 32-column tiles (the same bytes: two tile sets of h rows).
//   K2 col       a workgroup owns a PARITY tile (32 columns x h rows, the same 256 KiB): the h-point transform gives F(2k + parity),
//                PSD rows ky = 2k + parity are whole 128-B lines (+ mirror), the inverse gives E (even) or O (odd), rows 0..h/2 kept.
//   K3 row_c2r   transform y in [0, h/2] reads row y of E and O, G(y) = E + conj(w^y) O and G(h - y) = conj(E - conj(w^y) O) ride
//                the two-row packing; rows y, h - y and their point mirrors are written, every row once.
//   k_nyq        unchanged (K1 still stores the plain Nyquist bins of both rows).
// "colsets" (with "row16", nx <= 2048): between K1 and K2 a parity tile is laid out [n][e][cp][h] -- 16 bytes hold
// rows n and n + h/2 of ONE column -- so that K2 has its first register set complete after half of its loads; K2 writes the tile back
// in the plain form, K3 and k_nyq see no difference.
//
// All of them are HBM-bandwidth bound; see DESIGN.md for the byte accounting.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/b4d.h"
#include "b4d_common.hpp"
#include "b4d_fft.hpp"
#include "b4d_lanes.hpp"
#include "b4d_peak.hpp"

// Translation units that build a kernel with their own compiler flags (b4d_passes.hpp) define B4D_UNIT_TAG before including
// this header: the tag is a template argument of the kernels they launch, so that their instantiations are symbols of their
// own -- two units instantiating the SAME kernel name share one host-side stub, and which unit's device code a launch then
// runs is decided by registration order, not by the caller.
#ifndef B4D_UNIT_TAG
#define B4D_UNIT_TAG 0
#endif
// Which launch dispatchers a unit compiles (bit mask).  Every kernel a dispatcher names is instantiated in the including unit, with
// THAT unit's flags, under a symbol the other units share unless it carries the tag: a unit built with flags of its own therefore
// compiles only the pass it exists for (b4d_colpass.hip: the column pass, b4d_rowout.hip: the inverse row pass), so that no kernel
// symbol has two different device codes in the library (`make check-symbols`).
#define B4D_PASS_R2C 1
#define B4D_PASS_COL 2
#define B4D_PASS_NYQ 4
#define B4D_PASS_C2R 8
#ifndef B4D_UNIT_PASSES
#define B4D_UNIT_PASSES (B4D_PASS_R2C | B4D_PASS_COL | B4D_PASS_NYQ | B4D_PASS_C2R)
#endif

namespace b4d {

constexpr int E16 = 16;

typedef float f32x2 __attribute__((ext_vector_type(2)));   // plain vector values for accesses through address-space pointers
typedef float f32x4 __attribute__((ext_vector_type(4)));

// radix plans: N = 16 * R2 * R3 with 16 points per lane
constexpr int radix2(int n) { return n / 16 < 16 ? n / 16 : 16; }
constexpr int radix3(int n) { return n / (16 * radix2(n)); }
template <int N>
using RowGeom = FftGeom<N, E16, 16, radix2(N), radix3(N), 1>;
template <int N, int CI>
using ColGeom = FftGeom<N, E16, 16, radix2(N), radix3(N), CI>;
// single transforms (two image rows, or one Nyquist column) per workgroup: 256 lanes, fewer where the
// 64 KiB static LDS limit binds
constexpr int row_seq(int n) { return n == 4096 ? 1 : (n == 64 ? 32 : 256 / (n / 16)); }

// spectrum element index in the tile-major layout
__device__ __forceinline__ size_t spec_index(size_t frame, int nt, int ny, int ct_w, int y, int kx) {
    return ((frame * nt + (kx / ct_w)) * (size_t)ny + y) * ct_w + (kx % ct_w);
}

// the same index for power-of-two tile widths (16, or 8 at ny = 4096; always the case) with shifts and a 24-bit multiply: uniform
// part (frame) in 64 bits, lane part in 32 bits (< ny nx / 2 <= 2^23)
__device__ __forceinline__ size_t spec_index_pow2(size_t frame, int nt, int ny, int ct_w, int y, int kx) {
    const int cs = __builtin_ctz(ct_w);
    const unsigned lane = ((__umul24((unsigned)kx >> cs, (unsigned)ny) + (unsigned)y) << cs) + ((unsigned)kx & (unsigned)(ct_w - 1));
    return ((frame * nt * (size_t)ny) << cs) + lane;
}

// c = a * conj(b), optionally whitened: c / (|c| + eps)   (signal/tracking.py:280-281)
template <bool WHITEN>
__device__ __forceinline__ float2 cross_power(float2 a, float2 b, float eps) {
    float2 c = make_float2(fmaf(a.x, b.x, a.y * b.y), fmaf(a.y, b.x, -a.x * b.y));
    if (WHITEN) {
        // hardware square root and reciprocal (1 ulp each) and two multiplies: the IEEE sqrtf and the two divisions this replaces
        // were ~35 of the ~70 vector instructions the cross-power column pass spends per element (half of k_col_prod's stream)
        const float inv = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(fmaf(c.x, c.x, c.y * c.y)) + eps);
        c.x *= inv;
        c.y *= inv;
    }
    return c;
}

// ------------------------------------------------------------------------------------ K1
// Optional per-item source descriptor (tracking): item b reads frame `frame` of the input, only
// inside the ROI [y0,y1) x [x0,x1) (zero elsewhere), z-scored as (x - mean) / denom
// (signal/tracking.py:308-311 + geometry/roi.py:175-222 embed_roi with fill 0).
struct RowSrc {
    int frame, y0, y1, x0, x1;
    float mean, denom;
    int pad;
};

// grid (ceil(ny/2/(SEQ*ITER)), batch); block T*SEQ.  ct_w = tile width (complex columns) of the spectrum layout.
// ITER > 1 (full frames only): a workgroup transforms ITER consecutive groups of SEQ row pairs and issues the loads of ALL of
// them before the first transform -- ITER x the bytes in flight per workgroup at the same LDS footprint (the exchange buffer,
// not the register file, caps this kernel at four workgroups per CU).
#ifndef B4D_K1_ITER
#define B4D_K1_ITER 1
#endif
// YS ("ysplit" route, ny = 2048): transform p packs rows p and p + ny/2 and applies the first radix-2 stage of the COLUMN
// transform to their half spectra A, B: A + B -> row p of the even-ky tile set, (A - B) w^p -> row p of the odd one
// (w^p = tw_y[p], uniform per transform).  Layout [frame][parity][ct][p][c], ct_w columns per tile.
// W16 (YS only; "row16" of b4d_set_option): 16-byte stores.  The Hermitian split reads every bin from the exchange buffer, so the
// lane that stores a bin need not be the lane that transformed it: lane u splits bins k, k + 1, k = 2(u + T j), j < 4, and stores
// 16 bytes into the even and into the odd tile row (8 instead of 16 stores per lane, whole lines per wave instruction).  Same
// expressions, same values bit for bit; needs a 16-byte-aligned workspace (launch_r2c).  The loads stay one dword per lane: 16-byte
// loads, redistributed through the buffer or by quad transposes, were measured and dropped.
// CS (W16 only; "colsets" of b4d_set_option): the column-set tile layout [n][e][cp][h]: 16 bytes of a 32-column parity
// tile hold rows n and n + ny/4 of ONE column 2 cp + e.  The SEQ transforms of a workgroup are SEQ/2 couples, pairs q and q + ny/4;
// after every transform has written its bins to its buffer (a workgroup barrier: the partner may sit in another wave) the 2T lanes of
// a couple split bin k of BOTH transforms, each with its own w^pair, and store 16 bytes = (q, q + ny/4) into the even and into the odd
// tile: 4 bins and 8 stores per lane as with W16 alone, 16 consecutive lanes per 256-byte (n, e) run.  Same expressions per bin.
template <int NX, int SEQ, bool SRC, int ITER = 1, bool YS = false, bool W16 = false, bool CS = false>
__global__ void __launch_bounds__((NX / E16) * SEQ)
k_row_r2c(const float* __restrict__ in, float2* __restrict__ spec, float* __restrict__ nyq_rows,
          const float2* __restrict__ tw, int ny, int ct_w, const RowSrc* __restrict__ srcs, const float2* __restrict__ tw_y) {
    using G = RowGeom<NX>;
    constexpr int T = G::T, E = E16;
    constexpr bool WV = T <= 64;   // one transform = (part of) one wavefront: no workgroup barriers (fft_sync)
    static_assert(ITER == 1 || !SRC, "ROI sources run one group per workgroup");
    static_assert(!YS || !SRC, "the ysplit pairing takes full frames");
    static_assert(!W16 || YS, "16-byte stores: parity-tile route only");
    static_assert(!W16 || G::LDS_ELEMS % 2 == 0, "16-byte accesses to each transform's buffer");
    static_assert(!CS || (W16 && ITER == 1 && SEQ % 2 == 0), "column sets: couples of transforms, one group per workgroup");
    __shared__ __attribute__((aligned(16))) float2 lds_all[SEQ * G::LDS_ELEMS];
    const int seq = threadIdx.x / T, u = threadIdx.x % T;
    const size_t frame = blockIdx.y;
    if (SRC) {   // rows outside the ROI are zero: a workgroup without a ROI row writes NOTHING -- the column pass and k_nyq
                 // know the ROI rows (ColArgs::srcs / NyqArgs::srcs) and never read the others (a 121-px template in a
                 // 1024^2 frame: 88 % of the half spectrum is neither written here nor read there)
        const int wa = 2 * blockIdx.x * SEQ, wb = wa + 2 * SEQ;
        if (wb <= srcs[frame].y0 || wa >= srcs[frame].y1) return;
    }
    float2* lds = lds_all + seq * G::LDS_ELEMS;
    // CS with ONE couple per workgroup (nx = 2048): a workgroup reads four rows ny/4 apart where the two transforms of a plain workgroup
    // read two runs of two adjacent rows, and that alone cost the pass 7 %.  Workgroups b and b + 8 -- dealt to the
    // same XCD one after the other -- take the adjacent couples q, q + 1 instead.  Speed only: a bijection of the grid.
    int bx = blockIdx.x;
    if (CS && SEQ == 2 && gridDim.x % 16 == 0) bx = (bx & ~15) + 2 * (bx & 7) + ((bx >> 3) & 1);
    float2 va[ITER][E];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        float2(&v)[E] = va[it];
        // CS: transforms seq and seq + SEQ/2 are a couple, pairs q and q + ny/4
        const int pair = CS ? bx * (SEQ / 2) + seq % (SEQ / 2) + (ny / 4) * (seq / (SEQ / 2)) : (blockIdx.x * ITER + it) * SEQ + seq;
        const bool live = 2 * pair < ny;  // ragged last workgroup: idle transforms still take part in the barriers
        if (!live) {
#pragma unroll
            for (int j = 0; j < E; ++j) v[j] = make_float2(0.f, 0.f);
        } else if (SRC) {
            const RowSrc sd = srcs[frame];
            const int ya = 2 * pair, yb = ya + 1;
            const bool ina = ya >= sd.y0 && ya < sd.y1, inb = yb >= sd.y0 && yb < sd.y1;
            const float* r0 = in + ((size_t)sd.frame * ny + ya) * NX;
            const float* r1 = r0 + NX;
            const float inv = 1.0f / sd.denom;   // one division per item instead of 32 per lane (z-score: signal/tracking.py:308-311)
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int x = u + T * j;
                const bool inx = x >= sd.x0 && x < sd.x1;
                v[j].x = (ina && inx) ? (r0[x] - sd.mean) * inv : 0.f;
                v[j].y = (inb && inx) ? (r1[x] - sd.mean) * inv : 0.f;
            }
        } else {
            const float* r0 = in + (frame * ny + (YS ? 1 : 2) * (size_t)pair) * NX;
            const float* r1 = r0 + (YS ? (size_t)(ny / 2) * NX : (size_t)NX);
#pragma unroll
            for (int j = 0; j < E; ++j) v[j] = make_float2(r0[u + T * j], r1[u + T * j]);
        }
    }
    const int nt = (NX / 2) / ct_w;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        float2(&v)[E] = va[it];
        const int pair = CS ? bx * (SEQ / 2) + seq % (SEQ / 2) + (ny / 4) * (seq / (SEQ / 2)) : (blockIdx.x * ITER + it) * SEQ + seq;
        const bool live = 2 * pair < ny;
        if (it > 0) fft_sync<WV>();   // the previous group's Hermitian split has read the buffer
        Fft3<G, 1, WV>::run(v, v, u, 0, lds, tw);
        fft_sync<WV>();
#pragma unroll
        for (int j = 0; j < E; ++j) lds[u + T * j] = v[j];
        if (CS) {
            constexpr int H = SEQ / 2, L = 2 * T, CW = 32;   // couples per workgroup, lanes per couple, columns per parity tile
            static_assert((NX / 2) % CW == 0 && (NX / 2) / L == 4, "four bins per lane, whole tiles");
            const int sq = seq % H, q = bx * H + sq, m0 = u + T * (seq / H);
            const bool both = q < ny / 4;   // a couple is live or idle as a whole
            const float2* lp[2] = {lds_all + sq * G::LDS_ELEMS, lds_all + (sq + H) * G::LDS_ELEMS};
            const int pr[2] = {q, q + ny / 4};
            float2 wp2[2] = {make_float2(1.f, 0.f), make_float2(1.f, 0.f)};
            if (both) {
                wp2[0] = tw_y[pr[0]];
                wp2[1] = tw_y[pr[1]];
            }
            __syncthreads();   // every path, idle transforms included: the partner's bins are read below
            if (both) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + L * i;   // slot (tile, e, cp) of the lane: m = 32 tile + 16 e + cp
                    const int k = (m & ~(CW - 1)) + 2 * (m & 15) + ((m >> 4) & 1);   // bin = column 2 cp + e of that tile
                    float2 ev[2], od[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float2 z = lp[h][k], zr = lp[h][(NX - k) & (NX - 1)];
                        float2 a = make_float2(0.5f * (z.x + zr.x), 0.5f * (z.y - zr.y));
                        float2 b = make_float2(0.5f * (z.y + zr.y), 0.5f * (zr.x - z.x));
                        if (k == 0) {  // DC bins are real; the (real) Nyquist bins of both rows go to the side array
                            const float2 zn = lp[h][NX / 2];
                            a = make_float2(z.x, 0.f);
                            b = make_float2(z.y, 0.f);
                            nyq_rows[frame * ny + pr[h]] = zn.x;
                            nyq_rows[frame * ny + pr[h] + ny / 2] = zn.y;
                        }
                        ev[h] = cadd(a, b);
                        od[h] = cmul(csub(a, b), wp2[h]);
                    }
                    // tile row n = q: 64 elements [e][cp][h], this lane's 16 bytes at 2 (16 e + cp)
                    const size_t o = ((2 * frame * nt + (m / CW)) * (size_t)(ny / 2)) * CW + (size_t)q * (2 * CW) + 2 * (m & (CW - 1));
                    *reinterpret_cast<f32x4*>(spec + o) = f32x4{ev[0].x, ev[0].y, ev[1].x, ev[1].y};
                    *reinterpret_cast<f32x4*>(spec + o + (size_t)(ny / 2) * (NX / 2)) = f32x4{od[0].x, od[0].y, od[1].x, od[1].y};
                }
            }
            continue;
        }
        fft_sync<WV>();
        if (W16) {
            if (live) {
                const float2 wp = tw_y[pair];
                const f32x4* l4 = reinterpret_cast<const f32x4*>(lds);
#pragma unroll
                for (int j = 0; j < E / 4; ++j) {
                    const int k = 2 * (u + T * j);
                    const f32x4 zz = l4[u + T * j];   // bins k, k + 1
                    const float2 z2[2] = {make_float2(zz.x, zz.y), make_float2(zz.z, zz.w)};
                    const float2 zr2[2] = {lds[(NX - k) & (NX - 1)], lds[NX - k - 1]};
                    float2 ev[2], od[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float2 z = z2[h], zr = zr2[h];
                        float2 a = make_float2(0.5f * (z.x + zr.x), 0.5f * (z.y - zr.y));
                        float2 b = make_float2(0.5f * (z.y + zr.y), 0.5f * (zr.x - z.x));
                        if (h == 0 && k == 0) {  // DC bins are real; the (real) Nyquist bins of both rows go to the side array
                            const float2 zn = lds[NX / 2];
                            a = make_float2(z.x, 0.f);
                            b = make_float2(z.y, 0.f);
                            nyq_rows[frame * ny + pair] = zn.x;
                            nyq_rows[frame * ny + pair + ny / 2] = zn.y;
                        }
                        ev[h] = cadd(a, b);
                        od[h] = cmul(csub(a, b), wp);
                    }
                    const size_t o = spec_index(2 * frame, nt, ny / 2, ct_w, pair, k);
                    *reinterpret_cast<f32x4*>(spec + o) = f32x4{ev[0].x, ev[0].y, ev[1].x, ev[1].y};
                    *reinterpret_cast<f32x4*>(spec + o + (size_t)(ny / 2) * (NX / 2)) = f32x4{od[0].x, od[0].y, od[1].x, od[1].y};
                }
            }
        } else if (live) {
            float2 wp = make_float2(1.f, 0.f);
            if (YS) wp = tw_y[pair];
#pragma unroll
            for (int j = 0; j < E / 2; ++j) {
                const int k = u + T * j;
                const float2 z = v[j], zr = lds[(NX - k) & (NX - 1)];
                float2 a = make_float2(0.5f * (z.x + zr.x), 0.5f * (z.y - zr.y));
                float2 b = make_float2(0.5f * (z.y + zr.y), 0.5f * (zr.x - z.x));
                if (k == 0) {  // DC bins are real; the (real) Nyquist bins of both rows go to the side array
                    const float2 zn = lds[NX / 2];
                    a = make_float2(z.x, 0.f);
                    b = make_float2(z.y, 0.f);
                    nyq_rows[frame * ny + (YS ? pair : 2 * pair)] = zn.x;
                    nyq_rows[frame * ny + (YS ? pair + ny / 2 : 2 * pair + 1)] = zn.y;
                }
                if (YS) {
                    const size_t o = spec_index(2 * frame, nt, ny / 2, ct_w, pair, k);
                    spec[o] = cadd(a, b);
                    spec[o + (size_t)(ny / 2) * (NX / 2)] = cmul(csub(a, b), wp);  // same row of the odd-ky tile set
                } else {
                    const size_t o = spec_index(frame, nt, ny, ct_w, 2 * pair, k);
                    spec[o] = a;
                    spec[o + ct_w] = b;  // next row of the same tile
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ K2
enum ColMode { COL_PSD_AC = 0, COL_FORWARD = 2 };   // (1 was the round-2 full-spectrum store: b4d_spectrum.hip replaced it)

struct ColArgs {
    float2* spec;     // tile-major half spectra, in/out
    float* psd;       // (batch, ny, nx) or null
    const float2* tw;
    const float2* tw_inv;  // the SAME table through a second, formally unrelated pointer: keeps the compiler from
                           // holding the forward pass's 30 twiddles in registers (or scratch) for the inverse pass
    float psd_scale;
    int nx;
    unsigned flags;
    int half_rows;    // COL_PSD_AC: the consumer uses R[-y,-x] = R[y,x]: only rows 0..ny/2+1 of the tile are stored
    const RowSrc* srcs;  // COL_FORWARD, optional: item i holds data in rows [srcs[i].y0, srcs[i].y1) only (zero-embedded ROI);
                         // the other rows are taken as zero WITHOUT being read (k_row_r2c does not write them)
#ifdef B4D_DIAG
    unsigned long long* diag;  // diagnostic build only: 8 s_memtime stamps per workgroup
#endif
};

#ifdef B4D_DIAG
// Diagnostic build (never shipped, never timed as a whole): phase stamps of wave 0 of each workgroup.
#define B4D_STAMP(i)                                                                              \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        unsigned long long t__;                                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");              \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (p.diag && threadIdx.x == 0) p.diag[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = t__; \
    } while (0)
#ifdef B4D_DIAG_DRAIN   // additionally separate issue from completion (perturbs the kernel: every phase waits for its memory traffic)
#define B4D_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define B4D_DRAIN() do {} while (0)
#endif
#else
#define B4D_STAMP(i) do {} while (0)
#define B4D_DRAIN() do {} while (0)
#endif

// Column-tile geometry: a lane holds NC = 2 adjacent columns (one 16-byte load per row), CPT lanes span the
// tile (CT = NC*CPT columns = whole 128-B lines per row at CT = 16), T = NY/16 lanes run along y.
//   NY <= 2048: CPT = 8 -> CT = 16; at 2048 the 256-KiB tile lives in the registers of 1024 lanes (16 waves,
//               <= 128 VGPRs each: 64 of data + butterflies; 4 waves per SIMD hide the LDS / twiddle latencies --
//               measured 1.23x faster than 512 lanes x 4 columns at 2 waves per SIMD)
//   NY == 4096: CPT = 4 -> CT = 8 (a 16-column tile would need the whole register file)
// __launch_bounds__(THREADS, 4) caps every variant at 128 VGPRs so that smaller NY run several workgroups per CU.
// YS ("ysplit" route of 2048-row frames, NY = 1024 here): the row passes do one radix-2 stage of the column transform, a
// workgroup owns one PARITY tile (the even or the odd ky of CT columns): CPT = 16 -> CT = 32 columns x 1024 rows, the same
// 256 KiB in 1024 lanes, whole 128-B lines in every direct PSD store.  (16-column parity tiles, 512 lanes and two workgroups
// per CU, were measured 20 % slower on the column pass: DESIGN.md §8.1.)
template <int NY, int YS = 0>
struct ColCfg {
    static constexpr int NC = 2;
    static constexpr int CPT = (NY == 4096 ? 4 : 8) * (YS ? 2 : 1);
    static constexpr int CT = NC * CPT;   // columns per tile
    static constexpr int THREADS = CPT * (NY / E16);
    static constexpr int WAVES_PER_EU = THREADS >= 256 ? 4 : 1;
    using G = ColGeom<NY, CPT>;
    static constexpr size_t LDS_BYTES = sizeof(float2) * (size_t)G::LDS_ELEMS * CPT;   // one exchange region (132 KiB at NY = 2048)
};

#define B4D_GLOBAL __attribute__((address_space(1)))
// Address = uniform base + 32-bit BYTE offset of the lane: the form global_load/store take with the base in SGPRs and ONE offset
// VGPR.  With element indices the compiler cannot fold the scaling into a 32-bit offset (it could wrap) and builds 64-bit
// per-lane addresses: two VGPRs each, kept live across the transforms at the 128-register cap of the 1024-lane kernels.
template <class V>
__device__ __forceinline__ V B4D_GLOBAL* at_bytes(void* base, unsigned boff) {
    return (V B4D_GLOBAL*)((char B4D_GLOBAL*)base + boff);
}
template <class V>
__device__ __forceinline__ const V B4D_GLOBAL* at_bytes(const void* base, unsigned boff) {
    return (const V B4D_GLOBAL*)((const char B4D_GLOBAL*)base + boff);
}
// a uniform pointer pinned in an SGPR pair and opaque to reassociation: `sgpr_base(p + const) + lane offset` stays
// "scalar base + 32-bit lane offset" instead of being folded into a 64-bit per-lane address plus constants
template <class V>
__device__ __forceinline__ V* sgpr_base(V* p) {
    asm volatile("" : "+s"(p));
    return p;
}

template <int NC>
__device__ __forceinline__ void store_cols(float2* __restrict__ rowp, const float2 (&c)[NC]) {
#pragma unroll
    for (int h = 0; h < NC / 2; ++h)
        *reinterpret_cast<float4*>(rowp + 2 * h) = make_float4(c[2 * h].x, c[2 * h].y, c[2 * h + 1].x, c[2 * h + 1].y);
}

// grid (nt, batch), block ColCfg<NY>::THREADS.
// CS (YS only; "colsets" of b4d_set_option): the tile comes in the column-set layout [n][e][cp][h] of k_row_r2c<.., CS>: one 16-byte
// load holds rows n and n + NY/2 of column 2 cp + e, i.e. v[e][j] and v[e][j + 8].  The eight loads of set 0 are issued by EVERY wave
// (a workgroup barrier that leaves them in flight) ahead of the eight of set 1, so set 0 is complete after half of the tile and goes
// through stage 1 ... exchange 2 while set 1 lands (Fft3::run_sets_staged).  For that no twiddle may queue behind set 1's loads: every
// lane loads one entry of the 1024-point table and one of the 64 stage-2 values first of all and puts them into LDS behind the
// exchange region before that barrier; the tables stay there, and the inverse transform reads its twiddles from them as well.  The
// direct PSD stores (whole lines) are non-temporal.  The tile is written back in the plain [row][column] form (every lane has read
// all of it by then), so the inverse row pass and k_nyq do not change.  Bit-identical to CS = 0.
template <int NY, int MODE, int UNIT = 0, int YS = 0, int CS = 0>
__global__ void __launch_bounds__((ColCfg<NY, YS>::THREADS), (ColCfg<NY, YS>::WAVES_PER_EU)) k_col(ColArgs p) {
    using Cfg = ColCfg<NY, YS>;
    static_assert(YS == 0 || MODE == COL_PSD_AC, "parity tiles: fused PSD + autocorrelation pass only");
    static_assert(CS == 0 || (YS && NY == 1024), "column sets: 1024-row parity tiles");
    static_assert(Cfg::NC == 2, "two columns per lane: one 16-byte load / store per row, one 8-byte PSD store");
    constexpr int NYF = YS ? 2 * NY : NY;   // rows of the frame (YS: this workgroup transforms every second ky of them)
    using G = typename Cfg::G;
    constexpr int T = G::T, E = E16, NC = Cfg::NC, CPT = Cfg::CPT, CT = Cfg::CT;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int cp = threadIdx.x % CPT, u = threadIdx.x / CPT;
    const int nt = gridDim.x;
    // Workgroups are dealt round-robin over the 8 XCDs (linear workgroup id % 8).  Neighbouring column tiles write
    // the two 64-B halves of every 128-B PSD line and share the 64-B sectors of the Hermitian-mirror stores (the
    // mirror of 16 aligned columns is misaligned by one float): those merge only in a common L2.  With batch % 8 == 0
    // every tile of frame f runs on XCD f % 8 (measured -6% on the 2048^2 kernel against per-XCD tile ranges, which
    // leave one tile boundary in eight split across two L2s); otherwise each XCD takes a contiguous tile range.
    // Speed only: any placement is correct.
    int ct, fr;
    if (gridDim.y % 8 == 0) {
        const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, k = lin / 8;
        fr = 8 * (k / gridDim.x) + lin % 8;
        ct = k % gridDim.x;
    } else {
        ct = (nt % 8 == 0) ? (blockIdx.x % 8) * (nt / 8) + blockIdx.x / 8 : blockIdx.x;
        fr = blockIdx.y;
    }
    // YS: slots [0, nt/2) are the even-ky tiles of the frame, [nt/2, nt) the odd-ky ones ([parity][ct] is the tile order in memory)
    const int par = (YS && ct >= nt / 2) ? 1 : 0;
    const int ctx = YS ? ct - par * (nt / 2) : ct;   // column tile
    const size_t frame = fr;
    const int nx = p.nx;
    float2* tile = p.spec + ((frame * nt + ct) * (size_t)NY) * CT;
    const unsigned toff = (unsigned)u * CT + NC * cp;  // element offset of (row u, first column of this lane)
    float2 v[NC][E];
    B4D_STAMP(0);
    int ry0 = 0, ry1 = NY;
    if (MODE == COL_FORWARD && p.srcs) {
        ry0 = p.srcs[fr].y0;
        ry1 = p.srcs[fr].y1;
    }
    if constexpr (CS != 0) {
        static_assert(NC == 2 && T == 64 && Cfg::THREADS == NY, "two sets of eight 16-byte loads; one entry of the stage-1 table per lane");
        float2* tws = lds + (size_t)G::LDS_ELEMS * CPT;   // stage-2 twiddles: entry q2 R3 + m1 = tw[R1 m1 q2]
        float2* tab = tws + G::M;                         // the whole table tw[i], i < NY, for stage 1
        const float2 t1 = p.tw[threadIdx.x];
        const float2 t2 = p.tw[G::R1 * ((threadIdx.x % G::R3) * (threadIdx.x / G::R3 % G::R2))];
        const unsigned toffc = ((unsigned)u * 2 * CT + 2 * cp) * 8u;   // byte offset of (row u, e = 0, cp, h = 0)
#pragma unroll
        for (int s = 0; s < NC; ++s) {
#pragma unroll
            for (int j = 0; j < E / 2; ++j) {
                const f32x4 q = *at_bytes<f32x4>(sgpr_base(tile + (size_t)(T * j * 2 * CT + s * CT)), toffc);
                v[s][j] = make_float2(q.x, q.y);
                v[s][j + E / 2] = make_float2(q.z, q.w);
            }
            if (s == 0) {   // the memory pipe sees set 0 of all waves ahead of any load of set 1; the loads stay in flight across it
                if (threadIdx.x < G::M) tws[threadIdx.x] = t2;
                tab[threadIdx.x] = t1;   // waits for the two oldest loads of the queue only
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // set 1's loads are issued here, not where the scheduler finds room for their registers
    } else {
#pragma unroll
        for (int h = 0; h < NC / 2; ++h) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                if (MODE == COL_FORWARD) {   // clamped row + select: the load stays unconditional (no branch per load), rows outside
                                             // the ROI re-read a ROI row that other lanes fetch anyway
                    const int ky = u + T * j, kc = min(max(ky, ry0), ry1 - 1);
                    float4 q = *reinterpret_cast<const float4*>(tile + (size_t)kc * CT + NC * cp + 2 * h);
                    if (ky < ry0 || ky >= ry1) q = make_float4(0.f, 0.f, 0.f, 0.f);
                    v[2 * h][j] = make_float2(q.x, q.y);
                    v[2 * h + 1][j] = make_float2(q.z, q.w);
                } else {
                    const f32x4 q = *at_bytes<f32x4>(sgpr_base(tile + (size_t)(T * j * CT) + 2 * h), toff * 8u);
                    v[2 * h][j] = make_float2(q.x, q.y);
                    v[2 * h + 1][j] = make_float2(q.z, q.w);
                }
            }
        }
    }
    B4D_DRAIN();
    B4D_STAMP(1);
    if constexpr (CS != 0)
        Fft3<G, 1>::template run_sets_staged<NC>(v, u, cp, lds, lds + (size_t)G::LDS_ELEMS * CPT, lds + (size_t)G::LDS_ELEMS * CPT + G::M);
    else
        Fft3<G, 1>::template run_sets<NC, MODE != COL_PSD_AC>(v, u, cp, lds, p.tw);
    B4D_STAMP(2);
    // v[c][j] = F[ky = u + T j][kx0 + c]   (COL_PSD_AC: after the stage-3 butterflies done below)
    const int kx0 = ctx * CT + NC * cp;

    if (MODE == COL_FORWARD) {  // keep the 2-D half spectrum in the tile
        // laundered offset: otherwise the 16 store addresses (= the load addresses) stay live in 32 registers across the
        // whole transform and the radix stages spill (8 dwords at 512 rows ... 28 at 4096)
        unsigned toff3 = toff;
        asm volatile("" : "+v"(toff3));
#pragma unroll
        for (int j = 0; j < E; ++j) {
            float2 c[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) c[k] = v[k][j];
            store_cols<NC>(tile + (size_t)(T * j * CT) + toff3, c);
        }
        return;
    }

    // ---- COL_PSD_AC: power spectrum, optional PSD store (direct + Hermitian mirror), inverse transform.
    // Two REAL power columns ride one complex transform (Pa + i Pb), separated afterwards with the
    // Hermitian symmetry in y: half the butterflies and LDS traffic of a column-by-column inverse.
    // The last forward butterflies are interleaved with the |F|^2 epilogue (register pressure), and the
    // row index is laundered so that the 32 store offsets are not precomputed at kernel entry.
    const float s = p.psd_scale;
    float* psd = p.psd ? p.psd + frame * (size_t)NYF * nx : nullptr;
    int uu = u;
    asm volatile("" : "+v"(uu));
    float2 w[NC / 2][E];
    constexpr int B3 = E / G::R3;
#pragma unroll
    for (int a = 0; a < B3; ++a) {
#pragma unroll
        for (int k = 0; k < NC; ++k) Fft3<G, 1>::stage3_one(v[k], a);
#pragma unroll
        for (int q = 0; q < G::R3; ++q) {
            const int j = a + B3 * q;
            const int ky = YS ? 2 * (uu + T * j) + par : uu + T * j;   // row of the frame's spectrum
            float pw[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) pw[k] = v[k][j].x * v[k][j].x + v[k][j].y * v[k][j].y;
            if (psd) {
                const unsigned rd = (unsigned)((ky + NYF / 2) & (NYF - 1)) * nx, rm = (unsigned)((NYF / 2 - ky) & (NYF - 1)) * nx;
                // direct half.  Column sets: 16 lanes write one whole aligned 128-byte line that nobody else touches -- streamed past
                // L2 (-2 % on the kernel); the 16-column tiles' half lines meet their other half there and stay cached
                if constexpr (CS != 0)
                    __builtin_nontemporal_store(f32x2{pw[0] * s, pw[1] * s}, at_bytes<f32x2>(psd, (rd + nx / 2 + kx0) * 4u));
                else
                    *at_bytes<f32x2>(psd, (rd + nx / 2 + kx0) * 4u) = f32x2{pw[0] * s, pw[1] * s};
                // Hermitian mirror: columns nx/2 - kx0 - 1, nx/2 - kx0 (column 0 has no mirror).  Two dword stores: ONE 8-byte
                // store on the 4-byte boundary (the mirror of an aligned pair starts one float off) measured +6 % on the kernel.
                // Cached on every route: the dwords merge into sectors in L2
                const unsigned mo = (rm + nx / 2 - kx0 - 1) * 4u;
                *at_bytes<float>(psd, mo) = pw[1] * s;
                if (kx0 >= 1) *at_bytes<float>(psd, mo + 4u) = pw[0] * s;
            }
            // inverse inputs, already (im, re)-swapped so that the forward code inverts: Pa + i Pb -> (Pb, Pa)
#pragma unroll
            for (int h = 0; h < NC / 2; ++h) w[h][j] = make_float2(pw[2 * h + 1], pw[2 * h]);
        }
    }
    B4D_STAMP(3);
    B4D_DRAIN();
    B4D_STAMP(4);
    if (kx0 == 0 && uu == 0 && par == 0 && (p.flags & B4D_REMOVE_MEAN)) w[0][0].y = 0.f;  // DC bin: ky = 0 <-> u = 0, j = 0
    // The lane position is derived AGAIN from the (laundered) thread index: otherwise the compiler keeps the load addresses and
    // the ~40 twiddle / LDS byte offsets of the forward pass alive, or u, cp and the tile offset in three registers where one
    // does -- at the 128-register cap one spilled dword reloaded here would be a scratch load, i.e. a vmcnt(0) that drains
    // every PSD store before the inverse transform may start
    const float2* tw2 = p.tw_inv;
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int cp2 = tid2 % CPT, u2 = tid2 / CPT;
    const unsigned toff2 = (unsigned)u2 * CT + NC * cp2;
    __syncthreads();
    if constexpr (CS != 0) {
        // the two tables are still in LDS behind the exchange region: no twiddle of the inverse queues behind the 48 PSD stores
        // (30 global loads per lane less; the same products, -3 % on the kernel)
        Fft3<G, 1>::template run_sets_staged<NC / 2>(w, u2, cp2, lds, lds + (size_t)G::LDS_ELEMS * CPT,
                                                     lds + (size_t)G::LDS_ELEMS * CPT + G::M);
        Fft3<G, 1>::stage3(w[0]);
    } else {
        Fft3<G, 1>::template run_sets<NC / 2>(w, u2, cp2, lds, tw2);
    }
    B4D_STAMP(5);
    // V[y] = Ga[y] + i Gb[y] with Ga, Gb Hermitian in y: split with V[-y], one set at a time through the exchange region
    float2 vr[NC / 2][E];
#pragma unroll
    for (int h = 0; h < NC / 2; ++h) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < E; ++j) lds[(u2 + T * j) * CPT + cp2] = make_float2(w[h][j].y, w[h][j].x);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < E; ++j) vr[h][j] = lds[((NY - (u2 + T * j)) & (NY - 1)) * CPT + cp2];
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        float2 c[NC];
#pragma unroll
        for (int h = 0; h < NC / 2; ++h) {
            const float2 z = make_float2(w[h][j].y, w[h][j].x), zr = vr[h][j];
            c[2 * h] = make_float2(0.5f * (z.x + zr.x), 0.5f * (z.y - zr.y));
            c[2 * h + 1] = make_float2(0.5f * (z.y + zr.y), 0.5f * (zr.x - z.x));
        }
        // streaming (non-temporal) stores: the tile is read once more, by the row pass, after a gigabyte of other traffic -- kept
        // out of L2 it leaves the cache to the PSD half lines that do meet there (-3 % on this kernel; PSD stores that are half
        // lines or single dwords must stay cached: non-temporal they doubled the kernel)
        // rows the row pass reads: pairs (2q, 2q + 1) up to 2q = NY/2; YS: rows 0 .. NY/2 of both parity tiles
        if (!p.half_rows || u2 + T * j <= (YS ? NY / 2 : NY / 2 + 1)) {
            __builtin_nontemporal_store(f32x4{c[0].x, c[0].y, c[1].x, c[1].y},
                                        (f32x4 B4D_GLOBAL*)at_bytes<f32x2>(sgpr_base(tile + (size_t)(T * j * CT)), toff2 * 8u));
        }
    }
    B4D_STAMP(6);
    B4D_DRAIN();
    B4D_STAMP(7);
}

// ------------------------------------------------------------------------------------ Nyquist column
enum NyqMode { NYQ_PSD_AC = 0, NYQ_FORWARD = 2, NYQ_PROD = 3, NYQ_PROD_WHITEN = 4 };

struct NyqArgs {
    const float* rows;   // (items, NY) real Nyquist bins from K1                      [PSD_AC, FORWARD]
    float2* f_out;       // (items, NY) complex column spectra                          [FORWARD]
    float* g_out;        // (items, NY) real inverse-column output, consumed by K3      [PSD_AC, PROD]
    float* psd;          // (items, NY, nx) or null: column 0 of the shifted PSD        [PSD_AC]
    const float2* fa;    // column spectra of the two operands + per-pair indices       [PROD]
    const float2* fb;
    const int* idx_a;
    const int* idx_b;
    const float2* tw;
    float psd_scale, eps;
    int nx, items;
    const RowSrc* srcs;  // NYQ_FORWARD, optional: rows outside [srcs[i].y0, srcs[i].y1) are zero and were not written by k_row_r2c
};

// grid (ceil(items/SEQ)), block T*SEQ: one length-NY transform per T lanes.
template <int NY, int SEQ, int MODE>
__global__ void __launch_bounds__((NY / E16) * SEQ) k_nyq(NyqArgs p) {
    using G = RowGeom<NY>;
    constexpr int T = G::T, E = E16;
    constexpr bool WV = T <= 64;
    __shared__ float2 lds_all[SEQ * G::LDS_ELEMS];
    const int seq = threadIdx.x / T, u = threadIdx.x % T;
    const int item = blockIdx.x * SEQ + seq;
    const bool live = item < p.items;
    const size_t it = live ? item : 0;
    float2* lds = lds_all + seq * G::LDS_ELEMS;
    float2 v[E];
    if (MODE == NYQ_PROD || MODE == NYQ_PROD_WHITEN) {
        const size_t ia = p.idx_a ? p.idx_a[it] : it, ib = p.idx_b ? p.idx_b[it] : it;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int ky = u + T * j;
            const float2 c = cross_power<MODE == NYQ_PROD_WHITEN>(p.fa[ia * NY + ky], p.fb[ib * NY + ky], p.eps);
            v[j] = make_float2(c.y, c.x);  // swapped: inverse transform
        }
        Fft3<G, 1, WV>::run(v, v, u, 0, lds, p.tw);
        if (live) {
#pragma unroll
            for (int j = 0; j < E; ++j) p.g_out[it * NY + u + T * j] = v[j].y;
        }
        return;
    }
    int ry0 = 0, ry1 = NY;
    if (MODE == NYQ_FORWARD && p.srcs) {
        ry0 = p.srcs[it].y0;
        ry1 = p.srcs[it].y1;
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int ky = u + T * j;
        v[j] = make_float2((ky >= ry0 && ky < ry1) ? p.rows[it * NY + ky] : 0.f, 0.f);
    }
    Fft3<G, 1, WV>::run(v, v, u, 0, lds, p.tw);
    if (MODE == NYQ_FORWARD) {
        if (live) {
#pragma unroll
            for (int j = 0; j < E; ++j) p.f_out[it * NY + u + T * j] = v[j];
        }
        return;
    }
    // NYQ_PSD_AC
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const float pw = v[j].x * v[j].x + v[j].y * v[j].y;
        if (live && p.psd) p.psd[(it * NY + ((u + T * j + NY / 2) & (NY - 1))) * (size_t)p.nx] = pw * p.psd_scale;
        v[j] = make_float2(0.f, pw);
    }
    fft_sync<WV>();
    Fft3<G, 1, WV>::run(v, v, u, 0, lds, p.tw);
    if (live) {
#pragma unroll
        for (int j = 0; j < E; ++j) p.g_out[it * NY + u + T * j] = v[j].y;
    }
}

// ------------------------------------------------------------------------------------ K3
struct RowOutArgs {
    const float2* g;     // tile-major inverse-column output
    const float* gnyq;   // (batch, ny) inverse-column output of the Nyquist column (real)
    float* out;          // (batch, ny, nx) float32 shifted
    float* peak;         // (batch) zero-lag values
    const float2* tw;
    float scale;         // used when !NORM_PEAK
    int ny, ct_w;
    unsigned flags;
    float* part_val;     // C2R_MAG: per-workgroup arg-max partials (batch, gridDim.x)
    int* part_idx;
    // C2R_MAG, optional (selw != null): the exact median's first select step, fused into the pass that produces the map.
    // pred_bin = top-11-bit key bin the median is EXPECTED in; per frame, at selw + frame * sel_stride: word 1 += elements
    // below that bin, word 2 += elements in it, word 3 = append cursor of compact + frame * ny * nx, which receives the bin's
    // elements (all zeroed by the caller).  b4d_track.hip checks the expectation and finishes on the gathered ~10 %.
    unsigned* selw;
    int sel_stride;
    unsigned pred_bin;
    float* compact;
    int half;            // C2R_OUT: the map is even (R[-y,-x] = R[y,x], autocorrelation): transform rows 0..ny/2 only
                         // and write every row together with its point mirror
    // C2R_MAG without the map (tracking): partials, counts and the gathered bin are everything the common path reads of the
    // 4 ny nx bytes -- except the 3 x 3 neighbourhood of the peak, which C2R_ROWS writes afterwards (three row pairs).
    int nomap;           // C2R_MAG: do not store the map
    int nblk;            // C2R_ROWS: partials per frame
    const unsigned* gate;   // C2R_MAG, optional: skip frame f when gate[f * gate_stride] != 0 (pairs that need no full map)
    int gate_stride;
    const float2* tw_y;     // YS kernels: ny-point twiddles (the last radix-2 stage of the inverse column transform)
};

enum RowOutMode { C2R_OUT = 0, C2R_PEAK = 1, C2R_MAG = 2, C2R_ROWS = 3 };

// grid (ceil(ny/2/SEQ), batch) -- or (1, batch) for C2R_PEAK; block T*SEQ.
//   C2R_OUT   shifted real output, scaled (flags & NORM_PEAK: by 1/peak[frame], zero lag forced to 1)
//   C2R_PEAK  only the zero-lag value of each frame -> peak[frame]
//   C2R_MAG   |value| * scale (signal/tracking.py:283-285) + per-workgroup arg-max partials
// YS ("ysplit" route, C2R_OUT / C2R_PEAK, always the half form): g holds the h-point inverse transforms E (even ky) and O (odd ky)
// of the power columns, rows 0 .. h/2 of each parity tile, h = ny/2.  Transform y combines row y of both:
// t = conj(w^y) O, G(y) = E + t, G(h - y) = conj(E - t), and packs THESE two rows; rows y, h - y and their point mirrors
// -y, h + y are written, every row of the map once.
// W16 (YS, C2R_OUT; "row16" of b4d_set_option): 16 bytes per lane in every global access, whole lines per wave instruction, the same
// values bit for bit; needs 16-byte-aligned workspace and output (launch_c2r).  The exchange buffer is free before stage 1 and
// after stage 3, so the lane that moves an element need not be the lane that transforms it:
//   loads   lane u loads bins k, k + 1, k = 2(u + T j), j < 4, of the E and O tile rows (8 instead of 16 loads), writes both
//           Hermitian halves to the buffer and reads all 16 registers back
//   stores  the scaled rows go through the buffer as pairs (row b, row a) at x; lane u stores output columns 4u + 4T i ... + 3 of the
//           two direct rows (x ascending from an aligned start) and of the two mirror rows (x = nx/2 - c descending: one 16-byte
//           and two 8-byte LDS reads) -- 16 instead of 64 stores
template <int NX, int SEQ, int MODE, int UNIT = 0, bool YS = false, bool W16 = false>
__global__ void __launch_bounds__((NX / E16) * SEQ) k_row_c2r(RowOutArgs p) {
    static_assert(!YS || MODE == C2R_OUT || MODE == C2R_PEAK, "ysplit: autocorrelation output only");
    static_assert(!W16 || (YS && MODE == C2R_OUT), "16-byte accesses: parity-tile autocorrelation output only");
    using G = RowGeom<NX>;
    constexpr int T = G::T, E = E16;
    constexpr bool WV = T <= 64;   // the transform's own exchanges are wave-local; the reductions ACROSS transforms below keep s_barrier
    static_assert(!W16 || G::LDS_ELEMS % 2 == 0, "16-byte accesses to each transform's buffer");
    __shared__ __attribute__((aligned(16))) float2 lds_all[SEQ * G::LDS_ELEMS];
    const int seq = threadIdx.x / T, u = threadIdx.x % T;
    const size_t frame = blockIdx.y;
    const int ny = p.ny, ct_w = p.ct_w, nt = (NX / 2) / ct_w;
    if (MODE == C2R_MAG && p.gate && p.gate[frame * p.gate_stride]) return;
    int peak_pair = 0;
    if (MODE == C2R_ROWS) {   // first-occurrence arg-max over the frame's partials -> the row pair that holds the peak
        float bv = -1.0f;
        int bi = 0x7fffffff;
        for (int i = threadIdx.x; i < p.nblk; i += T * SEQ) argmax_merge(bv, bi, p.part_val[frame * p.nblk + i], p.part_idx[frame * p.nblk + i]);
        // (wave_argmax of b4d_reduce.hpp, kept inline: through the helper this kernel's instructions come out different)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_down(bv, o, 64);
            const int oi = __shfl_down(bi, o, 64);
            argmax_merge(bv, bi, ov, oi);
        }
        float* sv = reinterpret_cast<float*>(lds_all);
        int* si = reinterpret_cast<int*>(lds_all) + 32;
        if ((threadIdx.x & 63) == 0) {
            sv[threadIdx.x >> 6] = bv;
            si[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        bv = sv[0];
        bi = si[0];
        for (int i = 1; i < (T * SEQ + 63) / 64; ++i) argmax_merge(bv, bi, sv[i], si[i]);
        __syncthreads();
        const int yr = bi == 0x7fffffff ? 0 : bi / NX;          // row of the shifted map
        peak_pair = ((yr + ny / 2) & (ny - 1)) >> 1;
    }
    const int nblk = gridDim.x, bx = blockIdx.x;
    // C2R_ROWS: the pairs peak - 1, peak, peak + 1 (cyclic) hold rows y - 1 .. y + 1 of the peak row y, whatever its parity
    const int pair = MODE == C2R_PEAK   ? 0
                     : MODE == C2R_ROWS ? (peak_pair + ny / 2 - 1 + min(bx * SEQ + seq, 2)) % (ny / 2)
                                        : bx * SEQ + seq;
    const bool live = YS ? 4 * pair <= ny : (MODE == C2R_OUT && p.half) ? 2 * pair <= ny / 2 : 2 * pair < ny;
    const int yl = live ? (YS ? pair : 2 * pair) : 0;
    float2* lds = lds_all + seq * G::LDS_ELEMS;
    float2 v[E];
    float2 wc = make_float2(1.f, 0.f);
    if (YS) {   // conj(w^y), uniform per transform
        wc = p.tw_y[yl];
        wc.y = -wc.y;
    }
    if (W16) {
#pragma unroll
        for (int j = 0; j < E / 4; ++j) {
            const int k = 2 * (u + T * j);
            const size_t o = spec_index(2 * frame, nt, ny / 2, ct_w, yl, k);
            const f32x4 e4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.g + o)),
                        o4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.g + o + (size_t)(ny / 2) * (NX / 2)));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float2 ev = h ? make_float2(e4.z, e4.w) : make_float2(e4.x, e4.y);
                const float2 t = cmul(h ? make_float2(o4.z, o4.w) : make_float2(o4.x, o4.y), wc);
                const float2 a = cadd(ev, t), d = csub(ev, t), b = make_float2(d.x, -d.y);
                if (h == 0 && k == 0) {  // DC and Nyquist bins of both rows are real
                    lds[0] = make_float2(b.x, a.x);
                    lds[NX / 2] = make_float2(p.gnyq[frame * ny + ny / 2 - yl], p.gnyq[frame * ny + yl]);
                } else {
                    lds[k + h] = make_float2(a.y + b.x, a.x - b.y);        // swap(A + iB)
                    lds[NX - k - h] = make_float2(b.x - a.y, a.x + b.y);  // swap(conj A + i conj B)
                }
            }
        }
    } else
#pragma unroll
    for (int j = 0; j < E / 2; ++j) {
        const int k = u + T * j;
        if (YS) {
            const size_t o = spec_index(2 * frame, nt, ny / 2, ct_w, yl, k);
            const f32x2 e_ = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p.g + o)),
                        o_ = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p.g + o + (size_t)(ny / 2) * (NX / 2)));
            const float2 ev = make_float2(e_.x, e_.y), t = cmul(make_float2(o_.x, o_.y), wc);
            const float2 a = cadd(ev, t), d = csub(ev, t), b = make_float2(d.x, -d.y);
            if (k == 0) {  // DC and Nyquist bins of both rows are real
                v[j] = make_float2(b.x, a.x);
                lds[NX / 2] = make_float2(p.gnyq[frame * ny + ny / 2 - yl], p.gnyq[frame * ny + yl]);
            } else {
                v[j] = make_float2(a.y + b.x, a.x - b.y);        // swap(A + iB)
                lds[NX - k] = make_float2(b.x - a.y, a.x + b.y);  // swap(conj A + i conj B)
            }
            continue;
        }
        // C2R_MAG (issue-bound, profiles/r03_pmc_cfg3_sq.txt): the tile index without the integer division by the run-time tile width
        // (a power of two) and with a 24-bit multiply -- the generic form costs ~40 quarter-rate multiplies per lane here.  The cfg2
        // instantiation keeps spec_index: there the same change cost K3 1 % (instruction order).
        const size_t o = MODE == C2R_MAG ? spec_index_pow2(frame, nt, ny, ct_w, yl, k) : spec_index(frame, nt, ny, ct_w, yl, k);
        // read once, written once: streaming hints on both sides of the row pass (-4 % on the cfg2 kernel)
        const f32x2 a_ = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p.g + o)),
                    b_ = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p.g + o + ct_w));
        const float2 a = make_float2(a_.x, a_.y), b = make_float2(b_.x, b_.y);
        if (k == 0) {  // DC and Nyquist bins of both rows are real
            v[j] = make_float2(b.x, a.x);                                                       // swap(A_dc + i B_dc)
            lds[NX / 2] = make_float2(p.gnyq[frame * ny + yl + 1], p.gnyq[frame * ny + yl]);  // swap(A_nyq + i B_nyq)
        } else {
            v[j] = make_float2(a.y + b.x, a.x - b.y);        // swap(A + iB)
            lds[NX - k] = make_float2(b.x - a.y, a.x + b.y);  // swap(conj A + i conj B)
        }
    }
    fft_sync<WV>();
#pragma unroll
    for (int j = W16 ? 0 : E / 2; j < E; ++j) v[j] = lds[u + T * j];
    fft_sync<WV>();
    Fft3<G, 1, WV>::run(v, v, u, 0, lds, p.tw);
    // v[j] = swap(z[x]), x = u + T j: row 2*pair = Re z = v.y, row 2*pair+1 = Im z = v.x
    if (MODE == C2R_PEAK) {
        if (threadIdx.x == 0) p.peak[frame] = v[0].y;
        return;
    }
    const int y0 = YS ? pair : 2 * pair;        // rows of the (unshifted) map in Re z and Im z: y0 and y0 + 1, YS: y0 and ny/2 - y0
    const int y1 = YS ? ny / 2 - pair : y0 + 1;
    const int ra = (y0 + ny / 2) & (ny - 1), rb = (y1 + ny / 2) & (ny - 1);
    float* o0 = p.out + (frame * ny + ra) * (size_t)NX;
    float* o1 = p.out + (frame * ny + rb) * (size_t)NX;
    if (MODE == C2R_OUT) {
        if (!W16 && !live) return;   // W16: idle transforms leave behind the barriers of the redistribution
        const bool norm = (p.flags & B4D_NORM_PEAK) != 0;
        float s = p.scale;
        bool unit_peak = false;   // corr / max|corr| only if the peak is > 0 (signal/corr.py:247-250): a constant frame stays 0
        if (norm) {
            const float pk = p.peak[frame];
            unit_peak = pk > 0.f;
            s = unit_peak ? 1.0f / pk : p.scale;
        }
        // half mode: rows 0..ny/2 are written directly, rows 1..ny/2-1 also as their point mirrors
        // YS: y0 = 0 writes rows 0 and ny/2 (their own mirrors), y0 = ny/4 holds the same row twice (written once, with its mirror)
        const bool wr1 = YS ? 4 * y0 < ny : !p.half || y0 + 1 <= ny / 2;
        const bool mir0 = YS ? y0 >= 1 : p.half && y0 >= 1 && y0 < ny / 2, mir1 = YS ? y0 >= 1 && 4 * y0 < ny : p.half && y0 + 1 < ny / 2;
        float* q0 = p.out + (frame * ny + ((ny / 2 - y0) & (ny - 1))) * (size_t)NX;
        float* q1 = p.out + (frame * ny + ((ny / 2 - y1) & (ny - 1))) * (size_t)NX;
        if (W16) {
            fft_sync<WV>();   // the transform's last exchange has been read
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int x = u + T * j;
                float r0 = v[j].y * s;
                const float r1 = v[j].x * s;
                if (unit_peak && pair == 0 && x == 0) r0 = 1.0f;  // peak normalisation: zero lag is 1 by definition
                lds[x] = make_float2(r1, r0);
            }
            fft_sync<WV>();
            if (!live) return;
            const f32x4* l4 = reinterpret_cast<const f32x4*>(lds);
#pragma unroll
            for (int i = 0; i < E / 4; ++i) {
                const int c = 4 * u + 4 * T * i, x = (c + NX / 2) & (NX - 1);   // columns c ... c + 3 hold x ... x + 3
                const f32x4 d0 = l4[x / 2], d1 = l4[x / 2 + 1];
                __builtin_nontemporal_store(f32x4{d0.y, d0.w, d1.y, d1.w}, reinterpret_cast<f32x4*>(o0 + c));
                if (wr1) __builtin_nontemporal_store(f32x4{d0.x, d0.z, d1.x, d1.z}, reinterpret_cast<f32x4*>(o1 + c));
                if (mir0 || mir1) {   // columns c ... c + 3 of a mirror row hold xs, xs - 1, xs - 2, xs - 3 (mod NX)
                    const int xs = (NX / 2 - c) & (NX - 1);
                    const float2 m0 = lds[xs], m3 = lds[(xs - 3) & (NX - 1)];
                    const f32x4 m12 = l4[((xs - 2) & (NX - 1)) / 2];
                    if (mir0) __builtin_nontemporal_store(f32x4{m0.y, m12.w, m12.y, m3.y}, reinterpret_cast<f32x4*>(q0 + c));
                    if (mir1) __builtin_nontemporal_store(f32x4{m0.x, m12.z, m12.x, m3.x}, reinterpret_cast<f32x4*>(q1 + c));
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int x = u + T * j, c = (x + NX / 2) & (NX - 1), cm = (NX / 2 - x) & (NX - 1);
            float r0 = v[j].y * s;
            const float r1 = v[j].x * s;
            if (unit_peak && pair == 0 && x == 0) r0 = 1.0f;  // peak normalisation: zero lag is 1 by definition
            __builtin_nontemporal_store(r0, o0 + c);
            if (wr1) __builtin_nontemporal_store(r1, o1 + c);
            if (mir0) __builtin_nontemporal_store(r0, q0 + cm);
            if (mir1) __builtin_nontemporal_store(r1, q1 + cm);
        }
        return;
    }
    if (MODE == C2R_ROWS) {   // the same values the map would hold, for the rows around the peak only
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int x = u + T * j, c = (x + NX / 2) & (NX - 1);
            o0[c] = fabsf(v[j].y * p.scale);
            o1[c] = fabsf(v[j].x * p.scale);
        }
        return;
    }
    // ---- C2R_MAG
    float bv = -1.0f;
    int bi = 0x7fffffff;
    // expected-median-bin bookkeeping (selw != null): per value one shift and two compares next to the store; bit j / 16 + j of
    // `hits` = value j of row a / b is in the bin (magnitudes are >= 0: the key's top 11 bits are 1024 + (bits >> 21))
    const unsigned pbx = (p.selw && p.pred_bin >= 1024u) ? p.pred_bin - 1024u : 0xffffffffu;
    unsigned cnt = 0, low = 0, hits = 0;
    if (live) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int x = u + T * j, c = (x + NX / 2) & (NX - 1);
            const float m0 = fabsf(v[j].y * p.scale), m1 = fabsf(v[j].x * p.scale);
            if (!p.nomap) {
                o0[c] = m0;
                o1[c] = m1;
            }
            if (pbx != 0xffffffffu) {
                // a NaN magnitude has the key bits 0x3fe: above every bin a finite median can be expected in -- neither counted
                // in the bin nor below it, without a select
                const unsigned b0 = __float_as_uint(m0) >> 21, b1 = __float_as_uint(m1) >> 21;
                hits |= (b0 == pbx ? 1u : 0u) << j | (b1 == pbx ? 1u : 0u) << (16 + j);
                low += (b0 < pbx ? 1u : 0u) + (b1 < pbx ? 1u : 0u);
            }
        }
        cnt = __popc(hits);
        // first-occurrence arg-max of the lane's 32 values: walked in ASCENDING flat index (row a before row b = row a + 1; inside a
        // row the shifted column of register j is u + T ((j + E/2) % E)), so a strict `>` keeps the first of equal maxima and the
        // index is rebuilt once from the winning slot -- three instructions per value instead of a (value, index) merge per value
        float lv = -1.0f;
        int ls = 0;
#pragma unroll
        for (int t = 0; t < 2 * E; ++t) {
            const int j = ((t % E) + E / 2) % E;
            const float m = fabsf((t < E ? v[j].y : v[j].x) * p.scale);
            if (m > lv) {   // NaN never wins (as argmax_merge)
                lv = m;
                ls = t;
            }
        }
        if (lv > -1.0f) {
            bv = lv;
            bi = (ls < E ? ra : rb) * NX + u + T * (ls % E);
        }
    }
    // (wave_argmax of b4d_reduce.hpp, kept inline: through the helper this kernel's instructions come out different)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_down(bv, o, 64);
        const int oi = __shfl_down(bi, o, 64);
        argmax_merge(bv, bi, ov, oi);
    }
    __syncthreads();  // everyone is done with lds_all (FFT exchange reads)
    float* sv = reinterpret_cast<float*>(lds_all);
    int* si = reinterpret_cast<int*>(lds_all) + 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (T * SEQ + 63) / 64;
    if (lane == 0) {
        sv[w] = bv;
        si[w] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < nw; ++i) argmax_merge(bv, bi, sv[i], si[i]);
        p.part_val[frame * nblk + bx] = bv;
        p.part_idx[frame * nblk + bx] = bi;
    }
    if (p.selw && p.pred_bin) {
        // counts of the magnitudes below / inside the expected median bin and the bin's elements themselves: lane counts,
        // a workgroup scan, THREE global atomics per workgroup (no per-element atomics, no second read of the map)
        constexpr int NW = (T * SEQ + 63) / 64;
        // (wave_scan_inclusive and wave_sum of b4d_reduce.hpp, kept inline: through the helper this kernel's instructions come out different)
        unsigned incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) low += __shfl_down(low, o, 64);
        unsigned* hl = reinterpret_cast<unsigned*>(lds_all) + 64;   // words 0..63: the arg-max partials above
        __syncthreads();
        if (lane == 63) hl[w] = incl;          // wave totals of the bin
        if (lane == 0) hl[NW + 1 + w] = low;   // wave totals below the bin
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned run = 0, lo = 0;
            for (int i = 0; i < NW; ++i) {
                const unsigned t = hl[i];
                hl[i] = run;
                run += t;
                lo += hl[NW + 1 + i];
            }
            unsigned* sw = p.selw + frame * p.sel_stride;
            if (lo) atomicAdd(&sw[1], lo);
            if (run) atomicAdd(&sw[2], run);
            hl[NW] = run ? atomicAdd(&sw[3], run) : 0u;
            hl[2 * NW + 1] = run;
        }
        __syncthreads();
        // The bin's elements go through the (free) exchange buffer: masked 4-byte LDS writes at the lane's offset, then one
        // coalesced copy to `compact` -- appended straight to global memory they cost as many (mostly empty) store
        // instructions as the map itself (+34 % on this kernel).
        constexpr int STAGE_WORDS = 2 * E * T * SEQ;   // every value of the workgroup may be in the bin
        static_assert(sizeof(lds_all) >= sizeof(unsigned) * (64 + 2 * NW + 2 + STAGE_WORDS), "exchange buffer too small for the staging");
        float* stg = reinterpret_cast<float*>(hl + 2 * NW + 2);
        if (cnt) {
            float* q = stg + hl[w] + (incl - cnt);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                if (hits & (1u << j)) *q++ = fabsf(v[j].y * p.scale);
                if (hits & (1u << (16 + j))) *q++ = fabsf(v[j].x * p.scale);
            }
        }
        __syncthreads();
        const unsigned total = hl[2 * NW + 1];
        float* dst = p.compact + frame * (size_t)ny * NX + hl[NW];
        for (unsigned i = threadIdx.x; i < total; i += T * SEQ) dst[i] = stg[i];
    }
}

}  // namespace b4d

// ===================================================================================== host
using namespace b4d;

struct b4d_plan {
    std::recursive_mutex mu;   // host-side re-entrancy: one plan may be called from several host threads (one stream)
    int ny, nx, chunk, ct_w;
    float2* tw_x = nullptr;    // nx-point twiddles
    float2* tw_y = nullptr;    // ny-point twiddles
    float2* tw_yh = nullptr;   // ny/2-point twiddles (ny = 2048: the parity-tile column pass of the "ysplit" route)
    float2* spec = nullptr;    // chunk * ny * nx/2
    float* nyq_rows = nullptr; // chunk * ny: Nyquist bins after the row pass
    float* gnyq = nullptr;     // chunk * ny: Nyquist column after the inverse column pass
    float* peak = nullptr;     // chunk
    size_t ws_bytes = 0;
    void* track_ws = nullptr;  // lazily grown arena of the xcorr / tracking entry points
    size_t track_bytes = 0;
    // general-length plans (b4d_general.hip): dense DFT matrices + three chunk-sized complex buffers
    bool general = false;
    float2* wx = nullptr;
    float2* wy = nullptr;
    float2* gbuf1 = nullptr;
    float2* gbuf2 = nullptr;
    float2* gbuf3 = nullptr;
    // general lengths beyond the DFT-matrix range: both axes through the fused P * A * B row transform (b4d_pm.hip)
    bool large = false;
    // both sides have in-register three-radix kernels (b4d_wiener_mr.hip): the transform-based entry points take those passes,
    // whatever the size class (228-px aggregator tiles as well as 2560 x 2160 frames); tw_x / tw_y are built for it
    bool wmr = false;
    unsigned route = 0;        // B4D_ROUTE_* bits of this plan (size_route below): what the entry points branch on
    LaneSync lanes;            // second stream and fork / join events of the two-lane drivers (b4d_lanes.hpp)
};

// b4d_general.hip
int make_dft_matrix(int n, float2** out);
int general_psd_autocorr(b4d_plan* pl, const float* frames, int batch, float* psd, float psd_scale, float* autocorr,
                         unsigned flags, hipStream_t st);
int general_fft2d(b4d_plan* pl, const float* frames, int batch, float2* out, hipStream_t st);
int general_xcorr(b4d_plan* pl, const float* a, const float* b, int batch, float* corr, unsigned flags, hipStream_t st);
int general_fft2d_c2c(b4d_plan* pl, const float2* in, int batch, int inverse, float2* out, hipStream_t st);
int general_dft2(const b4d_plan* pl, const void* X, bool x_real, int batch, int conj, float2* tmp, float2* F, hipStream_t st);
// b4d_track.hip: x[b] /= max|x[b]| for `batch` maps of n floats; scratch holds >= 256 * batch floats
int normalise_by_absmax(float* x, size_t n, int batch, float* scratch, hipStream_t st);

static inline bool pow2_ok(int n) { return n >= 64 && n <= 4096 && (n & (n - 1)) == 0; }
template <int NY>
static inline int col_ct_of() { return ColCfg<NY>::CT; }
static inline int col_ct(int ny) {
    switch (ny) {
        case 64: return col_ct_of<64>();
        case 128: return col_ct_of<128>();
        case 256: return col_ct_of<256>();
        case 512: return col_ct_of<512>();
        case 1024: return col_ct_of<1024>();
        case 2048: return col_ct_of<2048>();
        case 4096: return col_ct_of<4096>();
    }
    return 16;
}
static inline bool general_ok(int n) { return n >= 2 && n <= 512; }
// b4d_general.hip: the one place that decides which kernels a supported (ny, nx) runs.  plan_create_impl fills the plan from it,
// the entry points branch on the plan's copy, and b4d_size_route reports `bits` (B4D_ROUTE_*, include/b4d.h) without a GPU.
struct SizeRoute {
    unsigned bits;
    bool general;   // a general-length plan: every size that is not power of two on both sides, and every plan of b4d_plan_create_general
    bool large;     // general, a side beyond the DFT-matrix range: dft2 runs row transforms per axis (the complex entry points of a WMR plan too)
    bool wmr;
};
SizeRoute size_route(int ny, int nx, bool force_general);

static inline int make_twiddles(int n, float2** out) {
    std::vector<float2> h(n);
    for (int k = 0; k < n; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)n;
        h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    B4D_HIP(hipMalloc((void**)out, sizeof(float2) * n));
    B4D_HIP(hipMemcpy(*out, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    return B4D_OK;
}

#define B4D_PLAN_LOCK(pl) std::lock_guard<std::recursive_mutex> b4d_plan_lk__((pl)->mu)
#define B4D_SIZE_SWITCH(n, CALL)        \
    switch (n) {                        \
        case 64: return CALL(64);       \
        case 128: return CALL(128);     \
        case 256: return CALL(256);     \
        case 512: return CALL(512);     \
        case 1024: return CALL(1024);   \
        case 2048: return CALL(2048);   \
        case 4096: return CALL(4096);   \
    }

// The tiles one PSD + autocorrelation call hands from pass to pass.  psd_autocorr_impl (b4d_kernels.hip) decides them once per call;
// the three passes take them as given.
struct Route {
    bool parity;           // "ysplit" route of 2048-row frames: parity tiles of ny/2 rows; otherwise tiles of all ny rows
    int ct_w;              // complex columns per tile
    const float2* tw_col;  // twiddles of the transform the column pass runs: ny/2 points on parity tiles, ny points otherwise
    int row16;             // parity route: the row passes may move 16 bytes per lane ("row16"); their launchers check the alignment
    int colsets;           // parity route with row16, nx <= 2048: column-set tiles between the forward row pass and the column pass
                           // ("colsets"); BOTH launchers check the workspace's alignment (colsets_of)
};
// the one decision the forward row pass and the column pass must share: which layout the tiles between them have
static inline int colsets_of(const Route& rt, const void* spec) { return rt.parity && rt.row16 && ptr_aligned(spec, 16) ? rt.colsets : 0; }

// Launchers: one per pass, the route (YS: parity tiles) a template argument.  A dispatcher instantiates every kernel it names in the
// including unit: the plain-route ones (dispatch_r2c, dispatch_c2r) are ordinary functions, the *_route templates let the one unit
// that runs the parity-tile kernels of a pass build them.
#if B4D_UNIT_PASSES & B4D_PASS_COL
// grid: one workgroup per tile; YS: 1024-point parity tiles of 2048-row frames, a.tw / a.tw_inv = 1024-point twiddles
// CS: column-set tiles (k_col); the two twiddle tables (8.5 KiB) sit behind the exchange region
template <int NY, int MODE, int YS = 0, int CS = 0>
static int launch_col(const ColArgs& a, int batch, hipStream_t st) {
    using Cfg = ColCfg<NY, YS>;
    constexpr size_t LDS_BYTES = Cfg::LDS_BYTES + (CS ? sizeof(float2) * (Cfg::G::M + NY) : 0);
    if ((a.nx / 2) % Cfg::CT) return fail(B4D_ESIZE, "column pass: nx / 2 is no multiple of the tile width");
    return launch(k_col<NY, MODE, B4D_UNIT_TAG, YS, CS>, dim3((YS ? 2 : 1) * ((a.nx / 2) / Cfg::CT), batch), dim3(Cfg::THREADS), LDS_BYTES,
                  st, a);
}
template <int MODE>
static int dispatch_col(const b4d_plan* pl, const ColArgs& a, int batch, hipStream_t st) {
#define B4D_CALL(N) launch_col<N, MODE>(a, batch, st)
    B4D_SIZE_SWITCH(pl->ny, B4D_CALL)
#undef B4D_CALL
    return fail(B4D_ESIZE, "unsupported ny");
}
#endif  // B4D_PASS_COL

#if B4D_UNIT_PASSES & B4D_PASS_NYQ
template <int NY, int MODE>
static int launch_nyq(const NyqArgs& a, hipStream_t st) {
    constexpr int SEQ = row_seq(NY);
    hipLaunchKernelGGL((k_nyq<NY, SEQ, MODE>), dim3((a.items + SEQ - 1) / SEQ), dim3((NY / E16) * SEQ), 0, st, a);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
template <int MODE>
static int dispatch_nyq(const b4d_plan* pl, NyqArgs a, int items, hipStream_t st) {
    a.items = items;
    a.tw = pl->tw_y;
    a.nx = pl->nx;
#define B4D_CALL(N) launch_nyq<N, MODE>(a, st)
    B4D_SIZE_SWITCH(pl->ny, B4D_CALL)
#undef B4D_CALL
    return fail(B4D_ESIZE, "unsupported ny");
}
#endif  // B4D_PASS_NYQ

#if B4D_UNIT_PASSES & B4D_PASS_R2C
// YS: rows p and p + ny/2 per transform, parity tile sets (full frames only); otherwise srcs != null selects ROI / z-score sources
template <int NX, bool YS>
static int launch_r2c(const b4d_plan* pl, const float* in, float2* spec, float* nyq_rows, const RowSrc* srcs, int ct_w, int batch,
                      hipStream_t st, int row16, int colsets) {
    constexpr int SEQ = row_seq(NX);
    constexpr int ITER = NX >= 1024 ? B4D_K1_ITER : 1;   // groups of row pairs per workgroup, full frames only
    const dim3 block((NX / E16) * SEQ), grid((pl->ny / 2 + SEQ - 1) / SEQ, batch),
        grid_full((pl->ny / 2 + SEQ * ITER - 1) / (SEQ * ITER), batch);
    if (YS && srcs) return fail(B4D_EINVAL, "parity tiles take full frames");
    if constexpr (YS) {
        // 16-byte stores need a 16-byte-aligned workspace (the loads are dwords: the frames may sit anywhere); the narrow kernel otherwise
        if constexpr (SEQ % 2 == 0) {
            if (colsets && row16 && ptr_aligned(spec, 16)) {   // couples of transforms: one group of SEQ pairs per workgroup
                if (ct_w != 32 || (pl->ny / 2) % SEQ) return fail(B4D_ESIZE, "column-set tiles: 32 columns, whole workgroups");
                hipLaunchKernelGGL((k_row_r2c<NX, SEQ, false, 1, true, true, true>), grid, block, 0, st, in, spec, nyq_rows, pl->tw_x, pl->ny,
                                   ct_w, srcs, pl->tw_y);
                B4D_HIP(hipGetLastError());
                return B4D_OK;
            }
        } else if (colsets) {
            return fail(B4D_ESIZE, "column-set tiles need two transforms per workgroup");
        }
        if (row16 && ptr_aligned(spec, 16))
            hipLaunchKernelGGL((k_row_r2c<NX, SEQ, false, ITER, true, true>), grid_full, block, 0, st, in, spec, nyq_rows, pl->tw_x, pl->ny,
                               ct_w, srcs, pl->tw_y);
        else
            hipLaunchKernelGGL((k_row_r2c<NX, SEQ, false, ITER, true>), grid_full, block, 0, st, in, spec, nyq_rows, pl->tw_x, pl->ny, ct_w,
                               srcs, pl->tw_y);
    } else if (srcs)
        hipLaunchKernelGGL((k_row_r2c<NX, SEQ, true>), grid, block, 0, st, in, spec, nyq_rows, pl->tw_x, pl->ny, ct_w, srcs,
                           (const float2*)nullptr);
    else
        hipLaunchKernelGGL((k_row_r2c<NX, SEQ, false, ITER>), grid_full, block, 0, st, in, spec, nyq_rows, pl->tw_x, pl->ny, ct_w, srcs,
                           (const float2*)nullptr);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
template <bool YS>
static int dispatch_r2c_route(const b4d_plan* pl, const float* in, int batch, hipStream_t st, float2* spec, float* nyq_rows,
                              const RowSrc* srcs, int ct_w, int row16 = 0, int colsets = 0) {
#define B4D_CALL(N) launch_r2c<N, YS>(pl, in, spec, nyq_rows, srcs, ct_w, batch, st, row16, colsets)
    B4D_SIZE_SWITCH(pl->nx, B4D_CALL)
#undef B4D_CALL
    return fail(B4D_ESIZE, "unsupported nx");
}
// rows -> half spectra into `spec` / `nyq_rows` (default: the plan's chunk workspace), tiles of all ny rows; srcs != null selects
// ROI / z-score sources
static int dispatch_r2c(const b4d_plan* pl, const float* in, int batch, hipStream_t st, float2* spec = nullptr,
                        float* nyq_rows = nullptr, const RowSrc* srcs = nullptr) {
    return dispatch_r2c_route<false>(pl, in, batch, st, spec ? spec : pl->spec, nyq_rows ? nyq_rows : pl->nyq_rows, srcs, pl->ct_w);
}
#endif  // B4D_PASS_R2C

#if B4D_UNIT_PASSES & B4D_PASS_C2R
// mode: C2R_OUT (with a C2R_PEAK pre-pass when NORM_PEAK), C2R_MAG or C2R_ROWS.  ev: optional event sink (timed runs).
// YS: C2R_OUT on the parity tiles (a.ct_w, a.tw_y), always the half form.
template <int NX, bool YS>
static int launch_c2r(const b4d_plan* pl, const RowOutArgs& a, int batch, int mode, hipStream_t st,
                      std::vector<hipEvent_t>* ev, int* nblk, int row16) {
    constexpr int SEQ = row_seq(NX);
    const int npairs = (YS || (a.half && mode == C2R_OUT)) ? pl->ny / 4 + 1 : pl->ny / 2;
    const dim3 grid((npairs + SEQ - 1) / SEQ, batch), block((NX / E16) * SEQ);
    if (nblk) *nblk = grid.x;
    if (batch < 1) return B4D_OK;
    if constexpr (YS) {
        if (mode != C2R_OUT) return fail(B4D_EINVAL, "parity tiles: autocorrelation output only");
    } else {
        if (mode == C2R_MAG) {
            // with a.gate (full maps for the few frames that need them) the workgroups of every other frame leave at once; a loop
            // over row blocks inside the kernel instead of the full grid was tried: the compiler hoists the transform's twiddle
            // and address set out of it (92 -> 236 VGPRs, half the occupancy of the main pass that shares the instantiation)
            hipLaunchKernelGGL((k_row_c2r<NX, SEQ, C2R_MAG, B4D_UNIT_TAG>), grid, block, 0, st, a);
            B4D_HIP(hipGetLastError());
            return B4D_OK;
        }
        if (mode == C2R_ROWS) {   // three row pairs around each frame's peak (a.nblk partials per frame)
            hipLaunchKernelGGL((k_row_c2r<NX, SEQ, C2R_ROWS, B4D_UNIT_TAG>), dim3((3 + SEQ - 1) / SEQ, batch), block, 0, st, a);
            B4D_HIP(hipGetLastError());
            return B4D_OK;
        }
    }
    if (a.flags & B4D_NORM_PEAK) {
        hipLaunchKernelGGL((k_row_c2r<NX, SEQ, C2R_PEAK, B4D_UNIT_TAG, YS>), dim3(1, batch), block, 0, st, a);
        B4D_HIP(hipGetLastError());
        if (ev) {
            hipEvent_t e;
            B4D_HIP(hipEventCreate(&e));
            ev->push_back(e);
            B4D_HIP(hipEventRecord(e, st));
        }
    }
    if constexpr (YS) {
        // 16-byte accesses need 16-byte-aligned output (the C ABI does not promise it) and workspace: the narrow kernel otherwise
        if (row16 && ptr_aligned(a.g, 16) && ptr_aligned(a.out, 16))
            hipLaunchKernelGGL((k_row_c2r<NX, SEQ, C2R_OUT, B4D_UNIT_TAG, YS, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((k_row_c2r<NX, SEQ, C2R_OUT, B4D_UNIT_TAG, YS>), grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL((k_row_c2r<NX, SEQ, C2R_OUT, B4D_UNIT_TAG, YS>), grid, block, 0, st, a);
    }
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}
template <bool YS>
static int dispatch_c2r_route(const b4d_plan* pl, const RowOutArgs& a, int batch, hipStream_t st, int mode, std::vector<hipEvent_t>* ev,
                              int* nblk, int row16 = 0) {
#define B4D_CALL(N) launch_c2r<N, YS>(pl, a, batch, mode, st, ev, nblk, row16)
    B4D_SIZE_SWITCH(pl->nx, B4D_CALL)
#undef B4D_CALL
    return fail(B4D_ESIZE, "unsupported nx");
}
static int dispatch_c2r(const b4d_plan* pl, const RowOutArgs& a, int batch, hipStream_t st, int mode = C2R_OUT,
                        std::vector<hipEvent_t>* ev = nullptr, int* nblk = nullptr) {
    return dispatch_c2r_route<false>(pl, a, batch, st, mode, ev, nblk);
}
#endif  // B4D_PASS_C2R
