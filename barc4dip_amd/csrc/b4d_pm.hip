// b4d_pm.hip -- general-length 1-D transform engine on gfx950: the fallback for every length without a compiled power-of-two
// or mixed-radix kernel (the general plans of b4d_general.hip, the Wiener plan of b4d_wiener.hip).
//
// N = P * M with P <= 16 a power of two done as an in-register radix-P butterfly plus twiddles, and the length-M part
//
//   X[k1 + P k2] = sum_{n2 < M} W_M^{n2 k2} [ W_N^{n2 k1} sum_{n1 < P} x[M n1 + n2] W_P^{n1 k1} ]
//
// either fused in LDS when M = A * B splits into two small factors (k_pm_fused: one kernel per row pass), or as a dense
// DFT-matrix product (k_pm_pre, the complex GEMM of b4d_general.hip, k_pm_post), or, for the plans of b4d_general.hip, by
// Bluestein's chirp-z over two fused power-of-two transforms.  Also the batched complex transpose between two row passes.
#include "b4d_pm.hpp"

// complex GEMM of b4d_general.hip
int b4d_cgemm(const void* A, bool a_real, long long sA, int conj_a, const void* B, bool b_real, long long sB, int conj_b,
              float2* C, long long sC, int M, int N, int K, int batch, hipStream_t st);

namespace b4d {

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}

// step A: y[(s*P + k1)*M + n2] = W_N^{n2 k1} * sum_{n1} x[s*N + M n1 + n2] * W_P^{n1 k1}     (conj_in: x -> conj x)
// one lane per (s, n2); twN: N-point twiddles exp(-2 pi i k / N).  grid (ceil(M/256), S)
template <int P, bool REAL_IN>
__global__ void __launch_bounds__(256) k_pm_pre(const void* __restrict__ xin, float2* __restrict__ y, const float2* __restrict__ twN,
                                                int M, int conj_in) {
    const int n2 = blockIdx.x * blockDim.x + threadIdx.x;
    if (n2 >= M) return;
    const size_t s = blockIdx.y;
    const int N = P * M;
    float2 v[P];
#pragma unroll
    for (int n1 = 0; n1 < P; ++n1) {
        const size_t i = s * (size_t)N + (size_t)M * n1 + n2;
        if (REAL_IN) {
            v[n1] = make_float2(static_cast<const float*>(xin)[i], 0.f);
        } else {
            const float2 q = static_cast<const float2*>(xin)[i];
            v[n1] = conj_in ? make_float2(q.x, -q.y) : q;
        }
    }
    Dft<P>::run(v);
#pragma unroll
    for (int k1 = 0; k1 < P; ++k1) {
        const float2 w = k1 == 0 ? make_float2(1.f, 0.f) : twN[(size_t)((long long)n2 * k1 % N)];
        y[(s * P + k1) * (size_t)M + n2] = cmulf(v[k1], w);
    }
}

// step C: out[s*N + k1 + P k2] = z[(s*P + k1)*M + k2]  (* filt[same index], conj_out, * scale).  grid (ceil(N/256), S)
__global__ void __launch_bounds__(256) k_pm_post(const float2* __restrict__ z, float2* __restrict__ out, int P, int M,
                                                 const float2* __restrict__ filt, int conj_out, float scale) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P * M;
    if (k >= N) return;
    const size_t s = blockIdx.y;
    const int k1 = k % P, k2 = k / P;
    float2 v = z[(s * P + k1) * (size_t)M + k2];
    if (filt) v = cmulf(v, filt[s * (size_t)N + k]);
    if (conj_out) v.y = -v.y;
    out[s * (size_t)N + k] = make_float2(v.x * scale, v.y * scale);
}

// 32 x 32 LDS-tiled transpose of a (rows, cols) complex array.  grid (ceil(cols/32), ceil(rows/32)), block (32, 8)
__global__ void __launch_bounds__(256) k_transpose_c(const float2* __restrict__ in, float2* __restrict__ out, int rows, int cols) {
    __shared__ float2 t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    in += (size_t)blockIdx.z * rows * cols;   // grid.z = batch of equally shaped matrices
    out += (size_t)blockIdx.z * rows * cols;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + threadIdx.x;
        if (r < rows && c < cols) t[i][threadIdx.x] = in[(size_t)r * cols + c];
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + threadIdx.x;
        if (r < rows && c < cols) out[(size_t)c * rows + r] = t[threadIdx.x][i];
    }
}

// ---- Fused length-N transform of one row per workgroup when M = A * B splits into two small factors: the radix-P
// butterfly + twiddle of step A, then DFT_M as DFT_A (over a, n2 = B a + b), the twiddle W_M^{b c} and DFT_B (over b,
// k2 = c + A d), all in LDS; the two small DFTs are dense sums from LDS-resident tables (M (A + B) complex MACs per
// sequence instead of the M^2 of the DFT-matrix product).  Output k = k1 + P (c + A d), optional pointwise filter,
// conjugation and scale fused into the coalesced copy-out.  Safe in place.  Loads and stores: PmIn / PmOut (b4d_pm.hpp).
// grid (S), block FT, dynamic LDS pm_lds_elems() complex values (one or two row buffers + the small-DFT tables).
//
// Both small DFTs are one of three implementations below (the same one for both), each written once for
//   Y(col, r) = sum_{k < R} T_R[k][r] X(col, k)  (* W_N^{P col r} when TW)        r < R, col < ncol, for every k1 < P:
// column (k1, col) starts at in[src(k1, col)] with its elements `xstride` apart, its outputs at out[dst(k1, col)], `ostride` apart.
//   DFT_A: R = A, columns b < B, both strides B, twiddle;  DFT_B: R = B, columns c < A, strides 1 and P A (natural output order).
constexpr int FT_MAX = 1024, FT_ONEBUF = 512;
// acc += x * w (complex) in two packed FMAs
__device__ __forceinline__ v2f cmac(v2f acc, v2f x, v2f w) {
    v2f t, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(t) : "v"(x), "v"(w), "v"(acc));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(x), "v"(w), "v"(t));
    return r;
}

// (1) One-buffer variant: full table T[k * Rp + r] in LDS (Rp = R rounded up to 4, zero-padded), item = (k1, 4 outputs r,
// 2 columns): per k two x reads and one 4-wide table row feed 8 complex MACs in 4 x 2 register blocks of packed FMAs.
// Every lane owns at most one item, keeps its outputs in registers across a barrier and writes them back into the SAME row
// buffer: half the LDS, three workgroups per CU.
template <int P, bool TW, class Src, class Dst>
__device__ __forceinline__ void dft_small_blocks(const float2* __restrict__ tab, int R, int ncol, int xstride, int ostride, float2* buf,
                                                 const float2* __restrict__ twN, Src src, Dst dst) {
    const int Rp = (R + 3) & ~3, nRB = Rp / 4, nCP = (ncol + 1) / 2;
    const bool act = (int)threadIdx.x < P * nRB * nCP;
    const int it = act ? threadIdx.x : 0;
    const int cp = it % nCP, q = it / nCP, r0 = (q % nRB) * 4, k1 = q / nRB;
    const int c0 = 2 * cp, c1 = min(c0 + 1, ncol - 1);
    v2f acc[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = v2f{0.f, 0.f};
    if (act) {
        const float2* s0 = buf + src(k1, c0);
        const float2* s1 = buf + src(k1, c1);
        const float4* wrow = reinterpret_cast<const float4*>(tab + r0);
        for (int k = 0; k < R; ++k) {
            const v2f x0 = to_v(s0[xstride * k]), x1 = to_v(s1[xstride * k]);
            const float4 wa = wrow[k * (Rp / 2)], wb = wrow[k * (Rp / 2) + 1];
            const v2f w[4] = {v2f{wa.x, wa.y}, v2f{wa.z, wa.w}, v2f{wb.x, wb.y}, v2f{wb.z, wb.w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j][0] = cmac(acc[j][0], x0, w[j]);
                acc[j][1] = cmac(acc[j][1], x1, w[j]);
            }
        }
    }
    __syncthreads();
    if (act) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + j;
            if (r >= R) continue;
            buf[dst(k1, c0) + r * ostride] = TW ? cmulf(to_f(acc[j][0]), twN[(size_t)P * c0 * r]) : to_f(acc[j][0]);
            if (c0 + 1 < ncol) buf[dst(k1, c0 + 1) + r * ostride] = TW ? cmulf(to_f(acc[j][1]), twN[(size_t)P * (c0 + 1) * r]) : to_f(acc[j][1]);
        }
    }
}

// (2) Two-buffer variant, both factors <= 32: the small DFT on the matrix cores (the one dense contraction of this path;
// v_mfma_f32_16x16x4_f32 is exact f32 at the packed-FP32 flop rate, but one ds_read_b64 per operand feeds 4 MFMAs = 1024 complex
// MACs: ~12 x less LDS traffic than the 4 x 2 register blocks above).  Y(r, n) = sum_{k < R} T[k][r] * X(k, n) for r < R <= 32: one
// wave per strip of 16 columns n, two 16 x 16 complex tiles (rows 0..15, 16..31), k in steps of 4.
// Fragment maps (MI355X guide): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D: col = l & 15, row = 4 (l >> 4) + reg.
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct DftTiles {
    f32x4 r0, i0, r1, i1;
};
// tab: T[k * Tp + r]; x: this lane's column (nullptr = padding column), element k at x[k * xstride]
__device__ __forceinline__ DftTiles small_dft_mfma(const float2* __restrict__ tab, int R, int Tp, const float2* __restrict__ x, int xstride,
                                                   int lane) {
    const int j = lane & 15, kq = lane >> 4;
    DftTiles t;
    t.r0 = t.i0 = t.r1 = t.i1 = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool two = R > 16, row0 = j < R, row1 = 16 + j < R;
    for (int kk = 0; kk < R; kk += 4) {
        const int k = kk + kq;
        const bool vk = k < R;
        const float2 xv = (vk && x) ? x[k * xstride] : make_float2(0.f, 0.f);
        const float2 w0 = (vk && row0) ? tab[k * Tp + j] : make_float2(0.f, 0.f);
        t.r0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, xv.x, t.r0, 0, 0, 0);
        t.i0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, xv.y, t.i0, 0, 0, 0);
        if (two) {
            const float2 w1 = (vk && row1) ? tab[k * Tp + 16 + j] : make_float2(0.f, 0.f);
            t.r1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, xv.x, t.r1, 0, 0, 0);
            t.i1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, xv.y, t.i1, 0, 0, 0);
            t.r1 = __builtin_amdgcn_mfma_f32_16x16x4f32(-w1.y, xv.y, t.r1, 0, 0, 0);
            t.i1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, xv.x, t.i1, 0, 0, 0);
        }
        t.r0 = __builtin_amdgcn_mfma_f32_16x16x4f32(-w0.y, xv.y, t.r0, 0, 0, 0);
        t.i0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, xv.x, t.i0, 0, 0, 0);
    }
    return t;
}
// the column walk: strips of 16 of the P * ncol columns n = k1 * ncol + col (K1_MAJOR) or col * P + k1 (the order that makes a
// strip's stores contiguous); each lane keeps the base of its output column and strides it
template <int P, int FT, bool TW, bool K1_MAJOR, class Src, class Dst>
__device__ __forceinline__ void dft_small_mfma(const float2* __restrict__ tab, int R, int ncol, int xstride, int ostride, const float2* in,
                                               float2* out, const float2* __restrict__ twN, Src src, Dst dst) {
    const int Rp = (R + 3) & ~3;
    const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4;
    const int ncols = P * ncol;
    for (int strip = threadIdx.x >> 6; strip * 16 < ncols; strip += FT / 64) {
        const int n = strip * 16 + j;
        const bool vn = n < ncols;
        const int k1 = vn ? (K1_MAJOR ? n / ncol : n % P) : 0, col = vn ? (K1_MAJOR ? n % ncol : n / P) : 0;
        float2 tw0[4], tw1[4];   // W_M^{b c} of this lane's outputs: in flight under the matrix products
        if (TW) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * kq + i;
                tw0[i] = twN[(size_t)P * col * min(r, R - 1)];          // unconditional (clamped): loads under a branch serialise
                tw1[i] = twN[(size_t)P * col * min(r + 16, R - 1)];
            }
        }
        const DftTiles t = small_dft_mfma(tab, R, Rp, vn ? in + src(k1, col) : nullptr, xstride, lane);
        if (vn) {
            float2* o = out + dst(k1, col);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * kq + i;
                const float2 y0 = make_float2(t.r0[i], t.i0[i]), y1 = make_float2(t.r1[i], t.i1[i]);
                if (r < R) o[r * ostride] = TW ? cmulf(y0, tw0[i]) : y0;
                if (r + 16 < R) o[(r + 16) * ostride] = TW ? cmulf(y1, tw1[i]) : y1;
            }
        }
    }
}

// (3) Two-buffer variant, a factor > 32: only the R roots of unity T[k] = W_R^k in LDS; item = (k1, column, 4 outputs r),
// scalar FMAs, the table index r k mod R kept by addition.
template <int P, int FT, bool TW, class Src, class Dst>
__device__ __forceinline__ void dft_small_roots(const float2* __restrict__ tab, int R, int ncol, int xstride, int ostride, const float2* in,
                                                float2* out, const float2* __restrict__ twN, Src src, Dst dst) {
    const int nRB = (R + 3) / 4;
    for (int it = threadIdx.x; it < P * ncol * nRB; it += FT) {
        const int col = it % ncol, q = it / ncol, r0 = (q % nRB) * 4, k1 = q / nRB;
        float2 acc[4];
        int idx[4], rj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = make_float2(0.f, 0.f);
            idx[j] = 0;
            rj[j] = (r0 + j) % R;
        }
        const float2* x0 = in + src(k1, col);
#pragma unroll 4
        for (int k = 0; k < R; ++k) {
            const float2 x = x0[xstride * k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 w = tab[idx[j]];
                acc[j].x = fmaf(x.x, w.x, fmaf(-x.y, w.y, acc[j].x));
                acc[j].y = fmaf(x.x, w.y, fmaf(x.y, w.x, acc[j].y));
                idx[j] += rj[j];
                idx[j] -= idx[j] >= R ? R : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (r0 + j < R) out[dst(k1, col) + (r0 + j) * ostride] = TW ? cmulf(acc[j], twN[(size_t)P * col * (r0 + j)]) : acc[j];
    }
}

// complex LDS words of one row transform: two row buffers + the small-DFT tables (full A x A / B x B matrices, padded to
// multiples of 4 columns, when both factors are <= 32; otherwise the A + B roots of unity)
__host__ __device__ inline size_t pm_lds_elems(int P, int A, int B, bool onebuf = false) {
    const size_t tabs = (A <= 32 && B <= 32) ? (size_t)A * ((A + 3) & ~3) + (size_t)B * ((B + 3) & ~3) : (size_t)A + B;
    return (onebuf ? 1 : 2) * (size_t)P * A * B + tabs;
}
// one-buffer mode: blocked small DFTs whose item counts fit one round of FT_ONEBUF lanes (measured: 2560 = 16 * 16 * 10
// gains 1.5x from three workgroups per CU; 4104 = 8 * 27 * 19 with 560 items is faster on two 1024-lane workgroups)
inline bool pm_onebuf(int P, int A, int B) {
    if (!(A <= 32 && B <= 32)) return false;
    const int Ap = (A + 3) & ~3, Bp = (B + 3) & ~3;
    return P * (Ap / 4) * ((B + 1) / 2) <= FT_ONEBUF && P * ((A + 1) / 2) * (Bp / 4) <= FT_ONEBUF;
}

// sequence s of a launch: the frame's scale, and for the pair modes s = frame * hp + pair covering rows 2 pair, 2 pair + 1
struct PmSeq {
    size_t s;
    float fsc;       // max|frame| (Reflect* loads, Crop* stores)
    bool fok;
    int frame, pair;
    size_t row0;     // global index of the pair's first row
    bool has_b;      // the pair has a second row
};

// element idx = M n1 + n2 of sequence q.s as the transform reads it
template <PmIn IN>
__device__ __forceinline__ float2 pm_load(const void* __restrict__ xin, int n1, int n2, int M, int N, int conj_io, const FusedIO& io,
                                          const PmSeq& q) {
    const int idx = M * n1 + n2;
    const size_t i = q.s * (size_t)N + (size_t)M * n1 + n2;
    if (IN == PmIn::ReflectPair) {
        const int x = reflect_idx(idx - io.px, io.w);
        // loads and divisions are unconditional (clamped row) and masked afterwards: a load under a branch would wait
        // for its data before the next one is issued (measured: 16 serial round trips, 7.5 us per row)
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int row = min(2 * (int)q.s + e, io.rows - 1);
            const int y = reflect_idx(row - io.py, io.h);
            const float d = io.frame[(size_t)y * io.w + x] / q.fsc;
            v[e] = (q.fok && 2 * (int)q.s + e < io.rows) ? d : 0.f;
        }
        return make_float2(v[0], v[1]);
    } else if (IN == PmIn::RealPair) {
        const float* pa = static_cast<const float*>(xin) + q.row0 * N;
        return make_float2(pa[idx], q.has_b ? pa[N + idx] : 0.f);
    } else if (IN == PmIn::HermPair) {
        const int j = idx <= N / 2 ? idx : N - idx;
        const float2* pa = static_cast<const float2*>(xin) + q.row0 * io.half;
        const float2 fa = pa[j];
        const float2 fb = q.has_b ? pa[io.half + j] : make_float2(0.f, 0.f);
        // Ga + i Gb, Hermitian-extended beyond N/2; then the inverse's input conjugation
        const float2 z = idx <= N / 2 ? make_float2(fa.x - fb.y, fa.y + fb.x) : make_float2(fa.x + fb.y, fb.x - fa.y);
        return make_float2(z.x, -z.y);
    } else if (IN == PmIn::Reflect) {
        const int y = reflect_idx((int)q.s - io.py, io.h), x = reflect_idx(idx - io.px, io.w);
        const float d = io.frame[(size_t)y * io.w + x] / q.fsc;
        return make_float2(q.fok ? d : 0.f, 0.f);
    } else if (IN == PmIn::Real) {
        return make_float2(static_cast<const float*>(xin)[i], 0.f);
    } else {
        const float2 v = static_cast<const float2*>(xin)[i];
        return conj_io ? make_float2(v.x, -v.y) : v;
    }
}

// the transformed row `row` (N values in LDS, natural order) of sequence q.s as the pass writes it
template <PmOut OUT, int FT>
__device__ __forceinline__ void pm_store(const float2* row, int N, float2* __restrict__ out, const float2* __restrict__ filt, int conj_io,
                                         float scale, const FusedIO& io, const PmSeq& q) {
    if (OUT == PmOut::ShiftPair) {
        const float pk = io.norm_peak ? io.amax[q.frame] : 0.f;
        const bool unit = io.norm_peak && pk > 0.f;
        const float se = unit ? 1.0f / pk : scale;
        float* fo = io.crop + (size_t)q.frame * io.rows * N;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int y = 2 * q.pair + e;
            if (y >= io.rows) continue;
            float* orow = fo + (size_t)((y + io.rows / 2) % io.rows) * N;
            for (int x = threadIdx.x; x < N; x += FT) {
                const float2 z = row[x];
                float v = (e == 0 ? z.x : -z.y) * se;     // conj(row): real part row a, imaginary part row b
                if (unit && y == 0 && x == 0) v = 1.0f;
                orow[(x + N / 2) % N] = v;
            }
        }
    } else if (OUT == PmOut::HalfPair) {
        float2* oa = out + q.row0 * io.half;
        for (int k = threadIdx.x; k < io.half; k += FT) {
            const float2 z = row[k], w = row[k == 0 ? 0 : N - k];
            oa[k] = make_float2(0.5f * (z.x + w.x), 0.5f * (z.y - w.y));
            if (q.has_b) oa[io.half + k] = make_float2(0.5f * (z.y + w.y), 0.5f * (w.x - z.x));
        }
    } else if (OUT == PmOut::CropPair) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int y = 2 * (int)q.s + e - io.py;
            if (y < 0 || y >= io.h || 2 * (int)q.s + e >= io.rows) continue;
            for (int x = threadIdx.x; x < io.w; x += FT) {
                const float2 z = row[x + io.px];
                const float v = (e == 0 ? z.x : -z.y) * scale;   // conj(row): real part row a, imaginary part row b
                io.crop[(size_t)y * io.w + x] = clip_rescale(v, io.clip, q.fok, q.fsc);
            }
        }
    } else if (OUT == PmOut::Crop) {
        const int y = (int)q.s - io.py;
        if (y < 0 || y >= io.h) return;
        for (int x = threadIdx.x; x < io.w; x += FT)   // conj_io only flips the imaginary part
            io.crop[(size_t)y * io.w + x] = clip_rescale(row[x + io.px].x * scale, io.clip, q.fok, q.fsc);
    } else {
        for (int k = threadIdx.x; k < N; k += FT) {
            float2 v = row[k];
            if (filt) v = cmulf(v, filt[(io.filt_bcast ? 0 : q.s * (size_t)N) + k]);
            if (conj_io) v.y = -v.y;
            out[q.s * (size_t)N + k] = make_float2(v.x * scale, v.y * scale);
        }
    }
}

#ifdef B4D_DIAG
// Diagnostic build (never shipped, never timed as a whole): wall-clock stamps (100 MHz) of lane 0 at the phase boundaries.
__device__ unsigned long long* g_pm_diag = nullptr;
#ifndef B4D_DIAG_PM_IN
#define B4D_DIAG_PM_IN 3
#endif
#define B4D_PM_STAMP(i)                                                                       \
    do {                                                                                      \
        if (g_pm_diag && threadIdx.x == 0 && (int)IN == B4D_DIAG_PM_IN) g_pm_diag[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); \
    } while (0)
#else
#define B4D_PM_STAMP(i) do { } while (0)
#endif
// The body in five steps: small-DFT tables -> radix-P stage -> DFT_A -> DFT_B -> store.
template <int P, PmIn IN, PmOut OUT, bool ONEBUF>
// two 1024-lane workgroups per CU need <= 64 VGPRs: asked for explicitly where the radix-P stage leaves room (P <= 8)
__global__ void __launch_bounds__(ONEBUF ? FT_ONEBUF : FT_MAX, (!ONEBUF && P <= 8) ? 8 : 1) k_pm_fused(const void* __restrict__ xin, float2* __restrict__ out, const float2* __restrict__ twN,
                                                 int A, int B, const float2* __restrict__ filt, int conj_io, float scale, FusedIO io) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    constexpr int FT = ONEBUF ? FT_ONEBUF : FT_MAX;
    const int M = A * B, N = P * M;
    float2* buf0 = sm;
    float2* buf1 = ONEBUF ? sm : sm + N;   // one-buffer variant: the small DFTs write back into the row buffer they read
    float2* tabA = sm + (ONEBUF ? N : 2 * N);
    const bool blocked = A <= 32 && B <= 32;   // full small-DFT matrices in LDS (variants 1, 2); else the roots of unity (3)
    const int Ap = (A + 3) & ~3, Bp = (B + 3) & ~3;
    float2* tabB = tabA + (blocked ? A * Ap : A);
    B4D_PM_STAMP(0);
    // ---- 1. tables
#ifndef B4D_EXP_PM_NOTAB   // timing-only switch: what the per-row table build costs
    if (blocked) {   // tabA[a][c] = W_A^{a c} (c < A, else 0), tabB[b][d] = W_B^{b d}
        for (int i = threadIdx.x; i < A * Ap; i += FT) {
            const int a = i / Ap, c = i % Ap;
            tabA[i] = c < A ? twN[(size_t)(N / A) * ((a * c) % A)] : make_float2(0.f, 0.f);
        }
        for (int i = threadIdx.x; i < B * Bp; i += FT) {
            const int b = i / Bp, d = i % Bp;
            tabB[i] = d < B ? twN[(size_t)(N / B) * ((b * d) % B)] : make_float2(0.f, 0.f);
        }
    } else {
        for (int i = threadIdx.x; i < A; i += FT) tabA[i] = twN[(size_t)(N / A) * i];
        for (int i = threadIdx.x; i < B; i += FT) tabB[i] = twN[(size_t)(N / B) * i];
    }
#endif
    PmSeq q;
    q.s = blockIdx.x;
    q.fsc = 1.f;
    q.fok = true;
    if (IN == PmIn::Reflect || IN == PmIn::ReflectPair || OUT == PmOut::Crop || OUT == PmOut::CropPair) {
        q.fsc = io.amax[0];
        q.fok = scale_ok(q.fsc);
    }
    const int hp = (io.rows + 1) / 2 > 0 ? (io.rows + 1) / 2 : 1;
    q.frame = (int)(q.s / hp), q.pair = (int)(q.s % hp);
    q.row0 = (size_t)q.frame * io.rows + 2 * q.pair;
    q.has_b = 2 * q.pair + 1 < io.rows;
    B4D_PM_STAMP(1);
    // ---- 2. radix-P butterflies over n1 (stride M) and the twiddle W_N^{n2 k1}
    for (int n2 = threadIdx.x; n2 < M; n2 += FT) {
        float2 v[P];
#pragma unroll
        for (int n1 = 0; n1 < P; ++n1) v[n1] = pm_load<IN>(xin, n1, n2, M, N, conj_io, io, q);
#ifdef B4D_DIAG
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        B4D_PM_STAMP(6);
#endif
        Dft<P>::run(v);
#pragma unroll
        for (int k1 = 0; k1 < P; ++k1) buf0[k1 * M + n2] = k1 == 0 ? v[0] : cmulf(v[k1], twN[n2 * k1]);
        B4D_PM_STAMP(7);
    }
    __syncthreads();
    B4D_PM_STAMP(2);
#ifndef B4D_EXP_PM_SKIP23
    // ---- 3. DFT_A over a (n2 = B a + b) for every (k1, b), then the twiddle W_M^{b c} = W_N^{P b c}: buf0 -> buf1[k1 M + c B + b]
    {
        auto col = [=](int k1, int b) { return k1 * M + b; };   // where column (k1, b) starts, before and after
        if (ONEBUF)
            dft_small_blocks<P, true>(tabA, A, B, B, B, buf0, twN, col, col);
        else if (blocked)   // strip column n = k1 * B + b
            dft_small_mfma<P, FT, true, true>(tabA, A, B, B, B, buf0, buf1, twN, col, col);
        else
            dft_small_roots<P, FT, true>(tabA, A, B, B, B, buf0, buf1, twN, col, col);
    }
    __syncthreads();
    B4D_PM_STAMP(3);
    // ---- 4. DFT_B over b (k2 = c + A d) for every (k1, c): buf1 -> natural order k = k1 + P (c + A d) in buf0
    {
        auto src = [=](int k1, int c) { return k1 * M + c * B; };
        auto dst = [=](int k1, int c) { return k1 + P * c; };
        if (ONEBUF)
            dft_small_blocks<P, false>(tabB, B, A, 1, P * A, buf0, twN, src, dst);
        else if (blocked)   // strip column n = c * P + k1: consecutive lanes store consecutive k
            dft_small_mfma<P, FT, false, false>(tabB, B, A, 1, P * A, buf1, buf0, twN, src, dst);
        else
            dft_small_roots<P, FT, false>(tabB, B, A, 1, P * A, buf1, buf0, twN, src, dst);
    }
    __syncthreads();
#endif
    B4D_PM_STAMP(4);
    // ---- 5. store
    pm_store<OUT, FT>(buf0, N, out, filt, conj_io, scale, io, q);
    B4D_PM_STAMP(5);
}

}  // namespace b4d

using namespace b4d;

// N = P * M with the largest power of two P <= 16; M = A * B with the smallest A + B: fused LDS path when the two small DFTs
// are cheap and the row fits in LDS
PmAxis b4d::pm_axis(int n, const float2* tw, const float2* dm) {
    PmAxis ax;
    ax.n = n;
    ax.tw = tw;
    ax.dm = dm;
    while (ax.P < 16 && n % (2 * ax.P) == 0) ax.P *= 2;
    ax.M = n / ax.P;
    int best = 1;
    for (int f = 1; (long long)f * f <= ax.M; ++f)
        if (ax.M % f == 0) best = f;
    const int a = ax.M / best, b = best;
    const size_t lds = sizeof(float2) * pm_lds_elems(ax.P, a, b);
    if (a + b <= 320 && lds <= 150 * 1024) {   // beyond ~300 complex MACs per element the chirp-z / DFT-matrix routes win
        ax.A = a;
        ax.B = b;
    }
    return ax;
}

template <int P, PmIn IN, PmOut OUT>
static int pm_fused_launch2(const PmAxis& ax, const void* x, float2* out, int S, const float2* filt, int conj_io, float scale,
                            const FusedIO& io, hipStream_t st) {
    const bool onebuf = pm_onebuf(P, ax.A, ax.B);
    const size_t lds = sizeof(float2) * pm_lds_elems(P, ax.A, ax.B, onebuf);
    // the attribute is asked for once at a fixed 150 KiB, whatever this call needs (launch() then finds it set)
    auto go = [&](auto kernel, int threads) -> int {
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), 150 * 1024)) return rc;
        return launch(kernel, dim3(S), dim3(threads), lds, st, x, out, ax.tw, ax.A, ax.B, filt, conj_io, scale, io);
    };
    return onebuf ? go(&k_pm_fused<P, IN, OUT, true>, FT_ONEBUF) : go(&k_pm_fused<P, IN, OUT, false>, FT_MAX);
}

// the compiled load / store pairs of k_pm_fused
template <int P>
static int pm_fused_launch(const PmAxis& ax, const void* x, PmIn im, PmOut om, float2* out, int S, const float2* filt, int conj_io,
                           float scale, const FusedIO& io, hipStream_t st) {
#define B4D_PM_PAIR(I, O) \
    if (im == PmIn::I && om == PmOut::O) return pm_fused_launch2<P, PmIn::I, PmOut::O>(ax, x, out, S, filt, conj_io, scale, io, st)
    B4D_PM_PAIR(Complex, Complex);
    B4D_PM_PAIR(Real, Complex);
    B4D_PM_PAIR(Reflect, Complex);       // Wiener, one side fused: forward rows ...
    B4D_PM_PAIR(Complex, Crop);          // ... and inverse rows
    B4D_PM_PAIR(ReflectPair, HalfPair);  // Wiener, both sides fused
    B4D_PM_PAIR(HermPair, CropPair);
    B4D_PM_PAIR(RealPair, HalfPair);     // pm_rows_pair_fwd / _inv
    B4D_PM_PAIR(HermPair, ShiftPair);
#undef B4D_PM_PAIR
    return fail(B4D_EINVAL, "fused row transform: no kernel for this load / store pair");
}

template <int P>
static int pm_pre_launch(const void* x, bool real_in, float2* y, const float2* tw, int M, int S, int conj_in, hipStream_t st) {
    const dim3 grid((M + 255) / 256, S);
    if (real_in)
        hipLaunchKernelGGL((k_pm_pre<P, true>), grid, dim3(256), 0, st, x, y, tw, M, conj_in);
    else
        hipLaunchKernelGGL((k_pm_pre<P, false>), grid, dim3(256), 0, st, x, y, tw, M, conj_in);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

int b4d::dft_rows(const PmAxis& ax, const void* in, PmIn im, float2* tmp, float2* tmp2, float2* out, PmOut om, int S, bool inverse,
                  const float2* filt, float scale, hipStream_t st, const FusedIO* fio) {
    int rc;
    if (ax.A > 0) {  // fused LDS transform (M = A * B)
        const FusedIO io = fio ? *fio : FusedIO{};
        switch (ax.P) {
            case 1: return pm_fused_launch<1>(ax, in, im, om, out, S, filt, inverse, scale, io, st);
            case 2: return pm_fused_launch<2>(ax, in, im, om, out, S, filt, inverse, scale, io, st);
            case 4: return pm_fused_launch<4>(ax, in, im, om, out, S, filt, inverse, scale, io, st);
            case 8: return pm_fused_launch<8>(ax, in, im, om, out, S, filt, inverse, scale, io, st);
            case 16: return pm_fused_launch<16>(ax, in, im, om, out, S, filt, inverse, scale, io, st);
            default: return fail(B4D_ESIZE, "unsupported radix");
        }
    }
    if ((im != PmIn::Complex && im != PmIn::Real) || om != PmOut::Complex)
        return fail(B4D_EINVAL, "DFT-matrix row transform: plain rows only");
    const bool real_in = im == PmIn::Real;
    switch (ax.P) {
        case 1: rc = pm_pre_launch<1>(in, real_in, tmp, ax.tw, ax.M, S, inverse, st); break;
        case 2: rc = pm_pre_launch<2>(in, real_in, tmp, ax.tw, ax.M, S, inverse, st); break;
        case 4: rc = pm_pre_launch<4>(in, real_in, tmp, ax.tw, ax.M, S, inverse, st); break;
        case 8: rc = pm_pre_launch<8>(in, real_in, tmp, ax.tw, ax.M, S, inverse, st); break;
        case 16: rc = pm_pre_launch<16>(in, real_in, tmp, ax.tw, ax.M, S, inverse, st); break;
        default: return fail(B4D_ESIZE, "unsupported radix");
    }
    if (rc) return rc;
    // (S*P, M) x (M, M); rows are independent, so slice the batch to keep the launch grid.y within limits
    const long long rows = (long long)S * ax.P;
    if ((rc = b4d_cgemm(tmp, false, 0, 0, ax.dm, false, 0, 0, tmp2, 0, (int)rows, ax.M, ax.M, 1, st))) return rc;
    hipLaunchKernelGGL(k_pm_post, dim3((ax.n + 255) / 256, S), dim3(256), 0, st, tmp2, out, ax.P, ax.M, filt, inverse ? 1 : 0, scale);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

int b4d::transpose_batch(const float2* in, float2* out, int rows, int cols, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_transpose_c, dim3((cols + 31) / 32, (rows + 31) / 32, batch), dim3(32, 8), 0, st, in, out, rows, cols);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

// ---- the fused row transform as a general-length 1-D engine (b4d_general.hip)
namespace b4d {
bool pm_fusable(int n) { return pm_axis(n).A > 0; }

// ---- Bluestein (chirp-z) for lengths without a fused split (a prime factor beyond ~300: 1042 = 2 * 521, 1031; 2056 = 8 * 257
// is fused with A = 257): with c[n] = exp(-i pi n^2 / N),
//   X[k] = c[k] * sum_n (x[n] c[n]) conj(c[k - n]),
// a convolution carried by two fused power-of-two transforms of length L >= 2 N - 1 and a pointwise product with the
// precomputed spectrum of the chirp.  Per-length tables are cached for the life of the process.
__global__ void __launch_bounds__(256) k_blue_pre(const void* __restrict__ xin, int real_in, int conj_in, int N, int L,
                                                  const float2* __restrict__ chirp, float2* __restrict__ a) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= L) return;
    const size_t s = blockIdx.y;
    float2 v = make_float2(0.f, 0.f);
    if (n < N) {
        float2 x;
        if (real_in) {
            x = make_float2(static_cast<const float*>(xin)[s * N + n], 0.f);
        } else {
            x = static_cast<const float2*>(xin)[s * N + n];
            if (conj_in) x.y = -x.y;
        }
        v = cmulf(x, chirp[n]);
    }
    a[s * (size_t)L + n] = v;
}

__global__ void __launch_bounds__(256) k_blue_post(const float2* __restrict__ c, int N, int L, const float2* __restrict__ chirp,
                                                   int conj_out, float scale, float2* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const size_t s = blockIdx.y;
    float2 v = cmulf(c[s * (size_t)L + k], chirp[k]);
    if (conj_out) v.y = -v.y;
    out[s * (size_t)N + k] = make_float2(v.x * scale, v.y * scale);
}

namespace {
struct BluePlan {
    int n = 0;
    PmAxis ax;                 // the power-of-two length L >= 2 n - 1 with its twiddles
    float2* chirp = nullptr;   // c[n] = exp(-i pi n^2 / N), n < N
    float2* bspec = nullptr;   // FFT_L of b[m] = conj(c[|m|]) wrapped to length L
};
std::mutex g_blue_mu;
std::vector<BluePlan> g_blue_plans;
void* g_blue_ws = nullptr;
size_t g_blue_ws_bytes = 0;

int blue_len(int n) {
    int L = 64;
    while (L < 2 * n - 1) L *= 2;
    return L;
}

int blue_plan(int n, hipStream_t st, BluePlan* out) {
    for (const BluePlan& p : g_blue_plans)
        if (p.n == n) {
            *out = p;
            return B4D_OK;
        }
    BluePlan p;
    p.n = n;
    const int L = blue_len(n);
    std::vector<float2> c(n), b(L, make_float2(0.f, 0.f));
    for (int k = 0; k < n; ++k) {
        const long long q = ((long long)k * k) % (2LL * n);        // k^2 mod 2N keeps the phase exact
        const double a = -M_PI * (double)q / (double)n;
        c[k] = make_float2((float)std::cos(a), (float)std::sin(a));
        const float2 bk = make_float2(c[k].x, -c[k].y);
        b[k] = bk;
        if (k) b[L - k] = bk;
    }
    float2* twL = nullptr;
    int rc = make_twiddles(L, &twL);
    if (rc) return rc;
    p.ax = pm_axis(L, twL);
    B4D_HIP(hipMalloc((void**)&p.chirp, sizeof(float2) * n));
    B4D_HIP(hipMalloc((void**)&p.bspec, sizeof(float2) * L));
    B4D_HIP(hipMemcpy(p.chirp, c.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    B4D_HIP(hipMemcpy(p.bspec, b.data(), sizeof(float2) * L, hipMemcpyHostToDevice));
    if (p.ax.A <= 0) return fail(B4D_ESIZE, "Bluestein length has no fused split");
    if ((rc = dft_rows(p.ax, p.bspec, PmIn::Complex, nullptr, nullptr, p.bspec, PmOut::Complex, 1, false, nullptr, 1.f, st))) return rc;
    B4D_HIP(hipStreamSynchronize(st));
    g_blue_plans.push_back(p);
    *out = p;
    return B4D_OK;
}

int blue_rows(const void* in, bool real_in, float2* out, int S, int n, bool inverse, float scale, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_blue_mu);
    BluePlan bp;
    int rc = blue_plan(n, st, &bp);
    if (rc) return rc;
    const int L = bp.ax.n;
    const size_t need = sizeof(float2) * (size_t)S * L;
    if (need > g_blue_ws_bytes) {
        if (g_blue_ws) (void)hipFree(g_blue_ws);
        g_blue_ws = nullptr;
        g_blue_ws_bytes = 0;
        hipError_t e = hipMalloc(&g_blue_ws, need);
        if (e != hipSuccess) return fail(B4D_ENOMEM, std::string("Bluestein workspace: ") + hipGetErrorString(e));
        g_blue_ws_bytes = need;
    }
    float2* a = static_cast<float2*>(g_blue_ws);
    hipLaunchKernelGGL(k_blue_pre, dim3((L + 255) / 256, S), dim3(256), 0, st, in, real_in ? 1 : 0, inverse ? 1 : 0, n, L, bp.chirp, a);
    B4D_HIP(hipGetLastError());
    FusedIO io{};
    io.filt_bcast = 1;
    if ((rc = dft_rows(bp.ax, a, PmIn::Complex, nullptr, nullptr, a, PmOut::Complex, S, false, bp.bspec, 1.f, st, &io))) return rc;
    if ((rc = dft_rows(bp.ax, a, PmIn::Complex, nullptr, nullptr, a, PmOut::Complex, S, true, nullptr, 1.0f / (float)L, st))) return rc;
    hipLaunchKernelGGL(k_blue_post, dim3((n + 255) / 256, S), dim3(256), 0, st, a, n, L, bp.chirp, inverse ? 1 : 0, scale, out);
    B4D_HIP(hipGetLastError());
    B4D_HIP(hipStreamSynchronize(st));   // the shared workspace is reused by the next call
    return B4D_OK;
}
}  // namespace

bool pm_supported(int n) { return n >= 2 && (pm_fusable(n) || n <= 4096); }

int pm_rows(const void* in, bool real_in, float2* out, int S, int n, const float2* tw, bool inverse, float scale, hipStream_t st) {
    const PmAxis ax = pm_axis(n, tw);
    if (ax.A <= 0) {
        if (n <= 4096) return blue_rows(in, real_in, out, S, n, inverse, scale, st);
        return fail(B4D_ESIZE, "length " + std::to_string(n) + " has no P * A * B split that fits the fused transform");
    }
    return dft_rows(ax, in, real_in ? PmIn::Real : PmIn::Complex, nullptr, nullptr, out, PmOut::Complex, S, inverse, nullptr, scale, st);
}
int pm_rows_pair_fwd(const float* in, float2* half_out, int frames, int rows, int n, const float2* tw, hipStream_t st) {
    const PmAxis ax = pm_axis(n, tw);
    if (ax.A <= 0) return fail(B4D_ESIZE, "pair transform needs a fused split");
    FusedIO io{};
    io.half = n / 2 + 1;
    io.rows = rows;
    return dft_rows(ax, in, PmIn::RealPair, nullptr, nullptr, half_out, PmOut::HalfPair, frames * ((rows + 1) / 2), false, nullptr, 1.f, st, &io);
}
int pm_rows_pair_inv(const float2* half_in, float* real_out, int frames, int rows, int n, const float2* tw, float scale, const float* peak,
                     hipStream_t st) {
    const PmAxis ax = pm_axis(n, tw);
    if (ax.A <= 0) return fail(B4D_ESIZE, "pair transform needs a fused split");
    FusedIO io{};
    io.half = n / 2 + 1;
    io.rows = rows;
    io.crop = real_out;
    io.amax = peak;
    io.norm_peak = peak ? 1 : 0;
    return dft_rows(ax, half_in, PmIn::HermPair, nullptr, nullptr, nullptr, PmOut::ShiftPair, frames * ((rows + 1) / 2), true, nullptr, scale, st, &io);
}
}  // namespace b4d

#ifdef B4D_DIAG
extern "C" int b4d_debug_set_pm_diag(void* buf) {
    unsigned long long* p = static_cast<unsigned long long*>(buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(b4d::g_pm_diag), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif
