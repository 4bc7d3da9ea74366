// b4d_mfma.hpp -- v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate, bit-for-bit an fmaf chain) on a workgroup of four waves in
// 2 x 2: the accumulator type, the lane maps, and for the 128 x 128 real kernels (each wave 2 x 2 tiles of 32 x 32) the multiply
// over one K slab staged in LDS and the walk over the accumulators.  Staging and epilogues stay in the kernels.  The context is
// passed by value and the row index keeps the sum order base + register part + 4 lk: both hold the kernels' register counts.
// Lane maps (MI355X guide section 3), lane l of a wave with li = l & 31, lk = l >> 5:
//   A: the lane holds A[i = li][k = lk];  B: B[k = lk][j = li];  C/D: register reg is col = li, row = (reg & 3) + 8 (reg >> 2) + 4 lk.
#pragma once
#include <hip/hip_runtime.h>

namespace b4d {

struct WaveTile { int wr, wc, li, lk; };   // wave (wr, wc) of the 2 x 2, lane split (li, lk)
__host__ __device__ __forceinline__ WaveTile wave_tile(int tid) {   // tid = threadIdx.x of a 256-lane workgroup
    const int lane = tid & 63, wave = tid >> 6;
    return WaveTile{wave >> 1, wave & 1, lane & 31, lane >> 5};
}

// place of C/D register r inside a 32 x 32 tile whose first row is `base`
__host__ __device__ constexpr int mfma_row(int r, int lk, int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * lk; }
__host__ __device__ constexpr int mfma_col(int li) { return li; }

// f(row, col, value) over the 2 x 2 x 16 accumulator entries of a wave; (m0, n0) is the corner of the workgroup's 128 x 128 tile
template <class Acc, class F>
__host__ __device__ __forceinline__ void for_each(const Acc (&acc)[2][2], const WaveTile t, int m0, int n0, F&& f) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + 64 * t.wc + 32 * j + mfma_col(t.li);
#pragma unroll
            for (int r = 0; r < 16; ++r) f(mfma_row(r, t.lk, m0 + 64 * t.wr + 32 * i), col, acc[i][j][r]);
        }
}

#ifdef __HIPCC__
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void zero(f32x16& v) { v = 0.f; }
__device__ __forceinline__ void zero(f32x16 (&acc)[2][2]) { zero(acc[0][0]), zero(acc[0][1]), zero(acc[1][0]), zero(acc[1][1]); }

// acc += A . B over one slab in LDS: As[k][m], Bs[k][n], KD deep, rows of LD floats
template <int KD, int LD>
__device__ __forceinline__ void mma_slab(const float (*As)[LD], const float (*Bs)[LD], const WaveTile t, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int kk = 0; kk < KD; kk += 2) {
        const float a0 = As[kk + t.lk][64 * t.wr + t.li], a1 = As[kk + t.lk][64 * t.wr + 32 + t.li];
        const float b0 = Bs[kk + t.lk][64 * t.wc + t.li], b1 = Bs[kk + t.lk][64 * t.wc + 32 + t.li];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}
#endif

}  // namespace b4d
