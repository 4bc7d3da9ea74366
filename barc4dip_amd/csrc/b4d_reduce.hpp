// b4d_reduce.hpp -- the wave and workgroup reductions of every unit (device only).  The library promises fixed-order,
// bit-reproducible sums: the order of operations of each helper is part of its contract and is written out here once.
// All 64 lanes of a wave must be active at a call.  "Down" forms: step o = 32, 16, .., 1, lane l combines its value with that of
// lane l + o (lanes without a partner combine with their own), so ONLY LANE 0 holds the result: ((l0 + l32) + (l16 + l48)) + ..
// "All" forms: the same steps as a butterfly with lane l ^ o; every lane holds the result (for sums the same bits in
// every lane: lane l and its partner add the same two numbers at every step).
#pragma once
#include <hip/hip_runtime.h>

namespace b4d {

// ------------------------------------------------------------------------------------ wave level
template <class T>
__device__ __forceinline__ T wave_sum(T v) {   // result in lane 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_sum_all(T v) {   // result in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {   // fmaxf (a NaN never wins); result in lane 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_min(unsigned v) {   // result in lane 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_down(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_min_all(unsigned v) {   // result in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_max_all(unsigned v) {   // result in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// (value, flat index) arg-max with NumPy's first-occurrence rule: larger value wins, ties go to the lower index, a NaN never wins
template <class T>
__device__ __forceinline__ void argmax_merge(T& v, int& i, T ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
template <class T>
__device__ __forceinline__ void wave_argmax(T& v, int& i) {   // result in lane 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_down(v, o, 64);
        const int oi = __shfl_down(i, o, 64);
        argmax_merge(v, i, ov, oi);
    }
}
template <class T>
__device__ __forceinline__ void wave_argmax_all(T& v, int& i) {   // result in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        argmax_merge(v, i, ov, oi);
    }
}

// inclusive scan: lane l returns v[0] + .. + v[l] (steps o = 1, 2, .., 32: lane l >= o adds the running value of lane l - o)
__device__ __forceinline__ unsigned wave_scan_inclusive(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// ------------------------------------------------------------------------------------ workgroup level
// NV sums of doubles per lane over a workgroup of nw full waves indexed by threadIdx.x.  sh: LDS, nw rows of NV doubles, one row
// per wave.  Every form first takes the wave sums (lane 0 of wave w writes row w), passes ONE barrier -- the whole workgroup must
// call -- and then adds the rows in wave order starting FROM 0.0: s = 0.0; s += sh[0][k]; s += sh[1][k]; ..  (A combine
// written sh[0] + sh[1] + .. gives other bits for a first partial of -0.0 and is not one of these.)  There is no barrier behind
// the combine: a caller that writes sh again before its next barrier adds one.

// thread 0 adds every column; v is valid in thread 0 only
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh, int nw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) sh[wave * NV + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = 0.0;
            for (int w = 0; w < nw; ++w) s += sh[w * NV + k];
            v[k] = s;
        }
    }
}
// thread k < NV adds column k and returns it (the other threads return 0.0): thread 0 never holds NV x nw loads at once
template <int NV>
__device__ __forceinline__ double block_sum_columns(double (&v)[NV], double* sh, int nw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) sh[wave * NV + k] = v[k];
    }
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < NV)
        for (int w = 0; w < nw; ++w) s += sh[w * NV + threadIdx.x];
    return s;
}
// every lane adds every column (after wave_sum_all); v is valid in every lane
template <int NV>
__device__ __forceinline__ void block_sum_all(double (&v)[NV], double* sh, int nw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = wave_sum_all(v[k]);
        if (lane == 0) sh[wave * NV + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = 0.0;
        for (int w = 0; w < nw; ++w) v[k] += sh[w * NV + k];
    }
}

// Halving tree over a workgroup of exactly 256 threads, which must all call; sh: 256 doubles of LDS.  Thread t brings its partial a:
// sh[t] = a, then sh[t] += sh[t + o] for o = 128, 64, .., 1 with a barrier per step; every thread returns sh[0].  again: the caller
// writes sh again (a second call) before its next barrier, so a trailing barrier is passed.
__device__ __forceinline__ double block_tree_sum256(double a, double* sh, bool again) {
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double t = sh[0];
    if (again) __syncthreads();
    return t;
}

// Workgroup arg-max by argmax_merge's rule: every lane brings its own (bv, bi) and every lane returns with the merged pair of the
// workgroup: wave_argmax, then every lane merges the waves 1 .. nwaves - 1 into wave 0's pair in order.  sv / si: LDS, one word
// per wave (nwaves = blockDim.x / 64).  It contains a barrier: the WHOLE workgroup must call it, and sv / si must not be written
// again before the workgroup's next barrier.
__device__ __forceinline__ void block_argmax(float& bv, int& bi, float* sv, int* si, int nwaves) {
    wave_argmax(bv, bi);
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = bv;
        si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
    for (int k = 1; k < nwaves; ++k) argmax_merge(bv, bi, sv[k], si[k]);
}

}  // namespace b4d
