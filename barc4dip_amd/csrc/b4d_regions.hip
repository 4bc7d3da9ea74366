// b4d_regions.hip -- the three kernels behind region_list (b4d_regions.hpp).
#include "b4d_regions.hpp"

namespace b4d {

// ---- effective labels (0 where some frame is non-finite) and pixels per (span, region).  grid (nspan), one wave
template <bool LAB_READY>
__global__ void __launch_bounds__(64) k_rg_count(const int* __restrict__ labels, const uint8_t* __restrict__ bad, long long npix, int R,
                                                 long long span, uint8_t* __restrict__ lab, int* __restrict__ cnt) {
    __shared__ int n[RG_MAX_R + 1];
    const int lane = threadIdx.x;
    for (int r = lane; r <= RG_MAX_R; r += 64) n[r] = 0;
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * span, p1 = min(npix, p0 + span);
    for (long long g = p0; g < p1; g += 64) {
        const long long p = g + lane;
        int l = 0;
        if (p < p1) {
            l = LAB_READY ? (int)lab[p] : region_label(labels, p, R);
            if (bad && bad[p]) l = 0;
            lab[p] = (uint8_t)l;
        }
        for_each_label(l, [&](int r, int lead, bool, unsigned long long mask) {
            if (lane == lead) n[r] += __popcll(mask);
        });
    }
    __syncthreads();
    for (int r = lane; r < R; r += 64) cnt[(size_t)blockIdx.x * R + r] = n[r + 1];
}

// ---- exclusive prefix of the counts over the spans, per region: lane l takes the spans [l * per, (l + 1) * per).
// grid (R), one wave
__global__ void __launch_bounds__(64) k_rg_prefix(const int* __restrict__ cnt, int nspan, int R, int* __restrict__ base,
                                                  RegionMeta* __restrict__ meta) {
    __shared__ long long tot[64];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int per = (nspan + 63) / 64;
    const int b0 = min(nspan, lane * per), b1 = min(nspan, b0 + per);
    long long a = 0;
    for (int b = b0; b < b1; ++b) a += cnt[(size_t)b * R + r];
    tot[lane] = a;
    __syncthreads();
    long long run = 0;
    for (int k = 0; k < lane; ++k) run += tot[k];
    for (int b = b0; b < b1; ++b) {
        base[(size_t)b * R + r] = (int)run;
        run += cnt[(size_t)b * R + r];
    }
    if (lane == 63) meta->N[r] = run;
}

// ---- granule ranges of the regions and the pixel counts handed to the caller.  one thread
__global__ void k_rg_segments(RegionMeta* __restrict__ meta, int R, int gran, long long* __restrict__ n_pixels) {
    int g = 0;
    for (int r = 0; r < R; ++r) {
        meta->start[r] = g;
        g += (int)((meta->N[r] + gran - 1) / gran);
        if (n_pixels) n_pixels[r] = meta->N[r];
    }
    meta->start[R] = g;
}

void region_list(const int* labels, bool lab_ready, const uint8_t* bad, long long npix, int R, long long span, int nspan, int gran,
                 uint8_t* lab, int* cnt, int* base, RegionMeta* meta, long long* n_pixels, hipStream_t st) {
    hipLaunchKernelGGL(lab_ready ? k_rg_count<true> : k_rg_count<false>, dim3(nspan), dim3(64), 0, st, labels, bad, npix, R, span, lab,
                       cnt);
    hipLaunchKernelGGL(k_rg_prefix, dim3(R), dim3(64), 0, st, cnt, nspan, R, base, meta);
    hipLaunchKernelGGL(k_rg_segments, dim3(1), dim3(1), 0, st, meta, R, gran, n_pixels);
}

}  // namespace b4d
