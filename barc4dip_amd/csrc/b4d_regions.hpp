// b4d_regions.hpp -- the region-ordered pixel list of the label-map metrics (b4d_twotime.hip, b4d_multitau.hip; DESIGN.md
// section 20, "The region list").  From a label map and a per-pixel "non-finite in some frame" byte: every pixel of region 1,
// then of region 2, .., raster order within a region, each region padded to whole granules (a chunk of the two-time product, a
// wave of the multi-tau correlator).  The list fixes the order of every sum of both units, so it is built in one place:
//   count     effective labels as bytes (0 outside 1 .. R and where bad) and pixels per (span, region)
//   prefix    exclusive prefix of the counts over the spans, per region -> base[span][r], meta->N[r]
//   segments  granule ranges of the regions -> meta->start
// (region_list, b4d_regions.hip), after which a caller's one-wave-per-span kernel places its pixels with for_each_label and
// region_slot.  Spans are whole 64-pixel groups cut by pixel position; their length is the caller's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace b4d {

constexpr int RG_MAX_R = 64;

struct RegionMeta {
    long long N[RG_MAX_R];        // pixels of region r + 1
    int start[RG_MAX_R + 1];      // first granule of region r + 1; [R] = granules in use
};

// label of pixel p: 0 outside 1 .. R; without a label map every pixel is region 1
__device__ __forceinline__ int region_label(const int* __restrict__ labels, long long p, int R) {
    if (!labels) return 1;
    const int v = labels[p];
    return v < 1 || v > R ? 0 : v;
}

// By-label grouping of a wave: l is the lane's label (0 = none).  Each distinct label of the wave is visited once, in the order
// of the first lane that holds it: body(r, lead, mine, mask) with r the label, lead that lane, mine = "this lane holds r" and
// mask the ballot of mine.  All 64 lanes must call, and the body runs with the whole wave converged (it may shuffle and pass
// barriers).
template <class F>
__device__ __forceinline__ void for_each_label(int l, F body) {
    unsigned long long todo = __ballot(l > 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int r = __shfl(l, lead, 64);
        const bool mine = l == r;
        const unsigned long long mask = __ballot(mine);
        todo &= ~mask;
        body(r, lead, mine, mask);
    }
}

// Slot of a lane of label r in the list, inside for_each_label of a one-wave workgroup: run[r] (LDS, seeded with base[span][r - 1])
// is the region's pixels earlier in the span, the lanes of r below this one follow.  GRAN = pixels per granule.  Every lane
// reads run[r], barrier, the lead lane adds the group's pixels, barrier.
template <int GRAN>
__device__ __forceinline__ long long region_slot(const RegionMeta* __restrict__ meta, int* run, int r, int lead, int lane,
                                                 unsigned long long mask) {
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    const long long dst = (long long)meta->start[r - 1] * GRAN + run[r] + rank;
    __syncthreads();
    if (lane == lead) run[r] += __popcll(mask);
    __syncthreads();
    return dst;
}

// Launches count, prefix and segments on the stream.  lab_ready: lab already holds region_label's bytes (labels is not read);
// otherwise they are taken from labels.  bad may be null.  lab gets the effective labels, cnt and base nspan x R ints,
// n_pixels (device, may be null) the R pixel counts.  gran: pixels per granule.
void region_list(const int* labels, bool lab_ready, const uint8_t* bad, long long npix, int R, long long span, int nspan, int gran,
                 uint8_t* lab, int* cnt, int* base, RegionMeta* meta, long long* n_pixels, hipStream_t st);

}  // namespace b4d
