// b4d_common.hpp -- error plumbing shared by the translation units of libb4d.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>

#include "../../include/b4d.h"

namespace b4d {

// thread-local message behind b4d_last_error(); defined in b4d_kernels.hip
std::string& last_error();
inline int fail(int code, const std::string& msg) {
    last_error() = msg;
    return code;
}
// workspace carving: sizes rounded up to 256 bytes
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// pointer predicates of the entry points: p on a multiple of `bytes` (a power of two; null is aligned), and whether two byte
// ranges share an address (a null pointer never overlaps)
inline bool ptr_aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
inline bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + bbytes && b0 < a0 + abytes;
}
// lazily grown device scratch for second-stage reductions, one buffer per caller stream; defined in b4d_kernels.hip
int get_scratch(size_t bytes, void** out, hipStream_t stream);
// serialises the host side of every entry point that works in a scratch buffer (re-entrant calls from several host
// threads, e.g. joblib workers, on one stream); device-side ordering comes from the stream, and different streams get
// different buffers.  Defined in b4d_kernels.hip
std::recursive_mutex& scratch_mutex();
#define B4D_SCRATCH_LOCK() std::lock_guard<std::recursive_mutex> b4d_scratch_lk__(::b4d::scratch_mutex())

// b4d_set_option switches (defined next to it, b4d_kernels.hip): routes only, never results; read once per entry-point call
extern std::atomic<int> g_opt_track_predict;   // "track_predict_bin" 0 / 1 / 2
extern std::atomic<int> g_opt_lanes;           // "lanes": two-lane launch groups (Lanes, b4d_lanes.hpp); 0 = the caller's stream only
extern std::atomic<int> g_opt_ysplit;          // "ysplit": parity-tile route of 2048-row PSD + autocorrelation; 0 = off
extern std::atomic<int> g_opt_row16;           // "row16": 16-byte global accesses in the row passes of that route; 0 = narrow kernels
extern std::atomic<int> g_opt_colsets;         // "colsets": column-set tiles between the forward row pass and the column pass of that route
extern std::atomic<int> g_opt_exp;             // "exp": development A/B switch (kernel variants under test; 0 = shipped)

// hipFuncAttributeMaxDynamicSharedMemorySize >= bytes for `kernel` on the CURRENT device, set once per (kernel address, device):
// a flag per launcher template would be per process (a second GPU of the process never gets the attribute), one per
// function-pointer type would be shared by kernels of one signature.  Defined in b4d_kernels.hip.
int ensure_dynamic_lds(const void* kernel, size_t bytes);
// The library's own streams (b4d_kernels.hip): two non-blocking streams per device, created on first use and shared by every
// plan -- a process has few hardware queues (4 by default), and a second lane that lands on the queue of the caller's stream
// serialises behind it (measured: a two-lane Wiener pass 5.8 k frames/s against 7.3 k on one lane, 8.0 k on a queue of its own)
int lane_stream(int idx, hipStream_t* out);

#define B4D_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess)                                                             \
            return ::b4d::fail(B4D_EHIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// The launch of every kernel that takes dynamic LDS (and of any other): the dynamic-LDS attribute where lds != 0
// (ensure_dynamic_lds), the launch, and its one error check.  The arguments are converted to the kernel's own parameter types.
template <class... P, class... A>
static int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    if (lds)
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

}  // namespace b4d
