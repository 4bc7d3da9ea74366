// b4d_lanes.hpp -- two-lane launch groups: the fork / join of the caller's stream and the library's second one (host only).
#pragma once
#include <algorithm>

#include "b4d_common.hpp"

// What a plan keeps for its two-lane drivers: the library's shared lane_stream(0) and this plan's fork / join events, all made on
// first use.  b4d_plan embeds one.
struct LaneSync {
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

// A multi-pass transform whose intermediate is written and read once runs faster in groups whose workspace is about 64 MiB -- it
// stays in the 256-MB memory-side cache -- and with the groups dealt alternately to the caller's stream and a second one, so that
// the passes of one group run under those of the other (no drained chip between two launches, transform phases of one kernel under
// the memory phases of another).  Measured, frames/s (tools/dev_fft2d_chunk.py, tools/dev_pipe_chunk.py): fft2d 2048^2 61.7 k in
// 64-frame groups, 61.8 k in 4-frame groups, 66.5-67.7 k in 4-frame groups on two lanes; 1024^2 268 -> 277 k; 2160 x 2560
// 28.0 -> 31.4 k; psd + autocorr 2160 x 2560 20.0 -> 22.4 k, 1080 x 1920 55 -> 62.8 k, 228^2 1.72 -> 1.91 M.  (The power-of-two
// psd + autocorr pipeline gains 1 % at 2048^2 and keeps its single large groups.)
//
// A forked Lanes joins the second lane into the caller's stream on EVERY exit of its scope: close() on the success path (it
// returns the join's status), the destructor on an early return (best effort; last_error() keeps the message of the failure that
// caused the exit).  Without the join the shared lane would go on working in the plan's buffers unordered against the next call.
struct Lanes {
    LaneSync* ls = nullptr;
    hipStream_t st = nullptr;
    bool two = false;
    int sub = 1;   // frames per group; lane l works in slot l of the workspaces (slot stride: `sub` frames)
    bool forked = false;   // the second lane waits on ev_fork and has not been joined yet

    Lanes() = default;
    Lanes(const Lanes&) = delete;
    Lanes& operator=(const Lanes&) = delete;
    ~Lanes() {
        if (forked && hipEventRecord(ls->ev_join, ls->aux) == hipSuccess) (void)hipStreamWaitEvent(st, ls->ev_join, 0);
    }

    // the stream part alone (group sizes are the caller's)
    int fork(LaneSync& l, hipStream_t s, bool want_two) {
        ls = &l;
        st = s;
        two = want_two && b4d::g_opt_lanes.load() != 0;
        if (!two) return B4D_OK;
        if (!l.aux)
            if (const int rs = b4d::lane_stream(0, &l.aux)) return rs;
        if (!l.ev_fork) B4D_HIP(hipEventCreateWithFlags(&l.ev_fork, hipEventDisableTiming));
        if (!l.ev_join) B4D_HIP(hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming));
        B4D_HIP(hipEventRecord(l.ev_fork, st));
        B4D_HIP(hipStreamWaitEvent(l.aux, l.ev_fork, 0));
        forked = true;
        return B4D_OK;
    }
    // groups of about 64 MiB of intermediate out of a plan's `chunk` frames.  inter_bytes: intermediate bytes per frame; two lanes
    // need 2 * sub <= chunk and groups of at least min_group_bytes of input (below that the launches themselves are what a group
    // costs: 256^2 frames in two lanes of 64, 2.3 against 2.9 M frames/s)
    int open(LaneSync& l, int chunk, hipStream_t s, int batch, size_t inter_bytes, size_t frame_bytes, bool allow_two,
             size_t min_group_bytes) {
        const int want = (int)std::max<size_t>(1, ((size_t)64 << 20) / std::max<size_t>(1, inter_bytes));
        // two lanes need two slots of the workspaces and enough work to pay for the fork / join (a few microseconds of host time)
        const bool want_two = allow_two && b4d::g_opt_lanes.load() != 0 && batch >= 2 && chunk >= 2 &&
                              (size_t)batch * frame_bytes >= 2 * min_group_bytes &&
                              (size_t)std::min(want, chunk / 2) * frame_bytes >= min_group_bytes;
        sub = want_two ? std::min(want, chunk / 2) : chunk;   // one lane: the plan's own groups
        if (want_two) {   // an even number of groups of equal size
            int groups = (batch + sub - 1) / sub;
            groups += groups & 1;
            sub = (batch + groups - 1) / groups;
        }
        return fork(l, s, want_two);
    }
    hipStream_t stream(int g) const { return two && (g & 1) ? ls->aux : st; }
    int slot(int g) const { return two ? (g & 1) : 0; }
    // joins the second lane into the caller's stream; a second call (and the destructor after it) does nothing
    int close() {
        if (!forked) return B4D_OK;
        forked = false;
        B4D_HIP(hipEventRecord(ls->ev_join, ls->aux));
        B4D_HIP(hipStreamWaitEvent(st, ls->ev_join, 0));
        return B4D_OK;
    }
};
