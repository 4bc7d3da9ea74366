"""Time of the spatial rank filters, outlier repair and uint16 conversion (barc4dip_amd.preprocessing.rank, barc4dip_amd.utils;
csrc/b4d_rankfilt.hip) on a resident (64, 2048, 2048) float32 stack.

Prints one JSON line and writes it to profiles/filters_bench.json (``--out``).  Every case is timed in windows of a few calls
between two stream events; a window of plain device copies of the same stack (1 GiB read, 1 GiB written: the 8 B / px stream) is
timed right before each window of the case, alternating in one process, and the figures are the medians over ``--windows``
windows: seconds per call, frames per second, and ``share_of_stream`` = (8 B / px at the copy rate of the neighbouring windows)
/ (time of the case).  Cases:

  median_filter 3 / 5 / 7        register route, output written
  general route 3 / 7            the same medians through the counting passes (``_general=True``)
  range only 3                   no output frame: nanmin / nanmax per frame (4 B / px)
  remove_outliers 3 / 5          scale="mad", mask and counts not requested
  scale_to_u16 / to_uint16       the device part on the resident stack (range-only median + scaling: 4 + 6 B / px) and the public
                                 call on the host array (upload, mean, range, scaling, download; wall clock)
  scipy                          scipy.ndimage.median_filter of ONE frame on the host, 3 / 5 / 7

    python tools/bench_filters.py [--frames 64] [--windows 7] [--out profiles/filters_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2048


def _window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def _alternating(torch, fn, copy, windows):
    """Medians over `windows` pairs (copy window, case window): (seconds per call, seconds per copy, case / copy ratio)."""
    fn()
    copy()
    torch.cuda.synchronize()
    calls = max(1, min(20, int(0.02 / max(_window(torch, fn, 1), 1e-6))))
    ccalls = max(1, min(20, int(0.02 / max(_window(torch, copy, 1), 1e-6))))
    ts, cs = [], []
    for _ in range(windows):
        cs.append(_window(torch, copy, ccalls))
        ts.append(_window(torch, fn, calls))
    return statistics.median(ts), statistics.median(cs), statistics.median(t / c for t, c in zip(ts, cs)), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filters_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import scipy.ndimage as ndi
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi, utils
    from barc4dip_amd.preprocessing import rank as R

    torch.cuda.set_device(0)
    T = args.frames
    base = np.random.default_rng(0).poisson(3.0, (min(T, 8), N, N)).astype(np.float32)    # mean 3: to_uint16 takes the scaling branch
    host = np.ascontiguousarray(np.tile(base, (-(-T // base.shape[0]), 1, 1))[:T])
    host.reshape(-1)[::100003] = 4000.0                                               # zingers
    x = torch.from_numpy(host).cuda()
    dst = torch.empty_like(x)
    u16 = torch.empty(tuple(x.shape), dtype=torch.int16, device="cuda")
    npix = T * N * N

    def copy():
        dst.copy_(x)

    def device_u16():
        vmin, vmax = utils.filtered_minmax_range(x, 3)
        _ffi.check(_ffi.lib().b4d_scale_to_u16(D.ptr(x), npix, vmin * 0.95, 65535 / np.sqrt(2) / (vmax / 0.95 - vmin * 0.95), 1, D.ptr(u16),
                                               _ffi.stream_ptr()))

    cases = {
        "median_filter_3": (lambda: R.median_filter(x, 3, return_tensors=True), 8),
        "median_filter_5": (lambda: R.median_filter(x, 5, return_tensors=True), 8),
        "median_filter_7": (lambda: R.median_filter(x, 7, return_tensors=True), 8),
        "general_route_3": (lambda: R.median_filter(x, 3, return_tensors=True, _general=True), 8),
        "general_route_7": (lambda: R.median_filter(x, 7, return_tensors=True, _general=True), 8),
        "range_only_3": (lambda: R.run_rank_filter(x, T, N, N, 3, 3, 4, 1, 0.0, want_out=False, want_range=True), 4),
        "remove_outliers_3_mad": (lambda: R.remove_outliers(x, 3, scale="mad", return_tensors=True), 8),
        "remove_outliers_5_mad": (lambda: R.remove_outliers(x, 5, scale="mad", return_tensors=True), 8),
        "to_uint16_device_part": (device_u16, 10),
    }
    out = {"tool": "bench_filters", "device": torch.cuda.get_device_name(0), "frames": T, "frame": N, "windows": args.windows, "cases": {}}
    copies = []
    for name, (fn, bytes_per_px) in cases.items():
        t, c, ratio, calls = _alternating(torch, fn, copy, args.windows)
        copies.append(c)
        out["cases"][name] = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t, "bytes_per_px": bytes_per_px,
                              "achieved_bytes_per_s": bytes_per_px * npix / t, "copy_s": c, "time_over_copy": ratio,
                              "share_of_stream": 1.0 / ratio}
    out["copy_s"] = statistics.median(copies)
    out["copy_bytes_per_s"] = 8.0 * npix / out["copy_s"]
    out["copy_frames_per_s"] = T / out["copy_s"]

    wall = []
    for _ in range(3):                              # host staging and the download are part of this path: wall clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        utils.to_uint16(host)
        wall.append(time.perf_counter() - t0)
    out["to_uint16_host_array"] = {"wall_s": statistics.median(wall), "frames_per_s": T / statistics.median(wall),
                                   "host_bytes_in": 4.0 * npix, "host_bytes_out": 2.0 * npix}

    out["scipy_one_frame"] = {}
    for size in (3, 5, 7):
        t0 = time.perf_counter()
        ref = ndi.median_filter(host[0], size=size)
        s = time.perf_counter() - t0
        same = bool(np.array_equal(R.median_filter(host[0], size), ref))
        gpu = out["cases"][f"median_filter_{size}"]["frames_per_s"]
        out["scipy_one_frame"][f"median_filter_{size}"] = {"s": s, "frames_per_s": 1.0 / s, "gpu_over_scipy": gpu * s, "gpu_equals_scipy": same,
                                                           "threads": os.environ.get("OMP_NUM_THREADS")}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
