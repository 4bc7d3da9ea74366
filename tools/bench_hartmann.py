"""Time of the Hartmann spot centroids (barc4dip_amd.signal.hartmann; csrc/b4d_hartmann.hip) on a resident (64, 2048, 2048) float32
stack at pitch 32 (64 x 64 cells a frame), background "border", threshold 0.1: the centre of gravity ("cog") and the iteratively
weighted one ("iwcog", 8 iterations) on the same stack.

Prints one JSON line and writes it to profiles/hartmann_bench.json (``--out``).  The entry point is timed on the whole stack in
windows of a few calls between two stream events (median over ``--windows`` windows); ``spot_centroids`` is the public call with
``return_tensors=True`` on the same device tensor.

Byte model: 4 B per pixel read (every frame is read once, whatever the iterations) plus 112 B per cell written; the share is the
model's bytes at the achievable streaming rate of the microarchitecture guide, 6.29 TB/s, over the measured time.  The second
figure is iwcog over cog: what eight more passes over the staged cells cost.

    python tools/bench_hartmann.py [--frames 64] [--windows 7] [--out profiles/hartmann_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2048
PITCH = 32
ITERATIONS = 8
HBM_BYTES_PER_S = 6.29e12


def _window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def _timed(torch, fn, windows):
    fn()
    fn()
    torch.cuda.synchronize()
    calls = max(1, min(20, int(0.05 / max(_window(torch, fn, 1), 1e-6))))
    return statistics.median(_window(torch, fn, calls) for _ in range(windows)), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hartmann_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from barc4dip_amd import _ffi, synth
    from barc4dip_amd.signal import hartmann as H

    torch.cuda.set_device(0)
    T = args.frames
    rng = np.random.default_rng(0)
    cells = H.hartmann_cells((N, N), PITCH)
    gy, gx = cells["shape"]
    d = rng.uniform(-3.0, 3.0, (2, gy, gx))
    frame = synth.hartmann_frame((N, N), PITCH, (0, 0), (d[0], d[1]), sigma=2.0, background=5.0, seed=1).astype(np.float32)
    x = torch.from_numpy(frame).cuda()[None].expand(T, N, N).contiguous()
    out = torch.empty((T, gy, gx, len(H.QUANTITIES)), dtype=torch.float64, device="cuda")
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    ye, xe = cells["y_edges"], cells["x_edges"]
    sigma = 0.25 * PITCH

    def entry(method):
        return lambda: _ffi.check(lib.b4d_spot_centroids(
            C.c_void_p(x.data_ptr()), T, N, N, ye.ctypes.data_as(C.c_void_p), gy, xe.ctypes.data_as(C.c_void_p), gx, 3, 0.0, 0.1,
            method, sigma, ITERATIONS, float("inf"), C.c_void_p(out.data_ptr()), st))

    model_bytes = 4 * T * N * N + 112 * T * gy * gx
    res = {"tool": "bench_hartmann", "device": torch.cuda.get_device_name(0), "frames": T, "frame": N, "pitch": PITCH,
           "cells_per_frame": gy * gx, "iterations": ITERATIONS, "windows": args.windows, "hbm_model_bytes_per_s": HBM_BYTES_PER_S,
           "model_bytes": model_bytes, "kernel": {}, "public": {}}
    for code, name in enumerate(H.METHODS):
        t, calls = _timed(torch, entry(code), args.windows)
        res["kernel"][name] = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t, "cells_per_s": T * gy * gx / t,
                               "effective_bytes_per_s": model_bytes / t, "share_of_hbm_model": model_bytes / HBM_BYTES_PER_S / t}
        t, calls = _timed(torch, lambda: H.spot_centroids(x, cells, method=name, iterations=ITERATIONS, return_tensors=True), args.windows)
        res["public"][name] = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t}
    res["iwcog_over_cog"] = res["kernel"]["iwcog"]["s_per_call"] / res["kernel"]["cog"]["s_per_call"]
    # the centroids of the timed stack against the programmed shifts, so that the timing is of a call that measures something
    got = H.spot_centroids(x[:1], cells, method="iwcog", iterations=ITERATIONS)
    res["rms_error_px"] = float(np.sqrt(np.mean((got["cy"][0] - (cells["y"][:, None] + d[0])) ** 2)))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
