"""Cost of the fringe analysis (barc4dip_amd.signal.fringe_displacement: b4d_fringe_demodulate, b4d_fringe_compare,
b4d_phase_unwrap, b4d_fringe_shift) on T frames of N x N float32, window 32, step 16, two carriers.

Prints one JSON line and writes it to --out.  With the frames, the reference and every result resident on the device:

  demodulate    one b4d_fringe_demodulate call on the T frames (tables + the demodulation kernel).
  displacement  the whole of fringe_displacement(reference, frames, carriers=..., return_tensors=True): the demodulation of the
                frames and of the reference, the comparison, the unwrap of 2 T maps and the shift.

The two alternate window by window in one process; a window holds >= --min-s of work and is timed with device events.
Reported: seconds per call as the median and best of --reps windows, frames per second, and for the demodulation the achieved
bytes per second on the model of one read of every frame (4 B / px; the three harmonic maps written are 2.3 % of that) next to the
project's streaming yardstick, the temporal-statistics kernel at 5.9-6.1 TB/s.

    python tools/bench_fringes.py [--frames 64] [--size 2048] [--reps 5] [--min-s 0.5] [--out profiles/fringes_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CARRIERS = np.array([[0.004, 0.127], [0.123, -0.006]])
WINDOW, STEP = 32, 16
YARDSTICK_TBS = (5.9, 6.1)


def _window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fringes_bench.json"))
    ap.add_argument("--demodulate-only", action="store_true", help="time b4d_fringe_demodulate alone (for a kernel trace)")
    args = ap.parse_args()
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd.signal import fringes

    torch.cuda.set_device(0)
    T, N = args.frames, args.size
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    # frames built on the device: fringes at the two carriers, frame t shifted by a smooth field that grows with t, plus noise
    y = torch.arange(N, dtype=torch.float64, device="cuda")[:, None]
    x = torch.arange(N, dtype=torch.float64, device="cuda")[None, :]
    gen = torch.Generator(device="cuda").manual_seed(7)

    def frame(amp):
        uy, ux = amp * torch.sin(2.0 * np.pi * x / N), amp * torch.cos(2.0 * np.pi * y / N)
        f = torch.ones((N, N), dtype=torch.float64, device="cuda")
        for fy, fx in CARRIERS:
            f = f + 0.4 * torch.cos(2.0 * np.pi * (fy * (y - uy) + fx * (x - ux)))
        return (1000.0 * f).to(torch.float32) + 10.0 * torch.randn((N, N), dtype=torch.float32, device="cuda", generator=gen)

    ref = frame(0.0)
    frames = torch.stack([frame(0.8 * (t + 1) / T) for t in range(T)])
    g = fringes.fringe_grid((N, N), window=WINDOW, step=STEP)
    gy, gx = g["shape"]
    ws = torch.empty(int(lib.b4d_fringe_demodulate_workspace_bytes(2, N, N, WINDOW, WINDOW)), dtype=torch.uint8, device="cuda")
    harm = torch.empty((T, 3, gy, gx), dtype=torch.complex64, device="cuda")
    fbuf = (C.c_double * 4)(*CARRIERS.ravel().tolist())

    def demodulate():
        _ffi.check(lib.b4d_fringe_demodulate(D.ptr(frames), T, N, N, C.cast(fbuf, C.c_void_p), 2, WINDOW, WINDOW, STEP, STEP, D.ptr(ws),
                                             D.ptr(harm), st))

    def displacement():
        return fringes.fringe_displacement(ref, frames, carriers=CARRIERS, window=WINDOW, step=STEP, return_tensors=True)

    demodulate()
    res = displacement()
    torch.cuda.synchronize()
    out = {"tool": "bench_fringes", "device": torch.cuda.get_device_name(0), "frames": T, "ny": N, "nx": N, "window": WINDOW, "step": STEP,
           "carriers": CARRIERS.tolist(), "grid": [gy, gx], "reps": args.reps, "min_s": args.min_s,
           "largest_shift_px": float(torch.maximum(res["dy"].abs().max(), res["dx"].abs().max())),
           "smallest_peak": float(res["peak"].min())}
    routes = [("demodulate", demodulate)] + ([] if args.demodulate_only else [("displacement", displacement)])
    iters = {}
    for key, fn in routes:
        _window(fn, 2)
        iters[key] = max(2, int(np.ceil(args.min_s / _window(fn, 2))))
    times = {key: [] for key, _ in routes}
    for _ in range(args.reps):
        for key, fn in routes:
            times[key].append(_window(fn, iters[key]))
    for key, _ in routes:
        med = statistics.median(times[key])
        out[key] = {"s_median": med, "s_best": min(times[key]), "calls_per_window": iters[key], "frames_per_s": T / med}
    model_bytes = 4 * T * N * N          # every frame read once; kept with the benchmark
    out["demodulate"]["model_bytes"] = model_bytes
    out["demodulate"]["model_tb_per_s"] = model_bytes / out["demodulate"]["s_median"] / 1e12
    out["demodulate"]["yardstick_tb_per_s"] = list(YARDSTICK_TBS)
    out["demodulate"]["share_of_yardstick"] = out["demodulate"]["model_tb_per_s"] / YARDSTICK_TBS[0]
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
