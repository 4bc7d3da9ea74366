"""Cost of the phase-stepping analysis (barc4dip_amd.signal.stepping: b4d_stepping_fit, b4d_stepping_compare,
b4d_stepping_calibrate_step) on one scan of T frames of N x N float32 (default 16 x 2048^2, 256 MiB), resident on the device
before any timing.

Prints one JSON line and writes it to --out.  Timed, alternating window by window in one process:

  accumulate  b4d_temporal_accumulate over the same stack: the project's existing one-read-of-a-stack kernel, the yardstick of
              this run (it also reads and writes two float64 maps, 32 B / px, 1/2 of the stack at T = 16: not in its model).
  fit         b4d_stepping_fit, K = 1 (and fit_k2: K = 2), host tables included.
  compare     b4d_stepping_compare of the fitted coefficients against themselves as a shared reference.
  calibrate   b4d_stepping_calibrate_step: the frame sums over the stack plus the one-workgroup update (no host read).

A window holds >= --min-s of work and is timed with device events.  Reported per route: seconds per call as the median and best
of --reps windows, the bytes of the stack per second (4 B / px / frame; outputs are not in the model), and for the fit and the
calibration iteration that rate as a fraction of the accumulate rate of the same run.

    python tools/bench_stepping.py [--frames 16] [--size 2048] [--reps 5] [--min-s 0.3] [--out profiles/stepping_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--only", default=None, help="time one route alone (for a kernel trace or a counter run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stepping_bench.json"))
    args = ap.parse_args()
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd.signal import stepping as st

    torch.cuda.set_device(0)
    T, N = args.frames, args.size
    npix = N * N
    lib, sp = _ffi.lib(), _ffi.stream_ptr()
    # the scan, built on the device: fringes with a mean, visibility and phase that vary over the frame, steps off their nominal
    # positions, plus noise
    rng = np.random.default_rng(5)
    nominal = 2.0 * np.pi * np.arange(T) / T
    true = nominal.copy()
    true[1:] += rng.uniform(-0.2, 0.2, T - 1)
    y = torch.arange(N, dtype=torch.float32, device="cuda")[:, None]
    x = torch.arange(N, dtype=torch.float32, device="cuda")[None, :]
    a0 = 1000.0 * (1.0 + 0.3 * torch.cos(x / 170.0) * torch.sin(y / 110.0))
    vis = 0.3 + 0.1 * torch.sin(x / 130.0)
    ph = 2.0 * np.pi * (x / 9.7 + 2.0e-5 * (y - N / 2.0) ** 2)
    gen = torch.Generator(device="cuda").manual_seed(7)
    stack = torch.stack([a0 * (1.0 + vis * torch.cos(float(true[t]) + ph)) + 5.0 * torch.randn((N, N), device="cuda", generator=gen)
                         for t in range(T)]).reshape(1, T, npix).contiguous()
    del a0, vis, ph

    sx = torch.zeros(npix, dtype=torch.float64, device="cuda")
    sxx = torch.zeros(npix, dtype=torch.float64, device="cuda")
    coeff = {K: torch.empty((1, 2 * K + 1, npix), dtype=torch.float32, device="cuda") for K in (1, 2)}
    res = torch.empty((1, npix), dtype=torch.float32, device="cuda")
    ns = torch.empty((1, npix), dtype=torch.uint8, device="cuda")
    tabs = {K: st._tables(nominal, K) for K in (1, 2)}
    outs = [torch.empty((1, 1, npix), dtype=torch.float32, device="cuda") for _ in range(4)]
    trans = torch.empty((1, npix), dtype=torch.float32, device="cuda")
    valid = torch.empty((1, 1, npix), dtype=torch.uint8, device="cuda")
    cal_out = torch.empty(1 + 3 * T, dtype=torch.float64, device="cuda")
    delta = np.ascontiguousarray(nominal - nominal[0])
    inf = float("inf")

    def accumulate():
        _ffi.check(lib.b4d_temporal_accumulate(D.ptr(stack), T, npix, D.ptr(sx), D.ptr(sxx), sp))

    def fit(K=1):
        B, G, Gi = tabs[K]
        _ffi.check(lib.b4d_stepping_fit(D.ptr(stack), 1, T, npix, K, st._hp(B), st._hp(G), st._hp(Gi), inf, D.ptr(coeff[K]), D.ptr(res),
                                        D.ptr(ns), sp))

    def compare():
        _ffi.check(lib.b4d_stepping_compare(D.ptr(coeff[1]), D.ptr(coeff[1]), 0, 1, 1, npix, D.ptr(outs[0]), D.ptr(outs[1]), None,
                                            D.ptr(trans), D.ptr(outs[2]), D.ptr(outs[3]), D.ptr(valid), sp))

    def calibrate():
        B, _, Gi = tabs[1]
        _ffi.check(lib.b4d_stepping_calibrate_step(D.ptr(stack), T, npix, st._hp(B), st._hp(Gi), st._hp(delta), inf, D.ptr(cal_out), sp))

    routes = [("accumulate", accumulate), ("fit", fit), ("fit_k2", lambda: fit(2)), ("compare", compare)]
    if st.CAL_MIN_STEPS <= T <= st.CAL_MAX_STEPS:
        routes.append(("calibrate", calibrate))
    if args.only:
        routes = [r for r in routes if r[0] == args.only]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    out = {"tool": "bench_stepping", "device": torch.cuda.get_device_name(0), "frames": T, "ny": N, "nx": N, "reps": args.reps,
           "min_s": args.min_s, "stack_bytes": 4 * T * npix}
    if any(k == "calibrate" for k, _ in routes):      # the full calibration of this scan, for the record
        steps, info = st._calibrate_device(stack[0], nominal, inf, 1e-9, 200)
        out["calibration"] = {"iterations": info["iterations"], "change": info["change"],
                              "largest_step_error_rad": float(np.max(np.abs(steps - true)))}
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
        out[key] = {"s_median": med, "s_best": min(times[key]), "calls_per_window": iters[key]}
        if key != "compare":
            out[key]["stack_tb_per_s"] = 4 * T * npix / med / 1e12
    if "accumulate" in out:
        for key in ("fit", "fit_k2", "calibrate"):
            if key in out:
                out[key]["share_of_accumulate"] = out[key]["stack_tb_per_s"] / out["accumulate"]["stack_tb_per_s"]
    if "compare" in out:     # 2 coefficient sets of 12 B read, 4 maps + transmission of 4 B and a byte written per pixel
        out["compare"]["model_bytes"] = (24 + 21) * npix
        out["compare"]["model_tb_per_s"] = out["compare"]["model_bytes"] / out["compare"]["s_median"] / 1e12
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
