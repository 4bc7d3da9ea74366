"""Time of the two-time correlation (barc4dip_amd.metrics.two_time_correlation, b4d_two_time) on resident stacks.

Prints one JSON line and writes it to profiles/two_time_bench.json (``--out``).  For T = 256 frames of 2048^2 and T = 1024 frames
of 1024^2 (no labels, norm "pearson", full band): device time per call of ``two_time_correlation`` (stack resident, results left on
the device); the stage times of b4d_two_time_timed (scan, pack, product, reduce); the product kernel's TFLOP/s counting the
useful flop of the upper frame-block pairs of 128 (T (T + 128) K for T a multiple of 128, two flop per multiply-add) and its
share of the 155 TF float32 matrix rate; the scan and pack passes against their byte counts; the device's copy rate measured in
the same run and the bound max(flop / 155 TF, packed bytes / copy rate); and a float64 NumPy baseline (``d @ d.T`` with the
host's BLAS) on a size it can finish, scaled to the case by its flop count.

    python tools/bench_two_time.py [--reps 3] [--out profiles/two_time_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(256, 2048), (1024, 1024)]
MATRIX_TF = 155.0


def _time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def _copy_rate(torch, reps):
    src = torch.empty(1 << 30, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = _time(lambda: dst.copy_(src), reps)
    return 2.0 * src.numel() * 4 / t


def _stages(x, T, npix, reps):
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    ws = torch.empty(int(lib.b4d_two_time_workspace_bytes(T, npix, 1, T - 1)), dtype=torch.uint8, device=x.device)
    out = [torch.empty(n, dtype=torch.float64, device=x.device) for n in (T * T, T, T)]
    npx = torch.empty(1, dtype=torch.int64, device=x.device)
    ms = (C.c_float * 4)()
    best = [float("inf")] * 4
    for _ in range(reps + 1):
        _ffi.check(lib.b4d_two_time_timed(D.ptr(x), T, npix, None, 1, 0, T - 1, D.ptr(ws), D.ptr(out[0]), D.ptr(out[1]), D.ptr(out[2]),
                                          D.ptr(npx), _ffi.stream_ptr(), C.cast(ms, C.c_void_p)))
        best = [min(b, float(m) * 1e-3) for b, m in zip(best, ms)]
    return dict(zip(("scan_s", "pack_s", "product_s", "reduce_s"), best)), ws.numel()


def _numpy_baseline(T, K):
    import numpy as np

    d = np.random.default_rng(0).standard_normal((T, K))
    d @ d.T
    t0 = time.perf_counter()
    d @ d.T
    t = time.perf_counter() - t0
    return {"T": T, "pixels": K, "s": t, "gflops": 2.0 * T * T * K / t * 1e-9, "threads": os.environ.get("OMP_NUM_THREADS")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_time_bench.json"))
    args = ap.parse_args()
    import torch

    from barc4dip_amd.metrics import two_time_correlation

    torch.cuda.set_device(0)
    rate = _copy_rate(torch, args.reps)
    base = _numpy_baseline(256, 512 * 512)
    out = {"tool": "bench_two_time", "device": torch.cuda.get_device_name(0), "reps": args.reps, "matrix_tf": MATRIX_TF,
           "copy_bytes_per_s": rate, "numpy_float64": base, "cases": []}
    for T, n in CASES:
        npix = n * n
        x = torch.empty((T, n, n), dtype=torch.float32, device="cuda").exponential_(0.01)      # fully developed speckle, mean 100
        call = _time(lambda: two_time_correlation(x, return_tensors=True), args.reps)
        st, ws_bytes = _stages(x.reshape(T, npix), T, npix, args.reps)
        nb = -(-T // 128)
        flop = nb * (nb + 1) // 2 * 128 * 128 * 2.0 * npix
        stack_bytes = 4.0 * T * npix
        bound = max(flop / (MATRIX_TF * 1e12), 2.0 * stack_bytes / rate)
        case = {"T": T, "frame": n, "call_s": call, "workspace_bytes": ws_bytes, **st,
                "product_flop": flop, "product_tflops": flop / st["product_s"] * 1e-12,
                "product_share_of_matrix_rate": flop / st["product_s"] * 1e-12 / MATRIX_TF,
                "scan_bytes": stack_bytes, "scan_bytes_per_s": stack_bytes / st["scan_s"],
                "pack_bytes": 2.0 * stack_bytes, "pack_bytes_per_s": 2.0 * stack_bytes / st["pack_s"],
                "bound_s": bound, "bound_is": "flop" if flop / (MATRIX_TF * 1e12) >= 2.0 * stack_bytes / rate else "bytes",
                "numpy_float64_scaled_s": 2.0 * T * T * npix / (base["gflops"] * 1e9)}
        out["cases"].append(case)
        del x
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
