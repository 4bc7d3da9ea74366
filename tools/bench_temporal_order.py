"""Cost of the temporal order statistics (barc4dip_amd.metrics.order: b4d_temporal_quantiles, b4d_temporal_robust_mean) on
resident stacks of T frames of N x N float32 (default 2048^2 x T in {9, 32, 64, 256}).

Prints one JSON line and writes it to --out.  Per shape, device time between stream events, best (and median) of --reps calls:

  accumulate    b4d_temporal_accumulate over the same stack: the project's read-once floor, the yardstick of this run.
  median        b4d_temporal_quantiles, q = 0.5, midpoint.
  percentiles3  one call with the 5th, 50th and 95th percentile, linear.
  robust        b4d_temporal_robust_mean (MAD scale), mean + median + scale + n_kept.
  robust_full   the same with the (T, npix) outputs rejected and cleaned.
  *_general     median and robust with flags bit 0 at T <= 64: what the register route buys.
  torch_median, torch_quantile3   torch.median(dim=0) / torch.quantile of the same tensor: what a user of the library had to call.

Reported per route: seconds per call, the bytes of the stack per second (4 B / px / frame; outputs are not in the model) and that
rate as a fraction of the accumulate rate of the same shape.

    python tools/bench_temporal_order.py [--frames 9,32,64,256] [--size 2048] [--reps 5] [--out profiles/temporal_order_bench.json]
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


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="9,32,64,256")
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.median / torch.quantile comparators")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_order_bench.json"))
    args = ap.parse_args()
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi

    torch.cuda.set_device(0)
    N = args.size
    npix = N * N
    lib, sp, null = _ffi.lib(), _ffi.stream_ptr(), C.c_void_p(0)
    out = {"tool": "bench_temporal_order", "device": torch.cuda.get_device_name(0), "ny": N, "nx": N, "reps": args.reps, "shapes": {}}
    q1 = np.array([0.5], dtype=np.float64)
    q3 = np.array([0.05, 0.5, 0.95], dtype=np.float64)
    for T in [int(v) for v in args.frames.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(7)
        # counting noise around 400 with zingers in one sample of a thousand: ties and outliers, as in a stack of flats
        stack = torch.poisson(torch.full((T, npix), 400.0, device="cuda"), generator=gen)
        stack = torch.where(torch.rand((T, npix), device="cuda", generator=gen) < 1e-3, stack * 6.0, stack).contiguous()
        sx = torch.zeros(npix, dtype=torch.float64, device="cuda")
        sxx = torch.zeros(npix, dtype=torch.float64, device="cuda")
        res = torch.empty((3, npix), dtype=torch.float32, device="cuda")
        f = [torch.empty(npix, dtype=torch.float32, device="cuda") for _ in range(3)]
        nk = torch.empty(npix, dtype=torch.int16, device="cuda")
        rej = torch.empty((T, npix), dtype=torch.uint8, device="cuda")
        cl = torch.empty((T, npix), dtype=torch.float32, device="cuda")

        def accumulate():
            _ffi.check(lib.b4d_temporal_accumulate(D.ptr(stack), T, npix, D.ptr(sx), D.ptr(sxx), sp))

        def quant(q, method, flags=0):
            _ffi.check(lib.b4d_temporal_quantiles(D.ptr(stack), T, npix, npix, q.ctypes.data_as(C.c_void_p), int(q.size), method, 0, flags,
                                                  D.ptr(res), null, sp))

        def robust(full, flags=0):
            _ffi.check(lib.b4d_temporal_robust_mean(D.ptr(stack), T, npix, npix, 1, 5.0, 1.0, 0, flags, D.ptr(f[0]), D.ptr(f[1]), D.ptr(f[2]),
                                                    D.ptr(nk), D.ptr(rej) if full else null, D.ptr(cl) if full else null, npix, sp))

        routes = [("accumulate", accumulate), ("median", lambda: quant(q1, 4)), ("percentiles3", lambda: quant(q3, 0)),
                  ("robust", lambda: robust(False)), ("robust_full", lambda: robust(True))]
        if T <= 64 and T >= 32:
            routes += [("median_general", lambda: quant(q1, 4, 1)), ("robust_general", lambda: robust(False, 1))]
        if not args.no_torch:
            qt = torch.tensor([0.05, 0.5, 0.95], device="cuda")
            routes += [("torch_median", lambda: torch.median(stack, dim=0)), ("torch_quantile3", lambda: torch.quantile(stack, qt, dim=0))]
        shape = {"frames": T, "stack_bytes": 4 * T * npix}
        for key, fn in routes:
            try:
                fn()                       # warm-up: code objects, allocator
                torch.cuda.synchronize()
                times = [_timed(fn) for _ in range(args.reps)]
            except RuntimeError as e:      # torch.quantile refuses large inputs; the comparator is then absent
                shape[key] = {"error": str(e).splitlines()[0][:160]}
                continue
            best = min(times)
            shape[key] = {"s_best": best, "s_median": statistics.median(times), "stack_tb_per_s": 4 * T * npix / best / 1e12}
            print(f"T={T} {key}: {best * 1e3:.3f} ms", file=sys.stderr, flush=True)
        acc = shape["accumulate"]["stack_tb_per_s"]
        for key, _ in routes:
            if "stack_tb_per_s" in shape[key]:
                shape[key]["share_of_accumulate"] = shape[key]["stack_tb_per_s"] / acc
        out["shapes"][str(T)] = shape
        del stack, rej, cl
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
