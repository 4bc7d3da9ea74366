"""Throughput of distortion correction (barc4dip_amd.preprocessing.correct_distortion: b4d_spline_prefilter + b4d_warp_grid).

Prints one JSON line.  For order 1 and 3 with a grid field (the window grid of a (31, 16, 8) displacement map, +-8 px) on a
2048^2 frame, a T = 64 stack of 1024^2 frames with one shared field, and a 2160 x 2560 frame: device time per call, frames/s
and the fraction of 8 TB/s.  A call is the C-ABI launches of one correct_distortion (prefilter for order 3, then the warp) on
resident buffers, `--calls` of them back to back between two events, so that the Python overhead of the public function
(a few tens of microseconds, more than a 2048^2 order-1 warp takes) does not enter; `api_s` is the public call, timed the same
way.  Bytes model:
    order 1: 8 B/px (read the frame, write the output; the grid field is a few KB and stays in cache)
    order 3: 24 B/px (prefilter: read frame + write coefficients, then read + write them in place; warp: read + write)
    a dense field adds 8 B/px (its two float32 planes), reported once for order 1 on the stack.

    python tools/bench_distortion.py [--reps 5] [--calls 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12
BYTES_PER_PX = {1: 8, 3: 24}


def _time(fn, reps, calls):
    """Best over `reps` of the mean time of `calls` back-to-back calls."""
    import torch

    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3 / calls)
    return best


def _abi_call(x, field, order, mode="nearest"):
    """The launches of correct_distortion(x, field, order=order, mode=mode) on preallocated buffers, as a closure."""
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd._frames import mode_code
    from barc4dip_amd.preprocessing import distortion as DI

    lib, st = _ffi.lib(), _ffi.stream_ptr()
    H, W = (int(s) for s in x.shape[-2:])
    n = int(x.numel() // (H * W))
    p = DI.SPLINE_PAD if mode == "nearest" else 0
    coef = torch.empty((n, H + 2 * p, W + 2 * p), device="cuda") if order == 3 else None
    out = torch.empty((n, H, W), device="cuda")
    src = coef if order == 3 else x
    m = mode_code(mode)
    if isinstance(field, dict):
        f = DI._parse_field(field, tuple(x.shape))
        gy, gx = f["plane"]
        fy = torch.as_tensor(field["dy"], dtype=torch.float32, device="cuda").contiguous()
        fx = torch.as_tensor(field["dx"], dtype=torch.float32, device="cuda").contiguous()
        warp = lambda: lib.b4d_warp_grid(D.ptr(src), n, H, W, order, m, 0.0, D.ptr(fy), D.ptr(fx), 1, gy, gx,  # noqa: E731
                                         f["y0"], f["sy"], f["x0"], f["sx"], D.ptr(out), st)
    else:
        fy, fx = field
        warp = lambda: lib.b4d_warp_dense(D.ptr(src), n, H, W, order, m, 0.0, D.ptr(fy), D.ptr(fx), 1, D.ptr(out), st)  # noqa: E731

    def call():
        if order == 3:
            _ffi.check(lib.b4d_spline_prefilter(D.ptr(x), n, H, W, m, D.ptr(coef), st))
        _ffi.check(warp())
    return call


def _grid(shape, seed):
    import numpy as np

    from barc4dip_amd.signal import displacement_grid

    g = displacement_grid(shape, window=31, step=16, search=8)
    rng = np.random.default_rng(seed)
    return {"dy": rng.uniform(-8, 8, g["shape"]), "dx": rng.uniform(-8, 8, g["shape"]), "y": g["y"], "x": g["x"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch

    from barc4dip_amd import synth
    from barc4dip_amd.preprocessing import correct_distortion

    torch.cuda.set_device(0)
    out = {"tool": "bench_distortion", "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
           "hbm_bytes_per_s": HBM,
           "bytes_per_px": {"order1": 8, "order3": 24, "dense_field_extra": 8}, "cases": []}
    inputs = [("2048x2048", synth.speckle_stack_device(1, 2048)[0]), ("64x1024x1024", synth.speckle_stack_device(64, 1024)),
              ("2160x2560", synth.speckle_stack_device(1, 2560)[0, :2160].contiguous())]
    for name, x in inputs:
        H, W = (int(s) for s in x.shape[-2:])
        T = int(x.shape[0]) if x.ndim == 3 else 1
        g = _grid((H, W), seed=1)
        for order in (1, 3):
            t = _time(_abi_call(x, g, order), args.reps, args.calls)
            ta = _time(lambda: correct_distortion(x, g, order=order, return_tensors=True), args.reps, args.calls)
            px = T * H * W
            out["cases"].append({"input": name, "field": "grid", "order": order, "s": t, "frames_per_s": T / t,
                                 "px_per_s": px / t, "hbm_fraction": BYTES_PER_PX[order] * px / t / HBM, "api_s": ta})
        if T > 1:
            fy = torch.empty((H, W), device="cuda").uniform_(-8, 8)
            fx = torch.empty((H, W), device="cuda").uniform_(-8, 8)
            t = _time(_abi_call(x, (fy, fx), 1), args.reps, args.calls)
            out["cases"].append({"input": name, "field": "dense", "order": 1, "s": t, "frames_per_s": T / t,
                                 "px_per_s": T * H * W / t, "hbm_fraction": (8 + 8) * T * H * W / t / HBM})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
