"""Throughput of dense NCC displacement maps (barc4dip_amd.signal.displacement_map, b4d_displacement_map).

Prints one JSON line.  For each (window, step, search) on a 2048^2 pair and on a T = 64 stack of 1024^2 frames against one
reference: device time per call (frames resident, results left on the device), windows/s and pairs/s.  For comparison the
composed route on the same windows: boxes cut on the device + template_matching_batch (a power-of-two FFT canvas per box),
timed on the first `--composed-windows` windows of the 2048^2 grid (the rate is per window; the full grid would not fit its
canvases in memory for the small steps).

    python tools/bench_displacement.py [--reps 5] [--composed-windows 4096]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [(31, 16, 8), (63, 32, 32), (15, 4, 4)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-windows", type=int, default=4096)
    args = ap.parse_args()
    import torch

    from barc4dip_amd import synth
    from barc4dip_amd.signal import displacement_grid, displacement_map, template_matching_batch

    torch.cuda.set_device(0)
    out = {"tool": "bench_displacement", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": []}
    big = synth.speckle_stack_device(2, 2048)
    stack = synth.speckle_stack_device(65, 1024)
    for win, step, srch in CONFIGS:
        kw = dict(window=win, step=step, search=srch, return_tensors=True)
        g = displacement_grid((2048, 2048), window=win, step=step, search=srch)
        nwin = g["shape"][0] * g["shape"][1]
        t = _time(lambda: displacement_map(big[0], big[1], **kw), args.reps)
        case = {"window": win, "step": step, "search": srch, "frame": 2048, "pairs": 1, "windows": nwin, "s": t,
                "windows_per_s": nwin / t, "pairs_per_s": 1 / t}
        gs = displacement_grid((1024, 1024), window=win, step=step, search=srch)
        nws = gs["shape"][0] * gs["shape"][1] * 64
        ts = _time(lambda: displacement_map(stack[0], stack[1:], **kw), args.reps)
        case["stack"] = {"frame": 1024, "pairs": 64, "windows": nws, "s": ts, "windows_per_s": nws / ts, "pairs_per_s": 64 / ts}
        # composed route: cut boxes on the device + the FFT template tracker, same windows (a prefix of the grid)
        sel = list(np.ndindex(*g["shape"]))[:args.composed_windows]
        b = win + 2 * srch
        ys = torch.tensor([int(g["y0"][i]) - srch for i, _ in sel], device="cuda")
        xs = torch.tensor([int(g["x0"][j]) - srch for _, j in sel], device="cuda")
        ar = torch.arange(b, device="cuda")
        iy = (ys[:, None, None] + ar[None, :, None]).expand(-1, b, b)
        ix = (xs[:, None, None] + ar[None, None, :]).expand(-1, b, b)
        k = len(sel)
        idx = np.arange(k)
        roi = [[srch, srch + win, srch, srch + win]] * k

        def composed():
            boxes = big[1][iy, ix]
            tboxes = big[0][iy, ix]
            return template_matching_batch(boxes, tboxes, idx, roi, idx, idx, backend="opencv")

        tc = _time(composed, max(1, args.reps // 2))
        case["composed"] = {"windows": k, "s": tc, "windows_per_s": k / tc, "speedup_of_direct": (nwin / t) / (k / tc)}
        out["cases"].append(case)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
