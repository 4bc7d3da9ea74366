"""Throughput of speckle scanning (barc4dip_amd.signal.speckle_scan, b4d_speckle_scan).

Prints one JSON line and writes it to profiles/scanning_bench.json.  For (window, search) = (5, 2), (9, 4), (15, 4), flat and Hann
taper: device time per call on a 2048^2 scan of N = 25 positions and on M = 8 scans of 1024^2 against one reference (inputs
resident, results left on the device, time between stream events, best of ``--reps``), and pixels x shifts x positions per
second; also with ``subpixel=False`` and, on the 2048^2 scan, with a sample that is the displaced reference (the generated frames
are independent, which makes the sub-pixel sweep revisit every shift).  In the same run ``displacement_map(step=1, subpixel=False)`` is timed at the same window and search on one frame pair --
the only other way to a per-pixel field -- and N x that time is reported beside the scan with the ratio of the two.

    python tools/bench_scanning.py [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(5, 2), (9, 4), (15, 4)]
TAPERS = ("flat", "hann")
N_POSITIONS = 25


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


def _case(ref, smp, win, srch, reps, step1=True):
    from barc4dip_amd.signal import displacement_map, speckle_scan

    N, H, W = (int(s) for s in ref.shape)
    M = 1 if smp.ndim == 3 else int(smp.shape[0])
    work = M * N * (H - 2 * (win // 2 + srch)) * (W - 2 * (win // 2 + srch)) * (2 * srch + 1) ** 2
    out = {"frame": W, "scans": M, "positions": N, "pixel_shift_positions": work}
    for taper in TAPERS:
        t = _time(lambda: speckle_scan(ref, smp, window=win, search=srch, taper=taper, return_tensors=True), reps)
        out[taper] = {"s": t, "pixel_shift_positions_per_s": work / t}
    t = _time(lambda: speckle_scan(ref, smp, window=win, search=srch, subpixel=False, return_tensors=True), reps)
    out["hann_integer"] = {"s": t, "pixel_shift_positions_per_s": work / t}
    if smp.ndim == 3:
        # the frames of the generated stack are independent, so the peaks scatter and the sub-pixel sweep revisits every shift;
        # a sample that is the displaced reference is the other end: every pixel of a tile asks for the same four neighbours
        import torch

        moved = 0.8 * torch.roll(ref, (1, -2), dims=(-2, -1))
        t = _time(lambda: speckle_scan(ref, moved, window=win, search=srch, return_tensors=True), reps)
        out["hann_uniform_shift"] = {"s": t, "pixel_shift_positions_per_s": work / t}
        del moved
    if step1:
        pair = smp[0] if smp.ndim == 3 else smp[0, 0]
        td = _time(lambda: displacement_map(ref[0], pair, window=win, step=1, search=srch, subpixel=False, return_tensors=True), reps)
        out["displacement_map_step1_pair_s"] = td
        out["n_times_step1_s"] = M * N * td
        out["n_times_step1_over_scan"] = {taper: M * N * td / out[taper]["s"] for taper in TAPERS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    from barc4dip_amd import synth

    torch.cuda.set_device(0)
    out = {"tool": "bench_scanning", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": []}
    big = synth.speckle_stack_device(2 * N_POSITIONS, 2048)
    small = synth.speckle_stack_device(9 * N_POSITIONS, 1024)
    ref_s, smp_s = small[:N_POSITIONS], small[N_POSITIONS:].reshape(8, N_POSITIONS, 1024, 1024)
    for win, srch in CONFIGS:
        case = {"window": win, "search": srch}
        case.update(_case(big[:N_POSITIONS], big[N_POSITIONS:], win, srch, args.reps))
        case["batch"] = _case(ref_s, smp_s, win, srch, args.reps)
        out["cases"].append(case)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scanning_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
