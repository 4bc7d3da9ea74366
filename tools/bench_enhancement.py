"""Time of CLAHE (barc4dip_amd.preprocessing.enhancement; csrc/b4d_enhance.hip) on a resident (64, 2048, 2048) stack, grid 8 x 8,
clip_limit 2.0, at three depths: 8-bit levels (256 bins), 16-bit levels (65536 bins, the bin-slice path) and float32 frames at 4096
levels.

Prints one JSON line and writes it to profiles/enhancement_bench.json (``--out``).  Each of the three kernels is timed on its own,
on the whole stack with a workspace for the whole stack, in windows of a few calls between two stream events (median over
``--windows`` windows); ``clahe`` is the public call with ``return_tensors=True`` on a device tensor of the same frames (uint8 or float32),
which cuts the stack into chunks of at most 256 MiB of workspace and, for float frames, looks for each frame's range first.

Byte model (per frame of P pixels with B = tiles x levels bins; the share is the model's bytes at the achievable streaming rate of
the microarchitecture guide, 6.29 TB/s, over the measured time):

  tile_histogram   4 P read (above 32768 levels every further bin slice reads the tile again, from L2) + 4 B counts written
  equalize_lut     4 B counts read (the second read of the scan comes from L2) + 2 B table written
  lut_apply        4 P read + 4 P written + 2 B table read (gathered; every tile's table is read by many workgroups, from L2)
  all three        12 P + 12 B: at 256 levels B is 16 Ki bins, nothing; at 65536 levels 4 Mi bins, 50 MB against 50 MB of frames

    python tools/bench_enhancement.py [--frames 64] [--windows 7] [--out profiles/enhancement_bench.json]
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
GRID = (8, 8)
CLIP = 2.0
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhancement_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from barc4dip_amd import _ffi
    from barc4dip_amd.preprocessing import enhancement as E

    torch.cuda.set_device(0)
    T = args.frames
    rng = np.random.default_rng(0)
    tile = lambda a: torch.from_numpy(np.ascontiguousarray(np.tile(a, (-(-T // a.shape[0]), 1, 1))[:T])).cuda()  # noqa: E731
    stacks = {
        "u8_256": (tile(np.minimum(rng.poisson(40.0, (4, N, N)), 255).astype(np.float32)), 256, True, (0.0, 256.0)),
        "u16_65536": (tile(rng.poisson(40000.0, (4, N, N)).astype(np.float32)), 65536, True, (0.0, 65536.0)),
        "f32_4096": (tile(rng.normal(1.0, 0.1, (4, N, N)).astype(np.float32)), 4096, False, (0.5, 1.5)),
    }
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    tiles, npix = GRID[0] * GRID[1], T * N * N
    out = {"tool": "bench_enhancement", "device": torch.cuda.get_device_name(0), "frames": T, "frame": N, "grid": list(GRID),
           "clip_limit": CLIP, "windows": args.windows, "hbm_model_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}
    for name, (x, L, integer, (lo, hi)) in stacks.items():
        q = (np.tile(np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32), (T, 1)) if integer
             else np.tile(E.quantiser(np.float32(lo), np.float32(hi), L), (T, 1)))
        q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        counts = torch.empty((T, tiles, L), dtype=torch.int32, device="cuda")
        n_valid = torch.empty((T, tiles), dtype=torch.int32, device="cuda")
        lut = torch.empty((T, tiles, L), dtype=torch.int16, device="cuda")
        res = torch.empty_like(x)
        flags = 0 if integer else 1
        null = C.c_void_p(0)
        kernels = {
            "tile_histogram": lambda: _ffi.check(lib.b4d_tile_histogram(p(x), T, N, N, GRID[0], GRID[1], L, p(q), p(counts), p(n_valid), st)),
            "equalize_lut": lambda: _ffi.check(lib.b4d_equalize_lut(p(counts), p(n_valid), T, tiles, L, CLIP, 0, p(lut), null, st)),
            "lut_apply": lambda: _ffi.check(lib.b4d_lut_apply(p(x), T, N, N, GRID[0], GRID[1], L, p(q), p(lut), null, flags, p(res), st)),
        }
        bins = T * tiles * L
        model = {"tile_histogram": 4 * npix + 4 * bins, "equalize_lut": 6 * bins, "lut_apply": 8 * npix + 2 * bins}
        case = {"levels": L, "kernels": {}}
        total = 0.0
        for kname, fn in kernels.items():
            t, calls = _timed(torch, fn, args.windows)
            total += t
            case["kernels"][kname] = {"s_per_call": t, "calls_per_window": calls, "model_bytes": model[kname],
                                      "effective_bytes_per_s": model[kname] / t, "share_of_hbm_model": model[kname] / HBM_BYTES_PER_S / t}
        all_bytes = 12 * npix + 12 * bins
        case["kernels_total"] = {"s_per_call": total, "frames_per_s": T / total, "model_bytes": all_bytes,
                                 "count_and_table_bytes_per_frame": 12 * tiles * L, "frame_bytes_per_frame": 12 * N * N,
                                 "share_of_hbm_model": all_bytes / HBM_BYTES_PER_S / total}
        del counts, lut
        torch.cuda.empty_cache()
        kw = {} if integer else {"levels": L}
        if integer and L == 256:      # the public call decides the depth by dtype: a uint8 tensor (its cast to float32 is part of the call)
            xi = x.to(torch.uint8)
            t, calls = _timed(torch, lambda: E.clahe(xi, CLIP, GRID, return_tensors=True), args.windows)
            case["clahe_uint8_tensor"] = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t}
            del xi
        elif not integer:
            t, calls = _timed(torch, lambda: E.clahe(x, CLIP, GRID, return_tensors=True, **kw), args.windows)
            case["clahe_auto_range"] = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t}
            t, calls = _timed(torch, lambda: E.clahe(x, CLIP, GRID, value_range=(lo, hi), return_tensors=True, **kw), args.windows)
            case["clahe_given_range"] = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t}
        out["cases"][name] = case
        del x, res
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
