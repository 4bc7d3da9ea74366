"""Time of the multi-tau correlation (barc4dip_amd.metrics.multi_tau_correlation, b4d_multi_tau_*).

Prints one JSON line and writes it to profiles/multi_tau_bench.json (``--out``).  Best of ``--reps`` runs, stream events around
the public call (m = 16, chunk_frames = 256, no labels, results left on the device):

  resident   float32 stacks of 4096 x 512^2 and 1024 x 2048^2 on the device: the call (finiteness scan, init, pushes, finish) and
             the pushes alone (integer-style call without the scan, through the C ABI);
  streamed   a uint16 stack of 4096 x 512^2 in host memory behind a sliceable source, streamed through ingest.iter_device_chunks,
             next to ingest.temporal_stats_streamed on the same source and chunk size: the rate the ingest path is known to sustain;
  copy rate  a device-to-device copy of 4 GiB in the same run (bytes read + bytes written per second);
  model      the float64 NumPy model on a size it can finish, scaled to each case by its sample count T x pixels.

Per case: the call time, the bytes the kernels move by this file's own count (``kernel_bytes``: per push and level the new frames
read, the averaged frames written, the ring's m - 1 frames read and up to m - 1 written, the pixel list; plus the scan's one read of
the stack), the achieved rate against the copy rate, and ``ratio_to_one_read`` = call time / (stack bytes once / copy rate).

    python tools/bench_multi_tau.py [--reps 3] [--out profiles/multi_tau_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(4096, 512), (1024, 2048)]
M, CHUNK = 16, 256


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


def kernel_bytes(T, npix, m, n_levels, chunk, scan):
    """Bytes the kernels read and write, counted from the push sequence (one region, no padding)."""
    total = 4.0 * T * npix if scan else 0.0
    for t0 in range(0, T, chunk):
        n = min(chunk, T - t0)
        for l in range(n_levels):
            c = t0 >> l
            nl = ((t0 + n) >> l) - c
            if nl < 1:
                break
            out = 0 if l == n_levels - 1 else ((t0 + n) >> (l + 1)) - (t0 >> (l + 1))
            ring = min(c, m - 1) + min(nl, m - 1)
            total += 4.0 * npix * (nl + out + ring + (1 if l == 0 else 0))
    return total


def _pushes_only(x, reps):
    """init, pushes and finish through the C ABI, without the finiteness scan (what an integer source runs)."""
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd.metrics.multitau import lag_table

    T, npix = int(x.shape[0]), int(x.shape[1] * x.shape[2])
    lags, _, _, L = lag_table(T, M)
    lib = _ffi.lib()
    ws = torch.empty(int(lib.b4d_multi_tau_workspace_bytes(npix, 1, M, L, CHUNK)), dtype=torch.uint8, device=x.device)
    g2 = torch.empty((2, len(lags)), dtype=torch.float64, device=x.device)
    mean = torch.empty(1, dtype=torch.float64, device=x.device)
    npx = torch.empty(1, dtype=torch.int64, device=x.device)

    def run():
        st = _ffi.stream_ptr()
        _ffi.check(lib.b4d_multi_tau_init(None, None, npix, 1, M, L, CHUNK, D.ptr(ws), st))
        for t0 in range(0, T, CHUNK):
            part = x[t0:t0 + CHUNK]
            _ffi.check(lib.b4d_multi_tau_push(D.ptr(part), t0, int(part.shape[0]), npix, 1, M, L, CHUNK, D.ptr(ws), st))
        _ffi.check(lib.b4d_multi_tau_finish(T, npix, 1, M, L, CHUNK, D.ptr(ws), D.ptr(g2[0]), D.ptr(g2[1]), D.ptr(mean), D.ptr(npx), st))

    return _time(run, reps), ws.numel(), L


class HostSource:
    """A sliceable view of a host array that is not an ndarray: multi_tau_correlation streams it."""

    def __init__(self, a):
        self.a, self.shape, self.dtype = a, a.shape, a.dtype

    def __getitem__(self, key):
        return self.a[key]


def _numpy_model(T, n):
    """Level cascade and lag sums in float64 NumPy, one region; seconds per sample (T x pixels)."""
    import numpy as np

    I = np.random.default_rng(0).exponential(100.0, (T, n * n))
    t0 = time.perf_counter()
    l, out = 0, []
    while l == 0 or I.shape[0] >= M // 2 + 1:
        for j in range(0 if l == 0 else M // 2, M):
            k = I.shape[0] - j
            if k < 1:
                break
            a, b = I[:k], I[j:j + k]
            pr = a * b
            out.append((pr.mean() / (a.mean() * b.mean()), (pr * pr).mean()))
        half = I.shape[0] // 2
        I = 0.5 * (I[0:2 * half:2] + I[1:2 * half:2])
        l += 1
    t = time.perf_counter() - t0
    return {"T": T, "frame": n, "s": t, "s_per_sample": t / (T * n * n), "lags": len(out), "threads": os.environ.get("OMP_NUM_THREADS")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_tau_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from barc4dip_amd.ingest import temporal_stats_streamed
    from barc4dip_amd.metrics import multi_tau_correlation

    torch.cuda.set_device(0)
    rate = _copy_rate(torch, args.reps)
    base = _numpy_model(512, 128)
    out = {"tool": "bench_multi_tau", "device": torch.cuda.get_device_name(0), "reps": args.reps, "lags_per_level": M,
           "chunk_frames": CHUNK, "copy_bytes_per_s": rate, "numpy_float64": base, "resident": []}

    def figures(T, npix, L, call, scan):
        kb, stack = kernel_bytes(T, npix, M, L, CHUNK, scan), 4.0 * T * npix
        return {"call_s": call, "kernel_bytes": kb, "kernel_bytes_per_stack": kb / stack, "achieved_bytes_per_s": kb / call,
                "share_of_copy_rate": kb / call / rate, "ratio_to_one_read": call / (stack / rate)}

    for T, n in CASES:
        npix = n * n
        x = torch.empty((T, n, n), dtype=torch.float32, device="cuda").exponential_(0.01)      # fully developed speckle, mean 100
        call = _time(lambda: multi_tau_correlation(x, lags_per_level=M, chunk_frames=CHUNK, return_tensors=True), args.reps)
        push, ws_bytes, L = _pushes_only(x, args.reps)
        out["resident"].append({"T": T, "frame": n, "n_levels": L, "workspace_bytes": ws_bytes, "stack_bytes": 4.0 * T * npix,
                                **figures(T, npix, L, call, True),
                                "without_scan": figures(T, npix, L, push, False),
                                "numpy_float64_scaled_s": base["s_per_sample"] * T * npix})
        del x
        torch.cuda.empty_cache()

    T, n = CASES[0]
    words = np.random.default_rng(1).integers(0, 4096, (T, n, n), dtype=np.uint16)
    src = HostSource(words)
    wall = float("inf")
    for _ in range(args.reps):                      # host staging is part of this path: wall clock next to the events
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        multi_tau_correlation(src, lags_per_level=M, chunk_frames=CHUNK, return_tensors=True)
        torch.cuda.synchronize()
        wall = min(wall, time.perf_counter() - t0)
    call = _time(lambda: multi_tau_correlation(src, lags_per_level=M, chunk_frames=CHUNK, return_tensors=True), args.reps)
    ing = float("inf")
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        temporal_stats_streamed(src, chunk_frames=CHUNK, return_tensors=True)
        torch.cuda.synchronize()
        ing = min(ing, time.perf_counter() - t0)
    L = int(out["resident"][0]["n_levels"])
    out["streamed"] = {"T": T, "frame": n, "dtype": "uint16", "host_bytes": 2.0 * T * n * n, "wall_s": wall,
                       "frames_per_s": T / wall, **figures(T, n * n, L, call, False),
                       "temporal_stats_streamed_s": ing, "temporal_stats_streamed_frames_per_s": T / ing,
                       "share_of_ingest_rate": ing / wall}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
