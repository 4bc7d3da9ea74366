"""Time of connected-component labelling and region measurements (barc4dip_amd.geometry.labels, barc4dip_amd.metrics.regions;
csrc/b4d_label.hip) on resident (T, 2048, 2048) stacks of three kinds of frame: sparse spots (``synth.spot_field``, 2 000 spots),
a thresholded speckle frame (``synth.speckle_frame`` above its mean) and a random mask at the percolation density 0.593.

Prints one JSON line and writes it to profiles/regions_bench.json (``--out``).  ``b4d_label_regions`` and ``b4d_region_properties``
are timed as entry points on the whole stack in windows of a few calls between two stream events (median over ``--windows``
windows); ``find_spots`` is the public call, with its read-backs and host arithmetic, by the wall clock.

Byte model, per pixel unless said otherwise.  Labelling: the input (4 B, a mask 1 B), the links written by
the tile pass (4), read and written by the flatten pass (8), read by the numbering (4), read and written by the last pass (8).
Properties: the labels once for the boxes (4), then 8 B per BOX pixel per pass over the boxes (two passes: every region here has
flux) and 160 B per region written.  The share is the model's bytes at the achievable streaming rate of the microarchitecture
guide, 6.29 TB/s, over the measured time.  Next to it the time of ``scipy.ndimage.label`` + ``center_of_mass`` for one frame on
this machine's host, single-threaded: context, not a bar.

    python tools/bench_regions.py [--frames 8] [--windows 7] [--out profiles/regions_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2048
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


def _wall(torch, fn, windows):
    fn()
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy import ndimage

    from barc4dip_amd import _ffi, synth
    from barc4dip_amd.geometry import labels as L
    from barc4dip_amd.metrics import regions as R

    torch.cuda.set_device(0)
    T = args.frames
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    speckle = synth.speckle_frame(N, 1234)
    inputs = {
        "sparse_spots": (synth.spot_field((N, N), 2000, seed=1, sigma=2.0, amplitude=1000.0)[0].astype(np.float32), 50.0),
        "speckle": (speckle, float(speckle.mean())),
        "percolation_mask": ((np.random.default_rng(2).random((N, N)) < 0.593).astype(np.float32), 0.5),
    }
    res = {"tool": "bench_regions", "device": torch.cuda.get_device_name(0), "frames": T, "frame": N, "connectivity": 2,
           "windows": args.windows, "hbm_model_bytes_per_s": HBM_BYTES_PER_S, "inputs": {}}
    for name, (frame, thr) in inputs.items():
        x = torch.from_numpy(frame).cuda()[None].expand(T, N, N).contiguous()
        thr_t = torch.full((T,), thr, dtype=torch.float32, device="cuda")
        labels = torch.empty((T, N, N), dtype=torch.int32, device="cuda")
        n_dev = torch.empty((T,), dtype=torch.int32, device="cuda")

        def label():
            _ffi.check(lib.b4d_label_regions(C.c_void_p(x.data_ptr()), C.c_void_p(thr_t.data_ptr()), None, T, N, N, 2,
                                             C.c_void_p(labels.data_ptr()), C.c_void_p(n_dev.data_ptr()), st))

        t_label, calls_label = _timed(torch, label, args.windows)
        n = L.read_counts(n_dev)
        off = L.offsets_of(n)
        out = torch.empty((int(off[-1]), len(L.COLUMNS)), dtype=torch.float64, device="cuda")

        def props():
            _ffi.check(lib.b4d_region_properties(C.c_void_p(x.data_ptr()), C.c_void_p(labels.data_ptr()), T, N, N,
                                                 off.ctypes.data_as(C.c_void_p), 0.0, float("inf"), C.c_void_p(out.data_ptr()), st))

        t_props, calls_props = _timed(torch, props, args.windows)
        tab = out[:int(n[0])].cpu().numpy()
        col = {k: tab[:, i] for i, k in enumerate(L.COLUMNS)}
        box_pixels = float(np.sum((col["y1"] - col["y0"]) * (col["x1"] - col["x0"])))
        t_spots = _wall(torch, lambda: R.find_spots(x, thr, connectivity=2), args.windows)

        t0 = time.perf_counter()
        lab_host, n_host = ndimage.label(frame > np.float32(thr), ndimage.generate_binary_structure(2, 2))
        t_scipy_label = time.perf_counter() - t0
        t0 = time.perf_counter()
        com = np.array(ndimage.center_of_mass(frame.astype(np.float64), lab_host, np.arange(1, n_host + 1)))
        t_scipy_com = time.perf_counter() - t0
        same = bool(n_host == n[0] and np.array_equal(labels[0].cpu().numpy(), lab_host))
        worst = float(np.nanmax(np.abs(com - np.stack([col["wcy"], col["wcx"]], axis=1)))) if same and n_host else float("nan")

        label_bytes = T * N * N * (4 + 24)
        props_bytes = T * (N * N * 4 + 16 * box_pixels + 160 * int(n[0]))
        res["inputs"][name] = {
            "threshold": thr, "regions_per_frame": int(n[0]), "largest_area": int(col["area"].max()) if n[0] else 0,
            "box_pixels_per_frame": box_pixels, "equals_scipy_label": same, "centroid_max_abs_diff_to_scipy_px": worst,
            "label_regions": {"s_per_call": t_label, "calls_per_window": calls_label, "frames_per_s": T / t_label,
                              "model_bytes": label_bytes, "effective_bytes_per_s": label_bytes / t_label,
                              "share_of_hbm_model": label_bytes / HBM_BYTES_PER_S / t_label},
            "region_properties": {"s_per_call": t_props, "calls_per_window": calls_props, "frames_per_s": T / t_props,
                                  "model_bytes": props_bytes, "effective_bytes_per_s": props_bytes / t_props,
                                  "share_of_hbm_model": props_bytes / HBM_BYTES_PER_S / t_props},
            "find_spots": {"s_per_call": t_spots, "frames_per_s": T / t_spots},
            "scipy_host_one_frame": {"label_s": t_scipy_label, "center_of_mass_s": t_scipy_com},
        }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
