"""Throughput of the least-squares gradient integration (barc4dip_amd.signal.integrate_gradient, b4d_integrate_gradient).

Prints one JSON line and writes it to --out.  For each (ny, nx) x T, with the slope maps resident on the device and the result
left there: seconds per call (median and best of --reps timed windows, each window long enough to hold >= --min-s of work),
maps/s and achieved TFLOP/s of the four matrix products (4 T ny nx (ny + nx) flop; the right-hand side, the division and the
launches are inside the time but not in the count).  Next to it the same four products through torch.matmul on the device, on
the same right-hand side (computed beforehand, not timed) and the same float32 basis: a comparison bar for this tool only, the
product never takes that route.  The two routes alternate window by window in one process.

    python tools/bench_wavefront.py [--reps 7] [--min-s 0.2] [--out profiles/wavefront_bench.json]
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

CASES = [((126, 126), 256), ((510, 510), 64), ((2048, 2048), 1)]


def _basis(n):
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    c = np.sqrt(2.0 / n) * np.cos(np.pi * (2 * j + 1) * k / (2.0 * n))
    c[0] /= np.sqrt(2.0)
    return c


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavefront_bench.json"))
    args = ap.parse_args()
    import torch

    from barc4dip_amd.signal import integrate_gradient

    torch.cuda.set_device(0)
    torch.backends.cuda.matmul.allow_tf32 = False
    out = {"tool": "bench_wavefront", "device": torch.cuda.get_device_name(0), "reps": args.reps, "min_s": args.min_s, "cases": []}
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    for (ny, nx), T in CASES:
        gy = torch.randn((T, ny, nx), generator=g, device="cuda")
        gx = torch.randn((T, ny, nx), generator=g, device="cuda")
        hy, hx = 0.7, 1.9
        cy, cx = (torch.from_numpy(_basis(n).astype(np.float32)).cuda() for n in (ny, nx))
        cyt, cxt = cy.T.contiguous(), cx.T.contiguous()
        lam = (4.0 * np.sin(np.pi * np.arange(ny) / (2.0 * ny)) ** 2 / hy ** 2)[:, None] \
            + (4.0 * np.sin(np.pi * np.arange(nx) / (2.0 * nx)) ** 2 / hx ** 2)[None, :]
        lam[0, 0] = np.inf
        lam = torch.from_numpy(lam.astype(np.float32)).cuda()
        # right-hand side for the matmul route, from the same edge means (torch, not timed)
        ey, ex = 0.5 * (gy[:, :-1] + gy[:, 1:]) / hy, 0.5 * (gx[:, :, :-1] + gx[:, :, 1:]) / hx
        r = torch.zeros_like(gy)
        r[:, 1:] += ey
        r[:, :-1] -= ey
        r[:, :, 1:] += ex
        r[:, :, :-1] -= ex

        def ours():
            return integrate_gradient(gy, gx, dy=hy, dx=hx, return_tensors=True)

        def matmul():
            return torch.matmul(cyt, torch.matmul(torch.matmul(cy, torch.matmul(r, cxt)) / lam, cx))

        a, b = ours(), matmul()
        torch.cuda.synchronize()
        agree = float((a - b).abs().max() / (b.max() - b.min()))
        iters = {}
        for name, fn in (("ours", ours), ("matmul", matmul)):
            _window(fn, 3)                                                  # warm-up of this shape
            iters[name] = max(3, int(np.ceil(args.min_s / _window(fn, 3))))
        times = {"ours": [], "matmul": []}
        for _ in range(args.reps):
            for name, fn in (("ours", ours), ("matmul", matmul)):
                times[name].append(_window(fn, iters[name]))
        flop = 4.0 * T * ny * nx * (ny + nx)
        case = {"ny": ny, "nx": nx, "maps": T, "flop_per_call": flop, "max_abs_diff_of_routes_over_range": agree}
        for name in ("ours", "matmul"):
            med, best = statistics.median(times[name]), min(times[name])
            case[name] = {"s_median": med, "s_best": best, "iters_per_window": iters[name], "maps_per_s": T / med,
                          "tflops": flop / med * 1e-12}
        case["ours_over_matmul_time"] = case["ours"]["s_median"] / case["matmul"]["s_median"]
        out["cases"].append(case)
        del gy, gx, r, ey, ex, a, b
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
