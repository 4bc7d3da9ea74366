"""Cost of the weighted / masked gradient integration (barc4dip_amd.signal.integrate_gradient with weights,
b4d_integrate_gradient_weighted) next to the unweighted route on the same grid.

Prints one JSON line and writes it to --out.  For each (ny, nx) x T and each mask (a disc, the disc with 10 % random holes), with
slopes and weights resident on the device and the result left there: seconds per weighted call (median and best of --reps timed
windows, each long enough to hold >= --min-s of work), the iterations the maps took, seconds per iteration, and the ratio of one
iteration to one unweighted integrate_gradient call on the same grid.  An unweighted call is the right-hand side and the four
matrix products; an iteration is the same four products plus the vector kernels and reductions of conjugate gradients, so the
excess of the ratio over 1 is what those cost.  The time per iteration is (call time - time of the same call with max_iter = 1)
/ (iterations - 1): the set-up, the first preconditioner solve and the allocations drop out.  The two routes alternate window by
window in one process.  The timed call includes the host's reads of the per-map flags (every 4 iterations).

    python tools/bench_wavefront_weighted.py [--reps 7] [--min-s 0.2] [--out profiles/wavefront_weighted_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((126, 126), 256), ((512, 512), 16), ((2048, 2048), 1)]
MASKS = ("disc", "disc_holes")


def _mask(name, ny, nx, seed):
    v = (np.arange(ny) - 0.5 * (ny - 1)) / (0.5 * (ny - 1))
    u = (np.arange(nx) - 0.5 * (nx - 1)) / (0.5 * (nx - 1))
    m = (v[:, None] ** 2 + u[None, :] ** 2) <= 0.9
    if name == "disc_holes":
        m = m & (np.random.default_rng(seed).random((ny, nx)) >= 0.1)
    return m.astype(np.float32)


def _slopes(ny, nx, T, seed):
    """Gradient of a few smooth waves plus 2 % white noise, (T, ny, nx) float32 twice."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(ny) * 0.7, np.arange(nx) * 1.9, indexing="ij")
    ly, lx = (ny - 1) * 0.7, (nx - 1) * 1.9
    gy, gx = np.zeros((ny, nx)), np.zeros((ny, nx))
    for _ in range(4):
        ky, kx, ph, am = rng.uniform(0.5, 3.0) * np.pi / ly, rng.uniform(0.5, 3.0) * np.pi / lx, rng.uniform(0, 6.28), rng.uniform(0.2, 1)
        gy += am * ky * np.cos(ky * y + kx * x + ph)
        gx += am * kx * np.cos(ky * y + kx * x + ph)
    s = np.sqrt(0.5 * (np.mean(gy ** 2) + np.mean(gx ** 2)))
    noise = rng.normal(size=(2, T, ny, nx)).astype(np.float32) * np.float32(0.02 * s)
    return gy.astype(np.float32)[None] + noise[0], gx.astype(np.float32)[None] + noise[1]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavefront_weighted_bench.json"))
    args = ap.parse_args()
    import torch

    from barc4dip_amd.signal import integrate_gradient

    torch.cuda.set_device(0)
    warnings.simplefilter("ignore", RuntimeWarning)          # the max_iter = 1 calls stop unconverged on purpose
    out = {"tool": "bench_wavefront_weighted", "device": torch.cuda.get_device_name(0), "reps": args.reps, "min_s": args.min_s,
           "rtol": 1e-6, "cases": []}
    hy, hx = 0.7, 1.9
    for (ny, nx), T in CASES:
        hgy, hgx = _slopes(ny, nx, T, 7)
        gy, gx = torch.from_numpy(hgy).cuda(), torch.from_numpy(hgx).cuda()
        del hgy, hgx
        for name in MASKS:
            w = torch.from_numpy(_mask(name, ny, nx, 11)).cuda()

            def weighted():
                return integrate_gradient(gy, gx, dy=hy, dx=hx, weights=w, fill="harmonic", return_tensors=True)

            def one_iteration():
                return integrate_gradient(gy, gx, dy=hy, dx=hx, weights=w, fill="harmonic", max_iter=1, return_tensors=True)

            def unweighted():
                return integrate_gradient(gy, gx, dy=hy, dx=hx, return_tensors=True)

            _, info = integrate_gradient(gy, gx, dy=hy, dx=hx, weights=w, fill="harmonic", return_info=True, return_tensors=True)
            routes = (("weighted", weighted), ("one_iteration", one_iteration), ("unweighted", unweighted))
            iters = {}
            for key, fn in routes:
                _window(fn, 3)                                              # warm-up of this shape
                iters[key] = max(3, int(np.ceil(args.min_s / _window(fn, 3))))
            times = {key: [] for key, _ in routes}
            for _ in range(args.reps):
                for key, fn in routes:
                    times[key].append(_window(fn, iters[key]))
            case = {"ny": ny, "nx": nx, "maps": T, "mask": name, "valid_fraction": float(w.mean()),
                    "iterations_max": int(info["iterations"].max()), "iterations_min": int(info["iterations"].min()),
                    "residual_max": float(info["residual"].max()), "converged": bool(info["converged"].all())}
            for key, _ in routes:
                case[key] = {"s_median": statistics.median(times[key]), "s_best": min(times[key]), "calls_per_window": iters[key]}
            k = case["iterations_max"]
            per = (case["weighted"]["s_median"] - case["one_iteration"]["s_median"]) / (k - 1) if k > 1 else None
            case["s_per_iteration"] = per
            case["iteration_over_unweighted_call"] = None if per is None else per / case["unweighted"]["s_median"]
            case["weighted_over_unweighted_call"] = case["weighted"]["s_median"] / case["unweighted"]["s_median"]
            out["cases"].append(case)
            del w
        del gy, gx
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
