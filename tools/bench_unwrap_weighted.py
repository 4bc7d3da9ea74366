"""Cost of the weighted / masked phase unwrap (barc4dip_amd.signal.phase_unwrap with weights, b4d_phase_unwrap_weighted) next to the
unweighted unwrap on the same grid, and of fringe_displacement with and without a mask.

Prints one JSON line and writes it to --out.  For each (ny, nx) x T and each mask (a disc, the disc with 10 % random holes), with
the wrapped maps and the weights resident on the device and the result left there: seconds per weighted call (median and best of
--reps timed windows, each long enough to hold >= --min-s of work), the iterations the maps took, seconds per iteration and its
ratio to one unweighted phase_unwrap call (right-hand side, four matrix products, congruence step).  The time per iteration is
(call time - time of the same call with max_iter = 1) / (iterations - 1): the set-up, the first preconditioner solve, the seed
search, the congruence step and the allocations drop out.  The three routes alternate window by window in one process.  The timed
call includes the host's reads of the per-map flags (every 4 iterations).  The last entry times the whole of fringe_displacement on
--frames frames of --size^2, window 32, with min_level / min_visibility and without.

    python tools/bench_unwrap_weighted.py [--reps 7] [--min-s 0.2] [--frames 64] [--size 2048] [--out profiles/unwrap_weighted_bench.json]
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

CASES = [((127, 127), 128, 60.0), ((512, 512), 16, 200.0)]      # (127, 127) x 128: the two phase maps of 64 frames of 2048^2, window 32
MASKS = ("disc", "disc_holes")
CARRIERS = np.array([[0.004, 0.127], [0.123, -0.006]])


def _mask(name, ny, nx, seed):
    v = (np.arange(ny) - 0.5 * (ny - 1)) / (0.5 * (ny - 1))
    u = (np.arange(nx) - 0.5 * (nx - 1)) / (0.5 * (nx - 1))
    m = (v[:, None] ** 2 + u[None, :] ** 2) <= 0.9
    if name == "disc_holes":
        m = m & (np.random.default_rng(seed).random((ny, nx)) >= 0.1)
    return m.astype(np.float32)


def _phase(ny, nx, T, amp, seed):
    """Wrapped amp (v^2 + 0.8 u^2 + 0.3 u v) + 0.05 N(0, 1), u, v in [-1, 1]: (T, ny, nx) float32, fresh noise per map."""
    rng = np.random.default_rng(seed)
    v = ((np.arange(ny) - 0.5 * (ny - 1)) / (0.5 * (ny - 1)))[:, None]
    u = ((np.arange(nx) - 0.5 * (nx - 1)) / (0.5 * (nx - 1)))[None, :]
    p = amp * (v * v + 0.8 * u * u + 0.3 * u * v) + 0.05 * rng.standard_normal((T, ny, nx))
    return (p - 2.0 * np.pi * np.round(p / (2.0 * np.pi))).astype(np.float32)


def _window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def _alternate(routes, reps, min_s):
    iters = {}
    for key, fn in routes:
        _window(fn, 2)                                              # warm-up of this shape
        iters[key] = max(2, int(np.ceil(min_s / _window(fn, 2))))
    times = {key: [] for key, _ in routes}
    for _ in range(reps):
        for key, fn in routes:
            times[key].append(_window(fn, iters[key]))
    return {key: {"s_median": statistics.median(times[key]), "s_best": min(times[key]), "calls_per_window": iters[key]}
            for key, _ in routes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unwrap_weighted_bench.json"))
    args = ap.parse_args()
    import torch

    from barc4dip_amd import synth
    from barc4dip_amd.signal import fringe_displacement, phase_unwrap

    torch.cuda.set_device(0)
    warnings.simplefilter("ignore", RuntimeWarning)          # the max_iter = 1 calls stop unconverged on purpose
    out = {"tool": "bench_unwrap_weighted", "device": torch.cuda.get_device_name(0), "reps": args.reps, "min_s": args.min_s,
           "rtol": 1e-6, "cases": []}
    for (ny, nx), T, amp in CASES:
        ph = torch.from_numpy(_phase(ny, nx, T, amp, 7)).cuda()
        for name in MASKS:
            w = torch.from_numpy(_mask(name, ny, nx, 11)).cuda()
            routes = (("weighted", lambda: phase_unwrap(ph, weights=w, return_tensors=True)),
                      ("one_iteration", lambda: phase_unwrap(ph, weights=w, max_iter=1, return_tensors=True)),
                      ("unweighted", lambda: phase_unwrap(ph, return_tensors=True)))
            _, info = phase_unwrap(ph, weights=w, return_info=True, return_tensors=True)
            case = {"ny": ny, "nx": nx, "maps": T, "mask": name, "amp": amp, "valid_fraction": float(w.mean()),
                    "iterations_max": int(info["iterations"].max()), "iterations_min": int(info["iterations"].min()),
                    "residual_max": float(info["residual"].max()), "converged": bool(info["converged"].all())}
            case.update(_alternate(routes, args.reps, args.min_s))
            k = case["iterations_max"]
            per = (case["weighted"]["s_median"] - case["one_iteration"]["s_median"]) / (k - 1) if k > 1 else None
            case["s_per_iteration"] = per
            case["iteration_over_unweighted_call"] = None if per is None else per / case["unweighted"]["s_median"]
            case["weighted_over_unweighted_call"] = case["weighted"]["s_median"] / case["unweighted"]["s_median"]
            out["cases"].append(case)
            del w
        del ph
    # the whole of fringe_displacement: a round beam (logistic edge) on a magnified grating, with and without the mask
    N, F = args.size, args.frames
    y, x = np.arange(N, dtype=np.float64)[:, None], np.arange(N, dtype=np.float64)[None, :]
    c = (N - 1) / 2.0
    aperture = 1.0 / (1.0 + np.exp((np.hypot(y - c, x - c) - 0.45 * N) / 1.5))
    ref = synth.fringe_frame((N, N), CARRIERS, visibility=0.4, envelope=lambda yy, xx: aperture, mean=2000.0, seed=11).astype(np.float32)
    img = synth.fringe_frame((N, N), CARRIERS, lambda yy, xx: (0.01 * (yy - c) + 0.0 * xx, 0.01 * (xx - c) + 0.0 * yy), visibility=0.3,
                             envelope=lambda yy, xx: aperture, mean=2000.0, seed=12).astype(np.float32)
    tref = torch.from_numpy(ref + 32.0).cuda()
    timg = torch.from_numpy(img + 32.0).cuda()[None].expand(F, N, N).contiguous()
    kw = dict(carriers=CARRIERS, window=32, return_tensors=True)
    m = fringe_displacement(tref, timg, min_level=0.5, min_visibility=0.15, **kw)
    routes = (("masked", lambda: fringe_displacement(tref, timg, min_level=0.5, min_visibility=0.15, **kw)),
              ("unmasked", lambda: fringe_displacement(tref, timg, **kw)))
    case = {"frames": F, "ny": N, "nx": N, "window": 32, "grid": list(m["dy"].shape[-2:]), "valid_fraction": float(m["valid"].float().mean()),
            "iterations_max": int(m["meta"]["unwrap"]["iterations"].max()), "converged": bool(m["meta"]["unwrap"]["converged"].all())}
    case.update(_alternate(routes, args.reps, args.min_s))
    case["masked_over_unmasked"] = case["masked"]["s_median"] / case["unmasked"]["s_median"]
    out["fringe_displacement"] = case
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
