"""Cost of the focal-spot prediction (barc4dip_amd.signal.focal_spot: b4d_focal_spot) next to the route a user composes without it.

Prints one JSON line and writes it to --out.  For each case (T maps of (ny, nx), Z planes, canvas P x P), with the figure errors,
coefficients and plane positions resident on the device and every result left there:

  direct     one b4d_focal_spot call: statistics and both marginals of all T * Z planes, no intensity crop.
  composed   torch builds the complex canvases (float64 phase, sincos, zero padding) for as many maps at a time as fit 512 MB, the
             library's own complex transform (b4d_fft2d_c2c, shifted output) takes them, torch squares (abs()**2 / (sum A)^2) and
             reduces: total, peak and its index, both marginals in float64, the five moments.

The two routes alternate window by window in one process; a window holds >= --min-s of work and is timed with device events.
Reported: seconds per call as the median and best of --reps windows, planes per second of both routes, and their ratio.
The results of the two routes are compared once (Strehl and total) before anything is timed.

    python tools/bench_focus.py [--reps 5] [--min-s 0.2] [--out profiles/focus_bench.json]
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

LAM, H, Z0 = 1.24e-10, 1.04e-4, -0.75
COEFF = np.array([0.0, 1e-7, -2e-7, 1.0 / (2.0 * 0.75002), 2e-6, 1.0 / (2.0 * 0.74998)])
# (T, (ny, nx), Z, canvas, half span of the planes in metres)
CASES = [(16, (128, 128), 33, 1024, 1.5e-5), (64, (48, 40), 9, 256, 5e-5)]
GROUP_BYTES = 512 << 20


def _maps(shape, T, seed):
    rng = np.random.default_rng(seed)
    ny, nx = shape
    y, x = np.linspace(-1, 1, ny)[:, None], np.linspace(-1, 1, nx)[None, :]
    out = np.empty((T, ny, nx), np.float32)
    for t in range(T):
        e = sum(rng.normal() * np.cos(np.pi * (rng.uniform(0.5, 3) * y + rng.uniform(0.5, 3) * x) + rng.uniform(0, 6.28)) for _ in range(6))
        out[t] = e * (0.05 * LAM / np.sqrt(np.mean(e * e)))
    return out


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focus_bench.json"))
    ap.add_argument("--direct-only", action="store_true", help="time b4d_focal_spot alone (for a kernel trace)")
    args = ap.parse_args()
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd.signal import fft as gfft

    torch.cuda.set_device(0)
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    out = {"tool": "bench_focus", "device": torch.cuda.get_device_name(0), "reps": args.reps, "min_s": args.min_s, "cases": []}
    for T, (ny, nx), Z, P, half in CASES:
        err = torch.from_numpy(_maps((ny, nx), T, 5)).cuda()
        z = Z0 + np.linspace(-half, half, Z)
        zb = (C.c_double * Z)(*z.tolist())
        coeff = torch.from_numpy(np.repeat(COEFF[None], T, axis=0)).cuda()
        pl = _ffi.get_plan(P, P, general=True)
        ws = torch.empty(int(lib.b4d_focal_spot_workspace_bytes(pl.handle, T, Z)), dtype=torch.uint8, device="cuda")
        stats = torch.empty((T, Z, 10), dtype=torch.float64, device="cuda")
        mx = torch.empty((T, Z, P), dtype=torch.float64, device="cuda")
        my = torch.empty((T, Z, P), dtype=torch.float64, device="cuda")

        def direct():
            _ffi.check(lib.b4d_focal_spot(pl.handle, D.ptr(err), None, 0, T, ny, nx, D.ptr(coeff), H, H, LAM, C.cast(zb, C.c_void_p), Z, 0, 0,
                                          None, D.ptr(stats), D.ptr(mx), D.ptr(my), D.ptr(ws), st))

        # ---- the composed route
        v = ((torch.arange(ny, dtype=torch.float64, device="cuda") - 0.5 * (ny - 1)) * H)[:, None]
        u = ((torch.arange(nx, dtype=torch.float64, device="cuda") - 0.5 * (nx - 1)) * H)[None, :]
        zt = torch.from_numpy(z).cuda()
        p = (torch.arange(P, dtype=torch.float64, device="cuda") - P // 2)
        per_map = max(1, min(T, GROUP_BYTES // (Z * P * P * 8)))
        comp = {}

        def composed():
            res = []
            for t0 in range(0, T, per_map):
                e = err[t0:t0 + per_map].to(torch.float64)                                   # (g, ny, nx)
                g = int(e.shape[0])
                c = coeff[t0:t0 + g]
                poly = (c[:, 0, None, None] + c[:, 1, None, None] * u + c[:, 2, None, None] * v + c[:, 3, None, None] * u * u
                        + c[:, 4, None, None] * u * v + c[:, 5, None, None] * v * v)
                turns = ((e + poly) / LAM)[:, None] + ((u * u + v * v) / (2.0 * LAM))[None, None] / zt[None, :, None, None]
                turns = turns - torch.round(turns)
                ok = torch.isfinite(e)[:, None].expand(g, Z, ny, nx)
                U = torch.where(ok, torch.polar(torch.ones_like(turns), 2.0 * np.pi * turns), torch.zeros((), dtype=torch.complex128, device="cuda"))
                canvas = torch.zeros((g * Z, P, P), dtype=torch.complex64, device="cuda")
                canvas[:, :ny, :nx] = U.reshape(g * Z, ny, nx).to(torch.complex64)
                F = gfft._c2c(canvas, False)
                sa = torch.isfinite(e).sum(dim=(1, 2)).to(torch.float64)                     # (g,)
                I = (F.abs() ** 2).reshape(g, Z, P, P) / (sa * sa).to(torch.float32)[:, None, None, None]
                m_x, m_y = I.sum(dim=-2, dtype=torch.float64), I.sum(dim=-1, dtype=torch.float64)
                peak, idx = I.reshape(g, Z, -1).max(dim=-1)
                rq = (I * p.to(torch.float32)).sum(dim=-1, dtype=torch.float64)               # q-weighted row sums
                res.append((m_x.sum(-1), peak, idx, (m_y * p).sum(-1), (m_x * p).sum(-1), (m_y * p * p).sum(-1), (m_x * p * p).sum(-1),
                            (rq * p).sum(-1), m_x, m_y))
            comp["total"] = torch.cat([r[0] for r in res])
            comp["peak"] = torch.cat([r[1] for r in res])

        direct()
        case = {"maps": T, "ny": ny, "nx": nx, "planes": Z, "canvas": P, "plan_chunk": pl.chunk, "composed_maps_per_group": per_map}
        routes = [("direct", direct)]
        if not args.direct_only:
            composed()
            torch.cuda.synchronize()
            s = stats.cpu().numpy()
            case["strehl_max_rel_diff"] = float(np.max(np.abs(comp["peak"].cpu().numpy() - s[..., 1]) / s[..., 1]))
            case["total_max_rel_diff"] = float(np.max(np.abs(comp["total"].cpu().numpy() - s[..., 0]) / s[..., 0]))
            routes.append(("composed", composed))
        iters = {}
        for key, fn in routes:
            _window(fn, 2)
            iters[key] = max(2, int(np.ceil(args.min_s / _window(fn, 2))))
        times = {key: [] for key, _ in routes}
        for _ in range(args.reps):
            for key, fn in routes:
                times[key].append(_window(fn, iters[key]))
        for key, _ in routes:
            med = statistics.median(times[key])
            case[key] = {"s_median": med, "s_best": min(times[key]), "calls_per_window": iters[key], "planes_per_s": T * Z / med}
        if "composed" in case:
            case["direct_over_composed_planes_per_s"] = case["direct"]["planes_per_s"] / case["composed"]["planes_per_s"]
        # bytes the direct route must move per plane: canvas written, transform passes excluded, spectrum read once
        case["direct_bytes_per_plane_outside_transform"] = 2 * 8 * P * P
        out["cases"].append(case)
        del err, ws, stats, mx, my
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
