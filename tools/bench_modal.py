"""Cost of the modal fits (barc4dip_amd.signal.modal_fit: b4d_modal_fit, b4d_modal_residual) next to two yardsticks that are not
the code under test.

Prints one JSON line and writes it to --out.  For each (ny, nx) x T and each J in (6, 15, 36, 66), with maps and weights (a disc
with 10 % random holes, one map shared by the batch) resident on the device and the results left there: seconds per call of the
fit (Gram kernel + finish kernel) and of the residual kernel, each as the median and best of --reps timed windows that hold
>= --min-s of work; the achieved float64 FLOP/s of the fit, counting J (J + 1) + 2 J flops per valid node, and the bytes per
second over the 8 B per node it must read (map and weight).  Zernike modes; the J = 6 entry is also timed with Legendre modes.

Yardsticks, alternating window by window with the fit in the same process:
  poly2      b4d_poly2_fit_weighted (coefficients only) on the same grid, against the J = 6 Legendre fit
  composed   the basis as a float64 (nodes, J) torch tensor, A^T diag(w_t) A and A^T w_t phi_t per map through torch.matmul
             (w_t = w where phi_t is finite: the effective weights are per map), once with the basis built inside the timed
             region (explicit radial polynomials, cos and sin in torch) and once with it prebuilt.  The normal equations are
             left unsolved.

    python tools/bench_modal.py [--reps 5] [--min-s 0.1] [--out profiles/modal_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from math import factorial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((126, 126), 256), ((512, 512), 16), ((2048, 2048), 1)]
MODES = (6, 15, 36, 66)


def _mask(ny, nx, seed):
    v = (np.arange(ny) - 0.5 * (ny - 1)) / (0.5 * (ny - 1))
    u = (np.arange(nx) - 0.5 * (nx - 1)) / (0.5 * (nx - 1))
    m = ((v[:, None] ** 2 + u[None, :] ** 2) <= 0.9) & (np.random.default_rng(seed).random((ny, nx)) >= 0.1)
    return m.astype(np.float32)


def _maps(ny, nx, T, seed):
    rng = np.random.default_rng(seed)
    v, u = np.linspace(-1, 1, ny)[:, None], np.linspace(-1, 1, nx)[None, :]
    base = 0.3 + 0.5 * u - 0.2 * v + 0.8 * (u * u + v * v) + 0.1 * np.cos(3 * u + 2 * v)
    return (base[None] + 0.01 * rng.normal(size=(T, ny, nx))).astype(np.float32)


def _torch_zernike(torch, table, ny, nx, cy, cx, sy, sx):
    """(nodes, J) float64 on the device from the explicit formula."""
    v = ((torch.arange(ny, dtype=torch.float64, device="cuda") - cy) * sy)[:, None].expand(ny, nx).reshape(-1)
    u = ((torch.arange(nx, dtype=torch.float64, device="cuda") - cx) * sx)[None, :].expand(ny, nx).reshape(-1)
    rho, th = torch.sqrt(u * u + v * v), torch.atan2(v, u)
    cols = []
    for n, m in table:
        n, am = int(n), abs(int(m))
        R = torch.zeros_like(rho)
        for s in range((n - am) // 2 + 1):
            c = (-1) ** s * factorial(n - s) // (factorial(s) * factorial((n + am) // 2 - s) * factorial((n - am) // 2 - s))
            R = R + float(c) * rho ** (n - 2 * s)
        if m == 0:
            cols.append(np.sqrt(n + 1.0) * R)
        else:
            cols.append(np.sqrt(2.0 * (n + 1.0)) * R * (torch.cos(am * th) if m > 0 else torch.sin(am * th)))
    return torch.stack(cols, dim=1)


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
    ap.add_argument("--min-s", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modal_bench.json"))
    ap.add_argument("--no-yardsticks", action="store_true", help="time the modal kernels only (for a kernel trace)")
    args = ap.parse_args()
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from barc4dip_amd.signal import modal_table

    torch.cuda.set_device(0)
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    out = {"tool": "bench_modal", "device": torch.cuda.get_device_name(0), "reps": args.reps, "min_s": args.min_s,
           "flops_per_valid_node": "J (J + 1) + 2 J", "bytes_per_node": 8, "cases": []}
    for (ny, nx), T in CASES:
        phi = torch.from_numpy(_maps(ny, nx, T, 7)).cuda()
        w = torch.from_numpy(_mask(ny, nx, 11)).cuda()
        cy, cx = 0.5 * (ny - 1), 0.5 * (nx - 1)
        rad = min(cy, cx)
        valid = int((w > 0).sum().item()) * T        # the disc of the mask lies inside the unit disc of the fit
        resid, rms = torch.empty_like(phi), torch.empty(T, dtype=torch.float64, device="cuda")
        for J in MODES:
            ws = torch.empty(int(lib.b4d_modal_workspace_bytes(T, ny, nx, J)), dtype=torch.uint8, device="cuda")
            coeff = torch.empty((T, J), dtype=torch.float64, device="cuda")
            kept = torch.empty((T, J), dtype=torch.uint8, device="cuda")

            def fit(code=0, sy=1.0 / rad, sx=1.0 / rad):
                _ffi.check(lib.b4d_modal_fit(D.ptr(phi), D.ptr(w), 0, T, ny, nx, code, J, cy, cx, sy, sx, D.ptr(ws), D.ptr(coeff),
                                             D.ptr(kept), st))

            def residual():
                _ffi.check(lib.b4d_modal_residual(D.ptr(phi), D.ptr(w), 0, T, ny, nx, 0, J, cy, cx, 1.0 / rad, 1.0 / rad, D.ptr(coeff),
                                                  None, 1.0, 1, D.ptr(ws), D.ptr(resid), D.ptr(rms), None, st))

            routes = [("fit", fit), ("residual", residual)]
            if J == 6:
                c6 = torch.empty((T, 6), dtype=torch.float64, device="cuda")
                routes.append(("fit_legendre", lambda: fit(1, 1.0 / max(cy, 1.0), 1.0 / max(cx, 1.0))))
                if not args.no_yardsticks:
                    routes.append(("poly2", lambda: _ffi.check(lib.b4d_poly2_fit_weighted(D.ptr(phi), D.ptr(w), 0, T, ny, nx, 63, 1.0, 1,
                                                                                          D.ptr(c6), None, None, st))))
            if not args.no_yardsticks:
                table = modal_table("zernike", J)
                A = _torch_zernike(torch, table, ny, nx, cy, cx, 1.0 / rad, 1.0 / rad)
                w64 = w.reshape(-1).to(torch.float64)

                def gram(basis):
                    p = phi.reshape(T, -1).to(torch.float64)
                    wt = torch.where(torch.isfinite(p), w64[None, :], torch.zeros((), dtype=torch.float64, device="cuda"))
                    Aw = basis[None] * wt[:, :, None]
                    return torch.matmul(Aw.transpose(1, 2), basis[None]), torch.matmul(Aw.transpose(1, 2), p[:, :, None])

                routes.append(("composed_prebuilt", lambda: gram(A)))
                routes.append(("composed", lambda: gram(_torch_zernike(torch, table, ny, nx, cy, cx, 1.0 / rad, 1.0 / rad))))
            iters = {}
            for key, fn in routes:
                _window(fn, 2)
                iters[key] = max(2, int(np.ceil(args.min_s / _window(fn, 2))))
            times = {key: [] for key, _ in routes}
            for _ in range(args.reps):
                for key, fn in routes:
                    times[key].append(_window(fn, iters[key]))
            case = {"ny": ny, "nx": nx, "maps": T, "n_modes": J, "valid_nodes": valid, "kept_all": bool(kept.all().item())}
            for key, _ in routes:
                case[key] = {"s_median": statistics.median(times[key]), "s_best": min(times[key]), "calls_per_window": iters[key]}
            for key in ("fit", "fit_legendre"):
                if key in case:
                    case[key]["flops_per_s"] = valid * (J * (J + 1) + 2 * J) / case[key]["s_median"]
                    case[key]["bytes_per_s"] = 8.0 * T * ny * nx / case[key]["s_median"]
            for key in ("composed", "composed_prebuilt"):
                if key in case:
                    case[key + "_over_fit"] = case[key]["s_median"] / case["fit"]["s_median"]
            if "poly2" in case:
                case["poly2_over_fit_legendre"] = case["poly2"]["s_median"] / case["fit_legendre"]["s_median"]
            out["cases"].append(case)
            if not args.no_yardsticks:
                del A
        del phi, w, resid
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
