"""Time of SSIM, MS-SSIM and the frame errors (barc4dip_amd.metrics.perceptual; csrc/b4d_perceptual.hip) on resident
(64, 2048, 2048) float32 stacks: a reference stack (paired) or one reference frame (shared) against an image stack.

Prints one JSON line and writes it to profiles/perceptual_bench.json (``--out``).  Every case is warmed up and then timed in
windows of a few calls between two stream events; the figures are the medians over ``--windows`` windows: seconds per call,
frames per second, effective bytes per second under the case's traffic model and the share of that model at the achievable
streaming rate of the microarchitecture guide, 6.29 TB/s:

  means only, paired            8 B / px (both frames read once; the partial sums are a few bytes per tile)
  means only, shared reference  4 B / px, plus the reference once
  each map written              + 4 B / px
  frame errors                  8 B / px (4 with a shared reference)
  ms_ssim                       per scale the 8 B / px of its own pixels, plus 8 read and 2 written per pixel by the pooling

``data_range`` is given, so no call looks at the reference first.  ``composition`` is what a user can build from the library's
other public functions for the same score: five ``gaussian_filter(..., return_tensors=True)`` calls on r, x, r r, x x and r x, the
elementwise formula in torch and ``.mean()``; ``composition_over_fused`` is its time over that of the fused means-only call.

    python tools/bench_perceptual.py [--frames 64] [--windows 7] [--out profiles/perceptual_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2048
HBM_BYTES_PER_S = 6.29e12
DATA_RANGE = 64.0


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perceptual_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from barc4dip_amd.metrics import perceptual as P
    from barc4dip_amd.preprocessing import smooth as S

    torch.cuda.set_device(0)
    T = args.frames
    rng = np.random.default_rng(0)
    base = rng.poisson(40.0, (min(T, 4), N, N)).astype(np.float32)
    r = torch.from_numpy(np.ascontiguousarray(np.tile(base, (-(-T // base.shape[0]), 1, 1))[:T])).cuda()
    x = (r + 4.0 * torch.randn_like(r)).contiguous()
    r0 = r[0].contiguous()
    npix = T * N * N
    c1, c2 = (0.01 * DATA_RANGE) ** 2, (0.03 * DATA_RANGE) ** 2
    kw = {"data_range": DATA_RANGE, "return_tensors": True}
    box = {"window": "box", "size": 7, "sample_covariance": True}
    scales = len(P.MS_SSIM_WEIGHTS)
    ms_bytes = sum((8 + (10 if s + 1 < scales else 0)) / 4 ** s for s in range(scales))

    def composition():
        g = lambda a: S.gaussian_filter(a, 1.5, truncate=3.5, return_tensors=True)  # noqa: E731
        mr, mx = g(r), g(x)
        vr, vx, vrx = g(r * r) - mr * mr, g(x * x) - mx * mx, g(r * x) - mr * mx
        cs = (2 * vrx + c2) / (vr + vx + c2)
        return ((2 * mr * mx + c1) / (mr * mr + mx * mx + c1) * cs).mean(dim=(1, 2))

    cases = {
        "ssim_means_gaussian11_paired": (lambda: P.ssim(r, x, **kw), 8.0),
        "ssim_means_gaussian11_shared": (lambda: P.ssim(r0, x, **kw), 4.0 + 4.0 / T),
        "ssim_means_box7_paired": (lambda: P.ssim(r, x, **box, **kw), 8.0),
        "ssim_means_box7_shared": (lambda: P.ssim(r0, x, **box, **kw), 4.0 + 4.0 / T),
        "ssim_maps_gaussian11_paired": (lambda: P.ssim(r, x, full=True, **kw), 16.0),
        "ssim_maps_box7_paired": (lambda: P.ssim(r, x, full=True, **box, **kw), 16.0),
        "ms_ssim_paired": (lambda: P.ms_ssim(r, x, data_range=DATA_RANGE), ms_bytes),
        "ms_ssim_shared": (lambda: P.ms_ssim(r0, x, data_range=DATA_RANGE), None),
        "frame_errors_paired": (lambda: P.run_pair_errors(r, N * N, x, T, N, N), 8.0),
        "frame_errors_shared": (lambda: P.run_pair_errors(r0, 0, x, T, N, N), 4.0 + 4.0 / T),
        "composition_gaussian11_paired": (composition, None),
    }
    out = {"tool": "bench_perceptual", "device": torch.cuda.get_device_name(0), "frames": T, "frame": N, "windows": args.windows,
           "hbm_model_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}
    for name, (fn, bpp) in cases.items():
        t, calls = _timed(torch, fn, args.windows)
        torch.cuda.empty_cache()
        res = {"s_per_call": t, "calls_per_window": calls, "frames_per_s": T / t}
        if bpp is not None:
            res.update({"bytes_per_px": bpp, "effective_bytes_per_s": bpp * npix / t, "share_of_hbm_model": bpp * npix / HBM_BYTES_PER_S / t})
        out["cases"][name] = res
    fused = out["cases"]["ssim_means_gaussian11_paired"]["s_per_call"]
    out["composition_over_fused"] = out["cases"]["composition_gaussian11_paired"]["s_per_call"] / fused
    got = P.ssim(r[:2], x[:2], crop_border=False, **kw).cpu().numpy()
    ref = composition()[:2].cpu().numpy()
    out["fused_minus_composition_frames_0_1"] = [float(a - b) for a, b in zip(got, ref)]
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
