"""In-process A/B of the "ysplit" routes of b4d_psd_autocorr2d on the cfg2 workload (developer tool).

    python tools/dev_ab_ysplit.py [--rounds 5] [--steps 20] [--routes 0,1]

ONE plan and one set of tensors serve every route (the workspace address decides a few per cent of each kernel's time, DESIGN.md
8.6); the routes alternate inside every round, in rotating order.  Per round and route: the library's own per-kernel HIP-event
times (row R2C, column, peak, row C2R), milliseconds per step."""
import argparse
import ctypes as C
import sys

import torch

sys.path.insert(0, ".")
import barc4dip_amd  # noqa: E402
from barc4dip_amd import _ffi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--chunk", type=int, default=256)
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--routes", default="0,1")
a = ap.parse_args()
routes = [int(r) for r in a.routes.split(",")]
T, n = a.frames, a.n
stack = synth.speckle_stack_device(T, n)
psd = torch.empty_like(stack)
ac = torch.empty_like(stack)
plan = _ffi.Plan(n, n, a.chunk)
lib = _ffi.lib()
flags = _ffi.REMOVE_MEAN | _ffi.NORM_PEAK
call = (plan.handle, C.c_void_p(stack.data_ptr()), T, C.c_void_p(psd.data_ptr()), 1.0 / (n * n), C.c_void_p(ac.data_ptr()), flags,
        _ffi.stream_ptr())
try:
    for r in routes:   # untimed: spin-up and first-launch costs of every route
        barc4dip_amd.set_option("ysplit", r)
        for _ in range(8):
            _ffi.check(lib.b4d_psd_autocorr2d(*call))
    torch.cuda.synchronize()
    wins = 0
    for rnd in range(a.rounds):
        tot = {}
        for r in [routes[(k + rnd) % len(routes)] for k in range(len(routes))]:
            barc4dip_amd.set_option("ysplit", r)
            kms = (C.c_float * 4)()
            for _ in range(a.steps):
                _ffi.check(lib.b4d_psd_autocorr2d_timed(*call, kms))
            torch.cuda.synchronize()
            k = [v / a.steps for v in kms]
            tot[r] = k[0] + k[1] + k[3]
            ok = bool(torch.all(ac[:, n // 2, n // 2] == 1.0).item())
            print("round %d ysplit=%d  r2c %.4f  col %.4f  peak %.4f  c2r %.4f  K1+K2+K3 %.4f ms  zero lag == 1: %s" %
                  (rnd, r, k[0], k[1], k[2], k[3], tot[r], ok), flush=True)
        if 0 in tot:
            best = min(v for r, v in tot.items() if r != 0) if len(tot) > 1 else tot[0]
            wins += best < tot[0]
    print("rounds in which a ysplit route beat route 0: %d of %d" % (wins, a.rounds))
finally:
    plan.close()
