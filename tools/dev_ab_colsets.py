"""In-process A/B of the "colsets" option (column-set tiles between the forward row pass and the column pass of the parity-tile
route) on the cfg2 workload (developer tool).

    python tools/dev_ab_colsets.py [--rounds 5] [--steps 20] [--values 0,1]

ONE plan and one set of tensors serve every value (the workspace address decides a few per cent of each kernel's time, DESIGN.md
8.6); the values alternate inside every round, in rotating order.  Per round and value: the library's own per-kernel HIP-event
times (row R2C, column, peak, row C2R), milliseconds per step, and whether PSD and autocorrelation of the first, a middle and the
last frame are bit-identical to those of the first value."""
import argparse
import ctypes as C
import sys

import torch

sys.path.insert(0, ".")
import barc4dip_amd  # noqa: E402
from barc4dip_amd import _ffi, synth  # noqa: E402

COLSETS_DEFAULT = 1

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--chunk", type=int, default=256)
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--values", default="0,1")
a = ap.parse_args()
values = [int(r) for r in a.values.split(",")]
T, n = a.frames, a.n
stack = synth.speckle_stack_device(T, n)
psd = torch.empty_like(stack)
ac = torch.empty_like(stack)
plan = _ffi.Plan(n, n, a.chunk)
lib = _ffi.lib()
flags = _ffi.REMOVE_MEAN | _ffi.NORM_PEAK
call = (plan.handle, C.c_void_p(stack.data_ptr()), T, C.c_void_p(psd.data_ptr()), 1.0 / (n * n), C.c_void_p(ac.data_ptr()), flags,
        _ffi.stream_ptr())
probe = sorted({0, T // 2, T - 1})
try:
    outs = {}
    for v in values:   # untimed: spin-up and first-launch costs of every value, and the outputs to compare
        barc4dip_amd.set_option("colsets", v)
        for _ in range(8):
            _ffi.check(lib.b4d_psd_autocorr2d(*call))
        torch.cuda.synchronize()
        outs[v] = (psd[probe].clone(), ac[probe].clone())
        same = torch.equal(outs[v][0], outs[values[0]][0]) and torch.equal(outs[v][1], outs[values[0]][1])
        print("colsets=%d  outputs identical to colsets=%d: %s" % (v, values[0], same), flush=True)
    wins = {v: [0, 0] for v in values}
    for rnd in range(a.rounds):
        k2, ks = {}, {}
        for v in [values[(k + rnd) % len(values)] for k in range(len(values))]:
            barc4dip_amd.set_option("colsets", v)
            kms = (C.c_float * 4)()
            for _ in range(a.steps):
                _ffi.check(lib.b4d_psd_autocorr2d_timed(*call, kms))
            torch.cuda.synchronize()
            k = [x / a.steps for x in kms]
            k2[v], ks[v] = k[1], k[0] + k[1] + k[3]
            ok = bool(torch.all(ac[:, n // 2, n // 2] == 1.0).item())
            print("round %d colsets=%d  r2c %.4f  col %.4f  peak %.4f  c2r %.4f  K1+K2+K3 %.4f ms  zero lag == 1: %s" %
                  (rnd, v, k[0], k[1], k[2], k[3], ks[v], ok), flush=True)
        for v in values[1:]:
            wins[v][0] += k2[v] < k2[values[0]]
            wins[v][1] += ks[v] < ks[values[0]]
    for v in values[1:]:
        print("colsets=%d against colsets=%d: K2 lower in %d of %d rounds, K1+K2+K3 lower in %d of %d rounds" %
              (v, values[0], wins[v][0], a.rounds, wins[v][1], a.rounds))
finally:
    barc4dip_amd.set_option("colsets", COLSETS_DEFAULT)
    plan.close()
