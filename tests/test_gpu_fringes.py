"""Fringe analysis on the MI355X (b4d_fringe_demodulate, b4d_fringe_compare, b4d_phase_unwrap, b4d_fringe_shift through
barc4dip_amd/signal/fringes.py) against the float64 oracle of tests/test_fringes_host.py on the same float32 inputs.

Bars.  Harmonic maps: |S - S_oracle| / max S_0 at DEMOD_BAR, twice the largest value observed on the device over the demodulation
cases, under the cap of 1e-5 (the project's amplitude bar for transform outputs; a condition, not a measurement).  dy, dx: SHIFT_BAR
pixels, twice the observed maximum under the cap of 1e-4.  transmission, visibility, dark field: RATIO_BAR, twice the observed
maximum under the cap of 2e-5.  Carriers against the host oracle of the same algorithm: CARRIER_GPU_BAR cycles per pixel, twice the
observed; against the truth: the bars of the host file.  Chain: radii within 1e-3 relative, a cap.  Integer levels of the unwrap:
equal to the oracle's, every case asserting the oracle's rounding margin below 0.25.  Observed maxima on an MI355X are listed in
DESIGN.md section 17."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from test_fringes_host import (CARRIER_BARS, CARRIERS, CARRIERS_B, CASES, analyse, case_frames, case_oracle, demodulate,
                               estimate_carriers, unwrap, wrap)

pytestmark = pytest.mark.gpu

DEMOD_CAP, SHIFT_CAP, RATIO_CAP = 1e-5, 1e-4, 2e-5
DEMOD_BAR = 3.4e-7          # 2 x 1.70e-7 (the 48 x 4096 case; 3.8e-8 .. 1.5e-7 in the others)
SHIFT_BAR = 1.45e-6         # pixels: 2 x 7.24e-7 (dx of the sheared 256 x 320 case)
RATIO_BAR = 1.05e-6         # 2 x 5.22e-7 (dark field of the 256^2 case; transmission 1.9e-7, visibility 1.4e-7)
CARRIER_GPU_BAR = 9.2e-11   # cycles per pixel: 2 x 4.6e-11
assert DEMOD_BAR <= DEMOD_CAP and SHIFT_BAR <= SHIFT_CAP and RATIO_BAR <= RATIO_CAP

CARRIERS_4 = np.array([[0.004, 0.137], [0.133, -0.006], [0.2, 0.21], [-0.13, 0.25]])
CARRIERS_WIDE = np.array([[0.13, 0.127], [0.005, 0.3317]])


@pytest.fixture(scope="module")
def fr():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import fringes

    return fringes


@functools.lru_cache(maxsize=None)
def _frame(shape, key, dtype="float32", T=1):
    """Seeded frames (T, H, W): fringes at the carriers `key` under a smooth envelope plus white noise, read-only."""
    from barc4dip_amd import synth

    carriers = {"4": CARRIERS_4, "b": CARRIERS_B, "wide": CARRIERS_WIDE, "a": CARRIERS}[key]
    rng = np.random.default_rng(shape[0] * 7919 + shape[1])
    out = []
    for t in range(T):
        shift = lambda y, x, t=t: (0.3 * np.sin(y / 17.0 + t) + 0.0 * x, 0.2 * np.cos(x / 23.0 - t) + 0.0 * y)  # noqa: E731
        f = synth.fringe_frame(shape, carriers, shift, visibility=0.8 / len(carriers)) + 0.02 * rng.standard_normal(shape)
        out.append(30000.0 + 2000.0 * f if dtype == "uint16" else f)
    a = np.stack(out).astype(dtype)
    a.setflags(write=False)
    return a


def _check_harmonics(observe, name, got, frame, carriers, window, step):
    want = demodulate(frame.astype(np.float64), carriers, window, step)
    assert got.shape == want.shape and got.dtype == np.complex64
    assert np.all(got[0].imag == 0.0)
    err = float(np.max(np.abs(got - want)) / np.max(want[0].real))
    print(f"fringes.demod.{name}: {err:.3e}")
    observe(f"fringes.demod.{name}", err, DEMOD_BAR)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_demodulate_one_to_four_carriers(fr, observe, K):
    frame = _frame((96, 128), "4")[0]
    res = fr.fringe_demodulate(frame, CARRIERS_4[:K], window=16, step=8)
    assert res["harmonics"].shape == (K + 1, 11, 15)
    _check_harmonics(observe, f"k{K}", res["harmonics"], frame, CARRIERS_4[:K], (16, 16), (8, 8))
    np.testing.assert_array_equal(res["y"], 8 * np.arange(11) + 7.5)


DEMOD_CASES = {
    "odd_100x131": ((100, 131), "b", (24, 40), (12, 8)),            # odd frame, leftover rows and columns, unaligned rows
    "wide_48x4096": ((48, 4096), "wide", (16, 64), (16, 32)),       # large coordinates in the phase, several x tiles
    "one_node_64": ((64, 64), "a", (64, 64), (32, 32)),             # the window is the frame
    "step_over_window": ((96, 128), "4", (16, 16), (20, 24)),       # gaps between the windows
    "window_256": ((256, 300), "a", (256, 256), (128, 4)),          # the largest window
}


@pytest.mark.parametrize("name", list(DEMOD_CASES))
def test_demodulate_shapes(fr, observe, name):
    shape, key, window, step = DEMOD_CASES[name]
    carriers = {"4": CARRIERS_4[:2], "b": CARRIERS_B, "wide": CARRIERS_WIDE, "a": CARRIERS}[key]
    frame = _frame(shape, key)[0]
    res = fr.fringe_demodulate(frame, carriers, window=window, step=step)
    _check_harmonics(observe, name, res["harmonics"], frame, carriers, window, step)


def test_demodulate_uint16_stack_and_batch_independence(fr, observe):
    """A uint16 stack of three frames on a 30 000-count offset; frame t alone carries the bits it has inside the stack."""
    stack = _frame((96, 128), "4", "uint16", 3)
    res = fr.fringe_demodulate(stack, CARRIERS_4[:2], window=16, step=8)
    assert res["harmonics"].shape == (3, 3, 11, 15)
    for t in range(3):
        _check_harmonics(observe, "uint16", res["harmonics"][t], stack[t].astype(np.float32), CARRIERS_4[:2], (16, 16), (8, 8))
        alone = fr.fringe_demodulate(stack[t], CARRIERS_4[:2], window=16, step=8)
        np.testing.assert_array_equal(alone["harmonics"], res["harmonics"][t])


# ---- phase_unwrap
def _levels(out, ph):
    return np.round((out.astype(np.float64) - ph.astype(np.float64)) / (2.0 * np.pi)).astype(np.int64)


def test_unwrap_levels_of_the_sheared_case(fr):
    o = case_oracle("d_256x320_sheared")
    ph = o["wrapped"].astype(np.float32)
    want = [unwrap(p) for p in ph]
    assert max(w[2] for w in want) < 0.25
    assert max(int(w[1].max() - w[1].min()) for w in want) >= 2
    got = fr.phase_unwrap(ph)
    assert got.shape == ph.shape and got.dtype == np.float64
    for k in range(2):
        np.testing.assert_array_equal(_levels(got[k], ph[k]), want[k][1])
        np.testing.assert_allclose(got[k], want[k][0], rtol=0, atol=2e-6)     # float32 rounding of values up to 4 pi


def test_unwrap_edge_grids(fr):
    """A constant map and a map without wraps come back bit for bit; 1 x N and N x 1 ramps; a NaN node spoils its own map only."""
    import torch

    const = np.full((9, 14), 1.25, np.float32)
    np.testing.assert_array_equal(fr.phase_unwrap(const), const.astype(np.float64))
    rng = np.random.default_rng(5)
    smooth = (0.02 * np.add.outer(np.arange(33.0), 1.5 * np.arange(47.0)) - 1.0 + 0.01 * rng.standard_normal((33, 47))).astype(np.float32)
    smooth[3, 4] = -0.0
    assert np.abs(smooth).max() < np.pi
    out = fr.phase_unwrap(torch.from_numpy(smooth).cuda(), return_tensors=True)
    assert out.dtype == torch.float32 and out.is_cuda
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), smooth.view(np.uint32))
    for shape in ((1, 37), (37, 1), (2, 2), (1, 1)):
        ramp = wrap(0.7 * np.arange(shape[0] * shape[1], dtype=np.float64).reshape(shape)).astype(np.float32)
        want = unwrap(ramp)
        assert want[2] < 0.25
        np.testing.assert_array_equal(_levels(fr.phase_unwrap(ramp), ramp), want[1], err_msg=str(shape))
    pair = np.stack([smooth, smooth])
    pair[0, 10, 20] = np.nan
    got = fr.phase_unwrap(pair)
    assert np.all(np.isnan(got[0]))
    np.testing.assert_array_equal(got[1], smooth.astype(np.float64))


# ---- fringe_displacement
def _check_maps(observe, name, res, o, absolute=False):
    assert o["margin"] < 0.25
    for k in ("dy", "dx", "peak"):
        assert res[k].dtype == np.float64 and res[k].shape == o["dy"].shape
    if o["levels"] is not None:
        np.testing.assert_array_equal(np.round((res["phase"] - o["phase"]) / (2.0 * np.pi)), 0.0)
    for k in ("dy", "dx"):
        err = float(np.max(np.abs(res[k] - o[k])))
        print(f"fringes.shift.{name}.{k}: {err:.3e} px")
        observe(f"fringes.shift.{name}", err, SHIFT_BAR)
    keys = ("visibility", "peak") if absolute else ("visibility", "peak", "transmission", "dark_field")
    for k in keys:
        err = float(np.max(np.abs(res[k] - o[k])))
        print(f"fringes.ratio.{name}.{k}: {err:.3e}")
        observe(f"fringes.ratio.{name}", err, RATIO_BAR)
    if absolute:
        assert "transmission" not in res and "dark_field" not in res


@pytest.mark.parametrize("name", ["a_256_w32", "b_192x160_w24x40", "d_256x320_sheared", "e_256_poisson"])
def test_displacement_matches_the_oracle(fr, observe, name):
    shape, window, step, carriers, *_ = CASES[name]
    ref, img, _, _ = case_frames(name)
    res = fr.fringe_displacement(ref, img, carriers=carriers, window=window, step=step)
    assert res["phase"].shape == (2,) + res["dy"].shape and res["meta"]["unwrap"] and not res["meta"]["absolute"]
    _check_maps(observe, name, res, case_oracle(name))


def test_displacement_absolute_wrapped_and_tensors(fr, observe):
    import torch

    shape, window, step, carriers, *_ = CASES["a_256_w32"]
    ref, img, _, _ = case_frames("a_256_w32")
    res = fr.fringe_displacement(None, img, carriers=carriers, window=window, step=step)
    _check_maps(observe, "absolute", res, analyse(None, img, carriers, window, step), absolute=True)
    res = fr.fringe_displacement(ref, img, carriers=carriers, window=window, step=step, unwrap=False)
    o = analyse(ref, img, carriers, window, step, do_unwrap=False)
    assert np.max(np.abs(res["phase"])) <= np.float32(np.pi)
    _check_maps(observe, "wrapped", res, o)
    ten = fr.fringe_displacement(torch.from_numpy(ref).cuda(), torch.from_numpy(img).cuda(), carriers=carriers, window=window, step=step,
                                 unwrap=False, return_tensors=True)
    for k in ("dy", "dx", "peak", "phase", "visibility", "transmission", "dark_field"):
        assert torch.is_tensor(ten[k]) and ten[k].is_cuda
        np.testing.assert_array_equal(ten[k].cpu().numpy().astype(np.float64), res[k], err_msg=k)
    assert ten["dy"].dtype == torch.float64 and ten["phase"].dtype == torch.float32


MAP_KEYS = ("dy", "dx", "peak", "phase", "visibility", "transmission", "dark_field")


def test_displacement_same_bits_alone_in_a_stack_and_with_a_paired_reference(fr):
    shape, window, step, carriers, *_ = CASES["a_256_w32"]
    ref, img, _, _ = case_frames("a_256_w32")
    stack = np.stack([img, ref, np.roll(img, 3, axis=1)])
    kw = dict(carriers=carriers, window=window, step=step)
    shared = fr.fringe_displacement(ref, stack, **kw)
    paired = fr.fringe_displacement(np.stack([ref] * 3), stack, **kw)
    assert shared["dy"].shape == (3, 15, 15)
    for k in MAP_KEYS:
        np.testing.assert_array_equal(shared[k], paired[k], err_msg=k)
    for t in range(3):
        alone = fr.fringe_displacement(ref, stack[t], **kw)
        for k in MAP_KEYS:
            np.testing.assert_array_equal(alone[k], shared[k][t], err_msg=f"{k}[{t}]")
    np.testing.assert_allclose(shared["dy"][1], 0.0, rtol=0, atol=1e-6)          # the reference against itself
    np.testing.assert_array_equal(shared["transmission"][1], 1.0)


def test_carriers_match_the_host_oracle_and_the_truth(fr, observe):
    shape, window, step, carriers, *_ = CASES["d_256x320_sheared"]
    ref, img, _, _ = case_frames("d_256x320_sheared")
    got = fr.fringe_carriers(ref, window=window, step=step)
    want = estimate_carriers(ref, window, step)
    assert got.shape == (2, 2) and got.dtype == np.float64
    for k in range(2):
        print(f"fringes.carriers[{k}]: vs oracle {np.max(np.abs(got[k] - want[k])):.3e}, vs truth {np.max(np.abs(got[k] - carriers[k])):.3e}")
        observe("fringes.carriers.oracle", np.max(np.abs(got[k] - want[k])), CARRIER_GPU_BAR)
        observe(f"fringes.carriers.truth{k}", np.max(np.abs(got[k] - carriers[k])), CARRIER_BARS[k])
    auto = fr.fringe_displacement(ref, img, window=window, step=step)
    np.testing.assert_array_equal(auto["carriers"], got)
    given = fr.fringe_displacement(ref, img, carriers=got, window=window, step=step)
    np.testing.assert_array_equal(auto["dy"], given["dy"])


def test_chain_magnification_gives_the_radii(fr, observe):
    """Pure magnification m through wavefront_from_displacement(..., weights="peak"): radius = distance / m, within 1e-3 relative."""
    from barc4dip_amd.signal import wavefront_from_displacement

    shape, window, step, carriers, *_ = CASES["m_256_magnified"]
    ref, img, _, _ = case_frames("m_256_magnified")
    res = fr.fringe_displacement(ref, img, carriers=carriers, window=window, step=step)
    wf = wavefront_from_displacement(res, pixel_size=0.65e-6, distance=0.5, weights="peak")
    for key, m in (("radius_y", 0.03), ("radius_x", 0.025)):
        err = abs(wf[key][0] * m / 0.5 - 1.0)
        print(f"fringes.chain.{key}: {err:.3e}")
        observe(f"fringes.chain.{key}", err, 1e-3)


def test_c_abi_argument_errors(fr):
    import ctypes as C

    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    frames = torch.zeros((1, 64, 64), dtype=torch.float32, device="cuda")
    out = torch.zeros((1, 3, 3, 3), dtype=torch.complex64, device="cuda")
    ws = torch.zeros(int(lib.b4d_fringe_demodulate_workspace_bytes(2, 64, 64, 32, 32)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0 and int(lib.b4d_fringe_demodulate_workspace_bytes(5, 64, 64, 32, 32)) == 0
    assert int(lib.b4d_phase_unwrap_workspace_bytes(1, 2049, 4)) == 0
    f = (C.c_double * 4)(0.0, 0.125, 0.125, 0.0)

    def call(n=1, K=2, wy=32, wx=32, sty=16, stx=16):
        return lib.b4d_fringe_demodulate(D.ptr(frames), n, 64, 64, C.cast(f, C.c_void_p), K, wy, wx, sty, stx, D.ptr(ws), D.ptr(out),
                                         _ffi.stream_ptr())

    assert call() == 0
    torch.cuda.synchronize()
    for bad, rc in ((dict(K=0), -1), (dict(K=5), -1), (dict(wy=257), -2), (dict(wx=1), -2), (dict(sty=0), -1), (dict(n=0), -1),
                    (dict(wy=128), -1)):
        assert call(**bad) == rc, bad
