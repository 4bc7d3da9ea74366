"""Weighted / masked phase unwrapping on the MI355X (b4d_phase_unwrap_weighted, b4d_fringe_weights through
barc4dip_amd/signal/fringes.py) against the float64 oracle of tests/test_unwrap_weighted_host.py on the same float32 inputs.

Bars.  Integer levels: equal to the oracle's at every valid node, every case asserting the oracle's rounding margin below 0.25;
NaN exactly at the weight-0 nodes.  Values at the valid nodes: the float32 rounding of phase + 2 pi k, within one float32 spacing
of the value (the device may contract the multiply-add).  Harmonic fill at the weight-0 nodes against the float32 yardstick,
relative to the range of the map: FILL_BAR, twice the largest value observed on the device under the cap of 1e-5.  Node weights
against NumPy: the valid sets equal, the values within WEIGHT_BAR relative, twice the observed under the cap of 1e-6.  dy, dx of
the end-to-end recipe against the masked oracle: the SHIFT_BAR of tests/test_gpu_fringes.py.  Observed maxima are listed in
DESIGN.md section 18."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

from test_gpu_fringes import SHIFT_BAR
from test_unwrap_weighted_host import (CARRIERS, LEVEL_CASES, RECIPE, RECIPE_CARRIER_BARS, SMALL_CASES, batch_7x9, carrier_errors,
                                       fringe_valid, level_case, masked_case, recipe_error, recipe_frames, recipe_oracle,
                                       shared_7x9, small_case, unwrap_weighted_np, unwrap_weighted_pcg32)
from test_wavefront_weighted_host import weight_pattern

pytestmark = pytest.mark.gpu

FILL_CAP, WEIGHT_CAP = 1e-5, 1e-6
FILL_BAR = 1.6e-6          # 2 x 8.01e-7 (the 300 x 517 map; 9.4e-8 .. 5.3e-7 in the others)
WEIGHT_BAR = 1.2e-7        # 2 x 5.87e-8: the float32 rounding of the weight
assert FILL_BAR <= FILL_CAP and WEIGHT_BAR <= WEIGHT_CAP
TWO_PI = 2.0 * np.pi


@pytest.fixture(scope="module")
def fr():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd.signal import fringes

    return fringes


def _check_levels(got, ph, w, o, name):
    """Levels, NaN pattern and values of one map against the oracle dict o."""
    assert o["margin"] < 0.25, name
    valid = o["valid"]
    np.testing.assert_array_equal(np.isnan(got), ~valid, err_msg=name)
    k = np.round((got[valid] - ph.astype(np.float64)[valid]) / TWO_PI).astype(np.int64)
    np.testing.assert_array_equal(k, o["levels"][valid], err_msg=name)
    want = (ph.astype(np.float64)[valid] + TWO_PI * o["levels"][valid]).astype(np.float32)
    assert np.all(np.abs(got[valid] - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)), name


@pytest.mark.parametrize("shape,hole", SMALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_levels_on_degenerate_grids(fr, shape, hole):
    ph, w = small_case(shape, hole)
    got, info = fr.phase_unwrap(ph, weights=w, return_info=True)
    assert got.shape == ph.shape and got.dtype == np.float64
    _check_levels(got, ph, w, unwrap_weighted_np(ph, w), str(shape))
    assert info["converged"].all() and info["iterations"].shape == (1,)


def test_levels_of_a_batch_with_per_map_and_shared_weights(fr):
    ph, w = batch_7x9()
    got, info = fr.phase_unwrap(ph, weights=w, return_info=True)
    for t in range(3):
        _check_levels(got[t], ph[t], w[t], unwrap_weighted_np(ph[t], w[t]), f"7x9[{t}]")
    assert info["converged"].all() and np.all(info["iterations"] <= 500)
    ph, w = shared_7x9()
    got = fr.phase_unwrap(ph, mask=w > 0)
    for t in range(3):
        _check_levels(got[t], ph[t], w, unwrap_weighted_np(ph[t], w), f"7x9 shared[{t}]")


@pytest.mark.parametrize("name", list(LEVEL_CASES))
def test_levels_and_fill(fr, observe, name):
    """Levels with fill="nan"; with fill="harmonic" the same values at the valid nodes and the levelled p at the others, against
    the float32 yardstick.  The 300 x 517 map takes the workgroup-striding path (more than 256 workgroups of nodes per map)."""
    ph, w, _, o = level_case(name)
    got, info = fr.phase_unwrap(ph, weights=w, return_info=True)
    _check_levels(got, ph, w, o, name)
    print(f"unwrap_weighted.iterations.{name}: device {int(info['iterations'][0])}, oracle {o['iterations']}")
    assert info["converged"].all() and info["iterations"][0] <= 500
    filled = fr.phase_unwrap(ph, weights=w, fill="harmonic")
    valid = o["valid"]
    np.testing.assert_array_equal(filled[valid], got[valid])
    y = unwrap_weighted_pcg32(ph, w)
    err = float(np.max(np.abs(filled[~valid] - y["p"][~valid])) / np.ptp(y["p"]))
    print(f"unwrap_weighted.fill.{name}: {err:.3e}")
    observe(f"unwrap_weighted.fill.{name}", err, FILL_BAR)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy()).view(np.uint32)


def test_same_bits_alone_in_a_batch_repeated_and_with_shared_weights(fr):
    import torch

    names = ("37x53_disc", "37x53_disc_graded", "37x53_gap")        # 8, 28 and 12 iterations in float64
    ph = np.stack([level_case(n)[0] for n in names])
    w = np.stack([level_case(n)[1] for n in names])
    kw = dict(return_tensors=True, return_info=True)
    batch, info = fr.phase_unwrap(ph, weights=w, **kw)
    assert len(set(info["iterations"].tolist())) == 3
    again, info2 = fr.phase_unwrap(ph, weights=w, **kw)
    np.testing.assert_array_equal(_bits(batch), _bits(again))
    np.testing.assert_array_equal(info["iterations"], info2["iterations"])
    np.testing.assert_array_equal(info["residual"], info2["residual"])
    for t in range(3):
        alone, ia = fr.phase_unwrap(ph[t], weights=w[t], **kw)
        assert alone.shape == (37, 53) and alone.dtype == torch.float32
        np.testing.assert_array_equal(_bits(alone), _bits(batch[t]), err_msg=names[t])
        assert ia["iterations"][0] == info["iterations"][t] and ia["residual"][0] == info["residual"][t]
    shared = fr.phase_unwrap(ph, weights=w[1], return_tensors=True)
    repeated = fr.phase_unwrap(ph, weights=np.stack([w[1]] * 3), return_tensors=True)
    np.testing.assert_array_equal(_bits(shared), _bits(repeated))
    for fill in ("nan", "harmonic"):                                 # device tensors and bool masks take the same route
        a = fr.phase_unwrap(torch.from_numpy(ph).cuda(), mask=torch.from_numpy(w[0] > 0).cuda(), fill=fill, return_tensors=True)
        b = fr.phase_unwrap(ph, weights=(w[0] > 0).astype(np.uint8), fill=fill, return_tensors=True)
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_unweighted_calls_keep_todays_route_and_bits(fr):
    import torch

    ph = np.stack([level_case("37x53_disc")[0], masked_case((37, 53), 10.0, "disc_holes", 3)[0]])
    t = torch.from_numpy(ph).cuda()
    want = fr._unwrap_device(t)
    got, info = fr.phase_unwrap(ph, return_tensors=True, return_info=True)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert np.all(info["iterations"] == 0) and info["converged"].all() and np.all(info["residual"] == 0.0)
    np.testing.assert_array_equal(fr.phase_unwrap(ph), want.cpu().numpy().astype(np.float64))


def test_wrap_free_map_and_nan_under_a_mask(fr):
    rng = np.random.default_rng(5)
    smooth = (0.02 * np.add.outer(np.arange(33.0), 1.5 * np.arange(47.0)) - 1.0 + 0.01 * rng.standard_normal((33, 47))).astype(np.float32)
    smooth[16, 23] = -0.0
    assert np.abs(smooth).max() < np.pi
    w = weight_pattern("disc_holes", smooth.shape, 2)
    w[16, 23] = 1.0
    out = fr.phase_unwrap(smooth, weights=w, return_tensors=True).cpu().numpy()
    np.testing.assert_array_equal(out.view(np.uint32)[w > 0], smooth.view(np.uint32)[w > 0])        # -0.0 included
    assert np.all(np.isnan(out[w == 0]))
    ph, w, _, o = level_case("37x53_disc_holes")
    garbage = fr.phase_unwrap(ph, weights=w, fill="harmonic", return_tensors=True)
    holes = ph.copy()
    holes[w == 0] = np.nan
    holes[0, 0] = np.inf
    assert w[0, 0] == 0
    nan = fr.phase_unwrap(holes, weights=w, fill="harmonic", return_tensors=True)
    np.testing.assert_array_equal(_bits(nan), _bits(garbage))
    bad_w = w.copy()
    bad_w[0, 0], bad_w[0, 1], bad_w[1, 0] = np.nan, -3.0, np.inf
    np.testing.assert_array_equal(_bits(fr.phase_unwrap(holes, weights=bad_w, fill="harmonic", return_tensors=True)), _bits(garbage))
    self_masked = fr.phase_unwrap(holes, mask=np.ones(w.shape, bool))                               # NaN nodes mask themselves
    np.testing.assert_array_equal(self_masked, fr.phase_unwrap(ph, mask=w > 0))


def test_no_valid_node_and_max_iter(fr):
    ph = level_case("23x31_disc")[0]
    for fill in ("nan", "harmonic"):
        out, info = fr.phase_unwrap(np.stack([ph, ph]), weights=np.stack([np.zeros(ph.shape), np.ones(ph.shape)]), fill=fill,
                                    return_info=True)
        assert np.all(np.isnan(out[0])) and info["iterations"][0] == 0 and info["converged"][0]
        assert np.all(np.isfinite(out[1])) and info["iterations"][1] >= 1
    ph, w, _, o = level_case("37x53_disc_graded")
    assert o["iterations"] > 6
    with pytest.warns(RuntimeWarning, match="did not reach rtol"):
        out, info = fr.phase_unwrap(ph, weights=w, max_iter=3, return_info=True)
    assert not info["converged"][0] and info["iterations"][0] == 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out, info = fr.phase_unwrap(ph, weights=w, return_info=True)
    assert info["converged"][0] and info["iterations"][0] <= 500


# ---- b4d_fringe_weights
def _weights_np(S, R, min_level, min_visibility, mode):
    """(K, gy, gx) float64 of one frame: the formulas of include/b4d.h on complex128 copies of the complex64 harmonics."""
    S = S.astype(np.complex128)
    R = None if R is None else R.astype(np.complex128)
    ok = fringe_valid(S, R, min_level, min_visibility)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = S[0].real / np.abs(S[1:]) ** 2
        if R is not None:
            inv = inv + R[0].real / np.abs(R[1:]) ** 2
        val = np.ones(inv.shape) if mode == 0 else 1.0 / inv
    return np.where(ok[None] & np.isfinite(val) & (val > 0), val, 0.0)


@pytest.mark.parametrize("ref", ["none", "shared", "paired"])
def test_fringe_weights_against_numpy(fr, observe, ref):
    import torch

    n, K, gy, gx = 3, 2, 17, 19                     # 323 nodes: two workgroups per frame
    rng = np.random.default_rng(17)

    def harmonics(count):
        h = (rng.standard_normal((count, K + 1, gy, gx)) + 1j * rng.standard_normal((count, K + 1, gy, gx))) * 0.15
        h[:, 0] = rng.uniform(0.05, 1.0, (count, gy, gx))
        return h.astype(np.complex64)

    S = harmonics(n)
    S[1, 0, -1, -1] = 1.5                           # the maximum of frame 1 sits in the last node
    S[2, 0, 4, 5] = np.nan                          # a non-finite mean is never the maximum and is not valid
    S[0, 1, 2, 3] = 0.0                             # a dead harmonic: weight 0 in mode 1
    R = None if ref == "none" else harmonics(1 if ref == "shared" else n)
    tS = torch.from_numpy(S).cuda()
    tR = None if R is None else torch.from_numpy(R).cuda()
    for mode in (0, 1):
        for lvl, mv in ((0.5, 0.15), (0.0, 0.3), (0.3, 0.0), (0.0, 0.0)):
            got = fr._fringe_weights_device(tS, tR, ref == "paired", lvl, mv, bool(mode)).cpu().numpy()
            assert got.shape == (n, K, gy, gx) and got.dtype == np.float32
            for t in range(n):
                want = _weights_np(S[t], None if R is None else R[0 if ref == "shared" else t], lvl, mv, mode)
                np.testing.assert_array_equal(got[t] > 0, want > 0, err_msg=f"{ref} mode {mode} {lvl} {mv} frame {t}")
                pos = want > 0
                if mode == 0:
                    assert np.all(got[t][pos] == 1.0)
                elif pos.any():
                    observe(f"unwrap_weighted.weights.{ref}", np.max(np.abs(got[t][pos] / want[pos] - 1.0)), WEIGHT_BAR)
            if lvl > 0 and mv > 0:
                assert 0 < np.count_nonzero(got) < got.size


# ---- the end-to-end recipe
def test_recipe_masked_route_recovers_what_the_unmasked_route_loses(fr, observe):
    from barc4dip_amd.signal import wavefront_from_displacement

    ref, img, _, _ = recipe_frames()
    o = recipe_oracle(True)
    assert o["margin"] < 0.25
    kw = dict(carriers=CARRIERS, window=RECIPE["window"], step=RECIPE["step"])
    m = fr.fringe_displacement(ref, img, min_level=RECIPE["min_level"], min_visibility=RECIPE["min_visibility"], **kw)
    valid = m["valid"]
    assert valid.dtype == np.bool_ and valid.shape == m["dy"].shape
    np.testing.assert_array_equal(valid, o["valid"])
    for k in ("dy", "dx"):
        np.testing.assert_array_equal(np.isnan(m[k]), ~valid)
    np.testing.assert_array_equal(np.isnan(m["phase"]), np.broadcast_to(~valid, m["phase"].shape))
    err = recipe_error(m["dy"], m["dx"])[valid]
    print(f"unwrap_weighted.recipe: masked max {err.max():.3f} px over {valid.sum()} valid nodes")
    assert not np.any(err > 2.0)
    u = m["meta"]["unwrap"]
    print(f"unwrap_weighted.recipe: iterations {u['iterations'].tolist()}, oracle {o['iterations']}")
    assert u["iterations"].shape == (1, 2) and u["converged"].all() and np.all(u["iterations"] <= 500)
    np.testing.assert_array_equal(np.round((m["phase"][:, valid] - o["phase"][:, valid]) / TWO_PI), 0.0)
    for k in ("dy", "dx"):
        e = float(np.max(np.abs(m[k][valid] - o[k][valid])))
        print(f"unwrap_weighted.recipe.{k}: {e:.3e} px")
        observe(f"unwrap_weighted.recipe.{k}", e, SHIFT_BAR)
    plain = fr.fringe_displacement(ref, img, **kw)
    assert "valid" not in plain and plain["meta"]["unwrap"] is True
    miss = float(np.mean(recipe_error(plain["dy"], plain["dx"])[valid] > 2.0))
    print(f"unwrap_weighted.recipe: unmasked {miss:.3f} of the valid nodes beyond 2 px")
    assert miss >= 0.25
    wf = wavefront_from_displacement(m, pixel_size=0.65e-6, distance=0.5, mask=m["valid"])
    np.testing.assert_array_equal(np.isfinite(wf["wavefront"]), valid)
    np.testing.assert_array_equal(wf["valid"], valid)
    # graded weights move the seed to the window of largest weight, and with it the whole map by a constant number of levels (a
    # constant shift, the tilt of the wavefront): the field is the true one up to that constant
    snr = fr.fringe_displacement(ref, img, weights="snr", mask=valid, min_level=RECIPE["min_level"], **kw)
    np.testing.assert_array_equal(snr["valid"], valid)
    _, _, uy, ux = recipe_frames()
    ey, ex = (snr["dy"] - uy)[valid], (snr["dx"] - ux)[valid]
    assert not np.any(np.hypot(ey - np.median(ey), ex - np.median(ex)) > 2.0)


def test_recipe_stack_user_weights_mask_and_wrapped_mode(fr):
    """A stack with a shared mask and per-frame weight arrays gives each frame the bits of its own call; unwrap=False with a mask
    returns the wrapped phase with NaN at the invalid windows; tensors come back on the device."""
    import torch

    ref, img, _, _ = recipe_frames()
    valid = recipe_oracle(True)["valid"]
    kw = dict(carriers=CARRIERS, window=RECIPE["window"], step=RECIPE["step"])
    rng = np.random.default_rng(21)
    wts = rng.uniform(0.5, 2.0, (2,) + valid.shape)
    wts[1, 11, 13], wts[0, 5, 9] = np.nan, -1.0
    stack = np.stack([img, ref])
    both = fr.fringe_displacement(ref, stack, weights=wts, mask=valid, **kw)
    assert both["valid"].shape == (2,) + valid.shape and both["meta"]["unwrap"]["iterations"].shape == (2, 2)
    for t in range(2):
        alone = fr.fringe_displacement(ref, stack[t], weights=wts[t], mask=valid, **kw)
        for k in ("dy", "dx", "phase", "valid"):
            np.testing.assert_array_equal(alone[k], both[k][t], err_msg=f"{k}[{t}]")
    want = valid.copy()
    want[5, 9] = False
    np.testing.assert_array_equal(both["valid"][0], want)
    assert not both["valid"][1, 11, 13] and both["valid"][1].sum() == valid.sum() - 1
    np.testing.assert_allclose(both["dy"][1][both["valid"][1]], 0.0, rtol=0, atol=1e-6)          # the reference against itself
    wrapped = fr.fringe_displacement(ref, img, mask=valid, unwrap=False, **kw)
    plain = fr.fringe_displacement(ref, img, unwrap=False, **kw)
    np.testing.assert_array_equal(wrapped["valid"], valid)
    assert wrapped["meta"]["unwrap"] is False
    for k in ("dy", "dx"):
        np.testing.assert_array_equal(wrapped[k][valid], plain[k][valid])
        assert np.all(np.isnan(wrapped[k][~valid]))
    ten = fr.fringe_displacement(torch.from_numpy(ref).cuda(), torch.from_numpy(img).cuda(), mask=torch.from_numpy(valid).cuda(),
                                 return_tensors=True, **kw)
    assert ten["valid"].is_cuda and ten["valid"].dtype == torch.bool and ten["dy"].dtype == torch.float64
    np.testing.assert_array_equal(ten["valid"].cpu().numpy(), valid)


def test_recipe_carriers_with_a_level_mask(fr, observe):
    ref, _, _, _ = recipe_frames()
    got = fr.fringe_carriers(ref, window=RECIPE["window"], step=RECIPE["step"], min_level=0.5)
    err = carrier_errors(got)
    print(f"unwrap_weighted.recipe.carriers: {err}")
    for k in range(2):
        observe(f"unwrap_weighted.recipe.carriers{k}", err[k], RECIPE_CARRIER_BARS[k])


def test_c_abi_argument_errors(fr):
    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    assert int(lib.b4d_phase_unwrap_weighted_workspace_bytes(1, 2049, 4)) == 0 and int(lib.b4d_fringe_weights_workspace_bytes(0, 4, 4)) == 0
    n, ny, nx = 2, 5, 6
    ph = torch.zeros((n, ny, nx), dtype=torch.float32, device="cuda")
    w = torch.ones((n, ny, nx), dtype=torch.float32, device="cuda")
    out = torch.empty_like(ph)
    ws = torch.empty(int(lib.b4d_phase_unwrap_weighted_workspace_bytes(n, ny, nx)), dtype=torch.uint8, device="cuda")
    it = torch.empty((n,), dtype=torch.int32, device="cuda")
    rs = torch.empty((n,), dtype=torch.float64, device="cuda")

    def call(stride=ny * nx, rtol=1e-6, max_iter=10, o=out, nn=n):
        return lib.b4d_phase_unwrap_weighted(D.ptr(ph), D.ptr(w), stride, nn, ny, nx, rtol, max_iter, 1, D.ptr(ws), D.ptr(o), D.ptr(it),
                                             D.ptr(rs), _ffi.stream_ptr())

    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ph) and it.tolist() == [0, 0]
    for bad in (dict(stride=7), dict(rtol=-1.0), dict(max_iter=-1), dict(o=ph), dict(nn=0)):
        assert call(**bad) == -1, bad
    S = torch.ones((1, 3, 4, 4), dtype=torch.complex64, device="cuda")
    wo = torch.empty((1, 2, 4, 4), dtype=torch.float32, device="cuda")
    fws = torch.empty(int(lib.b4d_fringe_weights_workspace_bytes(1, 4, 4)), dtype=torch.uint8, device="cuda")

    def wcall(K=2, lvl=0.5, mv=0.1, mode=0, stride=0):
        return lib.b4d_fringe_weights(D.ptr(S), None, stride, 1, K, 4, 4, lvl, mv, mode, D.ptr(wo), D.ptr(fws), _ffi.stream_ptr())

    assert wcall() == 0
    torch.cuda.synchronize()
    assert torch.all(wo == 1.0)
    for bad in (dict(K=0), dict(K=5), dict(lvl=1.5), dict(lvl=-0.1), dict(mv=-1.0), dict(mode=2)):
        assert wcall(**bad) == -1, bad
