"""GPU tier of CLAHE, equalize_hist and the tile histograms (csrc/b4d_enhance.hip) against the NumPy model of
tests/enhancement_model.py.  Every comparison is on bits: integer results equal, float32 results bit-identical, counts equal.  A
float mismatch is an uncontrolled rounding in the kernel, not a tolerance to widen.

The cases are those of enhancement_model.CLAHE_CASES (what each is there for: tests/test_enhancement_host.py pins the branches):
tiles of 24 x 38 with padding on both axes under a non-square grid in OpenCV's order, exact multiples on the 16-byte path, 2 x 2
tiles with tiles of padding only, 65536 bins (the bin-slice path) at clip level 1 and with residual > L / 2, one occupied bin, float
frames with a NaN block that empties a tile, and frames that come back unchanged."""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enhancement_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

DATA = M.case_data()


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    g, w = (np.ascontiguousarray(a).ravel().view(f"u{a.itemsize}") for a in (got, want))
    bad = np.flatnonzero(g != w)
    if bad.size:
        k = bad[:5]
        raise AssertionError(f"{bad.size} of {got.size} values differ; first at {np.unravel_index(k, got.shape)}: "
                             f"{got.ravel()[k]} != {want.ravel()[k]}")


@functools.lru_cache(maxsize=None)
def model(name):
    key, kw, _ = M.CLAHE_CASES[name]
    return M.clahe_stack(DATA[key], **kw)[0]


def prep():
    import barc4dip_amd.preprocessing as p

    return p


@pytest.mark.parametrize("name", sorted(M.CLAHE_CASES))
def test_clahe_matches_the_model(name):
    key, kw, _ = M.CLAHE_CASES[name]
    same_bits(prep().clahe(DATA[key], **kw), model(name))


def test_frame_alone_gives_the_bits_of_the_batch():
    key, kw, _ = M.CLAHE_CASES["u8_clip2"]
    for k in range(3):
        same_bits(prep().clahe(DATA[key][k], **kw), model("u8_clip2")[k])
    key, kw, _ = M.CLAHE_CASES["f32_auto"]
    same_bits(prep().clahe(DATA[key][1], **kw), model("f32_auto")[1])


def test_tensor_in_and_tensor_out():
    import torch

    key, kw, _ = M.CLAHE_CASES["u8_clip2"]
    t = prep().clahe(torch.from_numpy(DATA[key]).cuda(), return_tensors=True, **kw)
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == DATA[key].shape
    same_bits(t.cpu().numpy(), model("u8_clip2").astype(np.float32))
    same_bits(prep().clahe(torch.from_numpy(DATA[key]).cuda(), **kw), model("u8_clip2"))
    key, kw, _ = M.CLAHE_CASES["f32_range"]
    t = prep().clahe(torch.from_numpy(DATA[key]).cuda(), return_tensors=True, **kw)
    same_bits(t.cpu().numpy(), model("f32_range"))
    one = prep().clahe(torch.from_numpy(DATA[key][0]).cuda(), return_tensors=True, **kw)
    assert tuple(one.shape) == DATA[key].shape[1:]
    same_bits(one.cpu().numpy(), model("f32_range")[0])


def test_transposed_input():
    key, kw, _ = M.CLAHE_CASES["u8_clip2"]
    tr = np.ascontiguousarray(DATA[key].transpose(0, 2, 1)).transpose(0, 2, 1)
    assert not tr.flags.c_contiguous
    same_bits(prep().clahe(tr, **kw), model("u8_clip2"))
    f = DATA["f32"]
    tr = np.ascontiguousarray(f.transpose(0, 2, 1)).transpose(0, 2, 1)
    same_bits(prep().clahe(tr, **M.CLAHE_CASES["f32_auto"][1]), model("f32_auto"))


def test_float_output_stays_in_range_and_keeps_nan():
    out = prep().clahe(DATA["f32"], **M.CLAHE_CASES["f32_range"][1])
    nan = np.isnan(DATA["f32"])
    assert np.array_equal(np.isnan(out), nan) and out[~nan].min() >= np.float32(0.2) and out[~nan].max() <= np.float32(0.8)


@pytest.mark.parametrize("key,kw", [("u8", {}), ("u16", {}), ("u16_dense", {}), ("f32", {"levels": 1024}),
                                    ("f32", {"levels": 1024, "value_range": (0.2, 0.8)}), ("f32", {}), ("u8_tiny", {})])
def test_equalize_hist_matches_the_model(key, kw):
    want, unchanged = M.equalize_stack(DATA[key], **kw)
    assert not any(unchanged)
    same_bits(prep().equalize_hist(DATA[key], **kw), want)


def test_equalize_hist_leaves_single_bin_frames_unchanged():
    import torch

    same_bits(prep().equalize_hist(DATA["u8_const"]), DATA["u8_const"])
    same_bits(prep().equalize_hist(DATA["f32_flat"]), DATA["f32_flat"])
    # all pixels inside one of 4 bins, though not equal; next to a frame that does change
    two = np.stack([np.linspace(0.30, 0.40, 16 * 24, dtype=np.float32).reshape(16, 24), DATA["f32"][0, 40:56, 60:84]])
    want, unchanged = M.equalize_stack(two, levels=4, value_range=(0.0, 1.0))
    assert unchanged == [True, False]
    got = prep().equalize_hist(two, levels=4, value_range=(0.0, 1.0))
    same_bits(got, want)
    same_bits(got[0], two[0])
    t = prep().equalize_hist(torch.from_numpy(DATA["u8"]).cuda(), return_tensors=True)
    same_bits(t.cpu().numpy(), M.equalize_stack(DATA["u8"])[0].astype(np.float32))


@pytest.mark.parametrize("key", ["u8", "u8_exact", "u8_tiny", "u16", "u16_dense", "u8_const"])
def test_frame_histogram_is_bincount(key):
    from barc4dip_amd.metrics import frame_histogram

    stack = DATA[key]
    L = 256 if stack.dtype == np.uint8 else 65536
    h = frame_histogram(stack)
    assert h["counts"].dtype == np.int64 and h["counts"].shape == (stack.shape[0], 1, 1, L) and h["n_valid"].shape == (stack.shape[0], 1, 1)
    for k, fr in enumerate(stack):
        assert np.array_equal(h["counts"][k, 0, 0], np.bincount(fr.ravel(), minlength=L))
        assert h["n_valid"][k, 0, 0] == fr.size
    one = frame_histogram(stack[0])
    assert one["counts"].shape == (1, 1, L) and np.array_equal(one["counts"][0, 0], np.bincount(stack[0].ravel(), minlength=L))
    assert np.all(h["lo"] == 0) and np.all(h["hi"] == L)


@pytest.mark.parametrize("key,kw", [("u8", {}), ("u16", {}), ("f32", {"levels": 1024}), ("f32", {"levels": 1024, "value_range": (0.2, 0.8)}),
                                    ("f32", {"levels": 40000})])
def test_frame_histogram_tiles_match_the_model(key, kw):
    from barc4dip_amd.metrics import frame_histogram

    stack = DATA[key]
    h = frame_histogram(stack, tile_grid_size=(4, 3), **kw)
    for k, fr in enumerate(stack):
        counts, n_valid, _ = M.frame_histogram(fr, (4, 3), **kw)
        assert np.array_equal(h["counts"][k], counts) and np.array_equal(h["n_valid"][k], n_valid)
    if key == "f32":
        assert h["n_valid"][0, 0, 0] == 0 and h["lo"].dtype == np.float32
        lo, hi = (M.frame_range(stack[0]) if "value_range" not in kw else np.float32(kw["value_range"]))
        assert h["lo"][0] == lo and h["hi"][0] == hi


def test_padding_only_tiles_are_counted():
    from barc4dip_amd.metrics import frame_histogram

    stack = DATA["u8_tiny"]
    h = frame_histogram(stack, tile_grid_size=(8, 8))
    for k, fr in enumerate(stack):
        counts, n_valid, seen = M.frame_histogram(fr, (8, 8))
        assert "pad_only_tile" in seen
        assert np.array_equal(h["counts"][k], counts) and np.all(h["n_valid"][k] == 4)


def test_c_entry_points_refuse_bad_arguments():
    import torch

    from barc4dip_amd import _ffi

    lib = _ffi.lib()
    f = torch.zeros((1, 16, 16), dtype=torch.float32, device="cuda")
    q = torch.tensor([[0.0, 1.0, 1.0, 0.0]], dtype=torch.float32, device="cuda")
    counts = torch.zeros((4, 256), dtype=torch.int32, device="cuda")
    nv = torch.zeros((4,), dtype=torch.int32, device="cuda")
    lut = torch.zeros((4, 256), dtype=torch.int16, device="cuda")
    out = torch.empty_like(f)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    null, st = C.c_void_p(0), _ffi.stream_ptr()
    EINVAL, ESIZE = -1, -2
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 2, 2, 65537, p(q), p(counts), p(nv), st) == ESIZE
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 2, 2, 1, p(q), p(counts), p(nv), st) == ESIZE
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 0, 2, 256, p(q), p(counts), p(nv), st) == EINVAL
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 2, 0, 256, p(q), p(counts), p(nv), st) == EINVAL
    assert lib.b4d_tile_histogram(null, 1, 16, 16, 2, 2, 256, p(q), p(counts), p(nv), st) == EINVAL
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 2, 2, 256, null, p(counts), p(nv), st) == EINVAL
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 2, 2, 256, p(q), null, p(nv), st) == EINVAL
    assert lib.b4d_tile_histogram(p(f), 0, 16, 16, 2, 2, 256, p(q), p(counts), p(nv), st) == EINVAL
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 2, 32, 256, p(q), p(counts), p(nv), st) == EINVAL      # 16 reflected rows of 16
    assert lib.b4d_tile_histogram(p(f), 1, 16, 16, 128, 64, 256, p(q), p(counts), p(nv), st) in (EINVAL, ESIZE)
    assert lib.b4d_equalize_lut(p(counts), p(nv), 1, 4, 65537, 2.0, 0, p(lut), null, st) == ESIZE
    assert lib.b4d_equalize_lut(p(counts), p(nv), 1, 0, 256, 2.0, 0, p(lut), null, st) == EINVAL
    assert lib.b4d_equalize_lut(null, p(nv), 1, 4, 256, 2.0, 0, p(lut), null, st) == EINVAL
    assert lib.b4d_equalize_lut(p(counts), p(nv), 1, 4, 256, -1.0, 0, p(lut), null, st) == EINVAL
    assert lib.b4d_equalize_lut(p(counts), p(nv), 1, 4, 256, 2.0, 2, p(lut), null, st) == EINVAL
    assert lib.b4d_equalize_lut(p(counts), p(nv), 1, 1, 256, 0.0, 1, p(lut), null, st) == EINVAL          # mode 1 without `unchanged`
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 2, 2, 65537, p(q), p(lut), null, 0, p(out), st) == ESIZE
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 0, 2, 256, p(q), p(lut), null, 0, p(out), st) == EINVAL
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 2, 2, 256, p(q), null, null, 0, p(out), st) == EINVAL
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 2, 2, 256, p(q), p(lut), null, 0, null, st) == EINVAL
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 2, 2, 256, p(q), p(lut), null, 4, p(out), st) == EINVAL
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 2, 2, 256, p(q), p(lut), null, 2, p(out), st) == EINVAL      # no interpolation: one tile
    assert lib.b4d_lut_apply(p(f), 1, 16, 16, 2, 2, 256, p(q), p(lut), null, 0, p(f), st) == EINVAL        # in == out
    assert b"b4d_lut_apply" in lib.b4d_last_error()
    torch.cuda.synchronize()
