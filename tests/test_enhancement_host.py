"""Host tier of CLAHE, equalize_hist and frame_histogram: the NumPy model of tests/enhancement_model.py against an example worked
out by hand, its tables and padding against their definitions, the branches that the GPU cases must reach, argument errors without
a device, and the wiring.  No GPU needed."""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enhancement_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    return M.case_data()


def test_hand_computed_example():
    """4 x 4 pixels, 2 x 2 tiles of 2 x 2 pixels, 4 levels, clip_limit 2: clip = max(int(2 * 4 / 4), 1) = 2, scale = 3 / 4.
    tile (0, 0): h = 3 1 0 0, excess 1 -> 2 1 0 0, residual 1, step 4, bin 0 gains 1 -> 3 1 0 0, cum 3 4 4 4, table 2 3 3 3
    tile (0, 1): h = 0 1 0 3, excess 1 -> 0 1 0 2 -> 1 1 0 2, cum 1 2 2 4, x 0.75 = .75 1.5 1.5 3, table 1 2 2 3 (half to even)
    tile (1, 0): h = 0 0 4 0, excess 2 -> 0 0 2 0, residual 2, step 2, bins 0 and 2 gain 1 -> 1 0 3 0, cum 1 1 4 4, table 1 1 3 3
    tile (1, 1): h = 1 1 1 1, no excess, cum 1 2 3 4, table 1 2 2 3
    Rows and columns 0 and 3 see one tile (weights 0.5 / 0.5 of the same table, or 1 / 0); row 1 has ya = 0 between tile rows 0 and
    1, row 2 has ya = 0.5; columns likewise.  E.g. pixel (2, 2) = 0: top = 2 * .5 + 1 * .5 = 1.5, bottom = 1 * .5 + 1 * .5 = 1,
    res = .75 + .5 = 1.25 -> 1; pixel (0, 2) = 1: 3 * .5 + 2 * .5 = 2.5 in both rows -> 2.5 -> 2 (half to even)."""
    frame = np.array([[0, 0, 1, 3], [0, 1, 3, 3], [2, 2, 0, 1], [2, 2, 2, 3]], dtype=np.uint8)
    want = np.array([[2, 2, 2, 3], [2, 3, 3, 3], [3, 3, 1, 2], [3, 3, 2, 3]], dtype=np.uint8)
    got, seen = M.clahe(frame, 2.0, (2, 2), levels=4)
    assert np.array_equal(got, want)
    assert {"excess+", "excess0", "batch0", "step>1", "residual0"} <= seen
    counts, n_valid, _ = M.frame_histogram(frame, (2, 2), levels=4)
    assert counts.tolist() == [[[3, 1, 0, 0], [0, 1, 0, 3]], [[0, 0, 4, 0], [1, 1, 1, 1]]] and n_valid.tolist() == [[4, 4], [4, 4]]
    seen = set()
    assert M.clahe_table(np.array([3, 1, 0, 0]), 4, 4, 2.0, seen).tolist() == [2, 3, 3, 3]
    assert M.clahe_table(np.array([0, 0, 4, 0]), 4, 4, 2.0, seen).tolist() == [1, 1, 3, 3]


@pytest.mark.parametrize("clip", [0, 0.01, 1.0, 2.0, 40.0, 1e30])
def test_tables_monotone_and_in_range(data, clip):
    for key, L in (("u8", 256), ("u16", 65536)):
        counts, n_valid, _ = M.frame_histogram(data[key][0], (4, 3))
        for j in range(3):
            for i in range(4):
                t = M.clahe_table(counts[j, i], n_valid[j, i], L, clip, set())
                assert t.shape == (L,) and np.all(np.diff(t) >= 0) and t[0] >= 0 and t[-1] == L - 1


def test_no_clip_is_the_cumulative_table(data):
    fr = data["u8"][0]
    h = np.bincount(fr.ravel(), minlength=256)
    want = np.clip(np.rint(np.cumsum(h).astype(np.float32) * (np.float32(255) / np.float32(fr.size))), 0, 255)
    assert np.array_equal(M.clahe_table(h, fr.size, 256, 0, set()), want.astype(np.int64))
    # one tile: all four tables are that table, and v * xa1 + v * xa rounds back to the whole number v
    got, _ = M.clahe(fr, 0, (1, 1))
    assert np.array_equal(got, want.astype(np.uint8)[fr])


def test_reflected_padding_is_numpy_reflect(data):
    a = data["u8"][0].astype(np.int64)
    for pad_y, pad_x in ((2, 2), (0, 5), (69, 149), (7, 0)):
        assert np.array_equal(M.extend(a, pad_y, pad_x), np.pad(a, ((0, pad_y), (0, pad_x)), mode="reflect"))
    tx, ty, th, tw, pad_y, pad_x = M.geometry(70, 150, (4, 3))
    assert (th, tw, pad_y, pad_x) == (24, 38, 2, 2)
    assert M.geometry(9, 13, (8, 8))[2:] == (2, 2, 7, 3)
    assert M.geometry(64, 96, (8, 8))[2:] == (8, 12, 0, 0)


def test_quantiser_edges():
    s, inv = M.quantiser(0.2, 0.8, 1024)
    x = np.array([-np.inf, 0.1, 0.2, 0.5, 0.8, 0.9, np.inf, np.nan], dtype=np.float32)
    b = M.bins(x, np.float32(0.2), s, 1024)
    assert b[0] == 0 and b[1] == 0 and b[2] == 0 and b[4] == 1023 and b[5] == 1023 and b[6] == 1023 and b[7] == -1 and 0 < b[3] < 1023
    assert np.array_equal(M.bins(np.arange(256, dtype=np.uint8), 0, 1, 256), np.arange(256))


@pytest.mark.parametrize("name", sorted(M.CLAHE_CASES))
def test_gpu_cases_reach_their_branches(data, name):
    key, kw, need = M.CLAHE_CASES[name]
    out, seen = M.clahe_stack(data[key], **kw)
    assert need <= seen, f"{name} no longer reaches {sorted(need - seen)}"
    assert out.shape == data[key].shape
    if name == "f32_flat":
        assert out.tobytes() == data[key].tobytes() and seen == set()
    if name == "u8_clip40":
        assert "excess+" not in seen
    if key == "f32":
        assert np.array_equal(np.isnan(out), np.isnan(data[key]))


def test_equalize_model(data):
    out, unchanged = M.equalize_stack(data["u8"])
    assert unchanged == [False] * 3 and out.dtype == np.uint8 and out.min() == 0 and out.max() == 255
    out, unchanged = M.equalize_stack(data["u8_const"])
    assert unchanged == [True] and np.array_equal(out, data["u8_const"])
    out, unchanged = M.equalize_stack(data["f32_flat"])
    assert unchanged == [True, True] and out.tobytes() == data["f32_flat"].tobytes()
    # two occupied bins: the first maps to 0, the second to L - 1
    fr = np.array([[3, 3], [3, 9]], dtype=np.uint8)
    assert M.equalize_hist(fr)[0].tolist() == [[0, 0], [0, 255]]


# ------------------------------------------------------------------------------------------------- the library, without a device
def test_argument_errors_need_no_device():
    from barc4dip_amd.metrics import frame_histogram
    from barc4dip_amd.preprocessing import clahe, equalize_hist

    f = np.zeros((16, 24), dtype=np.float32)
    u = np.zeros((16, 24), dtype=np.uint8)
    bad = [
        lambda: clahe(f, tile_grid_size=(0, 8)), lambda: clahe(f, tile_grid_size=(8, -1)), lambda: clahe(f, tile_grid_size=(8,)),
        lambda: clahe(f, tile_grid_size=8), lambda: clahe(f, tile_grid_size=(2.5, 2)), lambda: clahe(f, tile_grid_size=(8, 8, 8)),
        lambda: clahe(np.zeros((128, 128), np.float32), tile_grid_size=(65, 64)),      # more than 4096 tiles
        lambda: clahe(f, levels=1), lambda: clahe(f, levels=65537), lambda: clahe(f, levels=10.5),
        lambda: clahe(f, clip_limit=-1.0), lambda: clahe(f, clip_limit=float("nan")),
        lambda: clahe(np.zeros((3, 24), np.float32), tile_grid_size=(2, 8)),           # 3 rows, 8 tiles: 5 reflected rows > 2
        lambda: clahe(np.zeros((24, 3), np.float32), tile_grid_size=(8, 2)),
        lambda: clahe(np.zeros(16, np.float32)), lambda: clahe(np.zeros((2, 2, 16, 16), np.float32)), lambda: clahe(np.zeros((0, 16), np.float32)),
        lambda: clahe(f, value_range=(1.0, 0.0)), lambda: clahe(f, value_range=(0.0, float("inf"))), lambda: clahe(f, value_range=3.0),
        lambda: clahe(u, levels=1024), lambda: clahe(u, value_range=(0, 255)),
        lambda: equalize_hist(f, levels=1), lambda: equalize_hist(np.zeros(16, np.float32)),
        lambda: frame_histogram(f, levels=65537), lambda: frame_histogram(f, tile_grid_size=(8,)), lambda: frame_histogram(np.zeros(5, np.float32)),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


def test_geometry_helper_agrees_with_the_model():
    from barc4dip_amd.preprocessing import enhancement as E

    for (ny, nx), grid in (((70, 150), (4, 3)), ((9, 13), (8, 8)), ((64, 96), (8, 8)), ((2048, 2048), (8, 8)), ((16, 16), (2, 2))):
        tx, ty, th, tw, _, _ = M.geometry(ny, nx, grid)
        assert E.tile_geometry(ny, nx, grid) == (tx, ty, th, tw)
    q = E.quantiser(np.float32(0.2), np.float32(0.8), 1024)
    s, inv = M.quantiser(0.2, 0.8, 1024)
    assert q.dtype == np.float32 and q.shape == (1, 4) and q[0, 0] == np.float32(0.2) and q[0, 1] == s and q[0, 2] == inv
    for lo, hi in ((1.0, 1.0), (np.nan, np.nan), (-np.inf, 1.0), (0.0, np.inf)):
        assert E.quantiser(np.float32(lo), np.float32(hi), 256)[0, 1] == 0.0      # frame left unchanged


def test_exports_and_wiring():
    import inspect

    import barc4dip_amd.metrics as metrics
    import barc4dip_amd.preprocessing as prep
    from barc4dip_amd import _ffi

    assert {"clahe", "equalize_hist", "enhancement"} <= set(prep.__all__) and "frame_histogram" in metrics.__all__
    assert prep.clahe is prep.enhancement.clahe and prep.equalize_hist is prep.enhancement.equalize_hist
    p = inspect.signature(prep.clahe).parameters
    assert list(p)[:3] == ["image", "clip_limit", "tile_grid_size"] and p["clip_limit"].default == 2.0 and p["tile_grid_size"].default == (8, 8)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("levels", "value_range", "return_tensors"))
    p = inspect.signature(metrics.frame_histogram).parameters
    assert list(p) == ["images", "levels", "value_range", "tile_grid_size"] and p["tile_grid_size"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("b4d_tile_histogram", "b4d_equalize_lut", "b4d_lut_apply"):
        assert name in _ffi.SIGNATURES
    mk = open(os.path.join(ROOT, "barc4dip_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*\bb4d_enhance\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "barc4dip_amd", "csrc", "b4d_enhance.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "asm" not in src.replace("__asm_unused__", "")
    assert not re.search(r"atomicAdd\(\s*\(?\s*float", src) and "getenv" not in src
