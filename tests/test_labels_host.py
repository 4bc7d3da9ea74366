"""Connected-component labelling without a GPU: the model of tests/labels_model.py against scipy.ndimage one function at a time,
the numbering rule, hysteresis and selection on the model, every argument error of the Python entry points, and the union-find
core of csrc/b4d_label.hpp run serially by a small C++ program with a 4 x 8 tile and scan blocks of 16 pixels on the seam cases,
compared with scipy.ndimage.label."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import labels_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def scene():
    lab, n = M.label(M.random_mask((41, 57), 0.45, 5), 1)
    img = M.smooth_frame((41, 57), 6)
    return lab, n, img, M.properties(lab, img), np.arange(1, n + 1)


def test_model_sum_equals_sum_labels(scene):
    lab, n, img, p, idx = scene
    want = ndimage.sum_labels(img.astype(np.float64), lab, idx)
    assert np.allclose(p["sum"], want, rtol=1e-13, atol=0) and np.array_equal(p["area"], ndimage.sum_labels(np.ones(lab.shape), lab, idx))
    assert np.allclose(p["flux"], want, rtol=1e-13, atol=0)      # positive frame, background 0


def test_model_centroids_equal_center_of_mass(scene):
    lab, n, img, p, idx = scene
    geo = np.array(ndimage.center_of_mass(np.ones(lab.shape), lab, idx))
    wgt = np.array(ndimage.center_of_mass(img.astype(np.float64), lab, idx))
    assert np.allclose(p["cy"], geo[:, 0], atol=1e-11) and np.allclose(p["cx"], geo[:, 1], atol=1e-11)
    assert np.allclose(p["wcy"], wgt[:, 0], atol=1e-11) and np.allclose(p["wcx"], wgt[:, 1], atol=1e-11)


def test_model_extrema_equal_minimum_maximum_and_position(scene):
    lab, n, img, p, idx = scene
    assert np.array_equal(p["min"], ndimage.minimum(img, lab, idx)) and np.array_equal(p["max"], ndimage.maximum(img, lab, idx))
    flat = img.copy()
    flat[lab == 3] = 7.0                       # a tie over a whole region: the first pixel in raster order
    q = M.properties(lab, flat)
    pos = np.array(ndimage.maximum_position(flat, lab, idx))
    assert np.array_equal(q["max_y"], pos[:, 0]) and np.array_equal(q["max_x"], pos[:, 1])
    ys, xs = np.nonzero(lab == 3)
    assert (q["max_y"][2], q["max_x"][2]) == (ys[0], xs[0])


def test_model_boxes_equal_find_objects(scene):
    lab, n, img, p, idx = scene
    for k, sl in enumerate(ndimage.find_objects(lab)):
        assert (p["y0"][k], p["y1"][k], p["x0"][k], p["x1"][k]) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)


def test_model_moments_nan_saturation_and_gaps():
    lab = np.zeros((6, 7), np.int32)
    lab[1:4, 2:5] = 2                          # label 1 and 3 have no pixel
    img = np.arange(42, dtype=np.float32).reshape(6, 7)
    img[2, 3] = np.nan
    p = M.properties(lab, img, background=10.0, saturation=24.0, n=3)
    assert list(p["area"]) == [0, 9, 0] and list(p["n_nan"]) == [0, 1, 0] and list(p["n_saturated"]) == [0, 2, 0]
    assert np.isnan(p["cy"][0]) and np.isnan(p["min"][2]) and p["max_y"][0] == -1 and p["sum"][0] == 0.0
    v = img[1:4, 2:5].astype(np.float64)
    y, x = np.indices(v.shape)
    ok = ~np.isnan(v)
    w = np.maximum(v[ok] - 10.0, 0.0)
    wy, wx = np.sum(w * y[ok]) / w.sum(), np.sum(w * x[ok]) / w.sum()
    assert np.isclose(p["wcy"][1], 1 + wy) and np.isclose(p["wcx"][1], 2 + wx) and np.isclose(p["flux"][1], w.sum())
    assert np.isclose(p["var_y"][1], np.sum(w * (y[ok] - wy) ** 2) / w.sum())
    assert np.isclose(p["cov_yx"][1], np.sum(w * (y[ok] - wy) * (x[ok] - wx)) / w.sum())
    assert (p["max"][1], p["max_y"][1], p["max_x"][1]) == (25.0, 3, 4)


def test_numbering_is_the_raster_order_of_first_pixels():
    for conn in (1, 2):
        for d in M.DENSITIES:
            lab, n = M.label(M.random_mask((37, 53), d, 11), conn)
            first = [np.flatnonzero(lab.ravel() == k)[0] for k in range(1, n + 1)]
            assert first == sorted(first) and len(first) == n


def test_hysteresis_keeps_regions_whose_maximum_exceeds_high():
    img = np.zeros((5, 9), np.float32)
    img[1, 1:3] = (2.0, 6.0)       # kept: maximum 6 > 5
    img[3, 4:7] = (2.0, 5.0, 3.0)  # dropped: its maximum equals high
    img[1, 7] = 9.0                # kept
    lab, n = M.hysteresis(img, 1.0, 5.0, 1)
    assert n == 2 and lab[1, 1] == lab[1, 2] == 1 and lab[1, 7] == 2 and not lab[3].any()


def test_select_semantics_on_the_model():
    lab = np.zeros((8, 10), np.int32)
    lab[0, 0:2] = 1                # area 2, on the border
    lab[2:4, 2:4] = 2              # area 4
    lab[2:4, 6:8] = 3              # area 4: ties with 2
    lab[5:7, 1:4] = 4              # area 6
    lab[6, 8] = 5                  # area 1
    assert M.select(lab, min_area=2)[1] == 4 and M.select(lab, max_area=4)[1] == 4
    out, n = M.select(lab, clear_border=True)
    assert n == 4 and out[0, 0] == 0 and out[2, 2] == 1
    out, n = M.select(lab, largest=2)
    assert n == 2 and out[2, 2] == 1 and out[5, 1] == 2 and out[2, 6] == 0     # the tie goes to the lower label
    out, n = M.select(lab, keep=[True, False, True, False, True])
    assert n == 3 and out[0, 0] == 1 and out[2, 6] == 2 and out[6, 8] == 3


def test_select_mask_and_renumber_of_the_package_equal_the_model():
    from barc4dip_amd.geometry import labels as L

    labs = [M.label(M.random_mask((23, 31), 0.4, s), 1)[0] for s in (1, 2)]
    p = M.stack_properties(labs)
    for kw in (dict(min_area=2), dict(max_area=3, clear_border=True), dict(largest=2), dict(largest=0), dict(min_area=2, largest=3)):
        ok = L.select_mask(p["area"], p["y0"], p["y1"], p["x0"], p["x1"], p["n"], (23, 31), **kw)
        table, new_n = L.renumber(ok, p["n"])
        first = 0
        for t, lab in enumerate(labs):
            want, n = M.select(lab, **kw)
            got = np.concatenate(([0], table[first:first + p["n"][t]]))[lab]
            assert n == new_n[t] and np.array_equal(got, want), kw
            first += p["n"][t]


def test_spot_field_model_centroids_are_within_a_tenth_of_a_pixel():
    """The bar of the GPU test, met by the model alone for the committed seed."""
    from barc4dip_amd import synth

    frame, centres = synth.spot_field((256, 256), 64, seed=7, sigma=2.0, amplitude=1000.0)
    assert centres.shape == (64, 2)
    d = np.hypot(*(centres[:, None, :] - centres[None, :, :]).transpose(2, 0, 1))
    assert d[~np.eye(64, dtype=bool)].min() >= 16.0
    lab, n = M.label(M.threshold_mask(frame, 50.0), 2)
    p = M.properties(lab, frame)
    assert n == 64
    for cy, cx in centres:
        e = np.hypot(p["wcy"] - cy, p["wcx"] - cx)
        assert np.sum(e < 0.1) == 1 and np.sum(e < 8.0) == 1


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_come_before_the_device():
    from barc4dip_amd import geometry as G
    from barc4dip_amd import metrics as Q

    img, stack = np.zeros((8, 9), np.float32), np.zeros((3, 8, 9), np.float32)
    m = np.zeros((8, 9), bool)
    bad = [
        lambda: G.label_regions(),                                        # neither
        lambda: G.label_regions(img, 1.0, mask=m),                         # both
        lambda: G.label_regions(mask=m, threshold=1.0),
        lambda: G.label_regions(np.zeros(8), 1.0),                         # shapes
        lambda: G.label_regions(np.zeros((2, 2, 2, 2)), 1.0),
        lambda: G.label_regions(np.zeros((0, 9)), 1.0),                    # an empty side
        lambda: G.label_regions(mask=np.zeros((4, 0), bool)),
        lambda: G.label_regions(img, 1.0, connectivity=3),
        lambda: G.label_regions(img, 1.0, connectivity=0),
        lambda: G.label_regions(mask=m, connectivity=True),
        lambda: G.label_regions(img),                                      # no threshold
        lambda: G.label_regions(img, "high"),
        lambda: G.label_regions(img, float("nan")),
        lambda: G.label_regions(stack, np.zeros(2)),                       # a (T,) threshold of the wrong length
        lambda: G.label_regions(img, np.zeros(3)),
        lambda: G.label_regions(stack, np.zeros((3, 1))),
        lambda: G.label_regions(img, (2.0, 1.0)),                          # low > high
        lambda: G.label_regions(mask=np.zeros((8, 9), np.float32)),        # a mask that is neither bool nor uint8
        lambda: G.largest_region(np.zeros((8, 9), np.int32)),
        lambda: G.largest_region(m, connectivity=4),
        lambda: G.select_regions(np.full((4, 4), -1)),                     # negative labels
        lambda: G.select_regions(np.zeros((4, 4), np.float32)),
        lambda: G.select_regions(np.zeros(4, np.int32)),
        lambda: G.select_regions(np.zeros((4, 4), np.int32), largest=-1),
        lambda: G.select_regions(np.zeros((4, 4), np.int32), largest=1.5),
        lambda: G.select_regions(np.zeros((4, 4), np.int32), min_area="a"),
        lambda: G.select_regions(np.zeros((4, 4), np.int32), clear_border=1),
        lambda: G.select_regions(np.zeros((4, 4), np.int32), keep=np.zeros(3)),
        lambda: G.select_regions(np.zeros((4, 4), np.int32), properties={"area": []}),
        lambda: Q.region_properties(np.full((4, 4), -2)),
        lambda: Q.region_properties(np.zeros((4, 4), np.int32), np.zeros((4, 5))),     # shapes differ
        lambda: Q.region_properties(np.zeros((2, 4, 4), np.int32), np.zeros((4, 4))),
        lambda: Q.region_properties(np.zeros((4, 4), np.int32), background=float("inf")),
        lambda: Q.region_properties(np.zeros((4, 4), np.int32), saturation=float("nan")),
        lambda: Q.find_spots(img, 1.0, connectivity=8),
        lambda: Q.find_spots(img, (3.0, 1.0)),
        lambda: Q.find_spots(np.zeros((0, 4)), 1.0),
        lambda: Q.find_spots(img, 1.0, background="b"),
        lambda: Q.find_spots(img, 1.0, min_area="one"),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} raised nothing")
    for f in (lambda: G.label_regions(np.zeros((4, 4), np.complex64), 1.0), lambda: Q.find_spots(np.zeros((4, 4), complex), 1.0),
              lambda: Q.region_properties(np.zeros((4, 4), np.int32), np.zeros((4, 4), complex))):
        with pytest.raises(NotImplementedError):
            f()


def test_no_host_fallback():
    import torch

    from barc4dip_amd import _ffi
    from barc4dip_amd import geometry as G
    from barc4dip_amd import metrics as Q

    img = np.ones((8, 9), np.float32)
    if torch.cuda.is_available():
        return
    for f in (lambda: G.label_regions(img, 0.5), lambda: G.label_regions(mask=img > 0), lambda: G.largest_region(img > 0),
              lambda: G.select_regions(np.ones((8, 9), np.int32), min_area=1), lambda: Q.region_properties(np.ones((8, 9), np.int32), img),
              lambda: Q.find_spots(img, 0.5)):
        with pytest.raises(_ffi.B4DUnavailable):
            f()


def test_constants_of_the_package_equal_the_header():
    from barc4dip_amd.geometry import labels as L

    txt = open(os.path.join(ROOT, "barc4dip_amd", "csrc", "b4d_label.hpp")).read()
    assert f"LB_TY = {L.TILE[0]}, LB_TX = {L.TILE[1]}" in txt and f"LB_SCAN = {L.SCAN_BLOCK};" in txt
    assert f"RP_WAVE_AREA = {L.WAVE_AREA}, RP_NQ = {len(L.COLUMNS)}" in txt and L.COLUMNS == M.COLUMNS
    assert f"#define B4D_ELOOP ({L.ELOOP})" in open(os.path.join(ROOT, "include", "b4d.h")).read()


# ------------------------------------------------------------------------------------------------------------ the union-find core
PROGRAM = r"""
// Reads "cases" then per case "ny nx conn ty tx scan" and ny * nx digits; prints per case the region count and the labels.
#include <cstdio>
#include <vector>

#include "b4d_label.hpp"
using namespace b4d;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int cases = 0;
    if (std::fscanf(f, "%d", &cases) != 1) return 2;
    for (int k = 0; k < cases; ++k) {
        int ny, nx, conn, ty, tx, scan;
        if (std::fscanf(f, "%d %d %d %d %d %d", &ny, &nx, &conn, &ty, &tx, &scan) != 6) return 2;
        std::vector<uint8_t> fg((size_t)ny * nx);
        for (auto& v : fg) {
            int c;
            do c = std::fgetc(f);
            while (c == ' ' || c == '\n');
            if (c != '0' && c != '1') return 2;
            v = (uint8_t)(c - '0');
        }
        std::vector<int> labels((size_t)ny * nx), links((size_t)ty * tx);
        const int n = label_frame_serial(fg.data(), ny, nx, conn, ty, tx, scan, labels.data(), links.data());
        std::printf("%d", n);
        for (int v : labels) std::printf(" %d", v);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
"""

HOST_TILE = (4, 8)


def host_cases():
    ty, tx = HOST_TILE
    masks = []
    for shape in ((1, 1), (1, tx + 3), (ty + 3, 1), (2 * ty + 1, 2 * tx + 1), (13, 29)):
        masks += [M.random_mask(shape, d, 100 + k) for k, d in enumerate(M.DENSITIES)]
        masks += [np.zeros(shape, bool), np.ones(shape, bool), M.checkerboard(shape)]
    masks += list(M.corner_pairs(HOST_TILE))
    big = (3 * ty, 3 * tx)
    masks += [M.serpentine(big), M.spiral(big), M.comb(big), M.serpentine((3 * ty + 1, 3 * tx + 2)), M.spiral((3 * ty + 2, 3 * tx + 1))]
    return [(m, conn) for m in masks for conn in (1, 2)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("label_core")
    src, exe = d / "label.cpp", d / "label"
    src.write_text(PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the core
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe), d


def test_serial_union_find_on_the_seam_cases_equals_scipy(program):
    exe, d = program
    cases = host_cases()
    ty, tx = HOST_TILE
    lines = [str(len(cases))]
    for m, conn in cases:
        lines.append(f"{m.shape[0]} {m.shape[1]} {conn} {ty} {tx} 16")
        lines.append("".join("1" if v else "0" for v in m.ravel()))
    path = d / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    for k, ((m, conn), line) in enumerate(zip(cases, out)):
        v = np.array(line.split(), dtype=np.int64)
        want, n = M.label(m, conn)
        assert v[0] == n and np.array_equal(v[1:].reshape(m.shape), want), (k, m.shape, conn)


def test_generated_shapes_are_what_they_claim():
    big = (3 * HOST_TILE[0], 3 * HOST_TILE[1])
    for m in (M.serpentine(big), M.spiral(big), M.comb(big)):
        assert M.label(m, 1)[1] == 1 and m.sum() >= m.size // 2 - m.shape[1]
    a, b = M.corner_pairs(HOST_TILE)
    assert [M.label(a, 1)[1], M.label(a, 2)[1], M.label(b, 1)[1], M.label(b, 2)[1]] == [2, 1, 2, 1]
    c = M.checkerboard((5, 7))
    assert M.label(c, 1)[1] == 18 and M.label(c, 2)[1] == 1
