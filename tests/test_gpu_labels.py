"""Connected-component labelling, region measurements and selection on the device against tests/labels_model.py
(scipy.ndimage.label for the labels, plain float64 NumPy for the columns).  Labels and counts are compared exactly; the bounds of
the float columns are those of two float64 summation orders and are computed per region (labels_model.compare_properties), the
worst ratios are recorded through the `observe` fixture.  The shapes sit on the seams of the kernel's own tile (labels.TILE)."""
import numpy as np
import pytest

import labels_model as M
from barc4dip_amd import geometry as G
from barc4dip_amd import metrics as Q
from barc4dip_amd import synth
from barc4dip_amd.geometry import labels as L

pytestmark = pytest.mark.gpu

TY, TX = L.TILE
SHAPES = M.shapes(L.TILE)
BIG = (3 * TY, 3 * TX)


def check_labels(mask, conn):
    lab, n = G.label_regions(mask=mask, connectivity=conn)
    want, m = M.label(mask, conn)
    assert isinstance(n, int) and n == m and lab.dtype == np.int32 and np.array_equal(lab, want)
    return lab, n


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


# 1
@pytest.mark.parametrize("conn", (1, 2))
@pytest.mark.parametrize("density", M.DENSITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_masks_equal_scipy(shape, density, conn):
    check_labels(M.random_mask(shape, density, 17), conn)


# 2, 3
@pytest.mark.parametrize("shape", SHAPES)
def test_empty_full_and_checkerboard(shape):
    for conn in (1, 2):
        assert check_labels(np.zeros(shape, bool), conn)[1] == 0
        assert check_labels(np.ones(shape, bool), conn)[1] == 1
    c = M.checkerboard(shape)
    most = (shape[0] * shape[1] + 1) // 2
    assert check_labels(c, 1)[1] == most                      # the largest possible count, a scan across blocks
    assert check_labels(c, 2)[1] == (1 if min(shape) > 1 else most)     # a single row or column has no diagonal contact


# 4
def test_tile_corner_diagonals():
    for m in M.corner_pairs(L.TILE):
        assert check_labels(m, 1)[1] == 2 and check_labels(m, 2)[1] == 1


# 5, 6
@pytest.mark.parametrize("shape", (BIG, (BIG[0] + 1, BIG[1] + 2)))
def test_long_chains_and_the_late_merge(shape):
    for make in (M.serpentine, M.spiral):
        for conn in (1, 2):
            assert check_labels(make(shape), conn)[1] == 1
    for conn in (1, 2):
        lab, n = check_labels(M.comb(shape), conn)
        assert n == 1 and set(np.unique(lab)) == {0, 1}      # numbered by the first pixel of the merged set


# 7
def test_thresholding_rules():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 4, (TY + 5, TX + 9)).astype(np.float32)
    img[2, 3], img[2, 4], img[7, 7] = np.nan, np.inf, 2.0
    for conn in (1, 2):
        lab, n = G.label_regions(img, 2.0, connectivity=conn)
        want, m = M.label(M.threshold_mask(img, 2.0), conn)
        assert n == m and np.array_equal(lab, want)
        assert lab[2, 3] == 0 and lab[2, 4] > 0 and lab[7, 7] == 0           # NaN, +inf, v == threshold
        for mask in (img > 2.0, (img > 2.0).astype(np.uint8) * 7):
            assert np.array_equal(G.label_regions(mask=mask, connectivity=conn)[0], want)
    stack = np.stack([img, img, img])
    thr = np.array([0.0, 1.0, 2.0])
    lab, n = G.label_regions(stack, thr, connectivity=1)
    assert n.dtype == np.int64 and n.shape == (3,)
    for t in range(3):
        want, m = M.label(M.threshold_mask(img, thr[t]), 1)
        assert n[t] == m and np.array_equal(lab[t], want)
    lab_t, n_t = G.label_regions(stack, 1.0, return_tensors=True)
    assert lab_t.is_cuda and np.array_equal(lab_t.cpu().numpy()[1], lab[1])


# 8
def test_batch_equals_single_frames_and_repeats_bit_for_bit():
    shape = (2 * TY + 1, 2 * TX + 1)
    frames = np.stack([M.sprinkle(M.smooth_frame(shape, s, signed=s == 2), 40 + s) for s in (1, 2, 3)])
    thr = np.array([190.0, 20.0, 230.0], np.float32)
    lab, n = G.label_regions(frames, thr, connectivity=2)
    tab = Q.region_properties(lab, frames, background=5.0, saturation=4095.0)
    again = Q.region_properties(G.label_regions(frames, thr, connectivity=2)[0], frames, background=5.0, saturation=4095.0)
    first = 0
    for t in range(3):
        lab1, n1 = G.label_regions(frames[t], float(thr[t]), connectivity=2)
        assert n1 == n[t] and np.array_equal(lab1, lab[t])
        one = Q.region_properties(lab1, frames[t], background=5.0, saturation=4095.0)
        for k in L.COLUMNS:
            assert np.array_equal(bits(one[k]), bits(tab[k][first:first + n1])), (t, k)
        first += n1
    for k in L.COLUMNS + ("frame", "label", "n"):
        assert np.array_equal(bits(again[k]), bits(tab[k])), k
    assert np.array_equal(tab["n"], n) and tab["frame"].size == n.sum() and n.min() > 0


# 9
@pytest.mark.parametrize("conn", (1, 2))
@pytest.mark.parametrize("density", M.DENSITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_properties_equal_the_model(shape, density, conn, observe):
    lab, n = M.label(M.random_mask(shape, density, 17), conn)
    smooth = M.smooth_frame(shape, 5)
    for tag, img, kw in (("positive", smooth, {}), ("signed", M.smooth_frame(shape, 6, signed=True), {"background": -50.0}),
                         ("nan_saturated", M.sprinkle(smooth, 7), {"saturation": 4095.0, "background": 100.0})):
        got = Q.region_properties(lab, img, **kw)
        assert got["n"].tolist() == [n] and got["label"].tolist() == list(range(1, n + 1))
        assert all(got[k].dtype == (np.int64 if k in L.INTEGER_COLUMNS else np.float64) for k in L.COLUMNS)
        M.compare_properties(got, M.properties(lab, img, n=n, **kw), observe, (tag, shape, density, conn))
    geo = Q.region_properties(lab)
    M.compare_properties(geo, M.properties(lab, n=n), None, ("geometry", shape, density, conn))


# 10
def test_select_regions_hysteresis_and_largest_region():
    lab = np.zeros((TY + 8, TX + 10), np.int32)
    lab[0, 0:2] = 1
    lab[2:4, 2:4] = 2
    lab[TY - 1:TY + 1, TX - 1:TX + 1] = 3      # area 4 like region 2, across a tile corner
    lab[5:7, 10:13] = 4
    lab[TY + 6, 8] = 5
    for kw in (dict(min_area=2), dict(max_area=4), dict(clear_border=True), dict(largest=2), dict(largest=3, min_area=2),
               dict(keep=np.array([True, False, True, False, True]))):
        got, n = G.select_regions(lab, **kw)
        want, m = M.select(lab, **kw)
        assert n == m and np.array_equal(got, want), kw
    got, n = G.select_regions(lab, largest=2)
    assert n == 2 and got[2, 2] == 1 and got[5, 10] == 2 and got[TY, TX] == 0      # the tie goes to the lower label
    props = Q.region_properties(lab)
    assert np.array_equal(G.select_regions(lab, min_area=3, properties=props)[0], M.select(lab, min_area=3)[0])
    stack = np.stack([lab, (lab > 2) * lab])
    got, n = G.select_regions(stack, min_area=4)
    assert n.tolist() == [3, 2] and np.array_equal(got[1], M.select(stack[1], min_area=4)[0])

    img = M.smooth_frame((2 * TY + 1, 2 * TX + 1), 9, signed=True)
    for conn in (1, 2):
        got, n = G.label_regions(img, (60.0, 150.0), connectivity=conn)
        want, m = M.hysteresis(img, 60.0, 150.0, conn)
        assert n == m and m > 0 and np.array_equal(got, want) and M.label(M.threshold_mask(img, 60.0), conn)[1] > m

    mask = M.random_mask((2 * TY + 1, 2 * TX + 1), 0.55, 4)
    for conn in (1, 2):
        lab1, _ = M.label(mask, conn)
        area = np.bincount(lab1.ravel())[1:]
        big = G.largest_region(mask, conn)
        assert big.dtype == bool and np.array_equal(big, lab1 == 1 + int(np.argmax(area)))
    assert not G.largest_region(np.zeros((4, 5), bool)).any()


def test_find_spots_on_a_spot_field():
    frame, centres = synth.spot_field((256, 256), 64, seed=7, sigma=2.0, amplitude=1000.0)
    spots, lab = Q.find_spots(frame, 50.0, return_labels=True)
    assert spots["n"].tolist() == [64] and lab.max() == 64
    for cy, cx in centres:                      # every spot once, within a tenth of a pixel
        e = np.hypot(spots["wcy"] - cy, spots["wcx"] - cx)
        assert np.sum(e < 0.1) == 1 and np.sum(e < 8.0) == 1
    want = M.properties(M.label(M.threshold_mask(frame, 50.0), 2)[0], frame)
    M.compare_properties(spots, want, None, "spots")
    few = Q.find_spots(frame, (50.0, 2000.0))
    assert few["n"].tolist() == [0] and few["area"].size == 0
    cut = Q.find_spots(frame, 50.0, min_area=int(np.median(want["area"])) + 1)
    assert cut["n"][0] == np.sum(want["area"] > np.median(want["area"]))


# 11
def test_external_label_maps(observe):
    y, x = np.indices(BIG)
    img = M.sprinkle(M.smooth_frame(BIG, 12, signed=True), 13)
    scattered = ((y // 5 + x // 7) % 4 + 1).astype(np.int32)            # four regions, none connected
    gaps = np.where(scattered == 2, 0, scattered * 2).astype(np.int64)   # labels 2, 6, 8 of 1 .. 8
    whole = np.ones(BIG, np.int32)                                       # one box above the wave's area: the workgroup path
    far = np.zeros(BIG, np.int32)
    far[0, 1], far[BIG[0] - 1, BIG[1] - 2] = 1, 1                        # two pixels, a frame-sized box
    assert BIG[0] * BIG[1] > L.WAVE_AREA
    for tag, lab in (("scattered", scattered), ("gaps", gaps), ("whole", whole), ("far", far)):
        got = Q.region_properties(lab, img, background=-20.0, saturation=4095.0)
        M.compare_properties(got, M.properties(lab, img, background=-20.0, saturation=4095.0), observe, tag)
    assert Q.region_properties(gaps)["area"][[0, 2, 3]].tolist() == [0, 0, 0]
    empty = Q.region_properties(np.zeros((5, 6), np.int32), np.ones((5, 6)))
    assert empty["n"].tolist() == [0] and all(empty[k].size == 0 for k in L.COLUMNS)
