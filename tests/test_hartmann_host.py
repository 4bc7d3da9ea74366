"""CPU tier of the Hartmann analysis (barc4dip_amd.signal.hartmann): the cell geometry, the float64 model of the kernel
(tests/hartmann_model.py) against scipy.ndimage.center_of_mass, against analytic spots and against its own summation order, and
the argument checks, which all come before any device call.  No GPU and no library is needed here."""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hartmann_model as M  # noqa: E402

from barc4dip_amd import synth  # noqa: E402
from barc4dip_amd.signal import hartmann as H  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ geometry
def test_cells_of_the_ragged_lattice():
    """floor(o + i p + 0.5) for pitch (13.37, 17.5) from (3.2, 5.7) on 147 x 203: sides 13 / 14 and 17 / 18, cells starting at every
    alignment.  Every whole cell inside the frame is kept, which gives 10 x 11 cells; the `ragged` case takes the first 9 x 10 of
    them, ending at row 124 and column 181, and leaves the rest of the frame unread."""
    c = H.hartmann_cells((147, 203), (13.37, 17.5), (3.2, 5.7))
    assert c["y_edges"].dtype == np.int32 and c["x_edges"].dtype == np.int32
    assert c["y_edges"].tolist() == [3, 17, 30, 43, 57, 70, 83, 97, 110, 124, 137]
    assert c["x_edges"].tolist() == [6, 23, 41, 58, 76, 93, 111, 128, 146, 163, 181, 198]
    assert c["shape"] == (10, 11) and c["pitch"] == (13.37, 17.5) and c["origin"] == (3.2, 5.7)
    assert set(np.diff(c["y_edges"]).tolist()) == {13, 14} and set(np.diff(c["x_edges"]).tolist()) == {17, 18}
    assert set((c["x_edges"][:-1] % 4).tolist()) == {0, 1, 2, 3}
    np.testing.assert_allclose(c["y"], 3.2 + (np.arange(10) + 0.5) * 13.37 - 0.5, rtol=0, atol=1e-12)
    np.testing.assert_allclose(c["x"], 5.7 + (np.arange(11) + 0.5) * 17.5 - 0.5, rtol=0, atol=1e-12)
    # the next edge on either axis would leave the frame
    assert math.floor(3.2 + 11 * 13.37 + 0.5) > 147 and math.floor(5.7 + 12 * 17.5 + 0.5) > 203
    r = M.case_data()["ragged"][1]
    assert r["shape"] == (9, 10) and r["y_edges"][-1] == 124 and r["x_edges"][-1] == 181
    assert r["y_edges"].tolist() == c["y_edges"][:10].tolist() and r["x_edges"].tolist() == c["x_edges"][:11].tolist()


def test_cells_of_the_other_cases():
    d = M.case_data()
    assert d["aligned"][1]["shape"] == (4, 8) and d["aligned"][1]["x_edges"].tolist() == list(range(0, 257, 32))
    big = d["largest"][1]
    assert big["shape"] == (1, 2) and big["y_edges"].tolist() == [1, 129] and big["x_edges"].tolist() == [2, 130, 258]
    small = d["smallest"][1]
    assert small["shape"] == (4, 5) and set(np.diff(small["y_edges"]).tolist()) == {2} and set(np.diff(small["x_edges"]).tolist()) == {2}
    assert d["many"][1]["shape"] == (1, 1025)
    assert d["edge"][1]["shape"] == (4, 5)
    for name, (frames, cells) in d.items():
        assert frames.dtype == np.float32 and frames.shape[-2] >= cells["y_edges"][-1] and frames.shape[-1] >= cells["x_edges"][-1]
        finite = frames[np.isfinite(frames)]
        assert np.array_equal(finite, np.round(finite)), name       # whole-number counts: see the model's note on thresholds


def test_cells_negative_origin_and_a_regular_axis():
    from barc4dip_amd.preprocessing.distortion import _regular_axis

    c = H.hartmann_cells((100, 90), (10.5, 9.25), (-3.0, 20.0))
    assert c["y_edges"][0] == 8 and c["y_edges"][-1] <= 100 and c["x_edges"][0] == 2 and c["x_edges"][-1] <= 90
    assert c["y"][0] == pytest.approx(-3.0 + 1.5 * 10.5 - 0.5) and c["x"][0] == pytest.approx(20.0 - 1.5 * 9.25 - 0.5)
    for cells in [c] + [v[1] for v in M.case_data().values()]:
        gy, gx = cells["shape"]
        first, step = _regular_axis(cells["y"], gy, "y")
        assert first == cells["y"][0] and (gy == 1 or step == pytest.approx(cells["pitch"][0]))
        first, step = _regular_axis(cells["x"], gx, "x")
        assert first == cells["x"][0] and (gx == 1 or step == pytest.approx(cells["pitch"][1]))
        # every nominal position is the centre of its cell to within the rounding of the edges
        assert np.all(np.abs(cells["y"] - 0.5 * (cells["y_edges"][:-1] + cells["y_edges"][1:] - 1)) <= 0.5 + 1e-9)


def test_cells_errors():
    for bad in (0, -3.0, (8, 0), np.nan, (8, np.inf)):
        with pytest.raises(ValueError):
            H.hartmann_cells((64, 64), bad)
    for bad in ("8", (8, 8, 8), True, None):
        with pytest.raises(ValueError):
            H.hartmann_cells((64, 64), bad)
    with pytest.raises(ValueError):
        H.hartmann_cells((64, 64), 8, (0, "a"))
    with pytest.raises(ValueError, match="no whole cell"):
        H.hartmann_cells((20, 64), 24)
    with pytest.raises(ValueError, match="no whole cell"):
        H.hartmann_cells((30, 64), 24, (10.0, 0.0))
    with pytest.raises(NotImplementedError):
        H.hartmann_cells((600, 600), 129)
    with pytest.raises(NotImplementedError):
        H.hartmann_cells((64, 64), 1.4)
    assert H.hartmann_cells((600, 600), 128)["shape"] == (4, 4)
    assert H.hartmann_cells((64, 64), 2)["shape"] == (32, 32)


# ------------------------------------------------------------------------------------------------------------------ the model
def test_model_against_scipy_center_of_mass():
    """Non-negative frames, background none, threshold 0: the weight is the pixel, so the model's centre of gravity is
    center_of_mass over the cell's label.  1e-10 px: two float64 summations of at most 16 384 non-negative terms."""
    ndi = pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for name in ("ragged", "aligned", "largest", "smallest", "many"):
        frames, cells = M.case_data()[name]
        frame = frames.reshape((-1,) + frames.shape[-2:])[0].astype(np.float64)
        assert frame.min() >= 0.0
        gy, gx = cells["shape"]
        labels = np.zeros(frame.shape, dtype=np.int32)
        for i in range(gy):
            for j in range(gx):
                labels[cells["y_edges"][i]:cells["y_edges"][i + 1], cells["x_edges"][j]:cells["x_edges"][j + 1]] = 1 + i * gx + j
        com = np.array(ndi.center_of_mass(frame, labels, np.arange(1, gy * gx + 1))).reshape(gy, gx, 2)
        m = M.spot_model(frame, cells["y_edges"], cells["x_edges"], background="none", threshold=0.0, pitch=cells["pitch"])
        worst = max(worst, np.abs(m["cy"] - com[..., 0]).max(), np.abs(m["cx"] - com[..., 1]).max())
        assert np.array_equal(m["flux"], np.array(ndi.sum_labels(frame, labels, np.arange(1, gy * gx + 1))).reshape(gy, gx))
    assert worst <= 1e-10, worst


def test_model_against_analytic_spots():
    """Noiseless sigma = 2 spots at pitch 24, 5 x 5 cells, shifts uniform in +-3 px, background none, threshold 0.  The cell cuts
    the spot's tail: the mass of a sigma = 2 Gaussian beyond 9 px is erfc(9 / (2 sqrt 2)) = 7e-6, times the half cell about
    1e-4 px; the bound is ten times that.  The iteratively weighted form (sigma_w = 3, 12 rounds) is far inside it."""
    rng = np.random.default_rng(5)
    d = rng.uniform(-3.0, 3.0, (2, 5, 5))
    frame = synth.hartmann_frame((120, 120), 24, (0, 0), (d[0], d[1]), sigma=2.0)
    c = H.hartmann_cells((120, 120), 24)
    m = M.spot_model(frame, c["y_edges"], c["x_edges"], background="none", threshold=0.0, sigma=3.0, iterations=12,
                     check_margin=False)
    ty, tx = c["y"][:, None] + d[0], c["x"][None, :] + d[1]
    cog = max(np.abs(m["cy"] - ty).max(), np.abs(m["cx"] - tx).max())
    iw = max(np.abs(m["cy_iw"] - ty).max(), np.abs(m["cx_iw"] - tx).max())
    print(f"cog {cog:.2e} px, iwcog {iw:.2e} px")
    assert cog <= 1e-3 and iw <= 1e-3, (cog, iw)
    assert iw < cog
    # second moments of a whole Gaussian: sigma^2, less what the pixel grid and the cut tails take: 1 %
    assert np.abs(m["var_y"] - 4.0).max() <= 0.04 and np.abs(m["var_x"] - 4.0).max() <= 0.04 and np.abs(m["cov_yx"]).max() <= 0.04


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_model_does_not_depend_on_the_summation_order(name):
    """Forward, reversed and exactly rounded sums: the centroids of every case agree within 1e-10 px (sums about the cell centre
    of at most 16 384 non-negative terms: n 2^-53 relative, times a lever of at most 128 px)."""
    worst = 0.0
    for background, threshold in (("border", 0.2), ("none", 0.0), ("min", 0.2)):
        ref = M.case_model(name, background, threshold)
        for order in ("forward", "reverse"):
            m = M.case_model(name, background, threshold, order)
            for k in ("cy", "cx", "cy_iw", "cx_iw"):
                assert np.array_equal(np.isnan(m[k]), np.isnan(ref[k]))
                ok = ~np.isnan(ref[k])
                if ok.any():
                    worst = max(worst, np.abs(m[k][ok] - ref[k][ok]).max())
            for k in M.COUNTS + ("peak", "peak_y", "peak_x"):
                assert np.array_equal(m[k], ref[k], equal_nan=True)
    print(f"{name}: {worst:.2e} px")
    assert worst <= 1e-10, worst


def test_model_on_the_edge_frame():
    """What each special cell of the edge frame is there for."""
    frames, cells = M.case_data()["edge"]
    m = M.case_model("edge", "border", 0.2)
    at = M.EDGE_CELLS
    for name in ("constant", "all_nan"):
        i, j = at[name]
        assert m["flux"][i, j] == 0 and m["n_pixels"][i, j] == 0
        assert all(np.isnan(m[k][i, j]) for k in ("cy", "cx", "var_y", "var_x", "cov_yx", "cy_iw", "cx_iw"))
    i, j = at["constant"]
    assert m["peak"][i, j] == 7.0 and (m["peak_y"][i, j], m["peak_x"][i, j]) == (0.0, 0.0) and m["noise"][i, j] == 0.0
    i, j = at["all_nan"]
    assert m["n_nan"][i, j] == 576 and np.isnan(m["peak"][i, j]) and np.isnan(m["peak_y"][i, j]) and np.isnan(m["background"][i, j])
    i, j = at["nan_flank"]
    assert m["n_nan"][i, j] == 20 and m["flux"][i, j] > 0
    i, j = at["saturated"]
    assert m["n_saturated"][i, j] == 3 and m["n_saturated"].sum() == 3 and m["peak"][i, j] == M.SATURATION
    assert (m["peak_y"][i, j], m["peak_x"][i, j]) == (11.0, 24.0 * j + 11.0)
    i, j = at["negative"]
    assert m["peak"][i, j] < 0 and m["flux"][i, j] > 0
    assert M.case_model("edge", "none", 0.0)["flux"][i, j] == 0 and M.case_model("edge", "min", 0.0)["flux"][i, j] > 0
    i, j = at["corner"]
    assert (m["peak_y"][i, j], m["peak_x"][i, j]) == (24.0 * i + 23.0, 24.0 * j + 23.0)
    i, j = at["two_maxima"]
    assert (m["peak_y"][i, j], m["peak_x"][i, j]) == (24.0 * i + 9.0, 24.0 * j + 15.0)


def test_every_case_keeps_its_pixels_off_the_threshold():
    """The margin assertion of the model, over every case and option set (it raises inside spot_cell)."""
    for name in M.CASES:
        for background in M.BACKGROUNDS:
            for threshold in M.THRESHOLDS:
                M.case_model(name, background, threshold)
    with pytest.raises(AssertionError, match="threshold"):
        M.spot_cell(np.array([[0, 0, 0], [0, 10, 2.000001], [0, 0, 0]], np.float32), 0, 0, background="none", threshold=0.2, sigma=1.0,
                    iterations=0, saturation=np.inf)


# ------------------------------------------------------------------------------------------------------------------ synth
def test_hartmann_frame():
    f = synth.hartmann_frame((48, 72), 24, (0, 0), sigma=2.0, amplitude=100.0, background=3.0)
    assert f.shape == (48, 72) and f.dtype == np.float64 and f.min() >= 3.0
    # spots at (11.5, 11.5) + 24 k: the four pixels round each share the maximum
    assert f[11, 11] == pytest.approx(3.0 + 100.0 * math.exp(-0.5 * 0.5 / 4.0)) and f[11, 11] == pytest.approx(f[12, 36]) == pytest.approx(f[35, 60])
    g = synth.hartmann_frame((48, 72), 24, (0, 0), lambda y, x: (0.5 + 0 * y, -0.5 + 0 * x), sigma=2.0, amplitude=100.0)
    assert g[12, 11] == pytest.approx(100.0) and g[36, 59] == pytest.approx(100.0)
    a = synth.hartmann_frame((48, 72), 24, sigma=2.0, seed=3)
    assert np.array_equal(a, synth.hartmann_frame((48, 72), 24, sigma=2.0, seed=3)) and np.array_equal(a, np.round(a))
    assert not np.array_equal(a, synth.hartmann_frame((48, 72), 24, sigma=2.0, seed=4))


# ------------------------------------------------------------------------------------------------------------------ arguments
FRAME = np.zeros((96, 120), np.float32)
CELLS = H.hartmann_cells((96, 120), 24)

BAD_SPOT_OPTIONS = [
    {"background": "median"}, {"background": np.nan}, {"background": True}, {"background": None},
    {"threshold": 1.0}, {"threshold": -0.1}, {"threshold": np.nan}, {"threshold": "0.1"},
    {"method": "gauss"}, {"method": 1},
    {"sigma": 0.0}, {"sigma": -1.0}, {"sigma": np.inf}, {"sigma": "3"},
    {"iterations": -1}, {"iterations": 2.5}, {"iterations": True},
    {"saturation": np.nan}, {"saturation": "4095"},
]


@pytest.mark.parametrize("kw", BAD_SPOT_OPTIONS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_spot_options_are_checked_on_the_host(kw):
    with pytest.raises(ValueError):
        H.spot_centroids(FRAME, CELLS, **kw)
    with pytest.raises(ValueError):
        H.hartmann_lattice(FRAME, pitch=24, **kw)
    with pytest.raises(ValueError):
        H.hartmann_displacement(FRAME, FRAME, cells=CELLS, **kw)
    with pytest.raises(ValueError):
        H.hartmann_displacement(FRAME, FRAME, pitch=24, **kw)


def test_spot_centroids_arguments():
    for bad in (np.zeros(5), np.zeros((2, 2, 96, 120)), np.zeros((0, 96, 120))):
        with pytest.raises(ValueError):
            H.spot_centroids(bad, CELLS)
    with pytest.raises(ValueError, match="hartmann_cells dict"):
        H.spot_centroids(FRAME, {"y_edges": CELLS["y_edges"]})
    with pytest.raises(ValueError, match="hartmann_cells dict"):
        H.spot_centroids(FRAME, None)
    with pytest.raises(ValueError, match="leaves the frame"):
        H.spot_centroids(FRAME[:90], CELLS)
    with pytest.raises(ValueError, match="ascend"):
        H.spot_centroids(FRAME, {**CELLS, "y_edges": CELLS["y_edges"][::-1].copy()})
    with pytest.raises(ValueError, match="integer"):
        H.spot_centroids(FRAME, {**CELLS, "x_edges": CELLS["x_edges"].astype(np.float64)})
    with pytest.raises(NotImplementedError):
        H.spot_centroids(np.zeros((300, 120), np.float32), {**CELLS, "y_edges": np.array([0, 24, 48, 72, 201], np.int32)})
    with pytest.raises(NotImplementedError):
        H.spot_centroids(FRAME, {**CELLS, "y_edges": np.array([0, 24, 48, 72, 73], np.int32)})
    with pytest.raises(ValueError, match="one nominal position"):
        H.spot_centroids(FRAME, {**CELLS, "y": CELLS["y"][:-1]})


def test_lattice_and_displacement_arguments():
    for bad in (np.zeros((2, 96, 120)), np.zeros(7), np.zeros((0, 5))):
        with pytest.raises(ValueError):
            H.hartmann_lattice(bad, pitch=24)
    for bad in (0, -1, (24, 0), "24"):
        with pytest.raises(ValueError):
            H.hartmann_lattice(FRAME, pitch=bad)
    with pytest.raises(NotImplementedError):
        H.hartmann_lattice(np.zeros((300, 300), np.float32), pitch=150)
    for bad in (0, -0.1, None, True):
        with pytest.raises(ValueError):
            H.hartmann_lattice(FRAME, pitch=24, rotation_limit=bad)
    with pytest.raises(ValueError, match="return_tensors"):
        H.hartmann_lattice(FRAME, pitch=24, return_tensors=True)
    with pytest.raises(ValueError, match="needs cells"):
        H.hartmann_displacement(None, FRAME)
    with pytest.raises(ValueError, match="differ in shape"):
        H.hartmann_displacement(FRAME[:, :100], FRAME, cells=CELLS)
    with pytest.raises(ValueError, match="same T"):
        H.hartmann_displacement(np.zeros((3, 96, 120)), FRAME, cells=CELLS)
    with pytest.raises(ValueError, match="same T"):
        H.hartmann_displacement(np.zeros((3, 96, 120)), np.zeros((2, 96, 120)), cells=CELLS)
    with pytest.raises(ValueError):
        H.hartmann_displacement(FRAME, np.zeros(4), cells=CELLS)
    for bad in (np.nan, "3", None):
        with pytest.raises(ValueError, match="min_snr"):
            H.hartmann_displacement(FRAME, FRAME, cells=CELLS, min_snr=bad)
    with pytest.raises(ValueError, match="leaves the frame"):
        H.hartmann_displacement(None, FRAME[:90], cells=CELLS)


def test_exports():
    import barc4dip_amd.signal as S

    for name in ("hartmann_cells", "spot_centroids", "hartmann_lattice", "hartmann_displacement"):
        assert getattr(S, name) is getattr(H, name) and name in S.__all__
    assert H.QUANTITIES == M.QUANTITIES


# ------------------------------------------------------------------------------------------------------------------ lattice, host part
def _model_centroids(images, cells, *, background="border", threshold=0.1, method="cog", sigma=None, iterations=8, saturation=None):
    m = M.spot_model(images, cells["y_edges"], cells["x_edges"], background=background, threshold=threshold, sigma=sigma,
                     iterations=iterations, saturation=saturation, pitch=cells["pitch"], check_margin=False)
    if method == "iwcog":
        m["cy"], m["cx"] = m["cy_iw"], m["cx_iw"]
    return m


def _numpy_pitch(reference):
    a = np.asarray(reference, dtype=np.float64)
    ac = np.fft.fftshift(np.fft.ifft2(np.abs(np.fft.fft2(a - a.mean())) ** 2).real).astype(np.float32)
    ny, nx = ac.shape
    return H._first_peak(ac[ny // 2:, nx // 2] / ac.max()), H._first_peak(ac[ny // 2, nx // 2:] / ac.max())


@pytest.mark.parametrize("pitch,origin,seed", [((24.0, 24.0), (3.3, 1.7), None), ((23.3, 25.1), (23.1, 0.2), 1), ((17.5, 31.0), (11.0, 12.4), 2)])
def test_lattice_fit_on_model_centroids(monkeypatch, pitch, origin, seed):
    """Everything of hartmann_lattice behind its two device calls, with the model in the place of the kernel and a NumPy
    autocorrelation in the place of autocorr2d: the pitch estimate lands within a pixel, the fit within 1e-3 px on noiseless
    spots (background none, threshold 0: see the analytic test above) and 2e-2 px under Poisson noise with the default options,
    and the origin comes back in [-0.5, pitch - 0.5)."""
    monkeypatch.setattr(H, "spot_centroids", _model_centroids)
    monkeypatch.setattr(H, "_estimate_pitch", _numpy_pitch)
    ref = synth.hartmann_frame((246, 292), pitch, origin, sigma=2.0, seed=seed)
    est = _numpy_pitch(ref)
    assert abs(est[0] - pitch[0]) < 1.0 and abs(est[1] - pitch[1]) < 1.0, est
    lat = H.hartmann_lattice(ref, **(dict(background="none", threshold=0.0) if seed is None else {}))
    bar = 1e-3 if seed is None else 2e-2
    want = [np.mod(o + 0.5, p) - 0.5 for o, p in zip(origin, pitch)]
    assert max(abs(lat["pitch"][k] - pitch[k]) for k in (0, 1)) <= bar, lat["pitch"]
    assert max(abs(lat["origin"][k] - want[k]) for k in (0, 1)) <= bar, (lat["origin"], want)
    assert abs(lat["rotation"]) < 1e-3 and all(-0.5 <= lat["origin"][k] < pitch[k] - 0.5 for k in (0, 1))
    assert lat["shape"] == H.hartmann_cells((246, 292), pitch, origin)["shape"]


def test_lattice_rotation(monkeypatch):
    """A lattice turned by 4 mrad: reported within 5 %, refused where it carries a spot over more than the limit."""
    monkeypatch.setattr(H, "spot_centroids", _model_centroids)
    c = H.hartmann_cells((246, 292), 24.0, (3.3, 1.7))
    th = 4e-3
    yc, xc = c["y"].mean(), c["x"].mean()
    turn = lambda y, x: (th * (x - xc) + 0 * y, -th * (y - yc) + 0 * x)  # noqa: E731
    ref = synth.hartmann_frame((246, 292), 24.0, (3.3, 1.7), turn, sigma=2.0)
    lat = H.hartmann_lattice(ref, pitch=24.0, rotation_limit=0.25, background="none", threshold=0.0)
    assert lat["rotation"] == pytest.approx(th, rel=0.05) and abs(lat["pitch"][0] - 24.0) < 1e-2
    with pytest.raises(ValueError, match="rotated"):
        H.hartmann_lattice(ref, pitch=24.0, rotation_limit=0.04, background="none", threshold=0.0)
