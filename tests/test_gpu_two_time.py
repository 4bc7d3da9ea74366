"""GPU tier of the two-time correlation (barc4dip_amd.metrics.two_time_correlation, b4d_two_time) against the float64 model of
test_two_time_host.py, on the smallest shapes at which each path of the kernels can go wrong:

  a  T = 5, 37 x 53                      partial frame tile, odd pixel count, one partial chunk
  b  T = 130, 64 x 96                    two frame blocks (diagonal pair, off-diagonal pair and its mirror), ragged second block
  c  T = 33, 256 x 320, three rings      several chunks per region, region padding, an empty region (label 3 of R = 4)
  d  case b with 1 % NaN / +-Inf entries  pixels dropped in all frames
  e  T = 20, 64 x 96 uint16, 1 % contrast the centring (raw float32 products miss this by orders of magnitude)
  f  T = 300, 32 x 48, max_lag = 40      three frame blocks, pair (0, 2) skipped
  g  case a, a constant and a mean-0 frame  the NaN rules per norm
  h  AR(1) speckle                       physics: g2(tau) = rho^(2 tau)

The deviation is taken in Pearson units for all norms (test_two_time_host.deviation).  CAP = 1e-5 is the project's standing bar
for float32 transform paths; BAR is 4 x the largest deviation observed on an MI355X over all cases, under the cap; the observed
maxima are listed in DESIGN.md section 20."""
import functools

import numpy as np
import pytest

from barc4dip_amd.metrics import correlation_decay, two_time_correlation
from barc4dip_amd.metrics import twotime as tt
from test_two_time_host import (NORMS, RHO, ar1_stack, degenerate_stack, deviation, low_contrast_stack, model_two_time, ring_labels,
                                speckle_stack, with_bad_entries)

pytestmark = pytest.mark.gpu

CAP = 1e-5
BAR = 5.2e-6               # 4 x 1.292e-06 (case g: the integer-valued mean-0 frame, whose squares round one way in a float32
                            # sum; 1.6e-07 .. 3.9e-07 in the cases a .. f, 2.4e-07 at 1 % contrast)
assert BAR <= CAP

KEYS = ("two_time", "mean", "var", "contrast", "n_pixels", "g2", "g2_err")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "a":
        return speckle_stack(5, 37, 53, seed=11), {}
    if name == "b":
        return speckle_stack(130, 64, 96, seed=12), {}
    if name == "c":
        return speckle_stack(33, 256, 320, seed=13), {"labels": ring_labels()}
    if name == "d":
        return with_bad_entries(case("b")[0]), {}
    if name == "e":
        return low_contrast_stack(), {}
    if name == "f":
        return speckle_stack(300, 32, 48, seed=14), {"max_lag": 40}
    if name == "g":
        return degenerate_stack(), {}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def model(name, norm):
    images, kw = case(name)
    return model_two_time(images, norm=norm, **kw)


@functools.lru_cache(maxsize=None)
def device(name, norm):
    images, kw = case(name)
    return two_time_correlation(images, norm=norm, **kw)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in KEYS)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name", list("abcdefg"))
def test_cases_against_model(observe, name, norm):
    got, want = device(name, norm), model(name, norm)
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert got["lags"].tolist() == want["lags"].tolist() and got["meta"] == want["meta"]
    dev = deviation(got, want, norm)
    print(f"two_time.{name}.{norm}: deviation {dev:.3e}")
    C = got["two_time"]
    assert np.array_equal(C, np.swapaxes(C, -1, -2), equal_nan=True), "the matrix is not exactly symmetric"
    if norm == "pearson":
        d = np.diagonal(C, axis1=-2, axis2=-1)
        assert np.all(d[got["var"] > 0] == 1.0) and np.isnan(d[~(got["var"] > 0)]).all()
    assert np.array_equal(np.isnan(got["contrast"]), np.isnan(want["contrast"]))
    live = ~np.isnan(want["contrast"])
    crel = float(np.max(np.abs(got["contrast"][live] / want["contrast"][live] - 1.0))) if live.any() else 0.0
    print(f"two_time.{name}.{norm}: contrast {crel:.3e}")
    observe(f"two_time.{name}.{norm}", dev, BAR)
    # d c / c = d var / (2 var) + (d m / sd) contrast, and contrast <= about 1 here
    observe(f"two_time.contrast.{name}.{norm}", crel, 2 * BAR)


def test_case_c_has_chunks_padding_and_an_empty_region():
    got = device("c", "pearson")
    assert got["n_pixels"].max() > 2 * tt.CHUNK, "the largest region must span at least three chunks: enlarge the frame"
    assert np.all(got["n_pixels"][[0, 1, 3]] % tt.CHUNK != 0)             # every region ends in a padded chunk
    assert got["n_pixels"][2] == 0 and got["two_time"].shape == (4, 33, 33)
    for k in ("two_time", "mean", "var", "contrast", "g2", "g2_err"):
        assert np.isnan(got[k][2]).all(), k
        assert np.isfinite(got[k][[0, 1, 3]]).all(), k


def test_bad_entries_drop_pixels():
    got, want = device("d", "pearson"), model("d", "pearson")
    assert 0 < got["n_pixels"] == want["n_pixels"] < 64 * 96 // 2
    assert np.isfinite(got["two_time"]).all()


@pytest.mark.parametrize("norm", NORMS)
def test_band_is_the_full_run_inside_and_nan_outside(norm):
    images, _ = case("f")
    band, full = device("f", norm), two_time_correlation(images, norm=norm)
    i, j = np.indices((300, 300))
    inside = np.abs(i - j) <= 40
    assert np.isnan(band["two_time"][~inside]).all() and np.isfinite(full["two_time"]).all()
    assert np.array_equal(band["two_time"][inside], full["two_time"][inside])
    for k in ("mean", "var", "contrast", "n_pixels"):
        assert np.array_equal(band[k], full[k]), k
    assert np.array_equal(band["g2"], full["g2"][:41]) and np.array_equal(band["g2_err"], full["g2_err"][:41])
    assert band["lags"].tolist() == list(range(41)) and band["meta"]["max_lag"] == 40


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_two_runs_give_the_same_bits(name):
    images, kw = case(name)
    assert same_bits(device(name, "pearson"), two_time_correlation(images, norm="pearson", **kw))


@pytest.mark.parametrize("norm", NORMS)
def test_region_alone_equals_region_among_many(norm):
    images, kw = case("c")
    alone = two_time_correlation(images, norm=norm, mask=kw["labels"] == 2)
    many = device("c", norm)
    for k in KEYS:
        assert np.array_equal(many[k][1], alone[k]), k
    assert alone["two_time"].shape == (33, 33) and alone["meta"]["n_regions"] == 1


def test_tensor_input_and_tensor_output():
    import torch

    images, kw = case("c")
    want = device("c", "intensity")
    x = torch.from_numpy(images).cuda()
    got = two_time_correlation(x, norm="intensity", labels=torch.from_numpy(kw["labels"]).cuda())
    assert same_bits(got, want)
    dev = two_time_correlation(x, norm="intensity", return_tensors=True, **kw)
    for k in KEYS + ("lags",):
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda, k
    assert dev["two_time"].dtype == torch.float64 and dev["n_pixels"].dtype == torch.int64
    assert same_bits({k: dev[k].cpu().numpy() for k in KEYS}, want)
    assert np.array_equal(correlation_decay(dev), correlation_decay(want), equal_nan=True)
    # float64 frames reach the device as the float32 values the model uses
    assert same_bits(two_time_correlation(images.astype(np.float64), norm="intensity", **kw), want)


@pytest.mark.parametrize("norm", NORMS)
def test_nan_rules(norm):
    C = device("g", norm)["two_time"]
    nan_rows = {"pearson": [1], "intensity": [3], "covariance": []}[norm]
    for i in range(5):
        assert np.isnan(C[i]).all() == (i in nan_rows) and np.isnan(C[:, i]).all() == (i in nan_rows)
    got = device("g", norm)
    assert got["var"][1] == 0.0 and got["mean"][1] == 7.0 and got["mean"][3] == 0.0
    assert np.isnan(got["contrast"][[1, 3]]).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ar1_speckle_decorrelates_as_rho(seed):
    res = two_time_correlation(ar1_stack(seed))
    tau = np.arange(13)
    err = float(np.max(np.abs(res["g2"][:13] - RHO ** (2 * tau))))
    decay = float(correlation_decay(res))
    print(f"two_time.h.seed{seed}: |g2 - rho^2tau| {err:.4f}, decay {decay:.4f}")
    assert err <= 0.03
    assert abs(decay - (-1.0 / (2.0 * np.log(RHO)))) <= 0.15
