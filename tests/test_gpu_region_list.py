"""GPU tier of the region list (csrc/b4d_regions.hpp) that orders every sum of the two-time and the multi-tau correlator: both
run on label maps built for the list builder's edges, against the float64 models of the two host test modules.

  interleaved  8 x 72, label = 1 + (p mod 64)       R = 64; every wave holds 64 labels (64 rounds of the grouping), 9 pixels each
  exact        96 x 128, runs of 2048, 64, 4096     regions that end exactly on a chunk and on a wave: no padding
  ragged       37 x 53, random 0 .. 3, last = 5     partial last wave; empty region 4; region 5 is one pixel in the last live lane
  spans        520 x 520, random 0 .. 3, T = 4      more than 2^18 pixels: spans of two wave groups, a partial last span
  bad          ragged with 1 % NaN / +-Inf entries  a bad pixel leaves its region's count

Two-time: T = 6, all three norms; multi-tau: T = 20, lags_per_level = 8.  n_pixels must equal the model's exactly.  The model is
asserted finite wherever a region has two pixels or more, so that no NaN passes as "equal NaN".  A one-pixel region has no
variance: the two-time model defines it (covariance 0, Pearson NaN) and is compared in full; of the multi-tau result g2 and mean
are compared, g2_err is not (the variance of one pixel's products is a difference of second moments that are equal at one pair).
The bars are those of test_gpu_two_time.py and test_gpu_multi_tau.py where the deviations observed on an MI355X for these
cases lie within them (two-time 4.6e-07, multi-tau mean 4.3e-08 and g2_err 4.6e-07).  The multi-tau g2 of regions of 1 and 9
pixels does not: at the one lag with a single frame pair A and B are the level's float64 sum S less four frame sums, S carries
the float32 rounding of a run of eight frames, and nothing averages it down: 1.176e-06 (one pixel), 6.9e-07 (nine), against
1.7e-07 and less from 64 pixels on.  MT_G2_BAR is set for this file by the same rule, 4 x the largest observed, under CAP.  The
observed maxima are listed in DESIGN.md sections 20 and 21."""
import functools

import numpy as np
import pytest

from barc4dip_amd.metrics import multi_tau_correlation, two_time_correlation
from barc4dip_amd.metrics import twotime as tt
from test_gpu_multi_tau import BAR as MT_BAR
from test_gpu_multi_tau import ERR_BAR as MT_ERR_BAR
from test_gpu_two_time import BAR as TT_BAR
from test_gpu_two_time import CAP
from test_multi_tau_host import deviation as mt_deviation
from test_multi_tau_host import model_multi_tau
from test_two_time_host import NORMS, model_two_time, speckle_stack, with_bad_entries
from test_two_time_host import deviation as tt_deviation

pytestmark = pytest.mark.gpu

MT_G2_BAR = 4.71e-6        # 4 x 1.176e-06 (ragged and bad: the one-pixel region at the lag with one frame pair)
assert MT_BAR <= MT_G2_BAR <= CAP

CASES = ("interleaved", "exact", "ragged", "spans", "bad")
ALONE = {"interleaved": 40, "exact": 2, "ragged": 5, "spans": 2, "bad": 2}       # the region that is also run alone under mask=
TT_KEYS = ("two_time", "mean", "var", "contrast", "n_pixels", "g2", "g2_err")
MT_KEYS = ("g2", "g2_err", "mean", "n_pixels")


@functools.lru_cache(maxsize=None)
def labels(name):
    if name == "interleaved":
        return (1 + np.arange(8 * 72) % 64).reshape(8, 72).astype(np.int32)
    if name == "exact":
        lab = np.zeros(96 * 128, np.int32)
        lab[:2048], lab[2048:2112], lab[2112:6208] = 1, 2, 3
        return lab.reshape(96, 128)
    if name in ("ragged", "bad"):
        lab = np.random.default_rng(41).integers(0, 4, 37 * 53).astype(np.int32)
        lab[-1] = 5
        return lab.reshape(37, 53)
    if name == "spans":
        return np.random.default_rng(42).integers(0, 4, (520, 520)).astype(np.int32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def stack(name, T):
    if name == "bad":
        return with_bad_entries(stack("ragged", T))
    H, W = labels(name).shape
    return speckle_stack(4 if name == "spans" else T, H, W, seed=43 + CASES.index(name))


@functools.lru_cache(maxsize=None)
def tt_model(name, norm):
    return model_two_time(stack(name, 6), labels=labels(name), norm=norm)


@functools.lru_cache(maxsize=None)
def tt_device(name, norm):
    return two_time_correlation(stack(name, 6), labels=labels(name), norm=norm)


@functools.lru_cache(maxsize=None)
def mt_model(name):
    return model_multi_tau(stack(name, 20), labels=labels(name), lags_per_level=8)


@functools.lru_cache(maxsize=None)
def mt_device(name):
    return multi_tau_correlation(stack(name, 20), labels=labels(name), lags_per_level=8)


def pick(res, keys, rows):
    """The result with the per-region arrays cut to the regions `rows`."""
    return {k: (np.asarray(v)[rows] if k in keys else v) for k, v in res.items()}


def check_counts(name, npx):
    lab = labels(name)
    if name == "interleaved":
        assert npx.tolist() == [9] * 64
    if name == "exact":
        assert npx[0] % tt.CHUNK == 0 and npx[2] % tt.CHUNK == 0 and npx[1] == 64 and npx.tolist() == [2048, 64, 4096]
    if name == "ragged":
        assert lab.size == 1961 and npx[3] == 0 and npx[4] == 1 and npx[:3].min() > 64
    if name == "spans":
        assert lab.size > 2 ** 18 and lab.size % 128 == 64 and npx.min() > 2 ** 15
    if name == "bad":
        clean = np.bincount(lab.reshape(-1), minlength=6)[1:]
        assert np.all(npx[:3] < clean[:3]) and npx[:3].min() > 64


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name", CASES)
def test_two_time_against_model(observe, name, norm):
    got, want = tt_device(name, norm), tt_model(name, norm)
    full = want["n_pixels"] >= 2
    for k in ("mean", "var", "contrast", "g2", "g2_err", "two_time"):
        assert np.isfinite(want[k][full]).all(), f"the model's {k} is not finite in a region of two pixels or more"
    assert got["n_pixels"].dtype == np.int64 and np.array_equal(got["n_pixels"], want["n_pixels"])
    check_counts(name, got["n_pixels"])
    dev = tt_deviation(got, want, norm)
    print(f"region_list.two_time.{name}.{norm}: deviation {dev:.3e}")
    one = np.flatnonzero(want["n_pixels"] == 1)
    assert np.all(got["var"][one] == 0.0) and np.array_equal(got["mean"][one], want["mean"][one])
    empty = want["n_pixels"] == 0
    assert np.isnan(got["two_time"][empty]).all() and np.isnan(got["mean"][empty]).all()
    observe(f"region_list.two_time.{name}.{norm}", dev, TT_BAR)


@pytest.mark.parametrize("name", CASES)
def test_multi_tau_against_model(observe, name):
    got, want = mt_device(name), mt_model(name)
    full = want["n_pixels"] >= 2
    for k in ("g2", "g2_err", "mean"):
        assert np.isfinite(want[k][full]).all(), f"the model's {k} is not finite in a region of two pixels or more"
    assert got["n_pixels"].dtype == np.int64 and np.array_equal(got["n_pixels"], want["n_pixels"])
    check_counts(name, got["n_pixels"])
    rows = np.flatnonzero(want["n_pixels"] != 1)
    dg, de, dm = mt_deviation(pick(got, MT_KEYS, rows), pick(want, MT_KEYS, rows))
    one = np.flatnonzero(want["n_pixels"] == 1)
    if one.size:
        assert np.isfinite(want["g2"][one]).all() and np.isfinite(got["g2"][one]).all()
        dg = max(dg, float(np.max(np.abs(got["g2"][one] - want["g2"][one]))))
        dm = max(dm, float(np.max(np.abs(got["mean"][one] / want["mean"][one] - 1.0))))
    print(f"region_list.multi_tau.{name}: g2 {dg:.3e}, g2_err {de:.3e}, mean {dm:.3e}")
    observe(f"region_list.multi_tau.g2.{name}", dg, MT_G2_BAR)
    observe(f"region_list.multi_tau.mean.{name}", dm, MT_BAR)
    observe(f"region_list.multi_tau.g2_err.{name}", de, MT_ERR_BAR)


@pytest.mark.parametrize("name", CASES)
def test_region_alone_equals_region_among_many(name):
    r = ALONE[name]
    mask = labels(name) == r
    assert mask.any()
    for norm in NORMS:
        alone, many = two_time_correlation(stack(name, 6), mask=mask, norm=norm), tt_device(name, norm)
        for k in TT_KEYS:
            assert np.array_equal(many[k][r - 1], alone[k], equal_nan=True), (norm, k)
    alone, many = multi_tau_correlation(stack(name, 20), mask=mask, lags_per_level=8), mt_device(name)
    for k in MT_KEYS:
        assert np.array_equal(many[k][r - 1], alone[k], equal_nan=True), k
    assert alone["n_pixels"] == many["n_pixels"][r - 1] > 0
