"""GPU tier of the multi-tau correlation (barc4dip_amd.metrics.multi_tau_correlation, b4d_multi_tau_*) against the float64 model
of test_multi_tau_host.py, on the smallest shapes at which each path of the kernels can go wrong:

  a  T = 37, 37 x 53, m = 16, one push        odd T, partial wave, three levels, a lag with n = 1, a dropped unpaired frame
  b  case a, chunk_frames = 5                 odd pushes, unpaired frames and rings carried across pushes at every level
  c  T = 200, 64 x 96, m = 8, rings 1, 2, 4   the second template, several regions, empty region -> NaN and n_pixels = 0
  d  case c's stack, 1 % NaN / +-Inf entries   the scan; n_pixels equal to the model's exactly
  e  T = 64, 64 x 96 uint16, 1 % contrast     g2 - 1 = 1e-4
  f  T = 70, 16 x 24, m = 32                  the third template, level 0 only partly filled
  g  T = 1024, 32 x 48 AR(1), rho = 0.9       the closed form, bar 0.012 as on the host; correlation_decay
  h  an all-zero region; T = 2                NaN rules; the smallest stack

The deviation from the model is the largest |d g2|, and relative for g2_err and mean (test_multi_tau_host.deviation).  CAP = 1e-5
is the project's standing bar for float32 paths; BAR is 4 x the largest deviation of g2 and mean observed on an MI355X over the
cases a .. f, under the cap, and at most 1e-6 in case e (1 % of that case's signal).  ERR_BAR is 4 x the largest relative deviation
of g2_err observed over the same cases; it is a difference of second moments and has no cap fixed in advance.  The observed
maxima are listed in DESIGN.md section 21."""
import functools

import numpy as np
import pytest

from barc4dip_amd.metrics import correlation_decay, multi_tau_correlation
from test_multi_tau_host import (AR1_BAR, DECAY_BAR, ar1_closed_form, ar1_stack, deviation, low_contrast_stack, model_multi_tau, rings,
                                 speckle_stack, with_bad_entries, zero_region_case)

pytestmark = pytest.mark.gpu

CAP = 1e-5
BAR = 2.02e-7              # 4 x 5.029e-08 (case a; 4.0e-09 .. 4.4e-08 in the cases b .. f, 1.6e-08 in h, 5.3e-08 for b against a;
                           # the means agree to 1.1e-09)
BAR_E = min(BAR, 1e-6)     # case e: 7.9e-09 observed against a signal g2 - 1 of 1e-4
ERR_BAR = 5.7e-5           # 4 x 1.408e-05 (case e: at 1 % contrast the variance of the products is a difference of second
                           # moments that agree to 4e-4; 1.3e-08 .. 8.6e-08 in the other cases)
assert BAR <= CAP

KEYS = ("g2", "g2_err", "mean", "n_pixels", "lags", "level", "n_pairs")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "a":
        return speckle_stack(37, 37, 53, seed=21), {"lags_per_level": 16}
    if name == "b":
        return case("a")[0], {"lags_per_level": 16, "chunk_frames": 5}
    if name == "c":
        return speckle_stack(200, 64, 96, seed=22), {"lags_per_level": 8, "labels": rings()}
    if name == "d":
        return with_bad_entries(case("c")[0]), {"lags_per_level": 8, "labels": rings()}
    if name == "e":
        return low_contrast_stack(T=64), {"lags_per_level": 16}
    if name == "f":
        return speckle_stack(70, 16, 24, seed=23), {"lags_per_level": 32}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def model(name):
    images, kw = case(name)
    return model_multi_tau(images, **{k: v for k, v in kw.items() if k != "chunk_frames"})


@functools.lru_cache(maxsize=None)
def device(name):
    images, kw = case(name)
    return multi_tau_correlation(images, **kw)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in KEYS)


@pytest.mark.parametrize("name", list("abcdef"))
def test_cases_against_model(observe, name):
    got, want = device(name), model(name)
    dg, de, dm = deviation(got, want)
    print(f"multi_tau.{name}: g2 {dg:.3e}, g2_err {de:.3e}, mean {dm:.3e}")
    for k in ("lags_per_level", "n_levels", "n_regions", "n_frames"):
        assert got["meta"][k] == want["meta"][k], k
    observe(f"multi_tau.g2.{name}", dg, BAR_E if name == "e" else BAR)
    observe(f"multi_tau.mean.{name}", dm, BAR)
    observe(f"multi_tau.g2_err.{name}", de, ERR_BAR)


def test_case_a_reaches_what_it_is_for():
    got = device("a")
    assert got["g2"].shape == (25,) and got["level"].max() == 2 and got["n_pairs"][-1] == 1 and got["lags"][-1] == 32
    assert np.isfinite(got["g2"]).all() and np.isfinite(got["g2_err"]).all()
    assert got["n_pixels"] == 37 * 53 and (37 * 53) % 64 != 0


def test_odd_pushes_agree_with_one_push(observe):
    one, many = device("a"), device("b")
    assert many["meta"]["chunk_frames"] == 5 and one["meta"]["chunk_frames"] == 37
    dg, de, dm = deviation(many, one)
    print(f"multi_tau.b_vs_a: g2 {dg:.3e}, g2_err {de:.3e}, mean {dm:.3e}")
    observe("multi_tau.g2.b_vs_a", dg, BAR)
    observe("multi_tau.mean.b_vs_a", dm, BAR)
    observe("multi_tau.g2_err.b_vs_a", de, ERR_BAR)


def test_case_c_has_several_regions_and_an_empty_one():
    got = device("c")
    assert got["g2"].shape == (4, len(got["lags"])) and got["n_pixels"][2] == 0
    assert np.all(got["n_pixels"][[0, 1, 3]] > 64) and np.all(got["n_pixels"][[0, 1, 3]] % 64 != 0)   # each ends in a partial wave
    for k in ("g2", "g2_err", "mean"):
        assert np.isnan(got[k][2]).all(), k
        assert np.isfinite(got[k][[0, 1, 3]]).all(), k


def test_bad_entries_drop_pixels():
    got, want, clean = device("d"), model("d"), device("c")
    assert np.array_equal(got["n_pixels"], want["n_pixels"])
    assert np.all(got["n_pixels"][[0, 1, 3]] > 0) and np.all(got["n_pixels"][[0, 1, 3]] < clean["n_pixels"][[0, 1, 3]])
    assert np.isfinite(got["g2"][[0, 1, 3]]).all()


def test_low_contrast_signal():
    got = device("e")
    assert 0.5e-4 < got["g2"][0] - 1.0 < 2e-4           # (300 / 30000)^2


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_two_runs_give_the_same_bits(name):
    images, kw = case(name)
    assert same_bits(device(name), multi_tau_correlation(images, **kw))


def test_region_alone_equals_region_among_many():
    images, kw = case("c")
    alone = multi_tau_correlation(images, mask=kw["labels"] == 2, lags_per_level=8)
    many = device("c")
    for k in ("g2", "g2_err", "mean", "n_pixels"):
        assert np.array_equal(many[k][1], alone[k]), k
    assert alone["g2"].shape == many["lags"].shape and alone["meta"]["n_regions"] == 1


def test_max_level_returns_the_first_lags_unchanged():
    images, kw = case("c")
    full, capped = device("c"), multi_tau_correlation(images, max_level=1, **kw)
    n = int(np.sum(full["level"] <= 1))
    assert 8 < n < len(full["lags"]) and len(capped["lags"]) == n and capped["meta"]["n_levels"] == 2
    for k in ("lags", "level", "n_pairs"):
        assert np.array_equal(capped[k], full[k][:n]), k
    for k in ("g2", "g2_err"):
        assert np.array_equal(capped[k], full[k][:, :n], equal_nan=True), k
    assert np.array_equal(capped["mean"], full["mean"], equal_nan=True) and np.array_equal(capped["n_pixels"], full["n_pixels"])


def test_tensor_input_and_tensor_output():
    import torch

    images, kw = case("c")
    want = device("c")
    x = torch.from_numpy(images).cuda()
    assert same_bits(multi_tau_correlation(x, lags_per_level=8, labels=torch.from_numpy(kw["labels"]).cuda()), want)
    dev = multi_tau_correlation(x, return_tensors=True, **kw)
    for k in KEYS:
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda, k
    assert dev["g2"].dtype == torch.float64 and dev["n_pixels"].dtype == torch.int64 and dev["lags"].dtype == torch.int64
    assert same_bits({k: dev[k].cpu().numpy() for k in KEYS}, want)
    assert np.array_equal(correlation_decay(dev), correlation_decay(want), equal_nan=True)
    # float64 frames reach the device as the float32 values the model uses
    assert same_bits(multi_tau_correlation(images.astype(np.float64), **kw), want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ar1_speckle_follows_the_closed_form(seed):
    res = multi_tau_correlation(ar1_stack(seed, T=1024, H=32, W=48), chunk_frames=256)
    assert len(res["lags"]) == 64 and res["meta"]["n_levels"] == 7
    want = ar1_closed_form(res["lags"], res["level"])
    err = float(np.max(np.abs(res["g2"] - want)))
    decay, decay0 = float(correlation_decay(res)), float(correlation_decay(want, lags=res["lags"], baseline=1.0))
    print(f"multi_tau.g.seed{seed}: |g2 - closed form| {err:.4f}, decay {decay:.4f} against {decay0:.4f}")
    assert err <= AR1_BAR
    assert abs(decay - decay0) <= DECAY_BAR


def test_nan_rules_and_the_smallest_stack(observe):
    s, lab = zero_region_case()
    got, want = multi_tau_correlation(s, labels=lab), model_multi_tau(s, labels=lab)
    dg, de, dm = deviation(got, want)
    assert np.isnan(got["g2"][1]).all() and np.isnan(got["g2_err"][1]).all() and got["mean"][1] == 0.0
    assert np.isfinite(got["g2"][0]).all() and got["n_pixels"].tolist() == [8 * 24, 8 * 24]
    observe("multi_tau.g2.h", dg, BAR)
    two = speckle_stack(2, 16, 24, seed=28)
    got, want = multi_tau_correlation(two), model_multi_tau(two)
    assert got["lags"].tolist() == [0, 1] and got["n_pairs"].tolist() == [2, 1]
    dg, de, dm = deviation(got, want)
    print(f"multi_tau.h: g2 {dg:.3e}, g2_err {de:.3e}, mean {dm:.3e}")
    observe("multi_tau.g2.h", dg, BAR)
    observe("multi_tau.mean.h", dm, BAR)
    observe("multi_tau.g2_err.h", de, ERR_BAR)


# ---------------------------------------------------------------- streamed sources against the resident call
def test_streamed_uint16_memmap(tmp_path):
    rng = np.random.default_rng(31)
    words = np.rint(2000.0 + 400.0 * rng.standard_normal((96, 40, 56))).clip(0, 65535).astype(np.uint16)
    np.save(tmp_path / "words.npy", words)
    source = np.load(tmp_path / "words.npy", mmap_mode="r")
    assert isinstance(source, np.memmap)
    streamed = multi_tau_correlation(source, chunk_frames=16)        # six chunks: each rotating buffer is used three times
    resident = multi_tau_correlation(words, chunk_frames=16)
    assert same_bits(streamed, resident) and streamed["n_pixels"] == 40 * 56
    dg, de, dm = deviation(streamed, model_multi_tau(words))
    assert dg <= BAR and dm <= BAR and de <= ERR_BAR


def test_streamed_float_memmap_is_scanned_before_the_first_push(tmp_path):
    stack = speckle_stack(40, 24, 32, seed=32)
    stack[37, 5, 7] = np.nan                                         # the only bad entry sits in the last chunk
    np.save(tmp_path / "frames.npy", stack)
    source = np.load(tmp_path / "frames.npy", mmap_mode="r")
    lab = np.ones((24, 32), np.int32)
    lab[12:] = 2
    streamed = multi_tau_correlation(source, labels=lab, chunk_frames=16)
    resident = multi_tau_correlation(stack, labels=lab, chunk_frames=16)
    assert same_bits(streamed, resident)
    assert streamed["n_pixels"].tolist() == [12 * 32 - 1, 12 * 32] and np.isfinite(streamed["g2"]).all()
    dg, de, dm = deviation(streamed, model_multi_tau(stack, labels=lab))
    assert dg <= BAR and dm <= BAR and de <= ERR_BAR
