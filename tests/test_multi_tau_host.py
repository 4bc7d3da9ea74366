"""CPU tier of the multi-tau correlation: a float64 NumPy model of the definitions in include/b4d.h (b4d_multi_tau_*), checked
against a brute-force loop and the closed form for AR(1) speckle, the lag table of the library, and the host-side pieces of
barc4dip_amd.metrics.multitau (argument checks) and of correlation_decay (lag axis).  The GPU tier (test_gpu_multi_tau.py)
imports the model, the case builders and the deviation measure from here."""
import numpy as np
import pytest

from barc4dip_amd import _ffi
from barc4dip_amd.metrics import multitau as mt
from barc4dip_amd.metrics import twotime as tt
from test_two_time_host import ar1_stack, low_contrast_stack, speckle_stack, with_bad_entries  # noqa: F401  (shared builders)

RHO = 0.9
AR1_BAR = 0.012            # |g2 - closed form| over all 64 lags at T = 1024, 32 x 48: 0.0029 .. 0.0038 observed for the model on
                           # seeds 1 .. 3; the margin is statistical
# the 1/e crossing of the normalised curve g moves by at most (dg + level dg0) / |slope|: both g2 and g2[0] are off by at most
# AR1_BAR, and at the crossing of rho^(2 tau) the slope is 2 ln(rho) / e per frame
DECAY_BAR = AR1_BAR * (1.0 + np.exp(-1.0)) / (2.0 * abs(np.log(RHO)) * np.exp(-1.0))


# ---------------------------------------------------------------- the model
def model_lag_table(T, m, max_level=None):
    """(lags, level, n_pairs) from the text of the definition, independent of the library's table."""
    rows = [(j, 0, T - j) for j in range(m) if T - j >= 1]
    l = 1
    while (T >> l) >= m // 2 + 1 and (max_level is None or l <= max_level):
        rows += [(j << l, l, (T >> l) - j) for j in range(m // 2, m) if (T >> l) - j >= 1]
        l += 1
    a = np.array(rows, dtype=np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


def model_multi_tau(images, labels=None, mask=None, lags_per_level=16, max_level=None):
    """The definitions in float64, level averages included.  Frames are cast to float32 first: that is what the device sees."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(images).astype(np.float32).astype(np.float64)
    T, H, W = x.shape
    m = lags_per_level
    lags, level, pairs = model_lag_table(T, m, max_level)
    if labels is not None:
        lab, R = np.asarray(labels), int(np.max(labels))
    else:
        lab, R = (np.ones((H, W), int) if mask is None else np.asarray(mask).astype(int)), 1
    fin = np.isfinite(x).all(axis=0)
    g2, err = np.full((R, len(lags)), np.nan), np.full((R, len(lags)), np.nan)
    mean, npx = np.full(R, np.nan), np.zeros(R, np.int64)
    for r in range(1, R + 1):
        sel = (lab == r) & fin
        N = int(sel.sum())
        npx[r - 1] = N
        if N == 0:
            continue
        I = x[:, sel]
        mean[r - 1] = I.mean()
        for l in range(int(level.max()) + 1):
            for k in np.flatnonzero(level == l):
                j, n = int(lags[k] >> l), int(pairs[k])
                a, b = I[:n], I[j:j + n]
                pr = a * b
                p, q, den = pr.mean(), (pr * pr).mean(), a.mean() * b.mean()
                if den > 0:
                    g2[r - 1, k] = p / den
                    err[r - 1, k] = np.sqrt(max(q - p * p, 0.0) / (N * n)) / den
            half = I.shape[0] // 2
            I = 0.5 * (I[0:2 * half:2] + I[1:2 * half:2])
    res = {"g2": g2, "g2_err": err, "mean": mean, "n_pixels": npx}
    if labels is None:
        res = {k: v[0] for k, v in res.items()}
    res.update({"lags": lags, "level": level, "n_pairs": pairs})
    res["meta"] = {"lags_per_level": m, "n_levels": int(level.max()) + 1, "n_regions": R, "n_frames": T}
    return res


def ar1_closed_form(lags, level, rho=RHO):
    """g2 of I = |E|^2 for the AR(1) field of ar1_stack after averaging B = 2^l frames: 1 + the mean of rho^(2 |tau + d|) over the
    pairs of frames of the two bins, d = -(B - 1) .. B - 1 with weight (B - |d|) / B^2."""
    out = np.empty(len(lags))
    for k, (tau, l) in enumerate(zip(lags, level)):
        B = 1 << int(l)
        d = np.arange(-(B - 1), B)
        out[k] = 1.0 + np.sum((B - np.abs(d)) / B ** 2 * rho ** (2.0 * np.abs(int(tau) + d)))
    return out


def deviation(got, want):
    """(largest |d g2|, largest relative difference of g2_err, of mean) of `got` from the model `want`.  NaNs must coincide; the
    lag table and the pixel counts must be equal."""
    for k in ("lags", "level", "n_pairs", "n_pixels"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype == np.int64 and np.array_equal(a, b), k
    out = []
    for k, relative in (("g2", False), ("g2_err", True), ("mean", True)):
        g, w = np.asarray(got[k], float), np.asarray(want[k], float)
        assert g.shape == w.shape and got[k].dtype == np.float64, k
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"NaN entries of {k} differ from the model's"
        live = ~np.isnan(w)
        if relative:
            assert np.array_equal(g[live & (w == 0)], w[live & (w == 0)]), k
            live &= w != 0
        d = np.abs(g[live] - w[live]) / (np.abs(w[live]) if relative else 1.0)
        out.append(float(d.max()) if d.size else 0.0)
    return tuple(out)


# ---------------------------------------------------------------- case builders (shared with the GPU tier)
def rings(H=64, W=96):
    """Three rings (labels 1, 2, 4) around the centre and an unlabelled rest; label 3 is absent, so R = 4 with an empty region."""
    y, x = np.mgrid[:H, :W]
    rad = np.hypot(y - (H - 1) / 2.0, x - (W - 1) / 2.0)
    lab = np.zeros((H, W), np.int32)
    lab[rad < 14] = 1
    lab[(rad >= 14) & (rad < 24)] = 2
    lab[(rad >= 24) & (rad < 29)] = 4           # 616, 1188 and 840 pixels: none a whole number of waves
    return lab


def zero_region_case():
    """T = 6, 16 x 24, labels 1 and 2; region 2 is zero in every frame."""
    s = speckle_stack(6, 16, 24, seed=27)
    lab = np.ones((16, 24), np.int32)
    lab[8:] = 2
    s[:, 8:] = 0.0
    return s, lab


# ---------------------------------------------------------------- the lag table
def test_lag_table_counts():
    lags, level, pairs, L = mt.lag_table(37, 16)
    assert len(lags) == 25 and L == 3
    assert lags.tolist() == list(range(16)) + list(range(16, 32, 2)) + [32]
    assert level.tolist() == [0] * 16 + [1] * 8 + [2] and pairs[-1] == 1 and pairs[0] == 37
    lags, level, pairs, L = mt.lag_table(100_000, 16)
    assert len(lags) == 116 and lags[-1] == 90_112 and L == 14
    assert all(a.dtype == np.int64 for a in (lags, level, pairs))


@pytest.mark.parametrize("m", [8, 16, 32])
def test_lag_table_is_the_models(m):
    for T in (2, 3, 5, 9, 17, 37, 64, 70, 200, 1024, 4097, 100_000):
        for cap in (None, 0, 1, 3):
            got, want = mt.lag_table(T, m, cap), model_lag_table(T, m, cap)
            for a, b in zip(got[:3], want):
                assert np.array_equal(a, b), (T, m, cap)
            assert got[3] == int(want[1].max()) + 1
            assert np.all(want[2] >= 1) and np.all(np.diff(want[0]) > 0)


def test_lag_table_limits():
    lib = _ffi.load_library()
    assert lib.b4d_multi_tau_lags(1, 16, -1, None, None, None, None) == -1
    assert lib.b4d_multi_tau_lags(100, 12, -1, None, None, None, None) == -2
    assert lib.b4d_multi_tau_lags(2 ** 31, 16, -1, None, None, None, None) == -2
    assert lib.b4d_multi_tau_lags(2 ** 31 - 1, 8, -1, None, None, None, None) == -2      # 29 levels
    assert lib.b4d_multi_tau_lags(2 ** 31 - 1, 8, 23, None, None, None, None) == 8 + 23 * 4
    with pytest.raises(NotImplementedError):
        mt.lag_table(2 ** 31 - 1, 8)


# ---------------------------------------------------------------- the model against a double loop and a closed form
def test_level_0_against_a_double_loop():
    s = speckle_stack(11, 5, 7, seed=3)
    res = model_multi_tau(s, lags_per_level=8)
    x = s.astype(np.float64).reshape(11, -1)
    for k in range(8):
        assert res["level"][k] == 0 and res["lags"][k] == k and res["n_pairs"][k] == 11 - k
        P = Q = A = B = 0.0
        for t in range(11 - k):
            for p in range(35):
                pr = x[t, p] * x[t + k, p]
                P, Q, A, B = P + pr, Q + pr * pr, A + x[t, p], B + x[t + k, p]
        Nn = 35.0 * (11 - k)
        den = (A / Nn) * (B / Nn)
        assert res["g2"][k] == pytest.approx(P / Nn / den, rel=1e-12)
        assert res["g2_err"][k] == pytest.approx(np.sqrt((Q / Nn - (P / Nn) ** 2) / Nn) / den, rel=1e-9)
    assert res["mean"] == pytest.approx(x.mean(), rel=1e-13) and res["n_pixels"] == 35


def test_levels_average_pairs_and_drop_the_unpaired_frame():
    rng = np.random.default_rng(5)
    s = rng.random((37, 4, 6)).astype(np.float32) + 0.5
    res = model_multi_tau(s)
    x = s.astype(np.float64).reshape(37, -1)
    l1 = 0.5 * (x[0:36:2] + x[1:36:2])                   # frame 36 is dropped
    l2 = 0.5 * (l1[0:18:2] + l1[1:18:2])
    k = int(np.flatnonzero(res["lags"] == 20)[0])        # level 1, j = 10, n = 8
    assert res["level"][k] == 1 and res["n_pairs"][k] == 8
    assert res["g2"][k] == pytest.approx((l1[:8] * l1[10:18]).mean() / (l1[:8].mean() * l1[10:18].mean()), rel=1e-13)
    assert res["level"][-1] == 2 and res["n_pairs"][-1] == 1
    assert res["g2"][-1] == pytest.approx((l2[0] * l2[8]).mean() / (l2[0].mean() * l2[8].mean()), rel=1e-13)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ar1_speckle_follows_the_closed_form(seed):
    res = model_multi_tau(ar1_stack(seed, T=1024, H=32, W=48))
    assert len(res["lags"]) == 64
    want = ar1_closed_form(res["lags"], res["level"])
    assert want[0] == pytest.approx(2.0) and want[1] == pytest.approx(1.0 + RHO ** 2)
    err = float(np.max(np.abs(res["g2"] - want)))
    print(f"multi_tau.model.ar1.seed{seed}: |g2 - closed form| {err:.4f}")
    assert err <= AR1_BAR
    decay = float(tt.correlation_decay(res))
    assert abs(decay - float(tt.correlation_decay(want, lags=res["lags"], baseline=1.0))) <= DECAY_BAR


def test_nan_rules_and_regions():
    s, lab = zero_region_case()
    res = model_multi_tau(s, labels=lab)
    assert np.isfinite(res["g2"][0]).all() and np.isnan(res["g2"][1]).all() and np.isnan(res["g2_err"][1]).all()
    assert res["mean"][1] == 0.0 and res["n_pixels"].tolist() == [8 * 24, 8 * 24]
    s = speckle_stack(9, 16, 24, seed=2)
    s[2, 3, 4], s[8, 0, 0] = np.nan, np.inf
    lab = np.zeros((16, 24), int)
    lab[:8] = 2
    res = model_multi_tau(s, labels=lab, lags_per_level=8)
    assert res["n_pixels"].tolist() == [0, 8 * 24 - 2] and np.isnan(res["g2"][0]).all() and np.isnan(res["mean"][0])
    alone = model_multi_tau(s, mask=lab == 2, lags_per_level=8)
    assert np.array_equal(alone["g2"], res["g2"][1]) and np.array_equal(alone["g2_err"], res["g2_err"][1])


# ---------------------------------------------------------------- correlation_decay on a lag axis
def test_correlation_decay_with_lags():
    tau_c = 37.3
    lags, level, _, _ = mt.lag_table(4096, 16)
    g2 = 1.0 + 0.4 * np.exp(-lags / tau_c)
    k = int(np.flatnonzero(np.exp(-lags / tau_c) < np.exp(-1.0))[0])
    g = np.exp(-lags / tau_c)
    want = lags[k - 1] + (g[k - 1] - np.exp(-1.0)) / (g[k - 1] - g[k]) * (lags[k] - lags[k - 1])
    assert lags[k] - lags[k - 1] > 1                                  # the crossing lies on the coarse part of the axis
    got = float(tt.correlation_decay(g2, lags=lags, baseline=1.0))
    assert got == pytest.approx(want, abs=1e-9) and abs(got - tau_c) < 0.2
    res = {"g2": np.stack([g2, 1.0 + 0.1 * np.exp(-lags / 3.0)]), "lags": lags, "meta": {"lags_per_level": 16}}
    both = tt.correlation_decay(res)                                  # baseline 1 and the dict's lags by default
    assert both.shape == (2,) and both[0] == pytest.approx(want, abs=1e-9) and 2.9 < both[1] < 3.1
    with pytest.raises(ValueError):
        tt.correlation_decay(g2, lags=lags[:-1])


def test_correlation_decay_is_unchanged_on_arange():
    rng = np.random.default_rng(8)
    for _ in range(50):
        n = int(rng.integers(2, 40))
        g2 = np.sort(rng.random(n))[::-1] * rng.random() + rng.random((3, 1))
        level = float(rng.random())
        for row in g2:
            g = row / row[0]
            below = np.flatnonzero(g < level)
            want = np.nan if below.size == 0 else 0.0 if below[0] == 0 else (
                (below[0] - 1) + (g[below[0] - 1] - level) / (g[below[0] - 1] - g[below[0]]))
            a = tt.correlation_decay(row, level=level)
            b = tt.correlation_decay(row, level=level, lags=np.arange(n))
            c = tt.correlation_decay({"g2": row, "lags": np.arange(n), "meta": {"norm": "pearson"}}, level=level)
            assert np.array_equal(a, want, equal_nan=True) and np.array_equal(b, want, equal_nan=True)     # bit for bit
            assert np.array_equal(c, want, equal_nan=True)


# ---------------------------------------------------------------- argument errors come before the GPU
@pytest.fixture
def no_gpu(monkeypatch):
    def boom():
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_ffi, "require_gpu", boom)


def test_argument_errors_come_first(no_gpu):
    s = np.zeros((4, 8, 10), np.float32)
    lab = np.ones((8, 10), np.int32)
    bad = [
        dict(images=np.zeros((8, 10))),                             # not a stack
        dict(images=np.zeros((4, 8, 10, 2))),
        dict(images=np.zeros((4, 0, 10))),
        dict(images=np.zeros((1, 8, 10))),                          # T < 2
        dict(images=s, labels=lab, mask=lab > 0),                   # both
        dict(images=s, labels=-lab),                                # negative labels
        dict(images=s, labels=np.ones((8, 11), np.int32)),          # another shape
        dict(images=s, labels=lab.astype(np.float32)),              # not an integer map
        dict(images=s, labels=np.zeros((8, 10), np.int32)),         # no region
        dict(images=s, mask=np.ones((10, 8), bool)),
        dict(images=s, lags_per_level=12), dict(images=s, lags_per_level=64), dict(images=s, lags_per_level=16.5),
        dict(images=s, max_level=-1), dict(images=s, max_level=1.5),
        dict(images=s, chunk_frames=0), dict(images=s, chunk_frames=2.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            mt.multi_tau_correlation(**kw)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (2 ** 31 - 1, 2, 2), (0, 0, 0))
    for kw in (dict(images=s, labels=lab * 65), dict(images=s.astype(np.complex64)), dict(images=big, lags_per_level=8)):
        with pytest.raises(NotImplementedError):
            mt.multi_tau_correlation(**kw)
    with pytest.raises(AssertionError, match="GPU was touched"):     # valid arguments do reach the device
        mt.multi_tau_correlation(s, labels=lab, max_level=0, chunk_frames=3)


def test_library_limits_without_a_gpu():
    lib = _ffi.load_library()
    ws = lib.b4d_multi_tau_workspace_bytes
    assert ws(512 * 512, 1, 16, 8, 256) > 4 * 512 * 512 * (8 * 16 + 128 + 64)     # rings and the two scratch buffers
    assert ws(512 * 512, 1, 16, 1, 256) < 4 * 512 * 512 * 16 * 1.3                # one level: no scratch
    for npix, R, m, L, push in ((0, 1, 16, 3, 8), (2 ** 31, 1, 16, 3, 8), (100, 0, 16, 3, 8), (100, 65, 16, 3, 8), (100, 1, 12, 3, 8),
                                (100, 1, 16, 0, 8), (100, 1, 16, 25, 8), (100, 1, 16, 3, 0)):
        assert ws(npix, R, m, L, push) == 0
    assert lib.b4d_multi_tau_scan(None, 4, 100, None, None) == -1
    assert lib.b4d_multi_tau_init(None, None, 100, 1, 16, 3, 8, None, None) == -1
    assert lib.b4d_multi_tau_push(None, 0, 4, 100, 1, 16, 3, 8, None, None) == -1
    assert lib.b4d_multi_tau_finish(37, 100, 1, 16, 3, 8, None, None, None, None, None, None) == -1
    assert mt.LAGS_PER_LEVEL == (8, 16, 32) and mt.MAX_REGIONS == 64 and mt.MAX_LEVELS == 24
