"""CPU tier of the two-time correlation: a float64 NumPy model of the definitions in include/b4d.h (b4d_two_time), checked against
closed forms, plus the host-side pieces of barc4dip_amd.metrics.twotime (argument checks, correlation_decay).  The GPU tier
(test_gpu_two_time.py) imports the model, the case builders and the deviation measure from here."""
import numpy as np
import pytest

from barc4dip_amd import _ffi
from barc4dip_amd.metrics import twotime as tt

NORMS = ("pearson", "intensity", "covariance")
RHO = 0.9


# ---------------------------------------------------------------- the model
def _norm_matrix(cov, m, var, norm):
    with np.errstate(invalid="ignore", divide="ignore"):
        if norm == "covariance":
            return cov.copy()
        if norm == "pearson":
            den = var[:, None] * var[None, :]
            ok = (var[:, None] > 0) & (var[None, :] > 0)
            C = np.where(ok, cov / np.sqrt(np.where(ok, den, 1.0)), np.nan)
            C[np.diag(var > 0)] = 1.0
            return C
        den = m[:, None] * m[None, :]
        return np.where(den > 0, 1.0 + cov / np.where(den > 0, den, 1.0), np.nan)


def model_lags(C, L):
    T = C.shape[0]
    g2, err = np.empty(L + 1), np.empty(L + 1)
    for tau in range(L + 1):
        d = np.diagonal(C, tau)
        g2[tau] = d.mean()
        err[tau] = d.std() / np.sqrt(T - tau)
    return g2, err


def model_two_time(images, labels=None, mask=None, norm="pearson", max_lag=None):
    """The definitions in float64.  Frames are cast to float32 first: that is what the device sees."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(images).astype(np.float32).astype(np.float64)
    T, H, W = x.shape
    L = T - 1 if max_lag is None else int(max_lag)
    if labels is not None:
        lab, R = np.asarray(labels), int(np.max(labels))
    else:
        lab, R = (np.ones((H, W), int) if mask is None else np.asarray(mask).astype(int)), 1
    fin = np.isfinite(x).all(axis=0)
    out = {k: [] for k in ("two_time", "mean", "var", "contrast", "n_pixels", "g2", "g2_err")}
    band = np.abs(np.subtract.outer(np.arange(T), np.arange(T))) <= L
    for r in range(1, R + 1):
        sel = (lab == r) & fin
        N = int(sel.sum())
        if N == 0:
            cov, m = np.full((T, T), np.nan), np.full(T, np.nan)
        else:
            d = x[:, sel]
            m = d.mean(axis=1)
            dc = d - m[:, None]
            cov = dc @ dc.T / N
            cov = np.triu(cov) + np.triu(cov, 1).T
        var = np.diagonal(cov).copy()
        C = np.where(band, _norm_matrix(cov, m, var, norm), np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            contrast = np.where((var > 0) & (m > 0), np.sqrt(np.where(var > 0, var, np.nan)) / m, np.nan)
            g2, err = model_lags(C, L)
        for k, v in zip(out, (C, m, var, contrast, N, g2, err)):
            out[k].append(v)
    res = {k: np.array(v) for k, v in out.items()}
    res["n_pixels"] = res["n_pixels"].astype(np.int64)
    if labels is None:
        res = {k: v[0] for k, v in res.items()}
    res["lags"] = np.arange(L + 1)
    res["meta"] = {"norm": norm, "max_lag": L, "n_regions": R}
    return res


def deviation(got, want, norm):
    """Largest deviation of `got` from the model result `want` in Pearson units: |d cov_ij| / sqrt(var_i var_j), |d m_i| / sqrt(var_i),
    |d var_i| / var_i, and g2 / g2_err on the scale of their diagonal.  NaNs must sit in the same places; where the scale is not
    finite (a frame without variance) the values must be equal."""
    def one(g, w, scale):
        g, w, scale = np.broadcast_arrays(np.asarray(g, float), np.asarray(w, float), np.asarray(scale, float))
        assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN entries differ from the model's"
        live = ~np.isnan(w)
        exact = live & ~np.isfinite(scale)
        assert np.array_equal(g[exact], w[exact]), "entries of a frame without variance differ from the model's"
        rel = live & np.isfinite(scale)
        return float(np.max(np.abs(g[rel] - w[rel]) * scale[rel])) if rel.any() else 0.0

    worst = 0.0
    two = np.asarray(want["two_time"])
    lead = two.ndim == 3
    for r in range(two.shape[0] if lead else 1):
        pick = (lambda k, src: np.asarray(src[k])[r]) if lead else (lambda k, src: np.asarray(src[k]))
        m, var = pick("mean", want), pick("var", want)
        with np.errstate(invalid="ignore", divide="ignore"):
            sd = np.sqrt(np.where(var > 0, var, np.nan))
            pear = 1.0 / (sd[:, None] * sd[None, :])
            scale = {"covariance": pear, "pearson": np.ones_like(pear), "intensity": np.abs(m[:, None] * m[None, :]) * pear}[norm]
            scale = np.where(np.isnan(scale), np.inf, scale)
            worst = max(worst, one(pick("two_time", got), pick("two_time", want), scale))
            worst = max(worst, one(pick("mean", got), m, np.where(np.isnan(sd), np.inf, 1.0 / sd)))
            worst = max(worst, one(pick("var", got), var, np.where(var > 0, 1.0 / np.where(var > 0, var, 1.0), np.inf)))
            # a mean moves by at most the mean of its entries' errors, a standard deviation by at most their rms: with entry
            # errors of eps / scale_ij the diagonal's g2 is good to eps mean(1 / scale), g2_err to eps rms(1 / scale) / sqrt(n)
            L = len(pick("g2", want)) - 1
            inv = [1.0 / np.diagonal(scale, t) for t in range(L + 1)]
            s_g2 = np.array([1.0 / v.mean() if v.mean() > 0 else np.inf for v in inv])
            s_err = np.array([np.sqrt(len(v) / np.mean(v * v)) if v.any() else np.inf for v in inv])
        worst = max(worst, one(pick("g2", got), pick("g2", want), s_g2))
        worst = max(worst, one(pick("g2_err", got), pick("g2_err", want), s_err))
    assert np.array_equal(np.asarray(got["n_pixels"]), np.asarray(want["n_pixels"]))
    return worst


# ---------------------------------------------------------------- case builders (shared with the GPU tier)
def speckle_stack(T, H, W, seed, rho=0.95):
    """Fully developed speckle whose field keeps a correlation rho from frame to frame."""
    return ar1_stack(seed, T=T, H=H, W=W, rho=rho).astype(np.float32)


def ar1_stack(seed, T=40, H=64, W=96, rho=RHO):
    """E_t = rho E_{t-1} + sqrt(1 - rho^2) N_t with unit complex Gaussian N, I = 100 |E|^2: Pearson(I_t, I_{t+tau}) = rho^(2 tau)."""
    rng = np.random.default_rng(seed)
    noise = lambda: (rng.standard_normal((H, W)) + 1j * rng.standard_normal((H, W))) / np.sqrt(2.0)  # noqa: E731
    E = noise()
    out = np.empty((T, H, W))
    for t in range(T):
        if t:
            E = rho * E + np.sqrt(1.0 - rho * rho) * noise()
        out[t] = 100.0 * np.abs(E) ** 2
    return out


def low_contrast_stack(T=20, H=64, W=96, seed=5):
    """Detector words: 30 000 counts, 1 % contrast, a common pattern under per-frame noise."""
    rng = np.random.default_rng(seed)
    z0 = rng.standard_normal((H, W))
    return np.rint(30000.0 + 300.0 * (0.8 * z0 + 0.6 * rng.standard_normal((T, H, W)))).astype(np.uint16)


def ring_labels(H=256, W=320):
    """Three rings (labels 1, 2, 4) around the centre and an unlabelled rest; label 3 is absent, so R = 4 with an empty region."""
    y, x = np.mgrid[:H, :W]
    rad = np.hypot(y - (H - 1) / 2.0, x - (W - 1) / 2.0)
    lab = np.zeros((H, W), np.int32)
    lab[rad < 60] = 1
    lab[(rad >= 60) & (rad < 100)] = 2
    lab[(rad >= 100) & (rad < 125)] = 4
    return lab


def degenerate_stack():
    """Case a (T = 5, 37 x 53) with frame 1 constant and frame 3 of mean exactly 0."""
    s = speckle_stack(5, 37, 53, seed=11)
    s[1] = 7.0
    n = 37 * 53
    s[3] = np.random.default_rng(3).permutation(np.arange(n) - (n - 1) // 2).reshape(37, 53)
    return s


def with_bad_entries(stack, seed=9, fraction=0.01):
    rng = np.random.default_rng(seed)
    out = np.array(stack, dtype=np.float32)
    hit = rng.random(out.shape) < fraction
    out[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=int(hit.sum()))
    return out


# ---------------------------------------------------------------- the model against closed forms
def test_affine_copy_has_pearson_one():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 1000, (1, 16, 24)).astype(np.float64)
    res = model_two_time(np.concatenate([x, 2.0 * x + 3.0]))
    assert np.allclose(res["two_time"], 1.0, atol=1e-13)
    assert res["two_time"][0, 0] == 1.0 and res["two_time"][1, 1] == 1.0
    assert res["n_pixels"] == 16 * 24
    res = model_two_time(np.concatenate([x, 2.0 * x + 3.0]), norm="covariance")
    assert np.isclose(res["two_time"][0, 1], 2.0 * x.var(), rtol=1e-12) and np.isclose(res["var"][1], 4.0 * x.var(), rtol=1e-12)
    res = model_two_time(np.concatenate([x, 2.0 * x + 3.0]), norm="intensity")
    assert np.isclose(res["two_time"][0, 1], 1.0 + 2.0 * x.var() / (x.mean() * (2.0 * x.mean() + 3.0)), rtol=1e-12)


def test_independent_frames_decorrelate():
    rng = np.random.default_rng(1)
    res = model_two_time(rng.standard_normal((6, 64, 96)))
    off = res["two_time"][~np.eye(6, dtype=bool)]
    assert np.max(np.abs(off)) < 5.0 / np.sqrt(64 * 96)
    assert np.all(np.abs(res["g2"][1:]) < 5.0 / np.sqrt(64 * 96)) and res["g2"][0] == 1.0 and res["g2_err"][0] == 0.0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ar1_speckle_follows_rho(seed):
    res = model_two_time(ar1_stack(seed))
    tau = np.arange(13)
    assert np.max(np.abs(res["g2"][:13] - RHO ** (2 * tau))) <= 0.03
    assert abs(float(tt.correlation_decay(res)) - (-1.0 / (2.0 * np.log(RHO)))) <= 0.15
    assert np.allclose(res["contrast"], 1.0, atol=0.05)          # fully developed speckle


@pytest.mark.parametrize("norm", NORMS)
def test_nan_rules(norm):
    res = model_two_time(degenerate_stack(), norm=norm)
    C = res["two_time"]
    nan_rows = {"pearson": [1], "intensity": [3], "covariance": []}[norm]
    for i in range(5):
        assert np.isnan(C[i]).all() == (i in nan_rows) and np.isnan(C[:, i]).all() == (i in nan_rows)
    keep = [i for i in range(5) if i not in nan_rows]
    assert np.isfinite(C[np.ix_(keep, keep)]).all()
    assert res["var"][1] == 0.0 and res["mean"][1] == 7.0 and res["mean"][3] == 0.0
    assert np.isnan(res["contrast"][1]) and np.isnan(res["contrast"][3]) and np.isfinite(res["contrast"][[0, 2, 4]]).all()
    if norm == "covariance":
        assert np.all(C[1] == 0.0)
    if norm == "intensity":
        assert np.all(C[1, [0, 1, 2, 4]] == 1.0)


def test_pixels_with_a_bad_frame_and_empty_regions_drop_out():
    s = speckle_stack(6, 16, 24, seed=2)
    s[2, 3, 4], s[5, 0, 0], s[0, 15, 23] = np.nan, np.inf, -np.inf
    res = model_two_time(s)
    assert res["n_pixels"] == 16 * 24 - 3 and np.isfinite(res["two_time"]).all()
    keep = np.ones((16, 24), bool)
    keep[3, 4] = keep[0, 0] = keep[15, 23] = False
    clean = model_two_time(np.where(keep, s, 0.0), mask=keep)
    assert np.array_equal(clean["two_time"], res["two_time"])
    lab = np.zeros((16, 24), int)
    lab[:8] = 2
    res = model_two_time(s, labels=lab)
    assert res["n_pixels"].tolist() == [0, 8 * 24 - 2]
    assert np.isnan(res["two_time"][0]).all() and np.isnan(res["mean"][0]).all() and np.isnan(res["g2"][0]).all()


@pytest.mark.parametrize("norm", NORMS)
def test_symmetry_and_band(norm):
    s = speckle_stack(12, 16, 24, seed=4)
    full, band = model_two_time(s, norm=norm), model_two_time(s, norm=norm, max_lag=4)
    assert np.array_equal(full["two_time"], full["two_time"].T)
    i, j = np.indices((12, 12))
    inside = np.abs(i - j) <= 4
    assert np.isnan(band["two_time"][~inside]).all()
    assert np.array_equal(band["two_time"][inside], full["two_time"][inside])
    assert np.array_equal(band["g2"], full["g2"][:5]) and band["lags"].tolist() == [0, 1, 2, 3, 4]
    d1 = np.diagonal(full["two_time"], 1)
    assert np.isclose(full["g2"][1], d1.mean()) and np.isclose(full["g2_err"][1], d1.std() / np.sqrt(11))


def test_region_alone_equals_region_among_many():
    lab = np.arange(16 * 24).reshape(16, 24) % 3
    s = speckle_stack(7, 16, 24, seed=6)
    many = model_two_time(s, labels=lab)
    alone = model_two_time(s, mask=lab == 2)
    for k in ("two_time", "mean", "var", "contrast", "g2", "g2_err", "n_pixels"):
        assert np.array_equal(many[k][1], alone[k], equal_nan=True), k
    assert many["meta"]["n_regions"] == 2 and alone["meta"]["n_regions"] == 1


# ---------------------------------------------------------------- correlation_decay
def test_correlation_decay_on_an_exponential():
    tau_c = 4.746
    lags = np.arange(30)
    g2 = np.exp(-lags / tau_c)
    got = float(tt.correlation_decay(g2))
    k = 5                                                       # exp(-4 / tau_c) > 1/e > exp(-5 / tau_c)
    want = (k - 1) + (g2[k - 1] - np.exp(-1.0)) / (g2[k - 1] - g2[k])
    assert got == pytest.approx(want, abs=1e-12) and abs(got - tau_c) < 0.02
    # the XPCS form 1 + beta exp(-tau / tau_c) through the dict: baseline 1 by default
    res = {"g2": np.stack([1.0 + 0.3 * g2, 1.0 + 0.1 * np.exp(-lags / 2.0)]), "meta": {"norm": "intensity"}}
    got2 = tt.correlation_decay(res)
    assert got2.shape == (2,) and got2[0] == pytest.approx(want, abs=1e-9) and 1.9 < got2[1] < 2.1
    assert float(tt.correlation_decay(g2, level=0.5)) == pytest.approx(tau_c * np.log(2.0), abs=0.05)   # the chord lies above the curve
    assert np.isnan(tt.correlation_decay(np.ones(8))) and np.isnan(tt.correlation_decay(g2[:3]))
    assert np.isnan(tt.correlation_decay(np.full(6, np.nan)))
    assert float(tt.correlation_decay(0.2 + 0.8 * g2, baseline=0.2)) == pytest.approx(want, abs=1e-9)
    with pytest.raises(ValueError):
        tt.correlation_decay(np.ones((2, 3, 4)))


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
        dict(images=s, norm="g2"),
        dict(images=s, max_lag=4), dict(images=s, max_lag=-1), dict(images=s, max_lag=1.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            tt.two_time_correlation(**kw)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2049, 8, 10), (0, 0, 0))
    for kw in (dict(images=big), dict(images=s, labels=lab * 65), dict(images=s.astype(np.complex64))):
        with pytest.raises(NotImplementedError):
            tt.two_time_correlation(**kw)
    with pytest.raises(AssertionError, match="GPU was touched"):     # valid arguments do reach the device
        tt.two_time_correlation(s, labels=lab, max_lag=3)


def test_library_limits_without_a_gpu():
    lib = _ffi.load_library()
    assert lib.b4d_two_time_workspace_bytes(256, 2048 * 2048, 1, 255) > 4 * 256 * 2048 * 2048
    for T, npix, R, L in ((1, 100, 1, 0), (2049, 100, 1, 5), (8, 100, 65, 5), (8, 2 ** 31, 1, 5), (8, 100, 1, 8), (8, 100, 0, 3)):
        assert lib.b4d_two_time_workspace_bytes(T, npix, R, L) == 0
    assert lib.b4d_two_time_workspace_bytes(300, 1536, 1, 40) < lib.b4d_two_time_workspace_bytes(300, 1536, 1, 299)   # (0, 2) skipped
    assert lib.b4d_two_time(None, 8, 100, None, 1, 0, 7, None, None, None, None, None, None) == -1
    assert lib.b4d_two_time_lags(None, 1, 8, 7, None, None, None) == -1
    assert tt.CHUNK == 2048 and tt.NORMS == {"pearson": 0, "intensity": 1, "covariance": 2}
