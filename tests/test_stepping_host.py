"""CPU tier of the phase-stepping analysis: the float64 model (tests/stepping_model.py) against closed forms, and the host-side
argument checks of barc4dip_amd.signal.stepping, which must raise before the GPU or the library is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stepping_model as sm  # noqa: E402


def _synthetic(T, steps, K, shape=(6, 7), seed=3):
    """Noise-free float64 fringes with known (a0, a_k, phi_k)."""
    rng = np.random.default_rng(seed)
    a0 = rng.uniform(500.0, 1500.0, shape)
    amp = np.stack([a0 * rng.uniform(0.1, 0.4, shape) / (k + 1) for k in range(K)])
    ph = rng.uniform(-3.1, 3.1, (K,) + shape)
    p = np.asarray(steps)[:, None, None]
    I = a0 + sum(amp[k] * np.cos((k + 1) * p + ph[k]) for k in range(K))
    return I, a0, amp, ph


@pytest.mark.parametrize("T,periods", [(3, 1.0), (5, 1.0), (8, 2.0), (16, 3.0), (64, 5.0)])
def test_uniform_steps_equal_the_fft_bin(T, periods):
    rng = np.random.default_rng(T)
    I = rng.uniform(100.0, 2000.0, (T, 5, 9))
    f = sm.fit(I, sm.uniform_steps(T, periods), K=1)
    F = np.fft.fft(I, axis=0)
    b = int(periods)
    scale = np.max(np.abs(I))
    assert np.max(np.abs(f["mean"] - F[0].real / T)) <= 1e-12 * scale
    # I_t = a0 + c cos + s sin with bin b = sum I exp(-i phi): c = 2 Re F_b / T, s = -2 Im F_b / T
    assert np.max(np.abs(f["coeff"][1] - 2.0 * F[b].real / T)) <= 1e-12 * scale
    assert np.max(np.abs(f["coeff"][2] + 2.0 * F[b].imag / T)) <= 1e-12 * scale
    assert np.max(np.abs(sm.wrap(f["phase"][0] - np.angle(F[b])))) <= 1e-12 * scale / np.min(f["amplitude"])
    assert f["valid"].all() and (f["n_samples"] == T).all()


@pytest.mark.parametrize("K,T", [(1, 4), (1, 7), (2, 5), (2, 9)])
def test_known_fringes_are_recovered_with_non_uniform_steps(K, T):
    rng = np.random.default_rng(10 * K + T)
    steps = sm.uniform_steps(T) + rng.uniform(-0.2, 0.2, T)
    I, a0, amp, ph = _synthetic(T, steps, K)
    f = sm.fit(I, steps, K=K)
    assert np.max(np.abs(f["mean"] / a0 - 1.0)) <= 1e-10
    assert np.max(np.abs(f["amplitude"] / amp - 1.0)) <= 1e-10
    assert np.max(np.abs(sm.wrap(f["phase"] - ph))) <= 1e-10
    assert np.max(f["residual"] / a0) <= 1e-6     # sqrt of a cancelling float64 sum: 1e-16^(1/2) of the level at most


def test_dropped_samples():
    T = 5
    steps = sm.uniform_steps(T)
    B = sm.basis(steps, 1)
    one = np.delete(B, 2, axis=0)
    two = np.delete(B, [2, 3], axis=0)
    assert abs(np.linalg.cond(one.T @ one) - 3.8) < 0.05
    assert abs(np.linalg.cond(two.T @ two) - 16.0) < 0.5
    I, a0, amp, ph = _synthetic(T, steps, 1, shape=(1, 6))
    sat = 1.0e6
    I[2, 0, 1] = 2.0e6                      # one saturated sample
    I[2, 0, 2] = I[3, 0, 2] = 2.0e6         # two adjacent
    I[1, 0, 3] = I[2, 0, 3] = I[4, 0, 3] = 2.0e6   # three: M - 1 = 2 kept
    I[0, 0, 4] = np.nan                     # a NaN is a drop
    I[4, 0, 5] = np.inf
    f = sm.fit(I, steps, K=1, saturation=sat)
    assert f["n_samples"][0].tolist() == [5, 4, 3, 2, 4, 4]
    assert f["valid"][0].tolist() == [True, True, True, False, True, True]
    ok = f["valid"][0]
    assert np.max(np.abs(f["mean"][0][ok] / a0[0][ok] - 1.0)) <= 1e-10
    assert np.max(np.abs(sm.wrap(f["phase"][0, 0][ok] - ph[0, 0][ok]))) <= 1e-10
    for key in ("mean", "residual"):
        assert np.isnan(f[key][0, 3])
    assert np.isnan(f["amplitude"][0, 0, 3]) and np.isnan(f["phase"][0, 0, 3]) and np.isnan(f["coeff"][:, 0, 3]).all()
    # without a saturation level the large finite value is kept (and spoils the fit, but the pixel is valid)
    g = sm.fit(np.nan_to_num(I, nan=1.0, posinf=1.0), steps, K=1)
    assert (g["n_samples"] == 5).all() and g["valid"].all()
    # T = M with one drop: M - 1 kept samples, invalid
    h = sm.fit(I[:3], sm.uniform_steps(3), K=1, saturation=sat)
    assert not h["valid"][0, 1] and h["valid"][0, 0]


def test_compare_formulas():
    T = 6
    steps = sm.uniform_steps(T)
    Is, a0s, amps, phs = _synthetic(T, steps, 2, seed=1)
    Ir, a0r, ampr, phr = _synthetic(T, steps, 2, seed=2)
    c = sm.compare(sm.fit(Is, steps, K=2)["coeff"], sm.fit(Ir, steps, K=2)["coeff"])
    assert np.max(np.abs(c["transmission"] / (a0s / a0r) - 1.0)) <= 1e-10
    assert np.max(np.abs(sm.wrap(c["dpc"] - (phs - phr)))) <= 1e-10
    assert np.max(np.abs(c["dark_field"] / ((amps / a0s) / (ampr / a0r)) - 1.0)) <= 1e-10
    assert c["dpc"].max() <= np.pi and c["dpc"].min() > -np.pi and c["valid"].all()
    assert sm.wrap(np.pi) == np.pi and sm.wrap(-np.pi) == np.pi and abs(sm.wrap(np.pi + 1e-9) + np.pi - 1e-9) < 1e-15
    zero = np.zeros((5, 1))
    bad = sm.compare(np.array([[1.0], [0.3], [0.1], [0.0], [0.0]]), zero)
    assert not bad["valid"].any()


@pytest.mark.parametrize("T,shape,seed", [(5, (37, 53), 0), (6, (48, 80), 1), (8, (48, 80), 2), (12, (64, 64), 3)])
def test_calibration_converges(T, shape, seed):
    rng = np.random.default_rng(seed)
    nominal = sm.uniform_steps(T)
    true = nominal.copy()
    true[1:] += rng.uniform(-0.3, 0.3, T - 1)
    I = sm.calibration_fringes(T, shape[0], shape[1], true)[0]
    steps, info = sm.calibrate(I, nominal, tol=1e-9, max_iter=200)
    assert info["converged"] and info["iterations"] <= 200
    assert np.max(np.abs(steps - true)) <= 1e-6
    assert np.max(np.abs(info["dose"] - 1.0)) <= 1e-6
    ref = sm.fit(I, true)["phase"]
    ripple_nominal = np.max(np.abs(sm.wrap(sm.fit(I, nominal)["phase"] - ref)))
    ripple_calibrated = np.max(np.abs(sm.wrap(sm.fit(I, steps)["phase"] - ref)))
    assert ripple_nominal > 0.05
    assert ripple_calibrated < 1e-6


def test_public_functions_raise_before_the_gpu_is_touched(monkeypatch):
    """Every argument error is raised on the host: neither the GPU nor the library is there to be asked."""
    from barc4dip_amd import _ffi, signal

    def absent(*a, **k):
        raise AssertionError("the device or the library was touched before the arguments were checked")

    monkeypatch.setattr(_ffi, "require_gpu", absent)
    monkeypatch.setattr(_ffi, "lib", absent)
    monkeypatch.setattr(_ffi, "load_library", absent)
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    with pytest.raises(ValueError):
        signal.stepping_fit(z(2, 8, 8))                                   # T < 3
    with pytest.raises(NotImplementedError):
        signal.stepping_fit(z(65, 4, 4))                                  # T > 64
    with pytest.raises(ValueError):
        signal.stepping_fit(z(4, 8, 8), harmonics=2)                      # T < 2K + 1
    for h in (0, 3, 1.5, True, "1"):
        with pytest.raises(ValueError):
            signal.stepping_fit(z(8, 8, 8), harmonics=h)
    with pytest.raises(ValueError):
        signal.stepping_fit(z(5, 8, 8), steps=np.zeros(4))                # wrong length
    with pytest.raises(ValueError):
        signal.stepping_fit(z(5, 8, 8), steps=[0.0, 1.0, np.nan, 3.0, 4.0])
    with pytest.raises(ValueError):
        signal.stepping_fit(z(5, 8, 8), steps=[0.0, 1.0, np.inf, 3.0, 4.0])
    with pytest.raises(ValueError):
        signal.stepping_fit(z(8, 8))                                      # not a scan
    with pytest.raises(ValueError):
        signal.calibrate_steps(z(4, 8, 8))                                # calibration with T < 5
    with pytest.raises(NotImplementedError):
        signal.calibrate_steps(z(33, 8, 8))
    with pytest.raises(ValueError):
        signal.phase_stepping(z(4, 8, 8), z(4, 8, 8), calibrate=True)
    with pytest.raises(ValueError):
        signal.phase_stepping(z(5, 8, 8), z(5, 8, 9))                     # frames of different shape
    with pytest.raises(ValueError):
        signal.phase_stepping(z(5, 8, 8), z(6, 8, 8))
    with pytest.raises(ValueError):
        signal.phase_stepping(z(5, 8, 8), z(2, 5, 8, 8))                  # a paired reference needs paired samples
    with pytest.raises(ValueError):
        signal.phase_stepping(z(2, 8, 8), z(2, 8, 8))
    with pytest.raises(NotImplementedError):
        signal.phase_stepping(z(5, 2, 2049), z(5, 2, 2049), unwrap=True)  # the size limit of phase_unwrap
    with pytest.raises(ValueError):
        signal.phase_stepping(z(5, 8, 8), z(5, 8, 8), period=-1.0)


def test_no_host_fallback_without_a_gpu():
    import torch

    from barc4dip_amd import _ffi, signal

    if not torch.cuda.is_available():
        for fn in (lambda: signal.stepping_fit(np.ones((5, 8, 8), np.float32)),
                   lambda: signal.calibrate_steps(np.ones((5, 8, 8), np.float32)),
                   lambda: signal.phase_stepping(np.ones((5, 8, 8), np.float32), np.ones((5, 8, 8), np.float32))):
            with pytest.raises(_ffi.B4DUnavailable):
                fn()


def test_stepping_displacement_layout():
    from barc4dip_amd.signal import stepping_displacement
    from barc4dip_amd.signal.wavefront import _parse_displacement

    H, W, K = 12, 17, 1
    def result(seed):
        r = np.random.default_rng(seed)
        return {"dpc": r.uniform(-1, 1, (K, H, W)), "valid": r.uniform(size=(H, W)) > 0.1, "visibility": r.uniform(0.1, 0.5, (K, H, W)),
                "transmission": r.uniform(0.5, 1.0, (H, W)), "dark_field": r.uniform(0.5, 1.0, (K, H, W))}

    sx, sy = result(1), result(2)
    m = stepping_displacement(sx, sy, period=8.0)
    assert m["dy"].shape == m["dx"].shape == m["peak"].shape == m["valid"].shape == m["transmission"].shape == (H, W)
    assert m["dark_field"].shape == (2, H, W) and m["dy"].dtype == np.float64
    assert np.array_equal(m["y"], np.arange(H)) and np.array_equal(m["x"], np.arange(W))
    assert np.allclose(m["dx"], sx["dpc"][0] * 8.0 / (2 * np.pi), rtol=0, atol=1e-15)
    assert np.allclose(m["dy"], sy["dpc"][0] * 8.0 / (2 * np.pi), rtol=0, atol=1e-15)
    assert np.array_equal(m["peak"], np.minimum(sx["visibility"][0], sy["visibility"][0]))
    assert np.array_equal(m["valid"], sx["valid"] & sy["valid"])
    assert np.array_equal(m["transmission"], 0.5 * (sx["transmission"] + sy["transmission"]))
    dy, dx, shape, y, x, step_y, step_x = _parse_displacement(m)
    assert tuple(shape[-2:]) == (H, W) and step_y == 1.0 and step_x == 1.0 and y.shape == (H,) and x.shape == (W,)
    m2 = stepping_displacement(sx, sy, period=(6.0, 8.0))
    assert np.allclose(m2["dy"], sy["dpc"][0] * 6.0 / (2 * np.pi), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        stepping_displacement(sx, {"dpc": sy["dpc"]}, period=8.0)
    with pytest.raises(ValueError):
        stepping_displacement(sx, sy, period=0.0)
