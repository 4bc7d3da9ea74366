"""Float64 oracle of the fringe analysis (barc4dip_amd/signal/fringes.py) and its host-side tests: the
oracle against ground truth, ``fringe_grid``, argument errors and the coarse carrier search.  No GPU is needed here;
tests/test_gpu_fringes.py imports the oracle and the cases from this file.

The oracle is the definition itself: ``S_f = A_y . I . A_x^T`` with the banded complex matrices ``A_y (gy x H)``, ``A_x (gx x W)``
of the half-sample Hann taper times the phasor in absolute pixel coordinates, the comparison formulas, and the least-squares
unwrap with its congruence step (dense DCT-II matrices).  Every truth bar below is twice what this oracle gives on the case, the
observed value next to it."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from barc4dip_amd import synth
from barc4dip_amd.signal import fringes

CARRIERS = np.array([[0.004, 0.127], [0.123, -0.006]])
CARRIERS_B = np.array([[0.01, 0.19], [0.21, -0.013]])


# ---- the oracle
def hann(w: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(w) + 0.5) / w)


def band_matrix(n: int, w: int, st: int, f: float) -> np.ndarray:
    """A (g x n): row k holds h_w[j] exp(-2 pi i f (k st + j)) / sum h_w at column k st + j."""
    g = (n - w) // st + 1
    A = np.zeros((g, n), dtype=np.complex128)
    h = hann(w)
    for k in range(g):
        c = k * st + np.arange(w)
        A[k, c] = h * np.exp(-2j * np.pi * f * c) / h.sum()
    return A


def demodulate(frame, carriers, window, step) -> np.ndarray:
    """(K + 1, gy, gx) complex128: plane 0 is S_0, plane k + 1 the harmonic map of carrier k."""
    I = np.asarray(frame, dtype=np.float64)
    (wy, wx), (sty, stx) = window, step
    out = [band_matrix(I.shape[0], wy, sty, 0.0) @ I @ band_matrix(I.shape[1], wx, stx, 0.0).T]
    for fy, fx in np.atleast_2d(carriers):
        out.append(band_matrix(I.shape[0], wy, sty, fy) @ I @ band_matrix(I.shape[1], wx, stx, fx).T)
    return np.stack(out)


def _dct(n: int):
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    C = np.sqrt(2.0 / n) * np.cos(np.pi * (2 * j + 1) * k / (2.0 * n))
    C[0] *= np.sqrt(0.5)
    return C, 4.0 * np.sin(np.pi * np.arange(n) / (2.0 * n)) ** 2


def wrap(a):
    return a - 2.0 * np.pi * np.round(a / (2.0 * np.pi))


def unwrap(phase):
    """(unwrapped map, integer levels, margin): margin is the largest distance of (p - phase) / 2 pi from an integer."""
    ph = np.asarray(phase, dtype=np.float64)
    ny, nx = ph.shape
    sy, sx = wrap(np.diff(ph, axis=0)), wrap(np.diff(ph, axis=1))
    r = np.zeros_like(ph)
    r[1:] += sy
    r[:-1] -= sy
    r[:, 1:] += sx
    r[:, :-1] -= sx
    (Cy, ly), (Cx, lx) = _dct(ny), _dct(nx)
    lam = ly[:, None] + lx[None, :]
    lam[0, 0] = 1.0
    P = (Cy @ r @ Cx.T) / lam
    P[0, 0] = 0.0
    p = Cy.T @ P @ Cx
    p += ph[ny // 2, nx // 2] - p[ny // 2, nx // 2]
    q = (p - ph) / (2.0 * np.pi)
    k = np.round(q)
    return ph + 2.0 * np.pi * k, k.astype(np.int64), float(np.max(np.abs(q - k)))


def analyse(reference, frame, carriers, window, step, do_unwrap=True) -> dict:
    """The whole definition for one frame (reference None: absolute mode)."""
    M = np.asarray(carriers, dtype=np.float64)
    S = demodulate(frame, M, window, step)
    res = {"S": S, "visibility": 2.0 * np.abs(S[1:]) / S[0].real}
    if reference is None:
        phase = np.angle(S[1:])
    else:
        R = demodulate(reference, M, window, step)
        phase = np.angle(S[1:] * np.conj(R[1:]))
        res["R"] = R
        res["transmission"] = S[0].real / R[0].real
        res["dark_field"] = (np.abs(S[1:]) / S[0].real) / (np.abs(R[1:]) / R[0].real)
    phase = np.where(phase <= -np.pi, np.pi, phase)
    res["wrapped"] = phase
    res["levels"], res["margin"] = None, 0.0
    if do_unwrap:
        un = [unwrap(p) for p in phase]
        phase = np.stack([u[0] for u in un])
        res["levels"] = np.stack([u[1] for u in un])
        res["margin"] = max(u[2] for u in un)
    d = -np.tensordot(np.linalg.inv(M), phase, axes=(1, 0)) / (2.0 * np.pi)
    res.update(phase=phase, dy=d[0], dx=d[1], peak=np.min(res["visibility"], axis=0))
    return res


def psd_shifted(frame) -> np.ndarray:
    return np.abs(np.fft.fftshift(np.fft.fft2(np.asarray(frame, dtype=np.float64)))) ** 2


def estimate_carriers(frame, window, step, *, f_min=0.02, min_angle=30.0, refine=1) -> np.ndarray:
    """fringe_carriers in float64: the product's coarse search on the NumPy power spectrum, the refinement through the oracle."""
    g = fringes.fringe_grid(np.shape(frame), window=window, step=step)
    f = fringes.coarse_carriers(psd_shifted(frame), f_min=f_min, min_angle=min_angle)
    gy, gx = g["shape"]
    yc, xc = g["y"] - g["y"].mean(), g["x"] - g["x"].mean()
    A = np.stack([np.ones((gy, gx)), np.broadcast_to(yc[:, None], (gy, gx)), np.broadcast_to(xc[None, :], (gy, gx))], axis=-1).reshape(-1, 3)
    for _ in range(refine):
        S = demodulate(frame, f, g["window"], g["step"])
        for k in range(2):
            c = np.linalg.lstsq(A, unwrap(np.angle(S[k + 1]))[0].ravel(), rcond=None)[0]
            f[k] = fringes._representative(f[k] + c[1:] / (2.0 * np.pi))
    return f


# ---- the cases: name -> (shape, window, step, carriers, displacement, sample visibility, envelope, Poisson mean or None)
def smooth_shift(shape):
    H, W = shape
    return lambda y, x: (0.8 * np.sin(2.0 * np.pi * (0.6 * y / H + 0.3 * x / W) + 0.4) * np.cos(1.3 * x / W),
                         0.8 * np.cos(2.0 * np.pi * (0.35 * y / H - 0.5 * x / W) + 1.1) * np.cos(0.9 * y / H))


def sheared_shift(shape):
    cy, cx = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    return lambda y, x: (0.025 * (y - cy) + 0.3 * np.sin(x / 40.0), 0.03 * (x - cx) + 0.4 * np.cos(y / 50.0))


def magnification(shape, my=0.03, mx=0.025):
    cy, cx = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    return lambda y, x: (my * (y - cy) + 0.0 * x, mx * (x - cx) + 0.0 * y)


def gaussian_envelope(shape):
    cy, cx = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    s2 = (cy * cy + cx * cx) / (-np.log(0.6))          # 1.0 at the centre, 0.6 in the corners
    return lambda y, x: np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / s2)


CASES = {
    "a_256_w32": ((256, 256), (32, 32), (16, 16), CARRIERS, smooth_shift, 0.4, None, None),
    "b_192x160_w24x40": ((192, 160), (24, 40), (12, 8), CARRIERS_B, smooth_shift, 0.4, None, None),
    "c_256_w16": ((256, 256), (16, 16), (8, 8), CARRIERS, smooth_shift, 0.4, None, None),
    "d_256x320_sheared": ((256, 320), (32, 32), (16, 16), CARRIERS, sheared_shift, 0.3, gaussian_envelope, None),
    "e_256_poisson": ((256, 256), (32, 32), (16, 16), CARRIERS, smooth_shift, 0.4, None, 2000.0),
    "m_256_magnified": ((256, 256), (32, 32), (16, 16), CARRIERS, magnification, 0.4, None, None),
}
# largest |dy|, |dx| error in pixels against the true field at the window centres: (bar, bar) = 2 x the observed (dy, dx)
TRUTH_BARS = {
    "a_256_w32": (1.52e-2, 1.30e-2),
    "b_192x160_w24x40": (1.57e-2, 2.36e-2),
    "c_256_w16": (4.24e-2, 3.66e-2),
    "d_256x320_sheared": (4.32e-2, 4.06e-2),
    "e_256_poisson": (4.20e-2, 4.07e-2),
    "m_256_magnified": (2.78e-2, 2.41e-2),
}


@functools.lru_cache(maxsize=None)
def case_frames(name):
    """(reference, frame) float32, read-only, and the true (uy, ux) at the window centres."""
    shape, window, step, carriers, shift, vis, env, counts = CASES[name]
    mean = 1.0 if counts is None else counts
    ref = synth.fringe_frame(shape, carriers, visibility=0.4, mean=mean, seed=None if counts is None else 11)
    img = synth.fringe_frame(shape, carriers, shift(shape), visibility=vis, envelope=None if env is None else env(shape), mean=mean,
                             seed=None if counts is None else 12)
    ref, img = ref.astype(np.float32), img.astype(np.float32)
    g = fringes.fringe_grid(shape, window=window, step=step)
    uy, ux = shift(shape)(g["y"][:, None], g["x"][None, :])
    for a in (ref, img):
        a.setflags(write=False)
    return ref, img, np.broadcast_to(uy, g["shape"]), np.broadcast_to(ux, g["shape"])


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    shape, window, step, carriers, *_ = CASES[name]
    ref, img, _, _ = case_frames(name)
    return analyse(ref, img, carriers, window, step)


# ---- tests
def test_band_matrices_are_the_definition():
    """One node of S_f summed term by term, absolute coordinates in the phase; S_0 is real and equals the weighted mean."""
    rng = np.random.default_rng(3)
    I = rng.random((40, 52))
    S = demodulate(I, [[0.11, -0.07]], (16, 24), (8, 12))
    assert S.shape == (2, 4, 3)
    Y, X, y0, x0 = 2, 1, 16, 12
    hy, hx = hann(16), hann(24)
    acc = 0.0
    for j in range(16):
        for i in range(24):
            acc += hy[j] * hx[i] * I[y0 + j, x0 + i] * np.exp(-2j * np.pi * (0.11 * (y0 + j) - 0.07 * (x0 + i)))
    assert abs(S[1, Y, X] - acc / (hy.sum() * hx.sum())) < 1e-15
    assert np.all(S[0].imag == 0.0)
    assert np.all(hann(7) > 0.0) and np.allclose(hann(7), hann(7)[::-1]) and abs(hann(32).sum() - 16.0) < 1e-13


def test_float32_phase_misses_the_amplitude_bar_at_4096_columns():
    """Why the phasor argument is reduced modulo 1 in float64: with the phase 2 pi fx x formed in float32 the harmonic of the
    48 x 4096 case of the device tests is off by 1.03e-4 of max S_0 (observed), above the 1e-5 bar; with the argument reduced
    in float64 and only the reduced turn rounded to float32 it is 6.4e-9 (observed)."""
    fy, fx = 0.005, 0.3317
    y, x = np.arange(48.0)[:, None], np.arange(4096.0)[None, :]
    I = (1.0 + 0.4 * np.cos(2.0 * np.pi * (fy * y + fx * x))).astype(np.float32).astype(np.float64)
    window, step = (16, 64), (16, 32)
    want = demodulate(I, [[fy, fx]], window, step)

    def with_x_phasor(e):      # A_x with the phasor replaced; the taper and the sums stay float64
        Ax = np.abs(band_matrix(4096, 64, 32, 0.0)) * e[None, :]
        return band_matrix(48, 16, 16, fy) @ I @ Ax.T

    ph32 = (np.float32(2.0 * np.pi) * np.float32(fx)) * np.arange(4096, dtype=np.float32)
    assert ph32.dtype == np.float32
    naive = with_x_phasor(np.exp(-1j * ph32.astype(np.float64)))
    turn = fx * np.arange(4096.0)
    turn32 = (turn - np.round(turn)).astype(np.float32).astype(np.float64)
    reduced = with_x_phasor(np.exp(-2j * np.pi * turn32))
    e_naive = float(np.max(np.abs(naive - want[1])) / np.max(want[0].real))
    e_reduced = float(np.max(np.abs(reduced - want[1])) / np.max(want[0].real))
    print(f"fringes.phase32: float32 phase {e_naive:.3e}, reduced in float64 {e_reduced:.3e}")
    assert e_naive > 1e-5 and e_reduced < 1e-6


def test_fringe_grid():
    g = fringes.fringe_grid((100, 131), window=(24, 40), step=(12, 8))
    assert g["shape"] == (7, 12) and g["window"] == (24, 40) and g["step"] == (12, 8)
    np.testing.assert_array_equal(g["y0"], 12 * np.arange(7))
    np.testing.assert_array_equal(g["x"], 8 * np.arange(12) + 19.5)
    assert "search" not in g
    assert fringes.fringe_grid((64, 64), window=64)["shape"] == (1, 1)
    assert fringes.fringe_grid((64, 64))["step"] == (16, 16)
    assert fringes.fringe_grid((64, 64), window=8, step=20)["shape"] == (3, 3)
    with pytest.raises(ValueError):
        fringes.fringe_grid((20, 64), window=32)
    with pytest.raises(ValueError):
        fringes.fringe_grid((64, 64), window=0)
    for w in (1, 257):
        with pytest.raises(NotImplementedError):
            fringes.fringe_grid((512, 512), window=w)


def test_argument_errors_come_before_the_gpu():
    import torch

    from barc4dip_amd import _ffi

    z = np.zeros((64, 64), np.float32)
    f = CARRIERS
    bad = [
        (dict(reference=z, images=np.zeros((64, 65), np.float32), carriers=f), ValueError),          # shapes differ
        (dict(reference=np.zeros((2, 64, 64)), images=z, carriers=f), ValueError),                    # paired reference, single image
        (dict(reference=np.zeros((2, 64, 64)), images=np.zeros((3, 64, 64)), carriers=f), ValueError),
        (dict(reference=z, images=np.zeros((64,)), carriers=f), ValueError),
        (dict(reference=z, images=z, carriers=[[0.0, 0.51], [0.12, 0.0]]), ValueError),               # beyond Nyquist
        (dict(reference=z, images=z, carriers=[[0.4, 0.4], [0.12, 0.0]]), ValueError),                # |f| = 0.57
        (dict(reference=z, images=z, carriers=[[0.0, 0.125], [0.01, 0.125]]), ValueError),            # 4.6 degrees apart
        (dict(reference=z, images=z, carriers=[[0.0, 0.125]]), ValueError),                           # one carrier
        (dict(reference=z, images=z, carriers=[[0.0, 0.06], [0.125, 0.0]]), ValueError),              # 1.92 periods in 32 px
        (dict(reference=z, images=z, carriers=f, window=16), ValueError),                             # 0.127 * 16 = 2.03 ok, 0.123 * 16 < 2
        (dict(reference=z, images=z, carriers=f, window=(32, 0)), ValueError),
        (dict(reference=np.zeros((300, 300)), images=np.zeros((300, 300)), carriers=f, window=257), NotImplementedError),
        (dict(reference=None, images=np.zeros((8, 4200), np.float32), carriers=[[0.0, 0.5], [0.5, 0.0]], window=4, step=2), NotImplementedError),
    ]
    for kw, exc in bad:
        with pytest.raises(exc):
            fringes.fringe_displacement(**kw)
    with pytest.raises(ValueError):
        fringes.fringe_demodulate(z, np.zeros((5, 2)) + 0.1)
    with pytest.raises(ValueError):
        fringes.phase_unwrap(np.zeros(5))
    with pytest.raises(NotImplementedError):
        fringes.phase_unwrap(np.zeros((1, 2049), np.float32))
    if not torch.cuda.is_available():      # valid arguments reach the device check: no host fallback
        with pytest.raises(_ffi.B4DUnavailable):
            fringes.fringe_displacement(z, z, carriers=f)
        with pytest.raises(_ffi.B4DUnavailable):
            fringes.fringe_demodulate(z, f)
        with pytest.raises(_ffi.B4DUnavailable):
            fringes.phase_unwrap(z)
        with pytest.raises(_ffi.B4DUnavailable):
            fringes.fringe_carriers(z)


def test_coarse_carrier_search():
    """Within a bin of the truth in the representative sign; a second harmonic of f1 stronger than f2 and the conjugates are
    excluded by the angle rule; f_min removes the mean and a slow envelope."""
    shape = (256, 320)
    y, x = np.arange(256.0)[:, None], np.arange(320.0)[None, :]
    frame = synth.fringe_frame(shape, CARRIERS, visibility=(0.4, 0.2), envelope=gaussian_envelope(shape))
    frame = frame + 0.25 * np.cos(2.0 * np.pi * 2.0 * (CARRIERS[0, 0] * y + CARRIERS[0, 1] * x))
    f = fringes.coarse_carriers(psd_shifted(frame))
    assert np.all(np.abs(f - CARRIERS) <= [0.5 / 256 + 1e-12, 0.5 / 320 + 1e-12])
    flipped = fringes.coarse_carriers(psd_shifted(frame)[::-1, ::-1])       # the spectrum is symmetric up to the Nyquist row
    assert flipped[0, 1] > 0 and flipped[1, 0] > 0
    np.testing.assert_array_equal(fringes._representative(np.array([-0.1, -0.1])), [0.1, 0.1])
    np.testing.assert_array_equal(fringes._representative(np.array([0.2, -0.1])), [0.2, -0.1])
    np.testing.assert_array_equal(fringes._representative(np.array([-0.2, 0.1])), [0.2, -0.1])
    with pytest.raises(ValueError):
        fringes.coarse_carriers(np.zeros(8))


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_against_the_true_field(name):
    """Largest error of dy / dx against the true field at the window centres, bar = 2 x observed (pixels):
      a_256_w32          observed 7.57e-3 / 6.46e-3
      b_192x160_w24x40   observed 7.83e-3 / 1.18e-2
      c_256_w16          observed 2.12e-2 / 1.83e-2
      d_256x320_sheared  observed 2.16e-2 / 2.03e-2
      e_256_poisson      observed 2.10e-2 / 2.03e-2   (Poisson noise at 2000 counts)
      m_256_magnified    observed 1.39e-2 / 1.20e-2
    Every case asserts the unwrap's own rounding margin below 0.25: a case that the oracle cannot decide does not pass."""
    _, _, uy, ux = case_frames(name)
    o = case_oracle(name)
    assert o["margin"] < 0.25
    ey, ex = float(np.max(np.abs(o["dy"] - uy))), float(np.max(np.abs(o["dx"] - ux)))
    print(f"fringes.truth.{name}: dy {ey:.4e} dx {ex:.4e} px, unwrap margin {o['margin']:.2e}")
    assert ey <= TRUTH_BARS[name][0] and ex <= TRUTH_BARS[name][1]


def test_sheared_case_wraps_and_recovers_transmission_and_dark_field():
    """Case d: the wrapped maps hold more than one integer level and the unwrap recovers them exactly (margin observed
    5.7e-16, bar 1e-12); transmission against the envelope at the window centres observed 1.98e-3 (bar 2 x); dark field
    observed 0.7336 .. 0.7538 for a true 0.75 (bar 0.75 +- 2 x the larger deviation)."""
    shape, window, step, *_ = CASES["d_256x320_sheared"]
    o = case_oracle("d_256x320_sheared")
    spans = [int(l.max() - l.min()) for l in o["levels"]]
    print(f"fringes.sheared: level spans {spans}, margin {o['margin']:.2e}")
    assert max(spans) >= 2 and o["margin"] < 1e-12
    g = fringes.fringe_grid(shape, window=window, step=step)
    env = gaussian_envelope(shape)(g["y"][:, None], g["x"][None, :])
    et = float(np.max(np.abs(o["transmission"] - env)))
    lo, hi = float(o["dark_field"].min()), float(o["dark_field"].max())
    print(f"fringes.sheared: transmission {et:.4e}, dark field {lo:.4f} .. {hi:.4f}")
    assert et <= T_BAR and 0.75 - DF_BAR <= lo and hi <= 0.75 + DF_BAR


T_BAR = 3.96e-3     # 2 x 1.98e-3
DF_BAR = 0.0328     # 2 x 0.0164


def test_magnification_slopes():
    """Pure magnification 0.03 (y) / 0.025 (x): the fitted slopes of dy along y and dx along x, observed 0.02998842 and 0.02499845
    (relative errors 3.86e-4 and 6.2e-5); bar 2 x the larger."""
    shape, window, step, *_ = CASES["m_256_magnified"]
    o = case_oracle("m_256_magnified")
    g = fringes.fringe_grid(shape, window=window, step=step)
    sy = np.polyfit(g["y"], o["dy"].mean(axis=1), 1)[0]
    sx = np.polyfit(g["x"], o["dx"].mean(axis=0), 1)[0]
    print(f"fringes.magnification: slopes {sy:.8f} {sx:.8f}")
    assert abs(sy / 0.03 - 1.0) <= SLOPE_BAR and abs(sx / 0.025 - 1.0) <= SLOPE_BAR


SLOPE_BAR = 7.8e-4   # 2 x 3.86e-4


def test_carrier_estimation():
    """refine=1 on the reference of case d (256 x 320): observed errors 5.0e-7 and 5.9e-7 cycles/px against 1.1e-3 and 1.9e-3 after the coarse step;
    bar 2 x observed."""
    shape, window, step, carriers, *_ = CASES["d_256x320_sheared"]
    ref, _, _, _ = case_frames("d_256x320_sheared")
    coarse = fringes.coarse_carriers(psd_shifted(ref))
    f = estimate_carriers(ref, window, step)
    ec, er = np.max(np.abs(coarse - carriers), axis=1), np.max(np.abs(f - carriers), axis=1)
    print(f"fringes.carriers: coarse {ec}, refined {er}")
    assert np.all(er <= CARRIER_BARS) and np.all(er < ec)


CARRIER_BARS = (1.0e-6, 1.2e-6)   # cycles/px, 2 x observed


def test_absolute_mode_and_wrapped_mode():
    """Without a reference the phase is arg S_k and there is no transmission or dark field; without the unwrap the shifts are those of
    the wrapped phases, equal to the unwrapped ones where no level was added."""
    shape, window, step, carriers, *_ = CASES["a_256_w32"]
    ref, img, _, _ = case_frames("a_256_w32")
    a = analyse(None, img, carriers, window, step, do_unwrap=False)
    assert "transmission" not in a and "dark_field" not in a
    np.testing.assert_array_equal(a["wrapped"], np.angle(a["S"][1:]))
    w = analyse(ref, img, carriers, window, step, do_unwrap=False)
    o = case_oracle("a_256_w32")
    same = np.all(o["levels"] == 0, axis=0)
    assert same.any()
    np.testing.assert_array_equal(w["dy"][same], o["dy"][same])
