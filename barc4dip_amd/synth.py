"""Deterministic synthetic inputs: fully developed speckle with shot noise.

Host (NumPy) generators are used by the parity tests, the golden-vector script and the
CPU baseline; `speckle_stack_device` builds large stacks directly in HBM with torch so
that bench inputs are resident before the timed region starts.
"""
from __future__ import annotations

import numpy as np


def speckle_intensity(n: int, seed: int, *, pupil_div: int = 8, mean: float = 1000.0) -> np.ndarray:
    """Noise-free speckle intensity (n, n) float64: |ifft2(pupil * exp(2 pi i U))|^2, mean `mean`."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[-(n // 2):n - n // 2, -(n // 2):n - n // 2]
    pupil = (xx * xx + yy * yy) <= (n / pupil_div) ** 2
    field = np.fft.ifft2(np.fft.ifftshift(pupil * np.exp(2j * np.pi * rng.random((n, n)))))
    inten = np.abs(field) ** 2
    return inten * (mean / inten.mean())


def speckle_frame(n: int, seed: int, *, pupil_div: int = 8, mean: float = 1000.0,
                  dtype=np.float32) -> np.ndarray:
    """One Poisson-noised speckle frame; frame t of a stack uses seed = 1234 + t (§8d)."""
    rng = np.random.default_rng(seed + 7_000_000)
    return rng.poisson(speckle_intensity(n, seed, pupil_div=pupil_div, mean=mean)).astype(dtype)


def speckle_stack(t: int, n: int, *, seed0: int = 1234, dtype=np.float32) -> np.ndarray:
    return np.stack([speckle_frame(n, seed0 + i, dtype=dtype) for i in range(t)], axis=0)


def spiral_shifts(t: int, max_shift: int = 32) -> np.ndarray:
    """Integer (sy, sx) spiral, |s| <= max_shift, shifts[0] = (0, 0)."""
    k = np.arange(t)
    r = max_shift * k / max(t - 1, 1)
    ang = 0.61803398875 * 2 * np.pi * k
    s = np.stack([np.rint(r * np.sin(ang)), np.rint(r * np.cos(ang))], axis=1).astype(np.int64)
    s[0] = 0
    return s


def shifted_stack(t: int, n: int, *, seed: int = 1234, max_shift: int = 32, dtype=np.float32):
    """cfg3 stack: frame k = Poisson(roll(I0, shift_k)), fresh shot noise per frame.

    Returns (stack (t, n, n), shifts (t, 2) int64 with ground-truth (sy, sx))."""
    i0 = speckle_intensity(n, seed)
    sh = spiral_shifts(t, max_shift)
    out = np.empty((t, n, n), dtype=dtype)
    for k in range(t):
        rng = np.random.default_rng(5000 + k if k else seed)
        out[k] = rng.poisson(np.roll(i0, (int(sh[k, 0]), int(sh[k, 1])), axis=(0, 1))).astype(dtype)
    return out, sh


def speckle_stack_device(t: int, n: int, *, seed0: int = 1234, device="cuda", chunk: int = 8,
                         pupil_div: int = 8, mean: float = 1000.0):
    """(t, n, n) float32 speckle stack generated in HBM (same statistics as `speckle_frame`,
    different random stream: torch's counter-based generator).  Used for bench inputs only;
    parity tests use the host generators.  The generator itself calls torch.fft (rocFFT shows up as
    `fft_rtc_*` kernels in profiles of the input set-up): it builds test data outside every timed region and is
    not part of the product path, which has no rocFFT dependency."""
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(seed0)
    ax = torch.arange(n, device=device) - n // 2
    pupil = ((ax[None, :] ** 2 + ax[:, None] ** 2) <= (n / pupil_div) ** 2).to(torch.float32)
    pupil = torch.fft.ifftshift(pupil)
    out = torch.empty((t, n, n), dtype=torch.float32, device=device)
    for a in range(0, t, chunk):
        b = min(t, a + chunk)
        ph = torch.rand((b - a, n, n), generator=g, device=device) * (2 * np.pi)
        fld = torch.fft.ifft2(torch.polar(pupil.expand(b - a, n, n), ph))
        inten = fld.real ** 2 + fld.imag ** 2
        inten *= mean / inten.mean(dim=(1, 2), keepdim=True)
        out[a:b] = torch.poisson(inten, generator=g)
    return out


# ---- white speckle for tracker edge tests ------------------------------------------------------------------------------------
# `speckle_frame` has a correlation length of several pixels (pupil_div): on crops of 64 ... 128 rows a 21 ... 41-px template is
# lost in the noise of the whitened phase-correlation map.  White, fully developed speckle (exponential intensity statistics, no
# spatial correlation) keeps every spectral bin informative, so small templates still give one dominant peak at ANY cyclic shift.

def white_speckle_pairs(shape, shifts, *, seed: int, noise: float = 10.0, dtype=np.float32):
    """(base (H, W), stack (len(shifts), H, W)): base = Gamma(1, 100) intensities, frame i = roll(base, shifts[i]) + N(0, noise)."""
    H, W = shape
    rng = np.random.default_rng(seed)
    base = rng.gamma(1.0, 100.0, (H, W)).astype(dtype)
    stack = np.empty((len(shifts), H, W), dtype=dtype)
    for i, (dy, dx) in enumerate(shifts):
        stack[i] = np.roll(base, (int(dy), int(dx)), axis=(0, 1)) + rng.normal(0.0, noise, (H, W))
    return base, stack


def edge_shift_sweep(H: int, W: int):
    """54 cyclic shifts whose correlation peak lies on the first / last row or column of the fftshift-ed (H, W) map, next to them,
    and on both sides of the zero-shift seam of the unshifted map (dy, dx in {-1, 0})."""
    dys = (-(H // 2), -(H // 2) + 1, -2, -1, 0, 1, 2, H - H // 2 - 2, H - H // 2 - 1)
    dxs = (-(W // 2), -(W // 2) + 1, -1, 0, 1, W - W // 2 - 1)
    return [(dy, dx) for dy in dys for dx in dxs]


def edge_roi(shape, tpl_hw):
    """(y0, y1, x0, x1) of the template ROI used by the tracker edge tests: off-centre by (-3, +2)."""
    (H, W), (h, w) = shape, tpl_hw
    y0, x0 = (H - h) // 2 - 3, (W - w) // 2 + 2
    return y0, y0 + h, x0, x0 + w


# (frame shape, template shape, transform route of b4d_phase_correlation) of the tracker edge tests
TRACKING_EDGE_CASES = (
    ((64, 64), (31, 31), "pow2"),        # one workgroup recomputes the three row pairs around the peak, 32 pairs per workgroup
    ((64, 128), (31, 41), "pow2"),       # nx != ny
    ((128, 512), (41, 61), "pow2"),      # 8 row pairs per workgroup
    ((64, 2048), (31, 121), "pow2"),     # two workgroups for the three row pairs
    ((64, 4096), (31, 121), "pow2"),     # three
    ((100, 37), (41, 21), "dft"),        # DFT-matrix route, odd width
    ((171, 170), (61, 61), "dft"),
    ((228, 228), (61, 61), "mixed"),     # mixed-radix, odd quad count
    ((264, 520), (61, 81), "mixed"),     # mixed-radix, fused
)


def degenerate_tracking_inputs(shape, tpl_hw, *, seed: int):
    """name -> (template source frame, image, roi) of inputs whose phase-correlation map is all-zero ("const_*", "tpl_1x1"),
    all-NaN ("nan_*", "inf_image"), delta-like ("whole_frame") or without a dominant peak ("one_row")."""
    H, W = shape
    base, stack = white_speckle_pairs(shape, [(1, 2), (3, -2)], seed=seed)
    frame = stack[0]
    roi = edge_roi(shape, tpl_hw)
    y0, y1, x0, x1 = roi

    def poke(a, y, x, v):
        a = a.copy()
        a[y, x] = v
        return a

    flat_tpl = base.copy()
    flat_tpl[y0:y1, x0:x1] = 7.0
    return {
        "const_image": (base, np.full(shape, 7.0, np.float32), roi),
        "const_template": (flat_tpl, frame, roi),
        "tpl_1x1": (base, frame, (y0, y0 + 1, x0, x0 + 1)),
        "nan_image": (base, poke(frame, 5, 7, np.nan), roi),
        "nan_template": (poke(base, y0 + 4, x0 + 9, np.nan), frame, roi),
        "inf_image": (base, poke(frame, 5, 7, np.inf), roi),
        "whole_frame": (base, np.roll(base, (3, -2), axis=(0, 1)), (0, H, 0, W)),
        "one_row": (base, frame, edge_roi(shape, (1, 31))),
    }


def fringe_frame(shape, carriers, displacement=None, *, visibility=0.4, envelope=None, mean: float = 1.0, seed=None) -> np.ndarray:
    """Grating interferogram (H, W) float64: ``mean * envelope(y, x) * (1 + sum_k visibility_k cos(2 pi f_k . (r - u(r))))``.

    ``carriers``: (K, 2) rows (fy, fx) in cycles per pixel; ``visibility``: a number or one per carrier; ``displacement`` and
    ``envelope``: callables of the pixel coordinate arrays ``(y, x)`` ((H, 1) and (1, W)) returning ``(uy, ux)`` and the envelope
    (``None``: no displacement, envelope 1).  With ``seed`` the frame is Poisson noise of that intensity, ``mean`` in counts."""
    H, W = (int(s) for s in shape)
    f = np.atleast_2d(np.asarray(carriers, dtype=np.float64))
    vis = np.broadcast_to(np.asarray(visibility, dtype=np.float64), (f.shape[0],))
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    uy, ux = (0.0, 0.0) if displacement is None else displacement(y, x)
    frame = np.ones((H, W))
    for (fy, fx), v in zip(f, vis):
        frame = frame + v * np.cos(2.0 * np.pi * (fy * (y - uy) + fx * (x - ux)))
    frame *= mean * (1.0 if envelope is None else envelope(y, x))
    if seed is not None:
        frame = np.random.default_rng(seed).poisson(frame).astype(np.float64)
    return frame


def hartmann_frame(shape, pitch, origin=(0, 0), displacement=None, *, sigma: float = 2.0, amplitude: float = 1000.0,
                   background: float = 0.0, seed=None) -> np.ndarray:
    """Hartmann / Shack-Hartmann frame (H, W) float64: a Gaussian spot of ``amplitude`` and ``sigma`` px in every whole cell of
    the lattice ``signal.hartmann_cells(shape, pitch, origin)``, at the cell's nominal position plus its displacement, on a
    constant ``background``.

    ``displacement``: ``None``, a ``(dy, dx)`` pair that broadcasts to the (gy, gx) lattice, or a callable of the nominal positions
    ``(y, x)`` ((gy, 1) and (1, gx)) returning such a pair.  Every spot is drawn out to 8 sigma (1e-14 of its height).  With
    ``seed`` the frame is Poisson noise of that intensity."""
    from .signal.hartmann import hartmann_cells

    H, W = (int(s) for s in shape)
    cells = hartmann_cells((H, W), pitch, origin)
    gy, gx = cells["shape"]
    y0, x0 = cells["y"][:, None], cells["x"][None, :]
    dy, dx = (0.0, 0.0) if displacement is None else (displacement(y0, x0) if callable(displacement) else displacement)
    cy = np.broadcast_to(y0 + np.asarray(dy, dtype=np.float64), (gy, gx))
    cx = np.broadcast_to(x0 + np.asarray(dx, dtype=np.float64), (gy, gx))
    frame = np.full((H, W), float(background))
    reach = 8.0 * float(sigma)
    for i in range(gy):
        for j in range(gx):
            ya, yb = max(0, int(np.floor(cy[i, j] - reach))), min(H, int(np.ceil(cy[i, j] + reach)) + 1)
            xa, xb = max(0, int(np.floor(cx[i, j] - reach))), min(W, int(np.ceil(cx[i, j] + reach)) + 1)
            if ya >= yb or xa >= xb:
                continue
            ey = np.exp(-0.5 * ((np.arange(ya, yb) - cy[i, j]) / sigma) ** 2)
            ex = np.exp(-0.5 * ((np.arange(xa, xb) - cx[i, j]) / sigma) ** 2)
            frame[ya:yb, xa:xb] += amplitude * ey[:, None] * ex[None, :]
    if seed is not None:
        frame = np.random.default_rng(seed).poisson(frame).astype(np.float64)
    return frame


def spot_field(shape, n: int, *, seed: int, sigma: float = 2.0, amplitude: float = 1000.0, background: float = 0.0, noise: float = 0.0,
               min_separation=None):
    """Gaussian spots at random positions that lie on no lattice: (frame (H, W) float64, centres (n, 2) float64 rows (y, x)).

    The centres are drawn one by one, uniformly and at sub-pixel positions, at least ``min_separation`` px (``None``: 8 sigma)
    from each other and half of that from the frame's edges; each spot has ``amplitude`` and ``sigma`` px and is drawn out to
    8 sigma, on a constant ``background``, plus Gaussian noise of standard deviation ``noise``.  ValueError where ``n`` spots do
    not fit."""
    H, W = (int(s) for s in shape)
    sep = 8.0 * float(sigma) if min_separation is None else float(min_separation)
    if n < 0 or sigma <= 0 or sep < 0 or H <= sep or W <= sep:
        raise ValueError(f"cannot place {n} spots of sigma {sigma} at separation {sep} on {(H, W)}")
    rng = np.random.default_rng(seed)
    centres = np.empty((n, 2))
    k = tries = 0
    while k < n:
        tries += 1
        if tries > 1000 * (n + 1):
            raise ValueError(f"{n} spots at separation {sep} do not fit on {(H, W)}")
        c = np.array([rng.uniform(0.5 * sep, H - 1 - 0.5 * sep), rng.uniform(0.5 * sep, W - 1 - 0.5 * sep)])
        if k == 0 or np.min(np.hypot(*(centres[:k] - c).T)) >= sep:
            centres[k] = c
            k += 1
    frame = np.full((H, W), float(background))
    reach = 8.0 * float(sigma)
    for cy, cx in centres:
        ya, yb = max(0, int(np.floor(cy - reach))), min(H, int(np.ceil(cy + reach)) + 1)
        xa, xb = max(0, int(np.floor(cx - reach))), min(W, int(np.ceil(cx + reach)) + 1)
        ey = np.exp(-0.5 * ((np.arange(ya, yb) - cy) / sigma) ** 2)
        ex = np.exp(-0.5 * ((np.arange(xa, xb) - cx) / sigma) ** 2)
        frame[ya:yb, xa:xb] += amplitude * ey[:, None] * ex[None, :]
    if noise:
        frame = frame + rng.normal(0.0, float(noise), (H, W))
    return frame, centres
