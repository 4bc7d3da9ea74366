"""Fringe analysis of 2-D grating interferograms: displacement, transmission and dark-field maps by windowed Fourier
demodulation (``b4d_fringe_demodulate``, ``b4d_fringe_compare``, ``b4d_phase_unwrap``, ``b4d_fringe_shift``), with weighted and
masked unwrapping for apertured or blotched beams (``b4d_phase_unwrap_weighted``, ``b4d_fringe_weights``, ``b4d_fringe_shift_levels``).

Frames are (H, W), the window is ``(wy, wx)``, the step ``(sty, stx)`` (default ``window // 2``).  Window origins are
``y0 = k * sty`` for every k with ``y0 + wy <= H`` (likewise along x; no search margin), the axes are the window centres
``y0 + (wy - 1) / 2``.  With the half-sample Hann taper ``h_w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / w)`` the harmonic map of a
carrier ``f = (fy, fx)`` in cycles per pixel is

    S_f[Y, X] = sum_j sum_i h_wy[j] h_wx[i] I[y0+j, x0+i] exp(-2 pi i (fy (y0+j) + fx (x0+i))) / (sum h_wy * sum h_wx),

the phase in ABSOLUTE pixel coordinates, so that the maps of neighbouring windows are continuous and the carrier phase of a
sample cancels against a reference; ``S_0`` is the same sum with f = 0.  With sample harmonics S, reference harmonics R and the
carriers as the rows of ``M = [[f1y, f1x], [f2y, f2x]]``:

    phase_k = arg(S_k conj R_k) in (-pi, pi]     visibility_k = 2 |S_k| / S_0     transmission = S_0 / R_0
    dark_field_k = (|S_k| / S_0) / (|R_k| / R_0)     peak = min(visibility_1, visibility_2)     (dy, dx) = -M^-1 (phase_1, phase_2) / 2 pi

A fringe ``cos(2 pi f.(r - u))`` against ``cos(2 pi f.r)`` gives ``d = u``: frame(r) = ref(r - d), the convention of
``displacement_map`` and ``correct_distortion``.  The result of ``fringe_displacement`` is a ``displacement_map``-compatible
dict (``dy, dx, y, x, peak``), so ``wavefront_from_displacement(..., weights="peak")`` and everything after it take it as it is.
With ``weights``, ``mask``, ``min_level`` or ``min_visibility`` the phase maps are unwrapped over the valid windows only
 and the result carries ``valid``, which ``wavefront_from_displacement(m, mask=m["valid"])`` takes as it is.
Everything runs on the device (DESIGN.md sections 17 and 18); there is no host fallback.  Limits: windows of 2 .. 256 px per axis, 1 .. 4
carriers per demodulation, grids of at most 2048 nodes per side when unwrapping.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from .displacement import _pair, _shape
from .wavefront import _check_solver, _check_weights, _solver_info, _weights_device

MIN_WINDOW = 2
MAX_WINDOW = 256
MAX_CARRIERS = 4
MAX_UNWRAP_SIDE = 2048
MIN_PERIODS = 2.0           # fringe periods a window must hold along its better axis: below, the Hann taper no longer rejects DC
MIN_CARRIER_ANGLE = 5.0     # degrees between the two carriers of a displacement measurement


def fringe_grid(shape, *, window=32, step=None) -> dict:
    """Host-only grid geometry of the fringe functions for frames of ``shape`` = (H, W) (no device needed).

    Returns {"window", "step": (y, x) pairs, "y0", "x0": window origins (int64), "y", "x": window centres (float64), "shape":
    (gy, gx)}.  ValueError for arguments < 1 or a window that does not fit, NotImplementedError for a window outside 2 .. 256."""
    H, W = (int(s) for s in shape)
    wy, wx = _pair(window, "window")
    if step is None:
        sty, stx = max(1, wy // 2), max(1, wx // 2)
    else:
        sty, stx = _pair(step, "step")
    if min(wy, wx) < MIN_WINDOW or max(wy, wx) > MAX_WINDOW:
        raise NotImplementedError(f"window {(wy, wx)} is outside the kernel's range of {MIN_WINDOW} .. {MAX_WINDOW} px per axis")
    if H < wy or W < wx:
        raise ValueError(f"a {(wy, wx)} window does not fit in a {(H, W)} frame")
    y0 = sty * np.arange((H - wy) // sty + 1, dtype=np.int64)
    x0 = stx * np.arange((W - wx) // stx + 1, dtype=np.int64)
    return {"window": (wy, wx), "step": (sty, stx), "y0": y0, "x0": x0, "y": y0 + (wy - 1) / 2.0, "x": x0 + (wx - 1) / 2.0,
            "shape": (int(y0.size), int(x0.size))}


def _check_carriers(carriers, window, *, pair: bool) -> np.ndarray:
    """(K, 2) float64 carriers, rows (fy, fx), checked against the window (host only)."""
    try:
        f = np.array(carriers, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"carriers must be a (K, 2) array of (fy, fx) rows, got {carriers!r}") from None
    if f.ndim == 1 and f.size == 2 and not pair:
        f = f[None]
    if f.ndim != 2 or f.shape[1] != 2 or not 1 <= f.shape[0] <= MAX_CARRIERS:
        raise ValueError(f"carriers must be (K, 2) with 1 <= K <= {MAX_CARRIERS}, rows (fy, fx); got shape {f.shape}")
    if pair and f.shape[0] != 2:
        raise ValueError(f"a displacement needs exactly two carriers, got {f.shape[0]}")
    if not np.all(np.isfinite(f)):
        raise ValueError("carriers must be finite")
    mag = np.hypot(f[:, 0], f[:, 1])
    if np.any(mag > 0.5):
        raise ValueError(f"carriers beyond the Nyquist frequency (|f| > 0.5 cycles per pixel): {f.tolist()}")
    wy, wx = window
    periods = np.maximum(np.abs(f[:, 0]) * wy, np.abs(f[:, 1]) * wx)
    if np.any(periods < MIN_PERIODS):
        raise ValueError(f"a {(wy, wx)} window holds fewer than {MIN_PERIODS:g} fringe periods of carriers {f.tolist()}: "
                         "the taper no longer rejects the mean; use a larger window")
    if pair:
        det = f[0, 0] * f[1, 1] - f[0, 1] * f[1, 0]
        if abs(det) < np.sin(np.deg2rad(MIN_CARRIER_ANGLE)) * mag[0] * mag[1]:
            raise ValueError(f"the two carriers are closer than {MIN_CARRIER_ANGLE:g} degrees to parallel: {f.tolist()}")
    return f


def _frames_device(a):
    """(n, H, W) float32 device tensor of an (H, W) or (T, H, W) input."""
    t, _, _ = D.to_device_f32(a, ndim=(2, 3))
    return t.reshape((-1,) + tuple(int(s) for s in t.shape[-2:]))


def _demodulate_device(frames, carriers: np.ndarray, g: dict):
    """Harmonic maps (n, K + 1, gy, gx) complex64 of the device frames (n, H, W)."""
    torch = _ffi.require_gpu()
    lib = _ffi.lib()
    n, H, W = (int(s) for s in frames.shape)
    K = int(carriers.shape[0])
    (wy, wx), (sty, stx), (gy, gx) = g["window"], g["step"], g["shape"]
    ws = torch.empty(int(lib.b4d_fringe_demodulate_workspace_bytes(K, H, W, wy, wx)), dtype=torch.uint8, device=frames.device)
    out = torch.empty((n, K + 1, gy, gx), dtype=torch.complex64, device=frames.device)
    f = np.ascontiguousarray(carriers, dtype=np.float64)
    _ffi.check(lib.b4d_fringe_demodulate(D.ptr(frames), n, H, W, f.ctypes.data_as(C.c_void_p), K, wy, wx, sty, stx, D.ptr(ws), D.ptr(out),
                                         _ffi.stream_ptr()))
    return out


def _unwrap_device(phase):
    """Unwrapped copy of the device maps (n, ny, nx) float32."""
    torch = _ffi.require_gpu()
    lib = _ffi.lib()
    n, ny, nx = (int(s) for s in phase.shape)
    ws = torch.empty(int(lib.b4d_phase_unwrap_workspace_bytes(n, ny, nx)), dtype=torch.uint8, device=phase.device)
    out = torch.empty_like(phase)
    _ffi.check(lib.b4d_phase_unwrap(D.ptr(phase), n, ny, nx, D.ptr(ws), D.ptr(out), _ffi.stream_ptr()))
    return out


def _unwrap_weighted_device(phase, w, w_stride: int, rtol: float, max_iter: int, nan_invalid: bool):
    """(unwrapped maps, effective weights, iterations, residual) of the device maps (n, ny, nx) float32 with the weights w."""
    torch = _ffi.require_gpu()
    lib = _ffi.lib()
    n, ny, nx = (int(s) for s in phase.shape)
    if w_stride != 0 and int(w.shape[0]) != n:
        raise ValueError(f"{int(w.shape[0])} weight maps for {n} phase maps")
    ws = torch.empty(int(lib.b4d_phase_unwrap_weighted_workspace_bytes(n, ny, nx)), dtype=torch.uint8, device=phase.device)
    out = torch.empty_like(phase)
    iters = torch.empty((n,), dtype=torch.int32, device=phase.device)
    resid = torch.empty((n,), dtype=torch.float64, device=phase.device)
    _ffi.check(lib.b4d_phase_unwrap_weighted(D.ptr(phase), D.ptr(w), w_stride, n, ny, nx, rtol, max_iter, int(nan_invalid), D.ptr(ws),
                                             D.ptr(out), D.ptr(iters), D.ptr(resid), _ffi.stream_ptr()))
    weff = ws[:n * ny * nx * 4].view(torch.float32).reshape(n, ny, nx)
    return out, weff, iters, resid


def _fringe_weights_device(S, R, paired: bool, min_level: float, min_visibility: float, snr: bool):
    """Node weights (n, K, gy, gx) float32 of the phase maps from the device harmonics S (and R, or None)."""
    torch = _ffi.require_gpu()
    lib = _ffi.lib()
    n, K1, gy, gx = (int(s) for s in S.shape)
    ws = torch.empty(int(lib.b4d_fringe_weights_workspace_bytes(n, gy, gx)), dtype=torch.uint8, device=S.device)
    w = torch.empty((n, K1 - 1, gy, gx), dtype=torch.float32, device=S.device)
    _ffi.check(lib.b4d_fringe_weights(D.ptr(S), None if R is None else D.ptr(R), K1 * gy * gx if paired else 0, n, K1 - 1, gy, gx,
                                      min_level, min_visibility, int(snr), D.ptr(w), D.ptr(ws), _ffi.stream_ptr()))
    return w


def _threshold(v, name: str, top: float) -> float:
    """A threshold in [0, top]; None is 0, which switches the test off."""
    if v is None:
        return 0.0
    if isinstance(v, (bool, str)) or np.ndim(v) != 0:
        raise ValueError(f"{name} must be None or a number in [0, {top:g}], got {v!r}")
    try:
        t = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or a number in [0, {top:g}], got {v!r}") from None
    if not 0.0 <= t <= top:
        raise ValueError(f"{name} must be None or a number in [0, {top:g}], got {v!r}")
    return t


def _compare_device(S, R, paired: bool):
    """phase, visibility (n, K, gy, gx) float32, transmission (n, gy, gx) float32 or None, dark_field or None, peak float64."""
    torch = _ffi.require_gpu()
    n, K1, gy, gx = (int(s) for s in S.shape)
    K = K1 - 1
    dev = S.device
    phase = torch.empty((n, K, gy, gx), dtype=torch.float32, device=dev)
    vis = torch.empty_like(phase)
    peak = torch.empty((n, gy, gx), dtype=torch.float64, device=dev)
    trans = dark = None
    if R is not None:
        trans = torch.empty((n, gy, gx), dtype=torch.float32, device=dev)
        dark = torch.empty_like(phase)
    _ffi.check(_ffi.lib().b4d_fringe_compare(D.ptr(S), None if R is None else D.ptr(R), K1 * gy * gx if paired else 0, n, K, gy, gx,
                                             D.ptr(phase), D.ptr(vis), None if trans is None else D.ptr(trans),
                                             None if dark is None else D.ptr(dark), D.ptr(peak), _ffi.stream_ptr()))
    return phase, vis, trans, dark, peak


def fringe_demodulate(images, carriers, *, window=32, step=None, return_tensors: bool = False) -> dict:
    """Harmonic maps of ``images`` ((H, W) or (T, H, W), any real dtype or ROCm tensors) at ``carriers`` ((K, 2) rows (fy, fx) in
    cycles per pixel, 1 <= K <= 4; a single (fy, fx) pair is K = 1).

    Returns {"harmonics": complex64 (K + 1, gy, gx) or (T, K + 1, gy, gx), plane 0 the window mean S_0 and plane k + 1 the map of
    carrier k (module docstring); "y", "x": window centres; "carriers": (K, 2) float64; "meta"}.  A frame gives the same bits
    alone and inside any stack.  ValueError for bad shapes or carriers, NotImplementedError for a window outside 2 .. 256."""
    ims = _shape(images)
    if len(ims) not in (2, 3):
        raise ValueError(f"images must be (H, W) or (T, H, W), got {ims}")
    if 0 in ims:
        raise ValueError("empty images")
    g = fringe_grid(ims[-2:], window=window, step=step)
    f = _check_carriers(carriers, g["window"], pair=False)
    _ffi.require_gpu()
    out = _demodulate_device(_frames_device(images), f, g)
    if len(ims) == 2:
        out = out[0]
    return {"harmonics": out if return_tensors else out.cpu().numpy(), "y": g["y"], "x": g["x"], "carriers": f,
            "meta": {"window": g["window"], "step": g["step"]}}


def phase_unwrap(phase, *, weights=None, mask=None, fill="nan", rtol=1e-6, max_iter=500, return_info: bool = False,
                 return_tensors: bool = False):
    """Unwrapped phase maps, (ny, nx) or (T, ny, nx), by least squares plus a congruence step: the wrapped differences of
    neighbouring nodes are the edge slopes of a 5-point Neumann Poisson problem (the DCT solve of ``integrate_gradient``); its
    zero-mean solution ``p``, shifted to equal the input at node ``(ny // 2, nx // 2)``, only selects the level, and the result
    is ``phase + 2 pi round((p - phase) / 2 pi)``: the data are never smoothed, and a map without wraps comes back bit for bit.
    float32 on the device; returns float64 NumPy or the float32 device tensor.  Without ``weights`` and ``mask`` the unwrap is
    whole-grid and unweighted: a non-finite node spoils its map, as in the unweighted integrator.

    ``weights`` (>= 0) and ``mask`` (non-zero = valid) are (ny, nx), shared by the batch, or shaped like ``phase``; any real or
    bool dtype and layout, or ROCm tensors, as in ``integrate_gradient``.  The node weight is their product, and 0 where it is
    not finite and positive or where the phase is not finite: such nodes take no part.  Every edge carries the harmonic mean of
    its two node weights and ``p`` minimises the weighted squared differences from the wrapped ones, solved by the
    preconditioned conjugate gradients of ``integrate_gradient`` (``rtol``, ``max_iter``; a map that stops above ``rtol`` raises a
    RuntimeWarning and is still returned).  ``p`` is shifted to equal the input at the seed -- the valid node of largest weight,
    ties to the node nearest ``(ny // 2, nx // 2)``, then to the smallest row-major index -- and the levels are rounded at the
    valid nodes.  ``fill="nan"`` writes NaN at the weight-0 nodes, ``fill="harmonic"`` the levelled ``p`` (smooth, not congruent to
    the input).  Pieces of the valid region that no edge connects are levelled against each other as smoothly as possible: their
    relative level is levelled, not measured.  A map without a valid node is NaN with 0 iterations.
    ``return_info=True`` returns ``(out, {"iterations", "residual", "converged"})``, each (T,) (T = 1 for a 2-D call); without
    weights and mask that is 0 iterations, residual 0 and converged.
    ValueError for a wrong ndim, empty maps or bad weight, mask and solver arguments, NotImplementedError for a side above
    2048 -- all raised before the GPU is touched."""
    shape = _shape(phase)
    if len(shape) not in (2, 3):
        raise ValueError(f"phase must be (ny, nx) or (T, ny, nx), got {shape}")
    if 0 in shape:
        raise ValueError(f"empty phase maps {shape}")
    if max(shape[-2:]) > MAX_UNWRAP_SIDE:
        raise _ffi.B4DSizeError(f"phase unwrapping is limited to {MAX_UNWRAP_SIDE} nodes per side, got {shape[-2:]}")
    tol, iters_max = _check_solver(fill, rtol, max_iter)
    _check_weights(weights, mask, shape)
    _ffi.require_gpu()
    t, _, _ = D.to_device_f32(phase, ndim=(2, 3))
    t = t.reshape((-1,) + shape[-2:])
    if weights is None and mask is None:
        out = _unwrap_device(t)
        n = int(out.shape[0])
        info = {"iterations": np.zeros(n, np.int32), "residual": np.zeros(n), "converged": np.ones(n, bool)}
    else:
        w, stride = _weights_device(weights, mask, shape)
        out, _, it, res = _unwrap_weighted_device(t.contiguous(), w, stride, tol, iters_max, fill == "nan")
        info = _solver_info(it, res, tol, iters_max)
    out = out.reshape(shape)
    out = out if return_tensors else out.cpu().numpy().astype(np.float64)
    return (out, info) if return_info else out


def _representative(f: np.ndarray) -> np.ndarray:
    """Of f and -f the one with fx > 0 where |fx| >= |fy|, else the one with fy > 0."""
    lead = f[1] if abs(f[1]) >= abs(f[0]) else f[0]
    return -f if lead < 0 else f


def coarse_carriers(psd, *, f_min: float = 0.02, min_angle: float = 30.0) -> np.ndarray:
    """The two strongest carriers of a shifted 2-D power spectrum ``psd`` (ny, nx) (layout of ``psd2d``), pure NumPy.

    Bins with ``|f| < f_min`` are zeroed and the arg-max is f1; every bin whose direction lies within ``min_angle`` degrees of
    +-f1 is zeroed too (that excludes 2 f1 and the conjugate) and the arg-max of the rest is f2.  Returns (2, 2) float64, rows
    (fy, fx) in cycles per pixel on the bin grid, each in its representative sign."""
    P = np.array(psd, dtype=np.float64)
    if P.ndim != 2:
        raise ValueError(f"psd must be 2-D, got shape {P.shape}")
    if not 0.0 < min_angle < 90.0:
        raise ValueError(f"min_angle must lie in (0, 90) degrees, got {min_angle!r}")
    ny, nx = P.shape
    fy = np.fft.fftshift(np.fft.fftfreq(ny))[:, None]
    fx = np.fft.fftshift(np.fft.fftfreq(nx))[None, :]
    mag = np.hypot(fy, fx)
    P[mag < f_min] = 0.0
    i1 = np.unravel_index(int(np.argmax(P)), P.shape)
    f1 = np.array([fy[i1[0], 0], fx[0, i1[1]]])
    cross = np.abs(fy * f1[1] - fx * f1[0])
    P[cross < np.sin(np.deg2rad(min_angle)) * mag * np.hypot(*f1)] = 0.0
    i2 = np.unravel_index(int(np.argmax(P)), P.shape)
    f2 = np.array([fy[i2[0], 0], fx[0, i2[1]]])
    return np.stack([_representative(f1), _representative(f2)])


def _refine_carriers(frame, f: np.ndarray, g: dict, min_level: float = 0.0, min_visibility: float = 0.0) -> np.ndarray:
    """One refinement: demodulate the device frame (1, H, W) at f, unwrap, fit a plane to each phase map, add slope / 2 pi.  With a
    threshold the unwrap is masked and the planes are fitted over the valid nodes only."""
    S = _demodulate_device(frame, _check_carriers(f, g["window"], pair=False), g)
    phase = _compare_device(S, None, False)[0]
    gy, gx = g["shape"]
    phase = phase.reshape(-1, gy, gx)
    if min_level > 0.0 or min_visibility > 0.0:
        w = _fringe_weights_device(S, None, False, min_level, min_visibility, False).reshape(-1, gy, gx)
        ph = _unwrap_weighted_device(phase, w, gy * gx, 1e-6, 500, True)[0].cpu().numpy().astype(np.float64)
    else:
        ph = _unwrap_device(phase).cpu().numpy().astype(np.float64)
    yc, xc = g["y"] - g["y"].mean(), g["x"] - g["x"].mean()
    A = np.stack([np.ones((gy, gx)), np.broadcast_to(yc[:, None], (gy, gx)), np.broadcast_to(xc[None, :], (gy, gx))], axis=-1).reshape(-1, 3)
    out = f.copy()
    for k in range(f.shape[0]):
        ok = np.isfinite(ph[k].ravel())
        if np.count_nonzero(ok) < 3:
            raise ValueError(f"fringe_carriers: {np.count_nonzero(ok)} valid windows for carrier {k}, a plane needs three; lower "
                             "min_level / min_visibility")
        c = np.linalg.lstsq(A[ok], ph[k].ravel()[ok], rcond=None)[0]
        out[k] = _representative(f[k] + c[1:] / (2.0 * np.pi))
    return out


def fringe_carriers(reference, *, window=32, step=None, f_min: float = 0.02, min_angle: float = 30.0, refine: int = 1,
                    min_level=None, min_visibility=None) -> np.ndarray:
    """The two carriers of a grating frame ``reference`` (H, W): (2, 2) float64, rows (fy, fx) in cycles per pixel.

    Coarse step: ``coarse_carriers`` of ``psd2d(reference)`` (good to a bin, 1 / H and 1 / W).  Each of the ``refine`` rounds then
    demodulates the frame at the current carriers, unwraps the two phase maps, fits a plane to each and adds ``slope / 2 pi``.
    Representative sign: fx > 0 where |fx| >= |fy|, else fy > 0.  The frame must have a shape that ``psd2d`` supports.
    ``min_level`` (0 .. 1, a window's mean against the largest of the frame) and ``min_visibility`` (0 .. 2) keep the refinement to
    the windows that the beam covers: the unwrap is masked with them (``phase_unwrap``) and the planes are fitted over the valid
    windows only.  ValueError for a threshold outside its range, raised before the GPU is touched."""
    from .fft import psd2d

    lvl, mvis = _threshold(min_level, "min_level", 1.0), _threshold(min_visibility, "min_visibility", 2.0)

    shape = _shape(reference)
    if len(shape) != 2:
        raise ValueError(f"reference must be (H, W), got {shape}")
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError(f"refine must be an integer >= 0, got {refine!r}")
    g = fringe_grid(shape, window=window, step=step)
    _ffi.require_gpu()
    frame = _frames_device(reference)
    P = psd2d(frame[0], scale=False, return_tensors=True)[0]
    f = coarse_carriers(P.cpu().numpy(), f_min=f_min, min_angle=min_angle)
    for _ in range(int(refine)):
        f = _refine_carriers(frame, f, g, lvl, mvis)
    return f


def fringe_displacement(reference, images, *, carriers=None, window=32, step=None, unwrap: bool = True, weights=None, mask=None,
                        min_visibility=None, min_level=None, return_tensors: bool = False) -> dict:
    """Displacement, transmission and dark-field maps of grating frames ``images`` against ``reference``.

    reference (H, W) with images (H, W) or (T, H, W); reference (T, H, W) paired frame by frame with images (T, H, W); or
    ``reference=None`` (absolute mode: ``phase_k = arg S_k``, no transmission and no dark field).  NumPy arrays of any real dtype or
    ROCm tensors.  ``carriers``: (2, 2), rows (fy, fx) in cycles per pixel; ``None`` estimates them with ``fringe_carriers`` from the
    (first) reference, or from ``images[0]`` in absolute mode.  ``window``, ``step``: int or (y, x); ``step=None`` is ``window // 2``.
    ``unwrap=True`` unwraps both phase maps over the grid (``phase_unwrap``; without the four arguments below whole-grid and
    unweighted, a non-finite node spoils its map).
    ``weights``, ``mask``, ``min_level``, ``min_visibility``: if any is set the weighted route runs.  A window is valid if its mean
    ``S_0`` is at least ``min_level`` (0 .. 1) of the largest of its frame, the same for the reference, every visibility of sample
    and reference is at least ``min_visibility`` (0 .. 2), and ``mask`` ((gy, gx) or (T, gy, gx), non-zero = valid) keeps it.
    ``weights="snr"`` weights the valid windows of each phase map with the inverse shot-noise variance of its phase,
    ``1 / (S_0 / |S_k|^2 + R_0 / |R_k|^2)``; an array ((gy, gx) or (T, gy, gx), >= 0) is taken as it is for both maps; ``None`` is 1.
    Each phase map is unwrapped with its own carrier's weights (``phase_unwrap`` at its default ``rtol`` and ``max_iter``); ``dy``, ``dx``
    and ``phase`` are NaN at the windows that are invalid for either carrier, and the result gains "valid" (bool, shape of ``dy``)
    and ``meta["unwrap"]`` becomes {"iterations", "residual", "converged"}, each (T, 2).  Pieces of the valid region that no
    edge connects are levelled, not measured, and the absolute level of a map is that of its seed window (the valid window of
    largest weight, nearest the grid centre among equals): ``weights="snr"`` may move the whole field by a constant shift, a tilt
    of the wavefront.  The shifts are formed in float64 from the wrapped phase and the integer level.  ``wavefront_from_displacement(m, mask=m["valid"])`` takes the result as it is.
    Returns {"dy", "dx", "peak": float64 (gy, gx) or (T, gy, gx), ``peak`` the smaller of the sample's two visibilities; "phase",
    "visibility", "dark_field": (2, gy, gx) or (T, 2, gy, gx); "transmission": like dy; "y", "x": window centres; "carriers";
    "meta"}, formulas in the module docstring.  Maps are float64 NumPy; with ``return_tensors=True`` device tensors (dy, dx, peak
    float64, the others float32).  ValueError for shapes as in ``displacement_map``, for |f| > 0.5, for carriers within 5 degrees of
    parallel and for a window shorter than two fringe periods; NotImplementedError for a window outside 2 .. 256 or a grid side
    above 2048 when unwrapping -- all raised before the GPU is touched."""
    ims = _shape(images)
    rs = None if reference is None else _shape(reference)
    if len(ims) not in (2, 3) or (rs is not None and len(rs) not in (2, 3)):
        raise ValueError(f"reference and images must be (H, W) or (T, H, W), got {rs} and {ims}")
    if rs is not None:
        if rs[-2:] != ims[-2:]:
            raise ValueError(f"reference frames {rs[-2:]} and image frames {ims[-2:]} differ in shape")
        if len(rs) == 3 and (len(ims) != 3 or rs[0] != ims[0]):
            raise ValueError(f"a (T, H, W) reference needs (T, H, W) images with the same T, got {rs} and {ims}")
    if 0 in ims or (rs is not None and 0 in rs):
        raise ValueError("empty reference or images")
    g = fringe_grid(ims[-2:], window=window, step=step)
    gy, gx = g["shape"]
    if unwrap and max(gy, gx) > MAX_UNWRAP_SIDE:
        raise _ffi.B4DSizeError(f"phase unwrapping is limited to {MAX_UNWRAP_SIDE} nodes per side, the grid is {(gy, gx)}")
    f = None if carriers is None else _check_carriers(carriers, g["window"], pair=True)
    weighted = weights is not None or mask is not None or min_visibility is not None or min_level is not None
    lvl, mvis = _threshold(min_level, "min_level", 1.0), _threshold(min_visibility, "min_visibility", 2.0)
    tol, iters_max = 1e-6, 500                                  # the defaults of phase_unwrap
    snr = isinstance(weights, str)
    if snr and weights != "snr":
        raise ValueError(f'weights must be None, "snr" or an array, got {weights!r}')
    maps_shape = ims[:-2] + (gy, gx)
    _check_weights(None if snr else weights, mask, maps_shape)
    torch = _ffi.require_gpu()
    img = _frames_device(images)
    ref = None if reference is None else _frames_device(reference)
    if f is None:
        src = img if ref is None else ref
        f = _check_carriers(fringe_carriers(src[0], window=window, step=step, min_level=min_level, min_visibility=min_visibility),
                            g["window"], pair=True)
    S = _demodulate_device(img, f, g)
    R = None if ref is None else _demodulate_device(ref, f, g)
    paired = rs is not None and len(rs) == 3
    phase, vis, trans, dark, peak = _compare_device(S, R, paired)
    n = int(img.shape[0])
    info = valid = wrapped = None
    if weighted:
        w = _fringe_weights_device(S, R, paired, lvl, mvis, snr)
        if mask is not None or not (snr or weights is None):
            w = w * _weights_device(None if snr else weights, mask, maps_shape)[0][:, None]     # (1 or n, 1, gy, gx) on (n, 2, gy, gx)
        w = w.reshape(2 * n, gy, gx)
        if unwrap:
            wrapped = phase
            phase, weff, it, rs_ = _unwrap_weighted_device(phase.reshape(2 * n, gy, gx), w, gy * gx, tol, iters_max, True)
            info = {k: v.reshape(n, 2) for k, v in _solver_info(it, rs_, tol, iters_max).items()}
            weff = weff.reshape(n, 2, gy, gx)
        else:
            ok = torch.isfinite(w) & (w > 0) & torch.isfinite(phase.reshape(2 * n, gy, gx))      # the rule of the unwrap's set-up kernel
            weff = torch.where(ok, w, torch.zeros_like(w)).reshape(n, 2, gy, gx)
        valid = (weff[:, 0] > 0) & (weff[:, 1] > 0)
        phase = torch.where(valid[:, None], phase.reshape(n, 2, gy, gx), torch.full_like(weff, float("nan")))
    elif unwrap:
        phase = _unwrap_device(phase.reshape(2 * n, gy, gx)).reshape(n, 2, gy, gx)
    minv = np.ascontiguousarray(np.linalg.inv(f), dtype=np.float64)
    dy = torch.empty((n, gy, gx), dtype=torch.float64, device=img.device)
    dx = torch.empty_like(dy)
    if wrapped is not None:      # weighted unwrap: the shift from the wrapped phase and the integer level, in float64
        _ffi.check(_ffi.lib().b4d_fringe_shift_levels(D.ptr(wrapped), D.ptr(wrapped[:, 1]), D.ptr(phase), D.ptr(phase[:, 1]), 2 * gy * gx,
                                                      n, gy, gx, minv.ctypes.data_as(C.c_void_p), D.ptr(dy), D.ptr(dx), _ffi.stream_ptr()))
    else:
        _ffi.check(_ffi.lib().b4d_fringe_shift(D.ptr(phase), D.ptr(phase[:, 1]), 2 * gy * gx, n, gy, gx, minv.ctypes.data_as(C.c_void_p),
                                               D.ptr(dy), D.ptr(dx), _ffi.stream_ptr()))
    res = {"dy": dy, "dx": dx, "peak": peak, "phase": phase, "visibility": vis}
    if R is not None:
        res["transmission"], res["dark_field"] = trans, dark
    for k, v in res.items():
        if len(ims) == 2:
            v = v[0]
        res[k] = v if return_tensors else v.cpu().numpy().astype(np.float64)
    if valid is not None:
        if len(ims) == 2:
            valid = valid[0]
        res["valid"] = valid if return_tensors else valid.cpu().numpy()
    res.update({"y": g["y"], "x": g["x"], "carriers": f,
                "meta": {"window": g["window"], "step": g["step"], "unwrap": bool(unwrap) if info is None else info,
                         "absolute": reference is None}})
    return res
