"""Phase-stepping analysis of grating scans: per-pixel transmission, differential phase and dark field at detector resolution
from a scan of T frames (``b4d_stepping_fit``, ``b4d_stepping_compare``), with self-calibration of the step positions from the
data (``b4d_stepping_calibrate_step``).  DESIGN.md section 23.

Signal model.  A scan is (T, H, W): a grating or diffuser stepped over T positions.  Per pixel, with step phases ``phi_t``
(radians, t = 0 .. T - 1) and K = ``harmonics`` in {1, 2}:

    I_t = a0 + sum_{k=1..K} a_k cos(k phi_t + ph_k) = a0 + sum_k (c_k cos k phi_t + s_k sin k phi_t)

with ``c_k = a_k cos ph_k``, ``s_k = -a_k sin ph_k`` and ``ph_k = atan2(-s_k, c_k)``: M = 2K + 1 unknowns, kept in the order
(a0, c_1, s_1, c_2, s_2) and found by least squares over the kept samples.
Step phases.  ``steps=None`` means ``phi_t = 2 pi periods t / T``; otherwise ``steps`` is a (T,) array of radians, uniform or not.
Basis table.  The host forms ``B`` (T, M), rows (1, cos phi_t, sin phi_t, cos 2 phi_t, sin 2 phi_t), its normal matrix
``G = B^T B`` and ``G^-1`` in float64 and hands them to the device, so device and model use the same numbers.
Dropped samples.  A sample is dropped for its pixel if it is not finite, or if ``saturation`` is given and the sample is
``>= saturation``.
Valid pixels.  A pixel is valid if it keeps at least M samples and the Cholesky factorisation of its M x M normal matrix (that of
the kept samples) has every pivot ``> 1e-10 x`` the largest diagonal entry.  Otherwise every output of the pixel is NaN and
``valid`` is False.
Derived maps.  ``mean = a0``, ``amplitude_k = a_k``, ``phase_k = ph_k`` in (-pi, pi], ``visibility_k = a_k / a0``,
``residual = sqrt(max(sum I^2 - b^T x, 0) / n_kept)`` (the rms of the fit residual; b = sum_t B_t I_t, x the solution).  Sample
against reference: ``transmission = a0_s / a0_r``, ``dpc_k = wrap_(-pi, pi](ph_k,s - ph_k,r)`` formed in float64,
``dark_field_k = visibility_k,s / visibility_k,r``; harmonic k of a pixel is valid if both pixels are valid, both ``a0 > 0`` and
``a_k,r > 0``.  ``shift = dpc_1 period / 2 pi`` in pixels: with steps counted positive in the direction in which they move the
fringes across the detector, a sample that displaces the fringes by d (frame(r) = ref(r - d), the convention of
``displacement_map``) gives ``shift = d``.
Step self-calibration (``calibrate_steps``): the advanced iterative algorithm of Wang & Han (Opt. Lett. 29, 1671, 2004) for a mean
and modulation that vary from pixel to pixel.  One iteration fits (a0, c, s) per pixel with the current steps, then fits every
frame as ``I_t(p) ~ g_t a0(p) + u_t c(p) + v_t s(p)`` over the pixels without a dropped sample and sets
``delta_t <- atan2(v_t, u_t) - atan2(v_0, u_0)``; ``g_t`` is the dose factor of frame t and ``hypot(u_t, v_t)`` its modulation.
Limits: 3 <= T <= 64 and T >= M; calibration takes K = 1 and 5 <= T <= 32 (with 3 or 4 steps the steps are under-determined).
Everything runs on the device; there is no host fallback.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from .. import _device as D
from .. import _ffi
from .displacement import _shape

MIN_STEPS = 3
MAX_STEPS = 64
CAL_MIN_STEPS = 5
CAL_MAX_STEPS = 32
PIVOT_RTOL = 1e-10
MAX_UNWRAP_SIDE = 2048      # the limit of phase_unwrap


# ------------------------------------------------------------------------------------------------------------ host checks
def _harmonics(harmonics) -> int:
    if isinstance(harmonics, (bool, np.bool_)) or not isinstance(harmonics, (int, np.integer)) or int(harmonics) not in (1, 2):
        raise ValueError(f"harmonics must be 1 or 2, got {harmonics!r}")
    return int(harmonics)


def _scan_shape(stack, name: str):
    s = _shape(stack)
    if len(s) not in (3, 4):
        raise ValueError(f"{name} must be (T, H, W) or (N, T, H, W), got {s}")
    if 0 in s:
        raise ValueError(f"empty {name} {s}")
    return s


def _check_count(T: int, K: int):
    if T < MIN_STEPS:
        raise ValueError(f"a scan needs at least {MIN_STEPS} steps, got {T}")
    if T > MAX_STEPS:
        raise NotImplementedError(f"scans are limited to {MAX_STEPS} steps, got {T}")
    if T < 2 * K + 1:
        raise ValueError(f"{K} harmonics have {2 * K + 1} unknowns per pixel, the scan has only {T} steps")


def _step_phases(T: int, steps, periods) -> np.ndarray:
    """(T,) float64 step phases in radians (host only)."""
    if steps is None:
        try:
            p = float(periods)
        except (TypeError, ValueError):
            raise ValueError(f"periods must be a number, got {periods!r}") from None
        if not np.isfinite(p) or p == 0.0:
            raise ValueError(f"periods must be finite and non-zero, got {periods!r}")
        return 2.0 * np.pi * p * np.arange(T, dtype=np.float64) / T
    try:
        phi = np.array(steps.cpu() if D.is_tensor(steps) else steps, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"steps must be a (T,) array of radians, got {steps!r}") from None
    if phi.shape != (T,):
        raise ValueError(f"steps must have shape ({T},), one phase per frame, got {phi.shape}")
    if not np.all(np.isfinite(phi)):
        raise ValueError("steps must be finite")
    return phi


def _saturation(saturation) -> float:
    if saturation is None:
        return float("inf")
    if isinstance(saturation, (bool, str)) or np.ndim(saturation) != 0:
        raise ValueError(f"saturation must be None or a number, got {saturation!r}")
    s = float(saturation)
    if np.isnan(s):
        raise ValueError("saturation must not be NaN")
    return s


def basis_table(steps, harmonics: int = 1) -> np.ndarray:
    """(T, 2K + 1) float64 basis table of the step phases: columns 1, cos phi, sin phi, cos 2 phi, sin 2 phi (host only)."""
    p = np.asarray(steps, dtype=np.float64)
    cols = [np.ones_like(p)]
    for k in range(1, int(harmonics) + 1):
        cols += [np.cos(k * p), np.sin(k * p)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def _pivots_ok(G: np.ndarray) -> bool:
    """The validity rule of a normal matrix: every Cholesky pivot above PIVOT_RTOL x the largest diagonal entry."""
    M = G.shape[0]
    L = np.zeros_like(G)
    floor = PIVOT_RTOL * np.max(np.diag(G))
    for j in range(M):
        d = G[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > floor:
            return False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, M):
            L[i, j] = (G[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return True


def _tables(phi: np.ndarray, K: int):
    """(B, G, G^-1 or None) of the step phases, float64 and C-contiguous."""
    B = basis_table(phi, K)
    G = np.ascontiguousarray(B.T @ B)
    Gi = np.ascontiguousarray(np.linalg.inv(G)) if _pivots_ok(G) else None
    return B, G, Gi


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------------------ device calls
def _scans_device(stack):
    """(n, T, H * W) float32 device tensor of a (T, H, W) or (N, T, H, W) input."""
    t, _, _ = D.to_device_f32(stack, ndim=(3, 4))
    T, H, W = (int(s) for s in t.shape[-3:])
    return t.reshape(-1, T, H * W)


def _fit_device(scans, phi: np.ndarray, K: int, sat: float):
    """coeff (n, M, npix) float32, residual (n, npix) float32, n_samples (n, npix) uint8 of the device scans (n, T, npix).  phi is
    (T,), shared, or (n, T), one row per scan (then one launch per scan)."""
    torch = _ffi.require_gpu()
    lib = _ffi.lib()
    n, T, npix = (int(s) for s in scans.shape)
    M = 2 * K + 1
    coeff = torch.empty((n, M, npix), dtype=torch.float32, device=scans.device)
    res = torch.empty((n, npix), dtype=torch.float32, device=scans.device)
    ns = torch.empty((n, npix), dtype=torch.uint8, device=scans.device)
    if phi.ndim == 1:
        B, G, Gi = _tables(phi, K)
        _ffi.check(lib.b4d_stepping_fit(D.ptr(scans), n, T, npix, K, _hp(B), _hp(G), _hp(Gi), sat, D.ptr(coeff), D.ptr(res), D.ptr(ns),
                                        _ffi.stream_ptr()))
    else:
        for i in range(n):
            B, G, Gi = _tables(phi[i], K)
            _ffi.check(lib.b4d_stepping_fit(D.ptr(scans[i]), 1, T, npix, K, _hp(B), _hp(G), _hp(Gi), sat, D.ptr(coeff[i]), D.ptr(res[i]),
                                            D.ptr(ns[i]), _ffi.stream_ptr()))
    return coeff, res, ns


def _derive_device(coeff, K: int):
    """amplitude, phase, visibility (n, K, npix) float32 and valid (n, npix) bool of the device coefficients (n, M, npix)."""
    torch = _ffi.require_gpu()
    n, _, npix = (int(s) for s in coeff.shape)
    amp = torch.empty((n, K, npix), dtype=torch.float32, device=coeff.device)
    ph, vis = torch.empty_like(amp), torch.empty_like(amp)
    valid = torch.empty((n, K, npix), dtype=torch.uint8, device=coeff.device)
    _ffi.check(_ffi.lib().b4d_stepping_compare(D.ptr(coeff), None, 0, n, K, npix, D.ptr(ph), D.ptr(vis), D.ptr(amp), None, None, None,
                                               D.ptr(valid), _ffi.stream_ptr()))
    return amp, ph, vis, valid[:, 0].bool()


def _compare_device(cs, cr, paired: bool, K: int):
    """dpc, visibility, visibility_ref, dark_field (n, K, npix) float32, transmission (n, npix) float32, valid (n, K, npix) bool."""
    torch = _ffi.require_gpu()
    n, M, npix = (int(s) for s in cs.shape)
    dpc = torch.empty((n, K, npix), dtype=torch.float32, device=cs.device)
    vis, visr, dark = torch.empty_like(dpc), torch.empty_like(dpc), torch.empty_like(dpc)
    trans = torch.empty((n, npix), dtype=torch.float32, device=cs.device)
    valid = torch.empty((n, K, npix), dtype=torch.uint8, device=cs.device)
    _ffi.check(_ffi.lib().b4d_stepping_compare(D.ptr(cs), D.ptr(cr), M * npix if paired else 0, n, K, npix, D.ptr(dpc), D.ptr(vis), None,
                                               D.ptr(trans), D.ptr(visr), D.ptr(dark), D.ptr(valid), _ffi.stream_ptr()))
    return dpc, vis, visr, dark, trans, valid.bool()


def _calibrate_device(scan, phi0: np.ndarray, sat: float, tol: float, max_iter: int):
    """Steps and info of one device scan (T, npix) from the starting phases phi0."""
    torch = _ffi.require_gpu()
    lib = _ffi.lib()
    T, npix = (int(s) for s in scan.shape)
    out = torch.empty((1 + 3 * T,), dtype=torch.float64, device=scan.device)
    delta = np.ascontiguousarray(phi0 - phi0[0])
    change, it = float("inf"), 0
    dose, mod = np.full(T, np.nan), np.full(T, np.nan)
    while it < max_iter:
        B, _, Gi = _tables(delta, 1)
        if Gi is None:      # the current steps give a singular fit (e.g. all equal): nothing to iterate on
            change = float("nan")
            break
        _ffi.check(lib.b4d_stepping_calibrate_step(D.ptr(scan), T, npix, _hp(B), _hp(Gi), _hp(delta), sat, D.ptr(out), _ffi.stream_ptr()))
        h = out.cpu().numpy()                       # the one read of the iteration
        it += 1
        change = float(h[0])
        if not np.isfinite(change):
            break
        delta, dose, mod = np.ascontiguousarray(h[1:1 + T]), h[1 + T:1 + 2 * T].copy(), h[1 + 2 * T:].copy()
        if change <= tol:
            break
    converged = bool(change <= tol)
    if not converged:
        warnings.warn(f"calibrate_steps: the steps still changed by {change:.3e} rad after {it} iterations (tol {tol:.3e})",
                      RuntimeWarning, stacklevel=3)
    return delta + phi0[0], {"iterations": it, "change": change, "converged": converged, "dose": dose, "modulation": mod}


def _check_calibration(T: int, tol, max_iter):
    if T < CAL_MIN_STEPS:
        raise ValueError(f"step calibration needs at least {CAL_MIN_STEPS} steps (with 3 or 4 the steps are under-determined), got {T}")
    if T > CAL_MAX_STEPS:
        raise NotImplementedError(f"step calibration is limited to {CAL_MAX_STEPS} steps, got {T}")
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    if isinstance(tol, (bool, str)) or np.ndim(tol) != 0 or not float(tol) >= 0.0:
        raise ValueError(f"tol must be a number >= 0, got {tol!r}")
    return float(tol), int(max_iter)


def _host(t, return_tensors: bool, dtype=np.float64):
    return t if return_tensors else t.cpu().numpy().astype(dtype, copy=False)


def _fit_dict(coeff, res, ns, K: int, lead, H: int, W: int, phi, return_tensors: bool, meta: dict) -> dict:
    amp, ph, vis, valid = _derive_device(coeff, K)
    r = {"mean": _host(coeff[:, 0].reshape(lead + (H, W)), return_tensors),
         "amplitude": _host(amp.reshape(lead + (K, H, W)), return_tensors),
         "phase": _host(ph.reshape(lead + (K, H, W)), return_tensors),
         "visibility": _host(vis.reshape(lead + (K, H, W)), return_tensors),
         "residual": _host(res.reshape(lead + (H, W)), return_tensors),
         "n_samples": _host(ns.reshape(lead + (H, W)), return_tensors, np.uint8),
         "valid": _host(valid.reshape(lead + (H, W)), return_tensors, bool),
         "steps": phi, "meta": meta}
    return r


# ------------------------------------------------------------------------------------------------------------ public
def stepping_fit(stack, *, steps=None, periods=1.0, harmonics=1, saturation=None, return_tensors: bool = False) -> dict:
    """Per-pixel harmonic fit of a stepping scan ``stack``, (T, H, W) or (N, T, H, W); any real dtype and layout, or ROCm tensors.

    Returns {"mean", "residual": (..., H, W); "amplitude", "phase", "visibility": (..., K, H, W); "n_samples": (..., H, W) uint8,
    the kept samples; "valid": (..., H, W) bool; "steps": the (T,) radians used; "meta"} (module docstring).  Maps are float64
    NumPy, or float32 device tensors with ``return_tensors=True``.  ValueError for bad shapes, T < 3, T < 2K + 1, ``harmonics``
    outside {1, 2} and steps of the wrong length or not finite; NotImplementedError for T > 64 -- all before the GPU is touched."""
    s = _scan_shape(stack, "stack")
    K = _harmonics(harmonics)
    T, H, W = s[-3:]
    _check_count(T, K)
    phi = _step_phases(T, steps, periods)
    sat = _saturation(saturation)
    _ffi.require_gpu()
    scans = _scans_device(stack)
    coeff, res, ns = _fit_device(scans, phi, K, sat)
    return _fit_dict(coeff, res, ns, K, s[:-3], H, W, phi, return_tensors, {"harmonics": K, "saturation": saturation})


def calibrate_steps(stack, *, steps=None, periods=1.0, saturation=None, tol=1e-9, max_iter=200):
    """Step phases of a scan ``stack`` (T, H, W) recovered from the data itself (module docstring), starting from ``steps`` (or the
    uniform ones).  The first step keeps its value: the result is ``steps[0] + delta`` with ``delta_0 = 0``.  Pixels with a
    dropped sample take no part.

    Returns ``(steps, info)``: (T,) float64 radians and {"iterations", "change": the last max |change| in radians, "converged",
    "dose": (T,) the dose factor of every frame, "modulation": (T,) its fringe modulation against the mean of the scan}.  The host
    reads the change once per iteration and stops at ``tol`` or ``max_iter``; stopping above ``tol`` raises a RuntimeWarning and
    still returns.  ValueError for T < 5, NotImplementedError for T > 32, both before the GPU is touched."""
    s = _shape(stack)
    if len(s) != 3:
        raise ValueError(f"stack must be (T, H, W), got {s}")
    if 0 in s:
        raise ValueError(f"empty stack {s}")
    T = s[0]
    tol, max_iter = _check_calibration(T, tol, max_iter)
    phi = _step_phases(T, steps, periods)
    sat = _saturation(saturation)
    _ffi.require_gpu()
    scans = _scans_device(stack)
    return _calibrate_device(scans[0], phi, sat, tol, max_iter)


def phase_stepping(sample, reference, *, steps=None, periods=1.0, harmonics=1, saturation=None, calibrate: bool = False,
                   unwrap: bool = False, period=None, return_tensors: bool = False) -> dict:
    """Transmission, differential phase and dark field of a ``sample`` scan, (T, H, W) or (N, T, H, W), against a ``reference``
    scan: (T, H, W), shared by every sample scan, or (N, T, H, W), paired scan by scan.  Both scans have the same T and steps.

    ``calibrate=True`` recovers the steps of every scan from its own data first (``calibrate_steps`` at its default ``tol`` and
    ``max_iter``; K = 1 for the calibration, the fit then uses ``harmonics``).  ``unwrap=True`` sends ``dpc`` of the first harmonic through
    ``phase_unwrap`` with ``mask=valid`` (NaN at invalid pixels).  ``period``, the fringe period in pixels, adds
    ``shift = dpc_1 period / 2 pi``.
    Returns {"transmission": (..., H, W); "dpc", "dark_field", "visibility" (the sample's): (..., K, H, W); "valid": (..., H, W)
    bool, the flag of the first harmonic, "valid_harmonics": (..., K, H, W); "sample", "reference": the two ``stepping_fit``
    dicts; "steps": (2, T), sample row then reference row -- (2, N, T) when N sample scans were calibrated, each with its own
    steps; "shift" with ``period``; "meta"}.  ValueError for reference and sample frames of different shape or count and for
    everything ``stepping_fit`` and ``calibrate_steps`` refuse; NotImplementedError for T > 64 (32 when calibrating) and for a
    side above 2048 when unwrapping -- all before the GPU is touched."""
    ss, rs = _scan_shape(sample, "sample"), _scan_shape(reference, "reference")
    if ss[-2:] != rs[-2:]:
        raise ValueError(f"reference frames {rs[-2:]} and sample frames {ss[-2:]} differ in shape")
    if ss[-3] != rs[-3]:
        raise ValueError(f"reference and sample scans differ in their number of steps: {rs[-3]} and {ss[-3]}")
    if len(rs) == 4 and (len(ss) != 4 or rs[0] != ss[0]):
        raise ValueError(f"an (N, T, H, W) reference needs an (N, T, H, W) sample with the same N, got {rs} and {ss}")
    K = _harmonics(harmonics)
    T, H, W = ss[-3:]
    _check_count(T, K)
    phi = _step_phases(T, steps, periods)
    sat = _saturation(saturation)
    if calibrate:
        tol, max_iter = _check_calibration(T, 1e-9, 200)         # the defaults of calibrate_steps
    if unwrap and max(H, W) > MAX_UNWRAP_SIDE:
        raise _ffi.B4DSizeError(f"phase unwrapping is limited to {MAX_UNWRAP_SIDE} nodes per side, the frames are {(H, W)}")
    scale = None
    if period is not None:
        if isinstance(period, (bool, str)) or np.ndim(period) != 0 or not np.isfinite(float(period)) or float(period) <= 0.0:
            raise ValueError(f"period must be a positive number of pixels, got {period!r}")
        scale = float(period) / (2.0 * np.pi)
    torch = _ffi.require_gpu()
    S, R = _scans_device(sample), _scans_device(reference)
    n, paired = int(S.shape[0]), len(rs) == 4
    phi_s = phi_r = phi
    cal = None
    if calibrate:
        cs_ = [_calibrate_device(S[i], phi, sat, tol, max_iter) for i in range(n)]
        cr_ = [_calibrate_device(R[i], phi, sat, tol, max_iter) for i in range(int(R.shape[0]))]
        phi_s = np.stack([c[0] for c in cs_]) if len(ss) == 4 else cs_[0][0]
        phi_r = np.stack([c[0] for c in cr_]) if paired else cr_[0][0]
        cal = {"sample": [c[1] for c in cs_], "reference": [c[1] for c in cr_]}
    cs, res_s, ns_s = _fit_device(S, phi_s, K, sat)
    cr, res_r, ns_r = _fit_device(R, phi_r, K, sat)
    dpc, vis, _, dark, trans, validk = _compare_device(cs, cr, paired, K)
    lead = ss[:-3]
    valid = validk[:, 0].reshape(n, H, W)
    dpc = dpc.reshape(n, K, H, W)
    info = None
    if unwrap:
        from .fringes import phase_unwrap

        un, info = phase_unwrap(dpc[:, 0].contiguous(), mask=valid.to(torch.uint8), return_info=True, return_tensors=True)
        dpc = torch.cat([un.reshape(n, 1, H, W), dpc[:, 1:]], dim=1)
    meta = {"harmonics": K, "saturation": saturation, "calibrated": bool(calibrate), "unwrap": bool(unwrap) if info is None else info,
            "period": period}
    if cal is not None:
        meta["calibration"] = cal
    fit_meta = {"harmonics": K, "saturation": saturation}
    out = {"transmission": _host(trans.reshape(lead + (H, W)), return_tensors),
           "dpc": _host(dpc.reshape(lead + (K, H, W)), return_tensors),
           "dark_field": _host(dark.reshape(lead + (K, H, W)), return_tensors),
           "visibility": _host(vis.reshape(lead + (K, H, W)), return_tensors),
           "valid": _host(valid.reshape(lead + (H, W)), return_tensors, bool),
           "valid_harmonics": _host(validk.reshape(lead + (K, H, W)), return_tensors, bool),
           "sample": _fit_dict(cs, res_s, ns_s, K, lead, H, W, phi_s, return_tensors, fit_meta),
           "reference": _fit_dict(cr, res_r, ns_r, K, rs[:-3], H, W, phi_r, return_tensors, fit_meta)}
    if scale is not None:
        sh = dpc[:, 0].reshape(lead + (H, W)).double() * scale
        out["shift"] = sh if return_tensors else sh.cpu().numpy()
    if phi_s.ndim == 2:
        out["steps"] = np.stack([phi_s, phi_r if phi_r.ndim == 2 else np.broadcast_to(phi_r, phi_s.shape)])
    else:
        out["steps"] = np.stack([phi_s, phi_r])
    out["meta"] = meta
    return out


def stepping_displacement(scan_x, scan_y, *, period) -> dict:
    """A ``displacement_map``-compatible dict from two ``phase_stepping`` results of orthogonal gratings: ``scan_x`` stepped along
    x (its ``dpc`` measures the shift along x), ``scan_y`` along y.  ``period``: the fringe period in pixels, a number or a
    (period_y, period_x) pair.  Host only apart from elementwise arithmetic on device tensors, if the scans hold tensors.

    Returns {"dy", "dx": ``dpc_1 period / 2 pi`` of scan_y and scan_x, float64; "peak": the smaller first-harmonic visibility of
    the two sample scans; "valid": the AND of the two ``valid`` maps; "transmission": the mean of the two; "dark_field":
    (2, H, W) (or (N, 2, H, W)), first harmonic of scan_y then scan_x; "y", "x": ``arange(H)``, ``arange(W)``; "meta"}:
    ``wavefront_from_displacement(m, pixel_size=..., distance=..., mask=m["valid"])`` takes it as it is."""
    for name, s in (("scan_x", scan_x), ("scan_y", scan_y)):
        if not isinstance(s, dict) or any(k not in s for k in ("dpc", "valid", "visibility", "transmission", "dark_field")):
            raise ValueError(f"{name} must be a phase_stepping result")
    if np.ndim(period) == 0:
        py = px = period
    elif np.ndim(period) == 1 and len(period) == 2:
        py, px = period
    else:
        raise ValueError(f"period must be a number or a (period_y, period_x) pair, got {period!r}")
    if isinstance(py, (bool, str)) or isinstance(px, (bool, str)) or not (np.isfinite(float(py)) and np.isfinite(float(px))) \
            or float(py) <= 0.0 or float(px) <= 0.0:
        raise ValueError(f"period must be positive and finite, got {period!r}")
    sx, sy = _shape(scan_x["dpc"]), _shape(scan_y["dpc"])
    if sx != sy or len(sx) not in (3, 4):
        raise ValueError(f"the two scans must have dpc maps of one shape, (K, H, W) or (N, K, H, W); got {sx} and {sy}")
    H, W = sx[-2:]
    tens = D.is_tensor(scan_x["dpc"])
    if tens != D.is_tensor(scan_y["dpc"]):
        raise ValueError("the two scans must both hold NumPy arrays or both device tensors")

    def first(a):       # the first harmonic of a (..., K, H, W) map
        return a[..., 0, :, :]

    if tens:
        import torch

        dy = first(scan_y["dpc"]).double() * (float(py) / (2.0 * np.pi))
        dx = first(scan_x["dpc"]).double() * (float(px) / (2.0 * np.pi))
        peak = torch.minimum(first(scan_y["visibility"]), first(scan_x["visibility"])).double()
        dark = torch.stack([first(scan_y["dark_field"]), first(scan_x["dark_field"])], dim=-3)
        trans = 0.5 * (scan_y["transmission"].double() + scan_x["transmission"].double())
    else:
        dy = np.asarray(first(scan_y["dpc"]), dtype=np.float64) * (float(py) / (2.0 * np.pi))
        dx = np.asarray(first(scan_x["dpc"]), dtype=np.float64) * (float(px) / (2.0 * np.pi))
        peak = np.minimum(first(scan_y["visibility"]), first(scan_x["visibility"]))
        dark = np.stack([first(scan_y["dark_field"]), first(scan_x["dark_field"])], axis=-3)
        trans = 0.5 * (scan_y["transmission"] + scan_x["transmission"])
    return {"dy": dy, "dx": dx, "peak": peak, "valid": scan_y["valid"] & scan_x["valid"],
            "transmission": trans, "dark_field": dark,
            "y": np.arange(H, dtype=np.float64), "x": np.arange(W, dtype=np.float64),
            "meta": {"period": (float(py), float(px)), "source": "phase_stepping"}}
