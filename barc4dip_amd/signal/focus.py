"""Focal spot and caustic predicted from a measured wavefront map (``b4d_focal_spot``).

``wavefront_from_displacement(..., remove="quadratic")`` returns the two inputs of the Fresnel integral: the figure error ``e``
(metres) and the six coefficients ``c`` of ``(1, u, v, u^2, u v, v^2)``, ``u`` along x and ``v`` along y in metres from the grid
centre.  For a plane at the signed distance ``z != 0`` from the measurement plane (a beam diverging from a focus at the distance
R upstream has its focus at ``z = -R``) the pupil is ``U = A exp(i phi)`` on the valid nodes and 0 elsewhere, with

    phi = (2 pi / lambda) (e + c0 + c1 u + c2 v + c3 u^2 + c4 u v + c5 v^2) + (pi / (lambda z)) (u^2 + v^2)

in float64, placed at the corner of a zero canvas ``(Py, Px)``, and the plane's intensity is

    I = |fftshift(fft2(U_canvas))|^2 / (sum A)^2,

``sum A`` over the valid nodes.  Constant phase and amplitude prefactors of the Fresnel integral are dropped: the unit is the peak
of the aberration-free, in-focus pupil of the same amplitude, so the peak of a plane is its Strehl ratio, and
``sum I = Py Px sum A^2 / (sum A)^2``.  Bin ``j`` of the shifted plane sits at ``(j - Px // 2) lambda z / (Px hx)`` metres along
x, and likewise along y; with ``z < 0`` the axes descend, and they are returned as they are.

The transform is the complex-to-complex engine of the general-length plans; there is no host fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from ..maths.stats import width_at_fraction
from . import wavefront as _wf

MIN_CANVAS, MAX_CANVAS = 64, 4096


def _coefficients(coefficients, T=None) -> np.ndarray:
    try:
        c = np.asarray(coefficients.cpu() if D.is_tensor(coefficients) else coefficients, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"coefficients must be (6,) or (T, 6) numbers, got {coefficients!r}") from None
    if c.ndim == 1:
        c = c[None]
    if c.ndim != 2 or c.shape[1] != 6 or c.shape[0] < 1:
        raise ValueError(f"coefficients must be (6,) or (T, 6), got shape {np.shape(coefficients)}")
    if not np.all(np.isfinite(c)):
        raise ValueError("coefficients must be finite")
    if T is not None and c.shape[0] != T:
        if c.shape[0] != 1:
            raise ValueError(f"{c.shape[0]} coefficient sets for {T} maps")
        c = np.repeat(c, T, axis=0)
    return np.ascontiguousarray(c)


def _focus_of(c: np.ndarray) -> float:
    """z = -(Rx + Ry) / 2 with Rx = 1 / (2 c3), Ry = 1 / (2 c5), the radii averaged over the maps."""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = -0.5 * float(np.mean(1.0 / (2.0 * c[:, 3])) + np.mean(1.0 / (2.0 * c[:, 5])))
    if not np.isfinite(z) or z == 0.0:
        raise ValueError("planes=None places one plane at z = -(Rx + Ry) / 2, which is not finite and non-zero for these "
                         "coefficients: pass planes explicitly")
    return z


def _planes(planes, c: np.ndarray) -> np.ndarray:
    if planes is None:
        return np.array([_focus_of(c)])
    try:
        z = np.atleast_1d(np.asarray(planes, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"planes must be a number or a 1-D sequence of numbers, got {planes!r}") from None
    if z.ndim != 1 or z.size < 1:
        raise ValueError(f"planes must be a number or a non-empty 1-D sequence, got shape {z.shape}")
    if not np.all(np.isfinite(z)) or np.any(z == 0.0):
        raise ValueError("plane positions must be finite and non-zero (z is the distance from the measurement plane)")
    return np.ascontiguousarray(z)


def _pair_of(v, name: str):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (y, x) pair, got {v!r}") from None
    return a, b


def _canvas(ny: int, nx: int, pad, canvas):
    if canvas is None:
        if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 1:
            raise ValueError(f"pad must be an integer >= 1, got {pad!r}")
        sides = []
        for s in (ny, nx):
            p = 1
            while p < int(pad) * s:
                p *= 2
            sides.append(min(max(p, MIN_CANVAS), MAX_CANVAS))
        Py, Px = sides
    else:
        cv = (canvas, canvas) if isinstance(canvas, (int, np.integer)) and not isinstance(canvas, bool) else _pair_of(canvas, "canvas")
        for s in cv:
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
                raise ValueError(f"canvas must be an integer or a (Py, Px) pair of integers, got {canvas!r}")
        Py, Px = (int(s) for s in cv)
    if not (MIN_CANVAS <= Py <= MAX_CANVAS and MIN_CANVAS <= Px <= MAX_CANVAS):
        raise _ffi.B4DSizeError(f"canvas sides must lie in [{MIN_CANVAS}, {MAX_CANVAS}], got {(Py, Px)}")
    if Py < ny or Px < nx:
        raise _ffi.B4DSizeError(f"a ({ny}, {nx}) map does not fit the canvas {(Py, Px)}")
    if not _ffi.supported(Py, Px):
        raise _ffi.B4DSizeError(f"no transform plan for a canvas of {(Py, Px)}")
    return Py, Px


def _phase_step(ny, nx, hy, hx, lam, z, c):
    """(T, Z, 2): the largest node-to-node step (y, x) of the analytic phase over the grid.  The step is linear in (u, v), so its
    largest magnitude is attained at a corner of the rectangle of node pairs."""
    T, Z = c.shape[0], z.size
    out = np.zeros((T, Z, 2))
    k, ch = 2.0 * np.pi / lam, np.pi / (lam * z)                       # (Z,)
    u = (np.array([0.0, max(nx - 1, 0)]) - 0.5 * (nx - 1)) * hx       # extreme nodes
    v = (np.array([0.0, max(ny - 1, 0)]) - 0.5 * (ny - 1)) * hy
    c1, c2, c3, c4, c5 = (c[:, i][:, None, None, None] for i in range(1, 6))
    chz = ch[None, :, None, None]
    if nx > 1:
        ua = np.array([u[0], u[1] - hx])[None, None, :, None]          # first node of the first and of the last pair
        vv = v[None, None, None, :]
        dx = k * (c1 * hx + c3 * (2.0 * ua * hx + hx * hx) + c4 * hx * vv) + chz * (2.0 * ua * hx + hx * hx)
        out[:, :, 1] = np.max(np.abs(dx), axis=(2, 3))
    if ny > 1:
        va = np.array([v[0], v[1] - hy])[None, None, None, :]
        uu = u[None, None, :, None]
        dy = k * (c2 * hy + c5 * (2.0 * va * hy + hy * hy) + c4 * hy * uu) + chz * (2.0 * va * hy + hy * hy)
        out[:, :, 0] = np.max(np.abs(dy), axis=(2, 3))
    return out


def focus_geometry(shape, *, spacing, wavelength, planes, coefficients, pad=4, canvas=None) -> dict:
    """Host-only geometry of ``focal_spot`` for maps of ``shape`` = (ny, nx) (no device needed).

    spacing: node spacings ``(hy, hx)`` in metres; ``planes``: plane positions z (a number, a sequence, or None for the one plane
    at ``-(Rx + Ry) / 2``); ``coefficients``: (6,) or (T, 6).  The canvas is ``canvas`` (an integer or ``(Py, Px)``) or, per
    side, the next power of two >= ``pad`` x side, clipped to [64, 4096].
    Returns {"canvas": (Py, Px); "planes": (Z,); "y": (Z, Py), "x": (Z, Px): the plane axes in metres, bin j at
    ``(j - P // 2) lambda z / (P h)``, descending for z < 0; "pixel_size": (Z, 2), the magnitudes of the bin steps (y, x);
    "phase_step": (T, Z, 2), the largest node-to-node step (y, x) in radians of the ANALYTIC part of the pupil phase, polynomial
    plus chirp, over the grid rectangle -- the figure error and the mask are not part of it}.
    ValueError for bad arguments; B4DSizeError for a canvas outside [64, 4096], smaller than the map or without a plan."""
    try:
        ny, nx = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be (ny, nx), got {shape!r}") from None
    if ny < 1 or nx < 1:
        raise ValueError(f"shape must be (ny, nx) with sides >= 1, got {shape!r}")
    sy, sx = _pair_of(spacing, "spacing")
    hy, hx = _wf._spacing(sy, "spacing[0]"), _wf._spacing(sx, "spacing[1]")
    lam = _wf._spacing(wavelength, "wavelength")
    c = _coefficients(coefficients)
    z = _planes(planes, c)
    Py, Px = _canvas(ny, nx, pad, canvas)
    dy, dx = lam * z / (Py * hy), lam * z / (Px * hx)                  # signed bin steps, (Z,)
    return {"canvas": (Py, Px), "planes": z,
            "y": (np.arange(Py) - Py // 2)[None, :] * dy[:, None], "x": (np.arange(Px) - Px // 2)[None, :] * dx[:, None],
            "pixel_size": np.stack([np.abs(dy), np.abs(dx)], axis=1), "phase_step": _phase_step(ny, nx, hy, hx, lam, z, c)}


def _parse_input(w, pixel_size, spacing, mask, coefficients):
    """(maps, mask, coefficients or None, (hy, hx)) of a wavefront dict or plain maps; host only."""
    if isinstance(w, dict):
        if "wavefront" not in w:
            raise ValueError('a wavefront dict needs the key "wavefront"')
        maps = w["wavefront"]
        shape = _wf._shape(maps)
        if mask is None and "valid" in w:
            mask = w["valid"]
        if coefficients is None:
            if w.get("remove", None) != "quadratic" or "coefficients" not in w:
                raise ValueError('a wavefront dict must come from wavefront_from_displacement(..., remove="quadratic"), which '
                                 "leaves the figure error and its six coefficients; for any other map pass coefficients "
                                 "explicitly (the library cannot tell what was already subtracted)")
            coefficients = w["coefficients"]
        if spacing is None:
            if pixel_size is None or "y" not in w or "x" not in w:
                raise ValueError('a wavefront dict needs pixel_size (with its "y" and "x" axes in pixels) or spacing=(hy, hx)')
            if len(shape) not in (2, 3):
                raise ValueError(f"wavefront maps must be (ny, nx) or (T, ny, nx), got {shape}")
            from ..preprocessing.distortion import _regular_axis     # not at import time: preprocessing imports this package

            p = _wf._spacing(pixel_size, "pixel_size")
            spacing = (abs(_regular_axis(w["y"], shape[-2], "y")[1]) * p, abs(_regular_axis(w["x"], shape[-1], "x")[1]) * p)
    else:
        maps = w
        if spacing is None:
            raise ValueError("plain maps need spacing=(hy, hx) in metres")
        if coefficients is None:
            raise ValueError("plain maps need coefficients, (6,) or (T, 6): the quadratic part of the wavefront")
    shape = _wf._shape(maps)
    if len(shape) not in (2, 3):
        raise ValueError(f"wavefront maps must be (ny, nx) or (T, ny, nx), got {shape}")
    if 0 in shape:
        raise ValueError(f"empty wavefront maps {shape}")
    return maps, shape, mask, coefficients, spacing


def _crop(crop, Py, Px):
    if crop is None or crop is True:
        return Py, Px
    if crop is False:
        return None
    cv = (crop, crop) if isinstance(crop, (int, np.integer)) else _pair_of(crop, "crop")
    for s in cv:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1:
            raise ValueError(f"crop must be None, False, an integer >= 1 or a (cy, cx) pair of them, got {crop!r}")
    cy, cx = (int(s) for s in cv)
    if cy > Py or cx > Px:
        raise ValueError(f"the crop {(cy, cx)} exceeds the canvas {(Py, Px)}")
    return cy, cx


def focal_spot(w, *, wavelength, pixel_size=None, spacing=None, planes=None, amplitude=None, mask=None, coefficients=None, pad=4,
               canvas=None, crop=None, check_sampling=True, return_tensors=False, chunk=None) -> dict:
    """Intensity, Strehl ratio, centroid, widths and marginal profiles of the beam in the planes ``planes`` (module docstring).

    w: the dict of ``wavefront_from_displacement(..., remove="quadratic")`` -- its "wavefront" is the figure error, "valid" (if
    present) the mask when none is passed, "coefficients" the quadratic part, and the steps of "y" and "x" times ``pixel_size``
    the node spacings -- or plain maps (ny, nx) or (T, ny, nx) in metres with ``spacing=(hy, hx)`` and ``coefficients``.  A dict
    from another ``remove`` needs ``coefficients`` passed explicitly (ValueError otherwise).  NaN in a map, ``mask == False`` and
    an ``amplitude`` that is not finite and positive mean outside the aperture.  ``amplitude`` (>= 0) and ``mask`` are (ny, nx),
    shared by the maps, or shaped like them.  ``planes=None`` is the single plane ``z = -(Rx + Ry) / 2`` of the coefficients
    (the radii averaged over the maps).  ``crop``: None for the whole canvas, False for no intensity, or the window ``(cy, cx)``
    centred on the DC bin.  ``chunk``: (map, plane) pairs per pass through the transform (default: the plan's; results do not
    depend on it, bit for bit).

    The analytic part of the phase, polynomial plus chirp, must be sampled: ValueError when its largest node-to-node step
    ("phase_step") exceeds pi, unless ``check_sampling=False``.  The figure error and the mask are not part of that check.

    Returns {"intensity": (T, Z, cy, cx) float32 (a device tensor with ``return_tensors=True``; absent for ``crop=False``);
    "strehl": (T, Z) the peak; "peak_index": (T, Z, 2) its first (row, column) in the shifted canvas, -1 without one; "total";
    "centroid_y", "centroid_x", "sigma_y", "sigma_x": metres on the plane axes, from the moments over the whole canvas;
    "fwhm_y", "fwhm_x": metres, ``width_at_fraction(0.5)`` of the marginals; "profile_y": (T, Z, Py), "profile_x": (T, Z, Px),
    the marginals (sums of I over the other axis: the caustic images); "y", "x", "pixel_size", "phase_step", "canvas", "planes"
    as ``focus_geometry``; "sum_amplitude": (T,)}.  T = 1 for a 2-D call.  A map without a valid node gives NaN, no error.
    Argument errors are raised before the GPU is touched."""
    maps, shape, mask, coefficients, spacing = _parse_input(w, pixel_size, spacing, mask, coefficients)
    ny, nx = shape[-2:]
    T = shape[0] if len(shape) == 3 else 1
    c = _coefficients(coefficients, T)
    geo = focus_geometry((ny, nx), spacing=spacing, wavelength=wavelength, planes=planes, coefficients=c, pad=pad, canvas=canvas)
    hy, hx = (float(s) for s in spacing)
    lam = float(wavelength)
    z = geo["planes"]
    Z = int(z.size)
    Py, Px = geo["canvas"]
    if check_sampling and np.max(geo["phase_step"]) > np.pi:
        raise ValueError(f"the pupil phase is undersampled: its analytic part steps by up to {np.max(geo['phase_step']) / np.pi:.3g} pi "
                         "between neighbouring nodes (planes too far from the focus for this grid); check_sampling=False overrides")
    win = _crop(crop, Py, Px)
    _wf._check_weights(amplitude, mask, shape)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1):
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")

    torch = _ffi.require_gpu()
    err = D.to_device_f32(maps, ndim=(2, 3))[0].reshape(-1, ny, nx)
    n = int(err.shape[0])
    if mask is not None:
        m = (mask != 0) if D.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        m = m.to("cuda").reshape(-1, ny, nx)
        err = torch.where(m, err, torch.full((), float("nan"), dtype=torch.float32, device=err.device)).contiguous()
    if amplitude is None:
        amp, aptr, stride = None, None, 0
    else:
        amp = D.to_device_f32(amplitude, ndim=(2, 3))[0].reshape(-1, ny, nx).contiguous()
        if int(amp.shape[0]) not in (1, n):
            raise ValueError(f"{int(amp.shape[0])} amplitude maps for {n} wavefront maps")
        aptr, stride = D.ptr(amp), (ny * nx if int(amp.shape[0]) > 1 else 0)
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    pl = _ffi.get_plan(Py, Px, None if chunk is None else int(chunk), general=True)
    cdev = torch.from_numpy(c).to("cuda")
    zbuf = (C.c_double * Z)(*z.tolist())
    ws = torch.empty(max(1, int(lib.b4d_focal_spot_workspace_bytes(pl.handle, n, Z))), dtype=torch.uint8, device=err.device)
    stats = torch.empty((n, Z, 10), dtype=torch.float64, device=err.device)
    mx = torch.empty((n, Z, Px), dtype=torch.float64, device=err.device)
    my = torch.empty((n, Z, Py), dtype=torch.float64, device=err.device)
    inten = None if win is None else torch.empty((n, Z) + win, dtype=torch.float32, device=err.device)
    cy, cx = win if win is not None else (0, 0)
    _ffi.check(lib.b4d_focal_spot(pl.handle, D.ptr(err), aptr, stride, n, ny, nx, D.ptr(cdev), hy, hx, lam,
                                  C.cast(zbuf, C.c_void_p), Z, cy, cx, D.ptr(inten) if inten is not None else None, D.ptr(stats),
                                  D.ptr(mx), D.ptr(my), D.ptr(ws), st))
    s, px, py = stats.cpu().numpy(), mx.cpu().numpy(), my.cpu().numpy()
    res = dict(geo)
    if inten is not None:
        res["intensity"] = inten if return_tensors else inten.cpu().numpy()
    res.update(_derived(s, py, px, z, lam, hy, hx, Py, Px))
    res["profile_y"], res["profile_x"] = py, px
    return res


def _derived(s, py, px, z, lam, hy, hx, Py, Px) -> dict:
    """Host arithmetic on the (T, Z, 10) statistics and the marginals."""
    dy, dx = lam * z / (Py * hy), lam * z / (Px * hx)           # signed bin steps (Z,)
    tot = s[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mp, mq = s[..., 3] / tot, s[..., 4] / tot
        vp, vq = np.maximum(s[..., 5] / tot - mp * mp, 0.0), np.maximum(s[..., 6] / tot - mq * mq, 0.0)
    idx = s[..., 2]
    ok = np.isfinite(idx)
    flat = np.where(ok, idx, 0.0).astype(np.int64)
    peak = np.stack([np.where(ok, flat // Px, -1), np.where(ok, flat % Px, -1)], axis=-1)
    n, Z = tot.shape
    fy, fx = np.full((n, Z), np.nan), np.full((n, Z), np.nan)
    for t in range(n):
        for k in range(Z):
            if np.all(np.isfinite(py[t, k])) and np.all(np.isfinite(px[t, k])):
                fy[t, k] = width_at_fraction(py[t, k], fraction=0.5)[0]
                fx[t, k] = width_at_fraction(px[t, k], fraction=0.5)[0]
    return {"strehl": s[..., 1], "peak_index": peak, "total": tot,
            "centroid_y": mp * dy[None, :], "centroid_x": mq * dx[None, :],
            "sigma_y": np.sqrt(vp) * np.abs(dy)[None, :], "sigma_x": np.sqrt(vq) * np.abs(dx)[None, :],
            "fwhm_y": fy * np.abs(dy)[None, :], "fwhm_x": fx * np.abs(dx)[None, :],
            "moments": s[..., 3:8].copy(), "sum_amplitude": s[:, 0, 8].copy()}


def beam_caustic(w, *, span, n_planes, z_focus=None, wavelength, pixel_size=None, spacing=None, coefficients=None, crop=False,
                 **kwargs) -> dict:
    """``focal_spot`` in ``n_planes`` planes ``z_focus + linspace(-span / 2, span / 2, n_planes)``; ``z_focus`` defaults to
    ``-(Rx + Ry) / 2`` of the coefficients.  No intensity crop by default (``crop=False``); "profile_y" and "profile_x" are the
    y-z and x-z caustic images.  Adds "z", the plane positions, and "best_focus": (T,), the plane of largest Strehl ratio (NaN
    for a map without a valid node).  Other keywords as ``focal_spot``."""
    try:
        sp = float(span)
    except (TypeError, ValueError):
        raise ValueError(f"span must be a finite number >= 0, got {span!r}") from None
    if not np.isfinite(sp) or sp < 0.0:
        raise ValueError(f"span must be a finite number >= 0, got {span!r}")
    if isinstance(n_planes, bool) or not isinstance(n_planes, (int, np.integer)) or n_planes < 1:
        raise ValueError(f"n_planes must be an integer >= 1, got {n_planes!r}")
    if "planes" in kwargs:
        raise ValueError("beam_caustic builds its planes from span and n_planes; use focal_spot for explicit planes")
    if z_focus is None:
        _, shape, _, cf, _ = _parse_input(w, pixel_size, spacing, kwargs.get("mask"), coefficients)
        z0 = _focus_of(_coefficients(cf, shape[0] if len(shape) == 3 else 1))
    else:
        z0 = float(z_focus)
        if not np.isfinite(z0):
            raise ValueError(f"z_focus must be finite, got {z_focus!r}")
    z = z0 + np.linspace(-0.5 * sp, 0.5 * sp, int(n_planes))
    res = focal_spot(w, wavelength=wavelength, pixel_size=pixel_size, spacing=spacing, planes=z, coefficients=coefficients, crop=crop,
                     **kwargs)
    st = res["strehl"]
    best = np.full(st.shape[0], np.nan)
    for t in range(st.shape[0]):
        if np.any(np.isfinite(st[t])):
            best[t] = z[int(np.nanargmax(st[t]))]
    res["z"], res["best_focus"] = z, best
    return res
