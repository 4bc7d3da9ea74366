"""Wavefront reconstruction from slope maps (``b4d_integrate_gradient``, ``b4d_poly2_fit``).

``integrate_gradient(gy, gx, dy=hy, dx=hx)`` is the least-squares integral of a slope field given on the nodes of a regular grid, in
Southwell geometry: the slope on the edge between two neighbouring nodes is the mean of the two node slopes, and ``phi`` is the
zero-mean minimiser of

    sum ((phi[i+1, j] - phi[i, j]) / hy - (gy[i, j] + gy[i+1, j]) / 2)^2 + sum ((phi[i, j+1] - phi[i, j]) / hx - (gx[i, j] + gx[i, j+1]) / 2)^2.

The normal equations are a 5-point Neumann Laplacian, which the orthonormal DCT-II diagonalises exactly; the device solves them
with four float32 matrix products per map on the matrix cores.  ``wavefront_from_displacement`` turns a
``displacement_map`` into the wavefront, its 6-term quadratic fit, the radii of curvature and the figure error.  There is no
host fallback.  Limits: grids of 1 .. 2048 nodes per side.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi

MAX_SIDE = 2048
REMOVE = {None: 0b000000, "tilt": 0b000111, "quadratic": 0b111111}     # bit k: coefficient k of (1, u, v, u^2, uv, v^2)


def _shape(a):
    return tuple(int(s) for s in a.shape) if D.is_tensor(a) else np.shape(a)


def _spacing(v, name: str) -> float:
    try:
        h = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a positive finite number, got {v!r}") from None
    if not np.isfinite(h) or h <= 0.0:
        raise ValueError(f"{name} must be a positive finite number, got {v!r}")
    return h


def _check_slopes(gy, gx):
    sy, sx = _shape(gy), _shape(gx)
    if sy != sx:
        raise ValueError(f"gy {sy} and gx {sx} differ in shape")
    if len(sy) not in (2, 3):
        raise ValueError(f"slope maps must be (ny, nx) or (T, ny, nx), got {sy}")
    if 0 in sy:
        raise ValueError(f"empty slope maps {sy}")
    if max(sy[-2:]) > MAX_SIDE:
        raise _ffi.B4DSizeError(f"wavefront grids are limited to {MAX_SIDE} nodes per side, got {sy[-2:]}")
    return sy


def _integrate_device(gy, gx, shape, hy: float, hx: float):
    """phi (T, ny, nx) float32 on the device for slope maps already checked by _check_slopes."""
    torch = _ffi.require_gpu()
    ny, nx = shape[-2:]
    ty, _, _ = D.to_device_f32(gy, ndim=(2, 3))
    tx, _, _ = D.to_device_f32(gx, ndim=(2, 3))
    ty, tx = ty.reshape(-1, ny, nx), tx.reshape(-1, ny, nx)
    n = int(ty.shape[0])
    lib = _ffi.lib()
    ws = torch.empty(int(lib.b4d_integrate_workspace_bytes(n, ny, nx)), dtype=torch.uint8, device=ty.device)
    out = torch.empty((n, ny, nx), dtype=torch.float32, device=ty.device)
    _ffi.check(lib.b4d_integrate_gradient(D.ptr(ty), D.ptr(tx), n, ny, nx, hy, hx, D.ptr(ws), D.ptr(out), _ffi.stream_ptr()))
    return out


def integrate_gradient(gy, gx, *, dy=1.0, dx=1.0, return_tensors: bool = False):
    """Least-squares integral ``phi`` of the slopes ``gy = d phi / dy`` (along axis -2) and ``gx = d phi / dx`` (along axis -1).

    gy, gx: (ny, nx) or (T, ny, nx), NumPy arrays of any real dtype and layout or ROCm tensors; ``dy``, ``dx``: node spacings
    (> 0).  Returns ``phi`` of the same shape with zero mean per map (module docstring for the definition): float64 NumPy, or
    the float32 device tensor with ``return_tensors=True``.  The arithmetic is float32 on the device.  Non-finite input
    propagates and is not checked.  ValueError for differing shapes, a wrong ndim, empty maps or a bad spacing,
    NotImplementedError for a side above 2048 -- all raised before the GPU is touched."""
    shape = _check_slopes(gy, gx)
    hy, hx = _spacing(dy, "dy"), _spacing(dx, "dx")
    out = _integrate_device(gy, gx, shape, hy, hx).reshape(shape)
    return out if return_tensors else out.cpu().numpy().astype(np.float64)


def _parse_displacement(field):
    """(dy, dx, y axis, x axis, step_y, step_x) of a displacement_map dict or a dense (dy, dx) pair (host only)."""
    from ..preprocessing.distortion import _regular_axis     # not at import time: preprocessing imports this package

    if isinstance(field, dict):
        missing = [k for k in ("dy", "dx", "y", "x") if k not in field]
        if missing:
            raise ValueError(f"a grid field needs the keys dy, dx, y, x; missing {missing}")
        dy, dx = field["dy"], field["dx"]
        shape = _check_slopes(dy, dx)
        _, sy = _regular_axis(field["y"], shape[-2], "y")
        _, sx = _regular_axis(field["x"], shape[-1], "x")
        if sy < 0.0 or sx < 0.0:
            raise ValueError("grid axes y and x must ascend")
        y = np.asarray(field["y"].cpu() if D.is_tensor(field["y"]) else field["y"], dtype=np.float64)
        x = np.asarray(field["x"].cpu() if D.is_tensor(field["x"]) else field["x"], dtype=np.float64)
        return dy, dx, shape, y, x, sy, sx
    if isinstance(field, (tuple, list)) and len(field) == 2:
        dy, dx = field
        shape = _check_slopes(dy, dx)
        return dy, dx, shape, np.arange(shape[-2], dtype=np.float64), np.arange(shape[-1], dtype=np.float64), 1.0, 1.0
    raise ValueError("field must be a displacement_map dict (dy, dx, y, x) or a dense (dy, dx) pair")


def wavefront_from_displacement(field, *, pixel_size, distance, wavelength=None, remove="tilt", return_tensors: bool = False) -> dict:
    """Wavefront of a speckle displacement field.

    field: a ``displacement_map`` dict (``dy``, ``dx`` of shape (gy, gx) or (T, gy, gx) in pixels on the regular, ascending
    window-centre axes ``y``, ``x``) or a dense ``(dy, dx)`` pair (node spacing of one pixel).  The local slope of the wavefront
    is ``d * pixel_size / distance`` (so that ``dW/dx = dx * pixel_size / distance``), the node spacing ``step * pixel_size``;
    ``pixel_size``, ``distance`` and ``wavelength`` in metres.
    The six terms ``(1, u, v, u^2, u v, v^2)`` -- ``u`` along x and ``v`` along y, in metres from the grid centre -- are always
    fitted; ``remove`` selects what is subtracted from the returned wavefront: ``None`` nothing, ``"tilt"`` the first three
    (on a centred regular grid the tilt terms of the 6-term fit are the tilt-only fit), ``"quadratic"`` all six, which leaves
    the figure error.
    Returns {"wavefront": metres, shape of ``dy``; "phase": ``2 pi wavefront / wavelength`` (only with a wavelength); "y", "x":
    the grid axes in pixels; "coefficients": (T, 6) float64 in metres per metre^degree; "radius_x" = 1 / (2 c3), "radius_y"
    = 1 / (2 c5): (T,) float64 metres, inf where the coefficient is 0; "rms": (T,) float64, the standard deviation (ddof 0) of
    the returned wavefront}.  T = 1 for a 2-D field.  Maps are float64 NumPy, or float32 device tensors with
    ``return_tensors=True``.
    A per-window mask or weights (e.g. from the ``peak`` or ``snr`` maps) is out of scope: every window counts the same, and a
    non-finite shift spoils its whole map."""
    if remove not in REMOVE:
        raise ValueError(f'remove must be None, "tilt" or "quadratic", got {remove!r}')
    p, L = _spacing(pixel_size, "pixel_size"), _spacing(distance, "distance")
    lam = None if wavelength is None else _spacing(wavelength, "wavelength")
    dy, dx, shape, y, x, sy, sx = _parse_displacement(field)
    torch = _ffi.require_gpu()
    ny, nx = shape[-2:]
    # integrated in pixel units (shifts in px on a grid of `step` px), scaled to metres by the last kernel: float32 never sees
    # the physical magnitudes
    phi = _integrate_device(dy, dx, shape, sy, sx)
    n = int(phi.shape[0])
    scale = p * p / L
    coeff = torch.empty((n, 6), dtype=torch.float64, device=phi.device)
    rms = torch.empty((n,), dtype=torch.float64, device=phi.device)
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    res = {"y": y, "x": x}
    if lam is not None:
        phase = torch.empty_like(phi)
        _ffi.check(lib.b4d_poly2_fit(D.ptr(phi), n, ny, nx, REMOVE[remove], scale * 2.0 * np.pi / lam, D.ptr(coeff), D.ptr(phase),
                                     D.ptr(rms), st))
        res["phase"] = phase.reshape(shape)
    _ffi.check(lib.b4d_poly2_fit(D.ptr(phi), n, ny, nx, REMOVE[remove], scale, D.ptr(coeff), D.ptr(phi), D.ptr(rms), st))
    res["wavefront"] = phi.reshape(shape)
    if not return_tensors:
        for k in ("wavefront", "phase"):
            if k in res:
                res[k] = res[k].cpu().numpy().astype(np.float64)
    # normalised coordinates u = x_m / ax, v = y_m / ay with the half extents ax, ay in metres
    ax = (0.5 * (nx - 1) if nx > 1 else 1.0) * sx * p
    ay = (0.5 * (ny - 1) if ny > 1 else 1.0) * sy * p
    c = coeff.cpu().numpy() * scale / np.array([1.0, ax, ay, ax * ax, ax * ay, ay * ay])
    with np.errstate(divide="ignore"):
        res["radius_x"] = np.where(c[:, 3] != 0.0, 1.0 / (2.0 * c[:, 3]), np.inf)
        res["radius_y"] = np.where(c[:, 5] != 0.0, 1.0 / (2.0 * c[:, 5]), np.inf)
    res["coefficients"] = c
    res["rms"] = rms.cpu().numpy()
    return res
