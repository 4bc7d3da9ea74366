"""Wavefront reconstruction from slope maps (``b4d_integrate_gradient``, ``b4d_poly2_fit``).

``integrate_gradient(gy, gx, dy=hy, dx=hx)`` is the least-squares integral of a slope field given on the nodes of a regular grid, in
Southwell geometry: the slope on the edge between two neighbouring nodes is the mean of the two node slopes, and ``phi`` is the
zero-mean minimiser of

    sum ((phi[i+1, j] - phi[i, j]) / hy - (gy[i, j] + gy[i+1, j]) / 2)^2 + sum ((phi[i, j+1] - phi[i, j]) / hx - (gx[i, j] + gx[i, j+1]) / 2)^2.

The normal equations are a 5-point Neumann Laplacian, which the orthonormal DCT-II diagonalises exactly; the device solves them
with four float32 matrix products per map on the matrix cores.  ``wavefront_from_displacement`` turns a
``displacement_map`` into the wavefront, its 6-term quadratic fit, the radii of curvature and the figure error.  There is no
host fallback.  Limits: grids of 1 .. 2048 nodes per side.

With ``weights`` and / or ``mask`` every node carries a weight ``w >= 0`` (their product; a node whose weight is not finite and
positive, or whose slopes are not finite, has weight 0), every edge the harmonic mean ``2ab / (a + b)`` of its two node weights,
and ``phi`` minimises the weighted sum of the same squared edge residuals.  The device solves the weighted normal equations by
conjugate gradients started from 0 and preconditioned with the unweighted DCT solve.  That fixes what the
data leave open: the result is the minimiser of smallest unweighted Laplacian energy with zero mean over the whole grid, so
weight-0 nodes are filled harmonically and disconnected pieces of the valid region are levelled against each other as smoothly
as possible -- their relative pistons are levelled, not measured.
"""
from __future__ import annotations

import warnings

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


FILL = ("nan", "harmonic")


def _check_solver(fill, rtol, max_iter):
    if fill not in FILL:
        raise ValueError(f'fill must be "nan" or "harmonic", got {fill!r}')
    try:
        tol = float(rtol)
    except (TypeError, ValueError):
        raise ValueError(f"rtol must be a finite number >= 0, got {rtol!r}") from None
    if not np.isfinite(tol) or tol < 0.0:
        raise ValueError(f"rtol must be a finite number >= 0, got {rtol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    return tol, int(max_iter)


def _check_weights(weights, mask, shape):
    """Shapes of the weight operands against the slope maps `shape`: (ny, nx), shared by the batch, or `shape` itself."""
    for name, a in (("weights", weights), ("mask", mask)):
        if a is None:
            continue
        if isinstance(a, str):
            raise ValueError(f"{name} must be an array, got the string {a!r}")
        sa = _shape(a)
        if sa != tuple(shape[-2:]) and sa != tuple(shape):
            raise ValueError(f"{name} {sa} must have the shape of a map {tuple(shape[-2:])} or of the slopes {tuple(shape)}")
        if not D.is_tensor(a) and np.asarray(a).dtype.kind not in "biuf":
            raise ValueError(f"{name} must be real or bool, got dtype {np.asarray(a).dtype}")
        if D.is_tensor(a) and a.is_complex():
            raise ValueError(f"{name} must be real or bool, got dtype {a.dtype}")


def _weights_device(weights, mask, shape):
    """float32 device tensor of the node weights, (1, ny, nx) when shared by the batch or (T, ny, nx), and its map stride."""
    ny, nx = shape[-2:]
    w = None
    if weights is not None:
        w = D.to_device_f32(weights, ndim=(2, 3))[0].reshape(-1, ny, nx)
    if mask is not None:
        m = (mask != 0) if D.is_tensor(mask) else (np.asarray(mask) != 0)
        m = D.to_device_f32(m, ndim=(2, 3))[0].reshape(-1, ny, nx)
        w = m if w is None else w * m          # 0 or 1 times the float32 weight: exact (NaN and inf weights stay non-finite)
    w = w.contiguous()
    return w, (ny * nx if int(w.shape[0]) > 1 else 0)


def _integrate_weighted_device(gy, gx, shape, hy: float, hx: float, w, w_stride: int, rtol: float, max_iter: int, nan_invalid: bool):
    """(phi, effective weights, iterations, residual) on the device: (T, ny, nx) float32 twice, (T,) int32, (T,) float64."""
    torch = _ffi.require_gpu()
    ny, nx = shape[-2:]
    ty, _, _ = D.to_device_f32(gy, ndim=(2, 3))
    tx, _, _ = D.to_device_f32(gx, ndim=(2, 3))
    ty, tx = ty.reshape(-1, ny, nx), tx.reshape(-1, ny, nx)
    n = int(ty.shape[0])
    if w_stride != 0 and int(w.shape[0]) != n:
        raise ValueError(f"{int(w.shape[0])} weight maps for {n} slope maps")
    lib = _ffi.lib()
    ws = torch.empty(int(lib.b4d_integrate_weighted_workspace_bytes(n, ny, nx)), dtype=torch.uint8, device=ty.device)
    out = torch.empty((n, ny, nx), dtype=torch.float32, device=ty.device)
    iters = torch.empty((n,), dtype=torch.int32, device=ty.device)
    resid = torch.empty((n,), dtype=torch.float64, device=ty.device)
    _ffi.check(lib.b4d_integrate_gradient_weighted(D.ptr(ty), D.ptr(tx), D.ptr(w), w_stride, n, ny, nx, hy, hx, rtol, max_iter,
                                                   int(nan_invalid), D.ptr(ws), D.ptr(out), D.ptr(iters), D.ptr(resid),
                                                   _ffi.stream_ptr()))
    weff = ws[:n * ny * nx * 4].view(torch.float32).reshape(n, ny, nx)
    return out, weff, iters, resid


def _solver_info(iters, resid, rtol: float, max_iter: int) -> dict:
    """Host copies of the per-map solver state; warns for maps that stopped above rtol."""
    it, res = iters.cpu().numpy(), resid.cpu().numpy()
    ok = res <= rtol * (1.0 + 1e-12)
    if not np.all(ok):
        bad = np.flatnonzero(~ok)
        warnings.warn(f"weighted integration: {bad.size} of {ok.size} maps did not reach rtol = {rtol:g} within {max_iter} iterations "
                      f"(largest residual {np.max(res[bad]):.3g}, map {int(bad[np.argmax(res[bad])])})", RuntimeWarning, stacklevel=3)
    return {"iterations": it, "residual": res, "converged": ok}


def integrate_gradient(gy, gx, *, dy=1.0, dx=1.0, weights=None, mask=None, fill="nan", rtol=1e-6, max_iter=500,
                       return_info: bool = False, return_tensors: bool = False):
    """Least-squares integral ``phi`` of the slopes ``gy = d phi / dy`` (along axis -2) and ``gx = d phi / dx`` (along axis -1).

    gy, gx: (ny, nx) or (T, ny, nx), NumPy arrays of any real dtype and layout or ROCm tensors; ``dy``, ``dx``: node spacings
    (> 0).  Returns ``phi`` of the same shape with zero mean per map (module docstring for the definition): float64 NumPy, or
    the float32 device tensor with ``return_tensors=True``.  The arithmetic is float32 on the device.  ValueError for differing
    shapes, a wrong ndim, empty maps or a bad spacing, NotImplementedError for a side above 2048 -- all raised before the GPU is
    touched.

    Without ``weights`` and ``mask`` every node counts the same, the solve is direct, and non-finite input propagates through
    its map and is not checked.  ``weights`` (>= 0) and ``mask`` (non-zero = valid) are (ny, nx), shared by the batch, or shaped
    like ``gy``; any real or bool dtype and layout, or ROCm tensors; both are rounded to float32.  The node weight is their
    product, and 0 where it is not finite and positive or where ``gy`` or ``gx`` is not finite: such nodes take no part, no
    error is raised for them.  The weighted solve iterates (module docstring) until ``|r| <= rtol |b|`` or ``max_iter`` per
    map; a map that stops above ``rtol`` raises a RuntimeWarning and is still returned.  ``fill="nan"`` writes NaN at the
    weight-0 nodes, ``fill="harmonic"`` keeps the harmonic fill; the mean over the whole grid, fill included, is zero, and the
    relative heights of disconnected pieces are levelled, not measured.  ``return_info=True`` returns
    ``(phi, {"iterations", "residual", "converged"})``, each (T,) (T = 1 for a 2-D call); without weights and mask that is
    0 iterations, residual 0 and converged."""
    shape = _check_slopes(gy, gx)
    hy, hx = _spacing(dy, "dy"), _spacing(dx, "dx")
    tol, iters_max = _check_solver(fill, rtol, max_iter)
    _check_weights(weights, mask, shape)
    if weights is None and mask is None:
        out = _integrate_device(gy, gx, shape, hy, hx)
        n = int(out.shape[0])
        info = {"iterations": np.zeros(n, np.int32), "residual": np.zeros(n), "converged": np.ones(n, bool)}
    else:
        w, stride = _weights_device(weights, mask, shape)
        out, _, it, res = _integrate_weighted_device(gy, gx, shape, hy, hx, w, stride, tol, iters_max, fill == "nan")
        info = _solver_info(it, res, tol, iters_max)
    out = out.reshape(shape)
    out = out if return_tensors else out.cpu().numpy().astype(np.float64)
    return (out, info) if return_info else out


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


def _named_weights(weights, field):
    """The map that weights="peak" / "snr" names in a displacement_map dict."""
    if not isinstance(weights, str):
        return weights
    if weights not in ("peak", "snr"):
        raise ValueError(f'weights must be an array, "peak" or "snr", got {weights!r}')
    if not isinstance(field, dict):
        raise ValueError(f'weights="{weights}" needs a displacement_map dict, a plain (dy, dx) pair has no such map')
    if weights not in field:
        raise ValueError(f'weights="{weights}": the field has no key "{weights}"')
    return field[weights]


def wavefront_from_displacement(field, *, pixel_size, distance, wavelength=None, remove="tilt", weights=None, mask=None,
                                fill="nan", rtol=1e-6, max_iter=500, return_tensors: bool = False) -> dict:
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
    the grid axes in pixels; "remove": the argument, so that a consumer (``focal_spot``) knows what was subtracted;
    "coefficients": (T, 6) float64 in metres per metre^degree; "radius_x" = 1 / (2 c3), "radius_y"
    = 1 / (2 c5): (T,) float64 metres, inf where the coefficient is 0; "rms": (T,) float64, the standard deviation (ddof 0) of
    the returned wavefront}.  T = 1 for a 2-D field.  Maps are float64 NumPy, or float32 device tensors with
    ``return_tensors=True``.
    ``weights`` and ``mask`` weight the windows as in ``integrate_gradient`` (``fill``, ``rtol``, ``max_iter`` likewise);
    ``weights`` may also be ``"peak"`` or ``"snr"``, which takes that map of the field dict (ValueError if the key is absent or
    the field is a plain pair).  A window with a non-finite shift then has weight 0 instead of spoiling its map.  The fit, the
    radii and ``rms`` become the weighted ones (``u``, ``v`` stay the full-grid coordinates; ``rms`` is the weighted standard
    deviation over the valid windows), and the result gains "valid" (bool, shape of ``dy``: windows of positive weight),
    "iterations", "residual" and "converged" ((T,) each).  Without ``weights`` and ``mask`` every window counts the same and a
    non-finite shift spoils its whole map."""
    if remove not in REMOVE:
        raise ValueError(f'remove must be None, "tilt" or "quadratic", got {remove!r}')
    p, L = _spacing(pixel_size, "pixel_size"), _spacing(distance, "distance")
    lam = None if wavelength is None else _spacing(wavelength, "wavelength")
    tol, iters_max = _check_solver(fill, rtol, max_iter)
    weights = _named_weights(weights, field)
    dy, dx, shape, y, x, sy, sx = _parse_displacement(field)
    _check_weights(weights, mask, shape)
    weighted = weights is not None or mask is not None
    torch = _ffi.require_gpu()
    ny, nx = shape[-2:]
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    res = {"y": y, "x": x, "remove": remove}
    # integrated in pixel units (shifts in px on a grid of `step` px), scaled to metres by the last kernel: float32 never sees
    # the physical magnitudes
    if weighted:
        w, stride = _weights_device(weights, mask, shape)
        phi, weff, it, rs = _integrate_weighted_device(dy, dx, shape, sy, sx, w, stride, tol, iters_max, False)
        res.update(_solver_info(it, rs, tol, iters_max))
        valid = (weff > 0).reshape(shape)
        res["valid"] = valid if return_tensors else valid.cpu().numpy()
        nan_invalid = int(fill == "nan")

        def fit(scale, out):
            _ffi.check(lib.b4d_poly2_fit_weighted(D.ptr(phi), D.ptr(weff), ny * nx, n, ny, nx, REMOVE[remove], scale, nan_invalid,
                                                  D.ptr(coeff), D.ptr(out), D.ptr(rms), st))
    else:
        phi = _integrate_device(dy, dx, shape, sy, sx)

        def fit(scale, out):
            _ffi.check(lib.b4d_poly2_fit(D.ptr(phi), n, ny, nx, REMOVE[remove], scale, D.ptr(coeff), D.ptr(out), D.ptr(rms), st))
    n = int(phi.shape[0])
    scale = p * p / L
    coeff = torch.empty((n, 6), dtype=torch.float64, device=phi.device)
    rms = torch.empty((n,), dtype=torch.float64, device=phi.device)
    if lam is not None:
        phase = torch.empty_like(phi)
        fit(scale * 2.0 * np.pi / lam, phase)
        res["phase"] = phase.reshape(shape)
    fit(scale, phi)
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
