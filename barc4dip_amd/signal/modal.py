"""Modal fits of wavefront maps (``b4d_modal_fit``, ``b4d_modal_residual``, ``b4d_modal_eval``).

``modal_fit`` is the weighted least-squares fit of a wavefront map by Zernike modes on a round aperture or by products of
Legendre polynomials on the rectangular grid, ``modal_eval`` the synthesis, ``modal_table`` the list of modes.

Coordinates: ``v = (i - cy) dy`` along axis -2 and ``u = (j - cx) dx`` along axis -1, ``center = (cy, cx)`` in node indices
(default: the grid centre).

``basis="zernike"``: modes 1 .. ``n_modes`` in Noll's order and normalisation (rms 1 over the unit disc):
``sqrt(n+1) R_n^0`` and ``sqrt(2(n+1)) R_n^|m| cos(m theta)`` or ``sin(m theta)``, the even mode number the cosine, ``theta``
from +x towards +y (growing row index), ``rho = hypot(u, v) / radius``.  ``radius`` is in the units of ``dy``, ``dx`` and
defaults to the inscribed circle ``min(cy dy, cx dx)``.  Nodes with ``rho^2 > 1 + 1e-9`` have weight 0.

``basis="legendre"``: ``sqrt(2a+1) sqrt(2b+1) P_a(u') P_b(v')`` with ``u' = (j - cx) / max(cx, 1)`` and ``v'`` likewise (the
coordinates of the 6-term quadratic fit), ordered by total degree and within a degree by growing power of ``v``: (0,0), (1,0),
(0,1), (2,0), (1,1), (0,2), ...  ``dy``, ``dx`` and ``radius`` do not enter and ``center`` stays at its default.

The normal equations are formed in float64 on the device and factored by Cholesky without pivoting in mode order; a mode whose
remainder after the kept ones is not above 1e-12 of its own diagonal entry (or whose diagonal entry is not > 0) is dropped and
gets coefficient 0.  There is no host fallback.  Limits: sides 1 .. 2048, 1 .. 66 modes (radial order / total degree 10).
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from . import wavefront as _wf

MAX_MODES = 66
BASES = {"zernike": 0, "legendre": 1}
FILL = ("nan", "extend")


def _basis(basis) -> int:
    if not isinstance(basis, str) or basis not in BASES:
        raise ValueError(f'basis must be "zernike" or "legendre", got {basis!r}')
    return BASES[basis]


def _n_modes(n_modes) -> int:
    if isinstance(n_modes, bool) or not isinstance(n_modes, (int, np.integer)) or n_modes < 1:
        raise ValueError(f"n_modes must be an integer >= 1, got {n_modes!r}")
    if n_modes > MAX_MODES:
        raise NotImplementedError(f"at most {MAX_MODES} modes (radial order / total degree 10), got {int(n_modes)}")
    return int(n_modes)


def modal_table(basis, n_modes) -> np.ndarray:
    """(n_modes, 2) int array: ``(n, m)`` of Zernike mode j = row + 1 in Noll's order (m > 0 the cosine, m < 0 the sine), or the
    degrees ``(a, b)`` in u and v of the Legendre products.  Host only."""
    code, J = _basis(basis), _n_modes(n_modes)
    out = np.zeros((J, 2), dtype=np.int64)
    for k in range(J):
        n = 0
        while (n + 1) * (n + 2) // 2 <= k:
            n += 1
        off = k - n * (n + 1) // 2
        if code == 1:
            out[k] = (n - off, off)
            continue
        m = 2 * ((off + 1) // 2) if n % 2 == 0 else 2 * (off // 2) + 1
        out[k] = (n, m if (k + 1) % 2 == 0 else -m)
    return out


def _geometry(code: int, ny: int, nx: int, dy, dx, center, radius):
    """(cy, cx, sy, sx, radius or None) of the C ABI; host only."""
    cy, cx = 0.5 * (ny - 1), 0.5 * (nx - 1)
    if code == 1:
        if center is not None:
            raise ValueError('basis="legendre" is defined on the whole grid: center must be left at its default')
        if radius is not None:
            raise ValueError('basis="legendre" has no radius')
        return cy, cx, 1.0 / max(cy, 1.0), 1.0 / max(cx, 1.0), None
    hy, hx = _wf._spacing(dy, "dy"), _wf._spacing(dx, "dx")
    if center is not None:
        try:
            cy, cx = (float(c) for c in center)
        except (TypeError, ValueError):
            raise ValueError(f"center must be (cy, cx) in node indices, got {center!r}") from None
        if not (np.isfinite(cy) and np.isfinite(cx)):
            raise ValueError(f"center must be finite, got {center!r}")
    if radius is None:
        r = min(cy * hy, cx * hx)
        if not r > 0.0:
            raise ValueError(f"the inscribed circle of a ({ny}, {nx}) grid about ({cy}, {cx}) has no radius: pass radius explicitly")
    else:
        r = _wf._spacing(radius, "radius")
    return cy, cx, hy / r, hx / r, r


def _check_maps(shape):
    if len(shape) not in (2, 3):
        raise ValueError(f"wavefront maps must be (ny, nx) or (T, ny, nx), got {shape}")
    if 0 in shape:
        raise ValueError(f"empty wavefront maps {shape}")
    if max(shape[-2:]) > _wf.MAX_SIDE:
        raise _ffi.B4DSizeError(f"wavefront grids are limited to {_wf.MAX_SIDE} nodes per side, got {shape[-2:]}")


def _remove_flags(remove, J: int) -> np.ndarray:
    if isinstance(remove, str):
        if remove != "all":
            raise ValueError(f'remove must be "all", None or a sequence of mode numbers, got {remove!r}')
        return np.ones(J, dtype=np.uint8)
    flags = np.zeros(J, dtype=np.uint8)
    if remove is None:
        return flags
    try:
        modes = list(remove)
    except TypeError:
        raise ValueError(f'remove must be "all", None or a sequence of mode numbers, got {remove!r}') from None
    for j in modes:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 1 <= j <= J:
            raise ValueError(f"remove names modes 1 .. {J}, got {j!r}")
        flags[int(j) - 1] = 1
    return flags


def modal_fit(wavefront, *, basis="zernike", n_modes=15, weights=None, mask=None, dy=1.0, dx=1.0, center=None, radius=None,
              remove="all", fill="nan", return_tensors: bool = False) -> dict:
    """Weighted least-squares fit of ``n_modes`` Zernike or Legendre modes to every map (module docstring for the bases).

    wavefront: (ny, nx) or (T, ny, nx), a NumPy array of any real dtype and layout or a ROCm tensor, rounded to float32; or the
    dict of ``wavefront_from_displacement``, of which ``"wavefront"`` is fitted, ``"valid"`` (if present) is the mask when none
    is passed, and the steps of ``"y"`` and ``"x"`` are ``dy`` and ``dx``.  ``weights`` (>= 0) and ``mask`` (non-zero = valid)
    are as in ``integrate_gradient``: (ny, nx), shared by the batch, or shaped like the maps; the node weight is their product,
    and 0 where it is not finite and positive or where the map is not finite -- such a node is never read into a sum, so a
    ``fill="nan"`` wavefront needs no mask.
    Returns {"coefficients": (T, n_modes) float64 in the units of the map; "kept": (T, n_modes) bool, False for a dropped mode
    (coefficient 0); "residual": the map minus the modes named by ``remove`` -- ``"all"``, ``None`` or a sequence of 1-based mode
    numbers -- float64 NumPy, or a float32 tensor with ``return_tensors=True``; "rms": (T,) float64, the weighted standard
    deviation (ddof 0) of the residual over the valid nodes, NaN without one; "valid": bool maps, the nodes of positive weight;
    "modes": ``modal_table(basis, n_modes)``; "basis", "center", "radius" (None for Legendre)}.  T = 1 for a 2-D call.
    ``fill="nan"`` writes NaN at the weight-0 nodes of the residual, ``fill="extend"`` evaluates the modes there too, outside
    the disc included (a map value that is not finite stays so).  A map without a valid node gets all-zero coefficients.
    ValueError, B4DSizeError (a side above 2048) or NotImplementedError (more than 66 modes) are raised before the GPU is
    touched."""
    code, J = _basis(basis), _n_modes(n_modes)
    if isinstance(wavefront, dict):
        if "wavefront" not in wavefront:
            raise ValueError('a wavefront dict needs the key "wavefront"')
        maps = wavefront["wavefront"]
        if mask is None and "valid" in wavefront:
            mask = wavefront["valid"]
        shape = _wf._shape(maps)
        _check_maps(shape)
        if "y" in wavefront and "x" in wavefront:
            from ..preprocessing.distortion import _regular_axis     # not at import time: preprocessing imports this package

            dy = abs(_regular_axis(wavefront["y"], shape[-2], "y")[1])
            dx = abs(_regular_axis(wavefront["x"], shape[-1], "x")[1])
    else:
        maps = wavefront
        shape = _wf._shape(maps)
        _check_maps(shape)
    ny, nx = shape[-2:]
    if fill not in FILL:
        raise ValueError(f'fill must be "nan" or "extend", got {fill!r}')
    flags = _remove_flags(remove, J)
    _wf._check_weights(weights, mask, shape)
    cy, cx, sy, sx, rad = _geometry(code, ny, nx, dy, dx, center, radius)

    torch = _ffi.require_gpu()
    phi = D.to_device_f32(maps, ndim=(2, 3))[0].reshape(-1, ny, nx)
    n = int(phi.shape[0])
    if weights is None and mask is None:
        w, wptr, stride = None, None, 0
    else:
        w, stride = _wf._weights_device(weights, mask, shape)
        if stride != 0 and int(w.shape[0]) != n:
            raise ValueError(f"{int(w.shape[0])} weight maps for {n} wavefront maps")
        wptr = D.ptr(w)
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    ws = torch.empty(int(lib.b4d_modal_workspace_bytes(n, ny, nx, J)), dtype=torch.uint8, device=phi.device)
    coeff = torch.empty((n, J), dtype=torch.float64, device=phi.device)
    kept = torch.empty((n, J), dtype=torch.uint8, device=phi.device)
    rms = torch.empty((n,), dtype=torch.float64, device=phi.device)
    out = torch.empty_like(phi)
    rem = torch.from_numpy(flags).to(phi.device)
    flags_valid = torch.empty((n, ny, nx), dtype=torch.uint8, device=phi.device)     # written by the residual kernel
    _ffi.check(lib.b4d_modal_fit(D.ptr(phi), wptr, stride, n, ny, nx, code, J, cy, cx, sy, sx, D.ptr(ws), D.ptr(coeff), D.ptr(kept), st))
    _ffi.check(lib.b4d_modal_residual(D.ptr(phi), wptr, stride, n, ny, nx, code, J, cy, cx, sy, sx, D.ptr(coeff), D.ptr(rem), 1.0,
                                      int(fill == "nan"), D.ptr(ws), D.ptr(out), D.ptr(rms), D.ptr(flags_valid), st))
    out, valid = out.reshape(shape), flags_valid.view(torch.bool).reshape(shape)
    return {"coefficients": coeff.cpu().numpy(), "kept": kept.cpu().numpy().astype(bool),
            "residual": out if return_tensors else out.cpu().numpy().astype(np.float64), "rms": rms.cpu().numpy(),
            "valid": valid if return_tensors else valid.cpu().numpy(), "modes": modal_table(basis, J), "basis": basis,
            "center": (cy, cx), "radius": rad}


def modal_eval(coefficients, shape, *, basis="zernike", dy=1.0, dx=1.0, center=None, radius=None, return_tensors: bool = False):
    """Synthesis ``sum c_j mode_j`` on a grid of ``shape = (ny, nx)`` in the geometry of ``modal_fit``; nothing is masked.

    coefficients: (J,) or (T, J) with J <= 66, NumPy or a ROCm tensor, taken as float64.  Returns (ny, nx) or (T, ny, nx):
    float64 NumPy (evaluated in float64, rounded to float32 on the device), or the float32 device tensor with
    ``return_tensors=True``.  Argument errors are raised before the GPU is touched."""
    code = _basis(basis)
    cs = _wf._shape(coefficients)
    if len(cs) not in (1, 2) or 0 in cs:
        raise ValueError(f"coefficients must be (J,) or (T, J), got {cs}")
    J = _n_modes(int(cs[-1]))
    try:
        ny, nx = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be (ny, nx), got {shape!r}") from None
    if ny < 1 or nx < 1:
        raise ValueError(f"shape must be (ny, nx) with sides >= 1, got {shape!r}")
    if max(ny, nx) > _wf.MAX_SIDE:
        raise _ffi.B4DSizeError(f"wavefront grids are limited to {_wf.MAX_SIDE} nodes per side, got {(ny, nx)}")
    cy, cx, sy, sx, _ = _geometry(code, ny, nx, dy, dx, center, radius)
    torch = _ffi.require_gpu()
    if D.is_tensor(coefficients):
        c = coefficients.to(device="cuda", dtype=torch.float64)
    else:
        c = torch.from_numpy(np.ascontiguousarray(coefficients, dtype=np.float64)).to("cuda")
    c = c.reshape(-1, J).contiguous()
    n = int(c.shape[0])
    out = torch.empty((n, ny, nx), dtype=torch.float32, device=c.device)
    _ffi.check(_ffi.lib().b4d_modal_eval(D.ptr(c), n, ny, nx, code, J, cy, cx, sy, sx, D.ptr(out), _ffi.stream_ptr()))
    out = out.reshape((ny, nx) if len(cs) == 1 else (n, ny, nx))
    return out if return_tensors else out.cpu().numpy().astype(np.float64)
