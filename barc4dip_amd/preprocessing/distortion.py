"""Distortion correction: frames warped by a displacement field (``b4d_spline_prefilter``, ``b4d_warp_dense``, ``b4d_warp_grid``).

With ``dyp, dxp`` the field at pixel (y, x),

    out[t, y, x] = scipy.ndimage.map_coordinates(images[t].astype(float64), [y + dyp, x + dxp], order=order, mode=mode, cval=cval)

computed in float32 on the device.  With this sign ``correct_distortion(img, displacement_map(ref, img,
subpixel="newton"))`` is close to ``ref``.  The field is either the window grid of ``signal.displacement_map`` (a dict with
``dy``, ``dx``, ``y``, ``x``; bilinear between the window centres and held constant beyond the outermost ones, evaluated inside
the warp kernel) or a dense ``(dy, dx)`` pair of per-pixel arrays.  There is no host fallback.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import mode_code
from ..signal import displacement as _dm

ORDERS = (0, 1, 3)
MODES = ("nearest", "reflect", "mirror", "constant")     # no "wrap": the spline prefilter has no periodic form
SPLINE_PAD = 12     # "nearest", order 3: edge padding before the prefilter (b4d_spline_prefilter)


def _shape(a):
    return tuple(int(s) for s in a.shape) if D.is_tensor(a) else np.shape(a)


def _check_order_mode(order, mode) -> int:
    """The mode's code, after both checks."""
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or int(order) not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    return mode_code(mode)


def _regular_axis(v, n: int, name: str) -> tuple[float, float]:
    """(first point, step) of a regular axis of n points; a single point gets step 1."""
    a = np.asarray(v.cpu() if D.is_tensor(v) else v, dtype=np.float64)
    if a.ndim != 1 or a.size != n:
        raise ValueError(f"grid axis {name} must be 1-D with {n} points (the field's grid), got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"grid axis {name} must be finite")
    if n == 1:
        return float(a[0]), 1.0
    step = (a[-1] - a[0]) / (n - 1)
    if step == 0.0 or np.max(np.abs(np.diff(a) - step)) > 1e-9 * max(1.0, abs(step), np.max(np.abs(a))):
        raise ValueError(f"grid axis {name} must be regular (constant non-zero step)")
    return float(a[0]), float(step)


def _parse_field(field, ims) -> dict:
    """Shape checks of ``field`` against images of shape ``ims`` (host only)."""
    T = ims[0] if len(ims) == 3 else None
    if isinstance(field, dict):
        missing = [k for k in ("dy", "dx", "y", "x") if k not in field]
        if missing:
            raise ValueError(f"a grid field needs the keys dy, dx, y, x; missing {missing}")
        dy, dx = field["dy"], field["dx"]
        kind = "grid"
    elif isinstance(field, (tuple, list)) and len(field) == 2:
        dy, dx = field
        kind = "dense"
    else:
        raise ValueError("field must be a displacement_map dict (dy, dx, y, x) or a (dy, dx) pair of per-pixel arrays")
    fs, fx = _shape(dy), _shape(dx)
    if fs != fx:
        raise ValueError(f"dy {fs} and dx {fx} differ in shape")
    if len(fs) not in (2, 3):
        raise ValueError(f"the field must be 2-D (shared) or 3-D (one per frame), got {fs}")
    if 0 in fs:
        raise ValueError(f"empty field {fs}")
    if len(fs) == 3:
        if T is None or fs[0] != T:
            raise ValueError(f"a per-frame field {fs} needs (T, H, W) images with the same T, got {ims}")
    out = {"kind": kind, "dy": dy, "dx": dx, "frames": fs[0] if len(fs) == 3 else 1, "plane": fs[-2:]}
    if kind == "dense":
        if fs[-2:] != tuple(ims[-2:]):
            raise ValueError(f"a dense field {fs[-2:]} must match the frames {tuple(ims[-2:])}")
    else:
        out["y0"], out["sy"] = _regular_axis(field["y"], fs[-2], "y")
        out["x0"], out["sx"] = _regular_axis(field["x"], fs[-1], "x")
    return out


def _check_images(images):
    ims = _shape(images)
    if len(ims) not in (2, 3):
        raise ValueError(f"images must be (H, W) or (T, H, W), got {ims}")
    if 0 in ims:
        raise ValueError("empty images")
    return ims


def correct_distortion(images, field, *, order=3, mode="nearest", cval=0.0, return_tensors=False):
    """Warp ``images`` by ``field``: ``out[t, y, x] = images[t]`` sampled at ``(y + dy, x + dx)`` (module docstring).

    images: (H, W) or (T, H, W), NumPy of any real dtype or a ROCm tensor.  field: a ``displacement_map`` dict (``dy``, ``dx``
    of shape (gy, gx) or (T, gy, gx) on the regular window-centre axes ``y``, ``x``; edit ``dy`` / ``dx`` freely) or a dense
    ``(dy, dx)`` pair of (H, W) or (T, H, W) arrays.  A 2-D field applies to every frame, a 3-D one gives one field per frame.
    order: 0 (nearest sample, half-integers round up as scipy), 1 (bilinear) or 3 (cubic B-spline, prefiltered).
    mode: "nearest", "reflect", "mirror" or "constant" (``cval`` where a coordinate lies outside [0, side - 1]), as scipy.
    The output has the shape of ``images`` and is float32, computed in float32 -- unlike scipy, which keeps the input dtype
    (uint16 frames would be rounded to integers).  NumPy unless ``return_tensors=True``."""
    m = _check_order_mode(order, mode)
    ims = _check_images(images)
    f = _parse_field(field, ims)
    cval = float(cval)
    torch = _ffi.require_gpu()
    img, _, _ = D.to_device_f32(images, ndim=(2, 3))
    H, W = ims[-2:]
    img = img.reshape(-1, H, W)
    n = int(img.shape[0])
    fdy, _, _ = D.to_device_f32(f["dy"], ndim=(2, 3))
    fdx, _, _ = D.to_device_f32(f["dx"], ndim=(2, 3))
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    src = img
    if order == 3:
        p = SPLINE_PAD if mode == "nearest" else 0
        src = torch.empty((n, H + 2 * p, W + 2 * p), dtype=torch.float32, device=img.device)
        _ffi.check(lib.b4d_spline_prefilter(D.ptr(img), n, H, W, m, D.ptr(src), st))
    out = torch.empty((n, H, W), dtype=torch.float32, device=img.device)
    if f["kind"] == "dense":
        _ffi.check(lib.b4d_warp_dense(D.ptr(src), n, H, W, int(order), m, cval, D.ptr(fdy), D.ptr(fdx), f["frames"],
                                      D.ptr(out), st))
    else:
        gy, gx = f["plane"]
        _ffi.check(lib.b4d_warp_grid(D.ptr(src), n, H, W, int(order), m, cval, D.ptr(fdy), D.ptr(fdx), f["frames"],
                                     gy, gx, f["y0"], f["sy"], f["x0"], f["sx"], D.ptr(out), st))
    out = out.reshape(ims)
    return out if return_tensors else out.cpu().numpy()


def remove_distortion(reference, images, *, window=31, step=None, search=8, backend="opencv", order=3, mode="nearest", cval=0.0,
                      return_field=False, return_tensors=False):
    """``displacement_map(reference, images, window=..., step=..., search=..., backend=..., subpixel="newton")`` followed by
    ``correct_distortion(images, field, order=..., mode=..., cval=...)``: ``images`` registered onto ``reference``.
    Returns the corrected frames (float32, shape of ``images``), and the field dict as well when ``return_field=True``."""
    _check_order_mode(order, mode)
    rs, ims = _shape(reference), _check_images(images)
    if len(rs) == 3 and len(ims) == 2:
        raise ValueError(f"a (T, H, W) reference needs (T, H, W) images, got {rs} and {ims}")
    field = _dm.displacement_map(reference, images, window=window, step=step, search=search, backend=backend,
                                 subpixel="newton", return_tensors=return_tensors)
    out = correct_distortion(images, field, order=order, mode=mode, cval=cval, return_tensors=return_tensors)
    return (out, field) if return_field else out
