"""Transmission and dark-field maps of speckle tracking (``b4d_speckle_contrast``): the two signals that speckle-based imaging
(XST, UMPA and their relatives) defines next to the differential phase that ``displacement_map`` measures.

On the window grid of ``displacement_map`` (window ``(wy, wx)``, step, origins ``y0 = Sy + k * step_y``), window (y0, x0) with the
tracked displacement (dy, dx) compares

    r[j, i] = reference[y0 + j, x0 + i]      with      s[j, i] = image at (y0 + j + dy, x0 + i + dx),

the convention of ``correct_distortion``: the image window displaced by the tracked shift is the one that matches the reference
window.  ``order=0`` takes the pixel at ``floor(d + 0.5)``, ``order=1`` is bilinear in float64.  With weights ``h[j, i]`` that sum to 1
(``taper="flat"``, or ``"hann"``: the half-sample Hann of the fringe code per axis) and the weighted means Rm, Sm, variances VR, VS
and covariance C:

    transmission = Sm / Rm                              correlation = C / sqrt(VS VR)
    dark_field = (sqrt(VS) / Sm) / (sqrt(VR) / Rm)      visibility_ref = sqrt(VR) / Rm
    dark_field_fit = C / (VR transmission)              visibility = sqrt(VS) / Sm

``dark_field`` is the visibility ratio, which noise in the image raises; ``dark_field_fit`` is the least-squares slope of s on r
over the transmission, the UMPA estimate.  A quantity whose denominator is not above 0 is NaN, and so is the square root of a
variance that is not above 0 (a window without contrast has a transmission and nothing else).  A window whose displacement is not
finite, or that would read outside the frame, is NaN in all six maps; a displacement within the search range never is.
Everything runs on the device in float64 sums; there is no host fallback.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .displacement import BACKENDS, _shape, displacement_grid, displacement_map

PLANES = ("transmission", "dark_field", "dark_field_fit", "correlation", "visibility_ref", "visibility")
TAPERS = ("flat", "hann")


def _check_frames(reference, images):
    """(reference shape, images shape) under the pairing rules of ``displacement_map`` (host only)."""
    rs, ims = _shape(reference), _shape(images)
    if len(rs) not in (2, 3) or len(ims) not in (2, 3):
        raise ValueError(f"reference and images must be (H, W) or (T, H, W), got {rs} and {ims}")
    if rs[-2:] != ims[-2:]:
        raise ValueError(f"reference frames {rs[-2:]} and image frames {ims[-2:]} differ in shape")
    if len(rs) == 3 and (len(ims) != 3 or rs[0] != ims[0]):
        raise ValueError(f"a (T, H, W) reference needs (T, H, W) images with the same T, got {rs} and {ims}")
    if 0 in rs or 0 in ims:
        raise ValueError("empty reference or images")
    return rs, ims


def _check_sampling(order, taper) -> tuple[int, int]:
    if isinstance(order, (bool, np.bool_)) or order not in (0, 1):
        raise ValueError(f"order must be 0 (nearest) or 1 (bilinear), got {order!r}")
    if not isinstance(taper, str) or taper not in TAPERS:
        raise ValueError(f"taper must be one of {TAPERS}, got {taper!r}")
    return int(order), TAPERS.index(taper)


def _check_field(field, window, step, search, ims):
    """(grid, dy, dx) of a ``displacement_map`` dict or a (dy, dx) pair for images of shape ``ims`` (host only)."""
    if isinstance(field, dict):
        if window is not None or step is not None or search is not None:
            raise ValueError("window, step and search come from the meta of a displacement_map dict; pass them only with a (dy, dx) pair")
        missing = [k for k in ("dy", "dx", "meta") if k not in field]
        if not missing:
            missing = [f"meta[{k!r}]" for k in ("window", "step", "search") if k not in field["meta"]]
        if missing:
            raise ValueError(f"a field dict needs dy, dx and meta with window, step and search; missing {missing}")
        dy, dx, meta = field["dy"], field["dx"], field["meta"]
        window, step, search = meta["window"], meta["step"], meta["search"]
    elif isinstance(field, (tuple, list)) and len(field) == 2:
        dy, dx = field
        window = 31 if window is None else window
        search = 8 if search is None else search
    else:
        raise ValueError("field must be a displacement_map dict or a (dy, dx) pair")
    g = displacement_grid(ims[-2:], window=window, step=step, search=search)
    want = tuple(ims[:-2]) + g["shape"]
    for name, m in (("dy", dy), ("dx", dx)):
        if D.is_tensor(m):
            bad = m.is_complex()
        else:
            m = np.asarray(m)
            bad = m.dtype.kind not in "buif"
        if bad:
            raise ValueError(f"{name} must be a real array")
        if _shape(m) != want:
            raise ValueError(f"{name} has shape {_shape(m)}, the window grid of these frames is {want}")
    return g, dy, dx


def _field_device(dy, dx, n: int, gy: int, gx: int):
    """(dy, dx, field_stride) on the device in the layout of ``b4d_speckle_contrast``: the two planes of a ``displacement_map``
    output tensor as they are, anything else as two planar float64 maps."""
    torch = _ffi.require_gpu()
    if D.is_tensor(dy) and D.is_tensor(dx) and dy.is_cuda and dx.is_cuda and dy.dtype == dx.dtype == torch.float64:
        planar = (gy * gx, gx, 1)[3 - dy.ndim:]
        if (tuple(dy.stride()) == tuple(dx.stride()) == tuple(4 * s for s in planar)
                and dx.data_ptr() == dy.data_ptr() + 8):
            return dy, dx, 4 * gy * gx

    def up(m):
        if D.is_tensor(m):
            return m.to(device="cuda", dtype=torch.float64).contiguous()
        return torch.from_numpy(np.array(m, dtype=np.float64, order="C")).to("cuda")

    return up(dy), up(dx), gy * gx


def _contrast_device(ref, img, paired: bool, g: dict, dy, dx, order: int, taper: int):
    """(n, gy, gx, 6) float64 device tensor for the device frames ref (nref, H, W), img (n, H, W) and the field dy, dx."""
    torch = _ffi.require_gpu()
    nref, n = int(ref.shape[0]), int(img.shape[0])
    H, W = (int(s) for s in img.shape[-2:])
    (wy, wx), (sty, stx), (sy, sx), (gy, gx) = g["window"], g["step"], g["search"], g["shape"]
    pair_img = np.arange(n, dtype=np.int32)
    pair_ref = pair_img.copy() if paired else np.zeros(n, dtype=np.int32)
    dyt, dxt, stride = _field_device(dy, dx, n, gy, gx)
    out = torch.empty((n, gy, gx, 6), dtype=torch.float64, device=img.device)
    _ffi.check(_ffi.lib().b4d_speckle_contrast(
        D.ptr(ref), nref, D.ptr(img), n, pair_ref.ctypes.data_as(_ffi.C.c_void_p), pair_img.ctypes.data_as(_ffi.C.c_void_p), n,
        H, W, wy, wx, sty, stx, sy, sx, D.ptr(dyt), D.ptr(dxt), stride, order, taper, D.ptr(out), _ffi.stream_ptr()))
    return out


def _frames_device(a, shape):
    t, _, _ = D.to_device_f32(a, ndim=(2, 3))
    return t.reshape((-1,) + tuple(shape[-2:]))


def speckle_contrast(reference, images, field, *, window=None, step=None, search=None, order=1, taper: str = "flat",
                     return_tensors: bool = False) -> dict:
    """Transmission, dark-field, correlation and visibility maps of ``images`` against ``reference`` along a tracked field.

    reference (H, W) with images (H, W) or (T, H, W), or reference (T, H, W) paired frame by frame with images (T, H, W), as in
    ``displacement_map``; NumPy arrays of any real dtype or ROCm tensors.  ``field``: the dict that ``displacement_map`` returned
    for these frames (``subpixel="newton"`` for a sub-pixel field with each correction on its own axis) -- window, step and
    search come from its ``meta`` -- or a ``(dy, dx)`` pair with ``window``, ``step``, ``search`` given here (defaults of
    ``displacement_map``).  ``dy``, ``dx`` have the shape of the window grid, (gy, gx) or (T, gy, gx), NumPy or device tensors;
    the two planes of a ``displacement_map(..., return_tensors=True)`` result are read where they are.
    ``order``: 0 nearest, 1 bilinear.  ``taper``: "flat" or "hann".
    Returns {"transmission", "dark_field", "dark_field_fit", "correlation", "visibility", "visibility_ref": float64 (gy, gx) or
    (T, gy, gx), formulas in the module docstring; "y", "x": window centres; "meta"}; device tensors with
    ``return_tensors=True``.  A frame gives the same bits alone and inside any stack.
    ValueError for bad shapes, a field that does not match the window grid, a bad ``order`` or ``taper``; NotImplementedError for
    a window beyond 128 or a search beyond 32 px -- all raised before the GPU is touched."""
    rs, ims = _check_frames(reference, images)
    o, t = _check_sampling(order, taper)
    g, dy, dx = _check_field(field, window, step, search, ims)
    _ffi.require_gpu()
    out = _contrast_device(_frames_device(reference, rs), _frames_device(images, ims), len(rs) == 3, g, dy, dx, o, t)
    if len(ims) == 2:
        out = out[0]
    res = out if return_tensors else out.cpu().numpy()
    maps = {name: res[..., k] for k, name in enumerate(PLANES)}
    maps.update({"y": g["y"], "x": g["x"],
                 "meta": {"window": g["window"], "step": g["step"], "search": g["search"], "order": o, "taper": taper}})
    return maps


def speckle_imaging(reference, images, *, window=31, step=None, search=8, backend: str = "opencv", order=1, taper: str = "flat",
                    min_correlation=None, return_tensors: bool = False) -> dict:
    """Speckle tracking with all three signals: ``displacement_map(..., subpixel="newton")`` and ``speckle_contrast`` along its field,
    the field staying on the device in between.

    Arguments as in ``displacement_map`` and ``speckle_contrast``.  Returns one dict in the layout of ``fringe_displacement``:
    {"dy", "dx", "peak", "snr", "transmission", "dark_field", "dark_field_fit", "correlation", "visibility", "visibility_ref":
    float64 (gy, gx) or (T, gy, gx); "valid": bool, the windows where all of these but ``snr`` are finite and, with
    ``min_correlation`` (a number in [-1, 1]), ``correlation >= min_correlation``; "y", "x"; "meta"}, so that
    ``wavefront_from_displacement(m, ..., weights="peak")`` and ``mask=m["valid"]`` take it as it is.  Device tensors with
    ``return_tensors=True``.  Errors as in the two functions, raised before the GPU is touched."""
    rs, ims = _check_frames(reference, images)
    o, t = _check_sampling(order, taper)
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    if min_correlation is not None:
        if isinstance(min_correlation, (bool, str)) or np.ndim(min_correlation) != 0:
            raise ValueError(f"min_correlation must be None or a number in [-1, 1], got {min_correlation!r}")
        try:
            min_correlation = float(min_correlation)
        except (TypeError, ValueError):
            raise ValueError(f"min_correlation must be None or a number in [-1, 1], got {min_correlation!r}") from None
        if not -1.0 <= min_correlation <= 1.0:
            raise ValueError(f"min_correlation must be None or a number in [-1, 1], got {min_correlation!r}")
    g = displacement_grid(rs[-2:], window=window, step=step, search=search)
    torch = _ffi.require_gpu()
    ref, img = _frames_device(reference, rs), _frames_device(images, ims)
    m = displacement_map(ref if len(rs) == 3 else ref[0], img, window=window, step=step, search=search, backend=backend,
                         subpixel="newton", return_tensors=True)
    out = _contrast_device(ref, img, len(rs) == 3, g, m["dy"], m["dx"], o, t)
    res = {k: m[k] for k in ("dy", "dx", "peak", "snr")}
    res.update({name: out[..., k] for k, name in enumerate(PLANES)})
    valid = torch.isfinite(out).all(dim=-1) & torch.isfinite(res["dy"]) & torch.isfinite(res["dx"]) & torch.isfinite(res["peak"])
    if min_correlation is not None:
        valid &= res["correlation"] >= min_correlation
    res["valid"] = valid
    for k, v in res.items():
        if len(ims) == 2:
            v = v[0]
        res[k] = v if return_tensors else v.cpu().numpy()
    res.update({"y": g["y"], "x": g["x"],
                "meta": dict(m["meta"], order=o, taper=taper, min_correlation=min_correlation)})
    return res
