"""Dense NCC displacement maps: the local shift of every window of a regular grid (``b4d_displacement_map``).

Window ``(y0, x0)`` of size ``(wy, wx)`` searched ``+-(Sy, Sx)`` px gives exactly what

    template_matching(ref[y0:y0+wy, x0:x0+wx], img[y0-Sy:y0+wy+Sy, x0-Sx:x0+wx+Sx],
                      slices_yx=(slice(Sy, Sy+wy), slice(Sx, Sx+wx)), backend=backend, subpixel=subpixel, eps=eps)

returns: (dy, dx, peak, snr) of the NCC map over the (2Sy+1) x (2Sx+1) local shifts ("opencv" z-scores the search box, "skimage"
uses it raw).  Origins are ``y0 = Sy + k * step_y`` for every k with ``y0 + wy + Sy <= H`` (likewise for x): only windows whose
whole search box lies inside the frame.  The map is computed in direct space on the device, one workgroup per window
(DESIGN.md section 11); there is no host or FFT fallback.  Limits: window <= 128 and search <= 32 px per axis.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi

MAX_WINDOW = 128
MAX_SEARCH = 32
BACKENDS = ("opencv", "skimage")


def _pair(v, name: str) -> tuple[int, int]:
    if np.ndim(v) != 0:
        if np.ndim(v) != 1 or len(v) != 2:
            raise ValueError(f"{name} must be an int or a (y, x) pair, got {v!r}")
        y, x = v
    else:
        y = x = v
    out = []
    for a in (y, x):
        if isinstance(a, (bool, np.bool_)) or int(a) != a:
            raise ValueError(f"{name} must hold integers, got {v!r}")
        out.append(int(a))
    if min(out) < 1:
        raise ValueError(f"{name} must be >= 1 per axis, got {v!r}")
    return out[0], out[1]


def displacement_grid(shape, *, window=31, step=None, search=8) -> dict:
    """Host-only grid geometry of ``displacement_map`` for frames of ``shape`` = (H, W) (no device needed).

    Returns {"window", "step", "search": (y, x) pairs, "y0", "x0": window origins (int64), "y", "x": window centres (float64),
    "shape": (gy, gx)}.  Raises ValueError for arguments < 1 or a window plus search margin that does not fit, and
    NotImplementedError for a window or search beyond the kernel's limits."""
    H, W = (int(s) for s in shape)
    wy, wx = _pair(window, "window")
    if step is None:
        sty, stx = max(1, wy // 2), max(1, wx // 2)
    else:
        sty, stx = _pair(step, "step")
    sy, sx = _pair(search, "search")
    if wy > MAX_WINDOW or wx > MAX_WINDOW:
        raise NotImplementedError(f"window {(wy, wx)} exceeds the kernel's limit of {MAX_WINDOW} px per axis")
    if sy > MAX_SEARCH or sx > MAX_SEARCH:
        raise NotImplementedError(f"search {(sy, sx)} exceeds the kernel's limit of {MAX_SEARCH} px per axis")
    if H < wy + 2 * sy or W < wx + 2 * sx:
        raise ValueError(f"a {(wy, wx)} window searched +-{(sy, sx)} px does not fit in a {(H, W)} frame")
    y0 = sy + sty * np.arange((H - wy - 2 * sy) // sty + 1, dtype=np.int64)
    x0 = sx + stx * np.arange((W - wx - 2 * sx) // stx + 1, dtype=np.int64)
    return {"window": (wy, wx), "step": (sty, stx), "search": (sy, sx), "y0": y0, "x0": x0,
            "y": y0 + (wy - 1) / 2.0, "x": x0 + (wx - 1) / 2.0, "shape": (int(y0.size), int(x0.size))}


def _shape(a):
    return tuple(int(s) for s in a.shape) if D.is_tensor(a) else np.shape(a)


def _subpixel_code(subpixel) -> int:
    if isinstance(subpixel, str):
        if subpixel != "newton":
            raise ValueError(f'subpixel must be True, False or "newton", got {subpixel!r}')
        return 2
    return int(bool(subpixel))


def displacement_map(reference, images, *, window=31, step=None, search=8, backend: str = "opencv", subpixel=True,
                     eps: float = 1e-9, return_tensors: bool = False) -> dict:
    """NCC displacement map of ``images`` against ``reference`` on a regular window grid.

    reference (H, W) with images (H, W) or (T, H, W), or reference (T, H, W) paired frame by frame with images (T, H, W)
    (incremental tracking: ``displacement_map(stack[:-1], stack[1:])``).  NumPy arrays of any real dtype or ROCm tensors.
    ``window``, ``step``, ``search``: int or (y, x); ``step=None`` is ``window // 2``.
    ``subpixel``: True is the reference's 3x3 Taylor step, which puts the y correction on dx and the x correction on dy
    (kept for parity with ``template_matching``); ``"newton"`` is the same step with each correction on its own axis, the
    field that ``preprocessing.distortion.correct_distortion`` needs; False keeps integer shifts.
    Returns {"dy", "dx", "peak", "snr": float64 (gy, gx) or (T, gy, gx); "y", "x": window centres; "meta": {...}};
    with ``return_tensors=True`` the four maps are device tensors."""
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    sub = _subpixel_code(subpixel)
    rs, ims = _shape(reference), _shape(images)
    if len(rs) not in (2, 3) or len(ims) not in (2, 3):
        raise ValueError(f"reference and images must be (H, W) or (T, H, W), got {rs} and {ims}")
    if rs[-2:] != ims[-2:]:
        raise ValueError(f"reference frames {rs[-2:]} and image frames {ims[-2:]} differ in shape")
    if len(rs) == 3 and (len(ims) != 3 or rs[0] != ims[0]):
        raise ValueError(f"a (T, H, W) reference needs (T, H, W) images with the same T, got {rs} and {ims}")
    if 0 in rs or 0 in ims:
        raise ValueError("empty reference or images")
    g = displacement_grid(rs[-2:], window=window, step=step, search=search)
    torch = _ffi.require_gpu()
    ref, _, _ = D.to_device_f32(reference, ndim=(2, 3))
    img, _, _ = D.to_device_f32(images, ndim=(2, 3))
    ref = ref.reshape((-1,) + rs[-2:])
    img = img.reshape((-1,) + ims[-2:])
    nref, nimg = int(ref.shape[0]), int(img.shape[0])
    pair_img = np.arange(nimg, dtype=np.int32)
    pair_ref = pair_img.copy() if len(rs) == 3 else np.zeros(nimg, dtype=np.int32)
    (wy, wx), (sty, stx), (sy, sx), (gy, gx) = g["window"], g["step"], g["search"], g["shape"]
    H, W = rs[-2:]
    out = torch.empty((nimg, gy, gx, 4), dtype=torch.float64, device=img.device)
    _ffi.check(_ffi.lib().b4d_displacement_map(
        D.ptr(ref), nref, D.ptr(img), nimg, pair_ref.ctypes.data_as(_ffi.C.c_void_p), pair_img.ctypes.data_as(_ffi.C.c_void_p),
        nimg, H, W, wy, wx, sty, stx, sy, sx, int(backend == "opencv"), sub, float(eps), D.ptr(out), None,
        _ffi.stream_ptr()))
    if len(ims) == 2:
        out = out[0]
    res = out if return_tensors else out.cpu().numpy()
    return {"dy": res[..., 0], "dx": res[..., 1], "peak": res[..., 2], "snr": res[..., 3], "y": g["y"], "x": g["x"],
            "meta": {"window": (wy, wx), "step": (sty, stx), "search": (sy, sx), "backend": backend}}
