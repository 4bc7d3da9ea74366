"""Hartmann / Shack-Hartmann analysis: spot centroids over a lattice of cells, the lattice fit and slope maps
(``b4d_spot_centroids``).

A Hartmann mask or a lenslet array turns a beam into a lattice of spots, one per cell; the shift of a spot's centroid is the local
wavefront slope.  ``hartmann_cells`` lays the cells out (host only), ``spot_centroids`` measures every spot of every frame on the
device, ``hartmann_lattice`` finds pitch, origin and rotation of a reference frame, and ``hartmann_displacement`` returns the
``displacement_map`` layout, so that ``wavefront_from_displacement``, ``modal_fit`` and ``focal_spot`` work on it unchanged.
There is no host fallback for the centroids.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi

MIN_SIDE = 2
MAX_SIDE = 128
QUANTITIES = ("cy", "cx", "flux", "peak", "peak_y", "peak_x", "background", "noise", "var_y", "var_x", "cov_yx", "n_pixels",
              "n_saturated", "n_nan")
COUNTS = ("n_pixels", "n_saturated", "n_nan")
BACKGROUNDS = ("none", "min", "border")
METHODS = ("cog", "iwcog")


def _is_number(v) -> bool:
    """A real scalar that is not a bool."""
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _real_pair(v, name: str) -> tuple[float, float]:
    if np.ndim(v) == 0:
        y = x = v
    elif np.ndim(v) == 1 and len(v) == 2:
        y, x = v
    else:
        raise ValueError(f"{name} must be a number or a (y, x) pair, got {v!r}")
    out = []
    for a in (y, x):
        if not _is_number(a) or not np.isfinite(a):
            raise ValueError(f"{name} must hold finite numbers, got {v!r}")
        out.append(float(a))
    return out[0], out[1]


def _axis_edges(n: int, p: float, o: float):
    """Edges floor(o + i p + 0.5) of the whole cells inside [0, n] and the index i of the first of them."""
    i = np.arange(int(np.floor(-o / p)) - 2, int(np.ceil((n - o) / p)) + 3, dtype=np.int64)
    e = np.floor(o + i * p + 0.5).astype(np.int64)
    keep = (e >= 0) & (e <= n)
    return e[keep].astype(np.int32), (int(i[keep][0]) if keep.any() else 0)


def hartmann_cells(shape, pitch, origin=(0.0, 0.0)) -> dict:
    """Host-only cell geometry of a spot lattice on frames of ``shape`` = (H, W) (no device needed).

    ``pitch``: a number or a (y, x) pair in pixels, not necessarily whole; ``origin``: where cell 0 begins.  Cell row i spans the
    rows ``[floor(oy + i py + 0.5), floor(oy + (i + 1) py + 0.5))``, columns likewise; only whole cells inside the frame are kept.
    Returns {"pitch", "origin": (y, x) pairs, "y_edges", "x_edges": int32 (gy + 1,), (gx + 1,), "y", "x": the nominal spot
    positions ``o + (i + 0.5) p - 0.5`` (float64, a regular axis), "shape": (gy, gx)}.  ValueError for a pitch <= 0 or a frame that
    holds no whole cell, NotImplementedError for a cell side outside 2 .. 128."""
    H, W = (int(s) for s in shape)
    py, px = _real_pair(pitch, "pitch")
    oy, ox = _real_pair(origin, "origin")
    if py <= 0.0 or px <= 0.0:
        raise ValueError(f"pitch must be > 0, got {pitch!r}")
    if H < 1 or W < 1:
        raise ValueError(f"empty frame {(H, W)}")
    ye, iy = _axis_edges(H, py, oy)
    xe, ix = _axis_edges(W, px, ox)
    if ye.size < 2 or xe.size < 2:
        raise ValueError(f"a {(H, W)} frame holds no whole cell of pitch {(py, px)} from origin {(oy, ox)}")
    for e in (ye, xe):
        s = np.diff(e)
        if s.min() < MIN_SIDE or s.max() > MAX_SIDE:
            raise NotImplementedError(f"cell sides must be {MIN_SIDE} .. {MAX_SIDE} px, pitch {(py, px)} gives {int(s.min())} .. {int(s.max())}")
    y = oy + (iy + np.arange(ye.size - 1) + 0.5) * py - 0.5
    x = ox + (ix + np.arange(xe.size - 1) + 0.5) * px - 0.5
    return {"pitch": (py, px), "origin": (oy, ox), "y_edges": ye, "x_edges": xe, "y": y, "x": x,
            "shape": (int(ye.size - 1), int(xe.size - 1))}


def _shape(a):
    return tuple(int(s) for s in a.shape) if D.is_tensor(a) else np.shape(a)


def _check_cells(cells, frame_shape) -> tuple[np.ndarray, np.ndarray]:
    if not isinstance(cells, dict) or any(k not in cells for k in ("y_edges", "x_edges", "y", "x", "pitch")):
        raise ValueError("cells must be a hartmann_cells dict (pitch, y_edges, x_edges, y, x)")
    out = []
    for k, n in zip(("y_edges", "x_edges"), frame_shape):
        e = np.asarray(cells[k])
        if e.ndim != 1 or e.size < 2 or e.dtype.kind not in "iu":
            raise ValueError(f"cells[{k!r}] must be a 1-D integer array of at least two edges")
        e = np.ascontiguousarray(e, dtype=np.int32)
        s = np.diff(e.astype(np.int64))
        if s.min() < 1:
            raise ValueError(f"cells[{k!r}] must ascend")
        if e[0] < 0 or e[-1] > n:
            raise ValueError(f"cells[{k!r}] leaves the frame ({n} px)")
        if s.min() < MIN_SIDE or s.max() > MAX_SIDE:
            raise NotImplementedError(f"cell sides must be {MIN_SIDE} .. {MAX_SIDE} px, cells[{k!r}] gives {int(s.min())} .. {int(s.max())}")
        out.append(e)
    if np.shape(cells["y"]) != (out[0].size - 1,) or np.shape(cells["x"]) != (out[1].size - 1,):
        raise ValueError("cells['y'], cells['x'] must hold one nominal position per cell")
    return out[0], out[1]


def _spot_options(cells_pitch, background, threshold, method, sigma, iterations, saturation) -> dict:
    """The kernel's arguments after every host check."""
    if isinstance(background, str):
        if background not in BACKGROUNDS:
            raise ValueError(f'background must be one of {BACKGROUNDS} or a number, got {background!r}')
        mode, value = {"none": 0, "min": 2, "border": 3}[background], 0.0
    elif not _is_number(background) or not np.isfinite(background):
        raise ValueError(f'background must be one of {BACKGROUNDS} or a finite number, got {background!r}')
    else:
        mode, value = 1, float(background)
    if not _is_number(threshold) or not 0.0 <= threshold < 1.0:
        raise ValueError(f"threshold must be in [0, 1), got {threshold!r}")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if sigma is None:
        sigma = 0.25 * min(cells_pitch)
    elif not _is_number(sigma) or not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma must be None or a number > 0, got {sigma!r}")
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
    if saturation is None:
        saturation = np.inf
    elif not _is_number(saturation) or np.isnan(saturation):
        raise ValueError(f"saturation must be None or a number, got {saturation!r}")
    return {"background": background, "mode": mode, "value": value, "threshold": float(threshold), "method": method,
            "sigma": float(sigma), "iterations": int(iterations), "saturation": float(saturation)}


def _check_frames(a, name: str, ndims=(2, 3)) -> tuple:
    s = _shape(a)
    if len(s) not in ndims or 0 in s:
        want = " or ".join("(H, W)" if n == 2 else "(T, H, W)" for n in ndims)
        raise ValueError(f"{name} must be {want} and not empty, got shape {s}")
    return s


def _centroids_device(images, ye, xe, o):
    """(T, gy, gx, 14) float64 device tensor of b4d_spot_centroids."""
    torch = _ffi.require_gpu()
    img, _, _ = D.to_device_f32(images, ndim=(2, 3))
    H, W = int(img.shape[-2]), int(img.shape[-1])
    img = img.reshape(-1, H, W)
    T, gy, gx = int(img.shape[0]), int(ye.size - 1), int(xe.size - 1)
    out = torch.empty((T, gy, gx, len(QUANTITIES)), dtype=torch.float64, device=img.device)
    _ffi.check(_ffi.lib().b4d_spot_centroids(
        D.ptr(img), T, H, W, ye.ctypes.data_as(_ffi.C.c_void_p), gy, xe.ctypes.data_as(_ffi.C.c_void_p), gx, o["mode"], o["value"],
        o["threshold"], METHODS.index(o["method"]), o["sigma"], o["iterations"], o["saturation"], D.ptr(out), _ffi.stream_ptr()))
    return out


def _meta(cells, o) -> dict:
    return {"pitch": tuple(cells["pitch"]), "origin": tuple(cells.get("origin", (np.nan, np.nan))),
            **{k: o[k] for k in ("background", "threshold", "method", "sigma", "iterations", "saturation")}}


def spot_centroids(images, cells, *, background="border", threshold=0.1, method="cog", sigma=None, iterations=8, saturation=None,
                   return_tensors: bool = False) -> dict:
    """Centroid, flux, peak, background, noise and second moments of the spot in every cell of every frame.

    ``images``: (H, W) or (T, H, W), a NumPy array of any real dtype or a ROCm tensor; ``cells``: a ``hartmann_cells`` dict.
    ``background``: "none" (0), "min" (the cell's minimum), "border" (the mean of the cell's one-pixel outer ring) or a number.
    Pixels weigh ``max(v - t, 0)`` with ``t = b + threshold (peak - b)``, ``0 <= threshold < 1``.  ``method``: "cog", the centre
    of gravity, or "iwcog", ``iterations`` rounds of the centre of gravity under a Gaussian window of ``sigma`` px (``None``: a
    quarter of the smaller pitch) that follows the estimate.  ``saturation``: pixels at or above it are counted (``None``: off).
    Returns {"cy", "cx", "flux", "peak", "peak_y", "peak_x", "background", "noise", "var_y", "var_x", "cov_yx": float64 (gy, gx)
    or (T, gy, gx), positions in frame coordinates; "n_pixels", "n_saturated", "n_nan": int64; "y", "x": the nominal positions;
    "meta"}.  A cell without flux (constant, empty, all NaN) has NaN centroid and moments.  With ``return_tensors=True`` all
    fourteen maps are float64 device tensors."""
    ims = _check_frames(images, "images")
    ye, xe = _check_cells(cells, ims[-2:])
    o = _spot_options(cells["pitch"], background, threshold, method, sigma, iterations, saturation)
    out = _centroids_device(images, ye, xe, o)
    if len(ims) == 2:
        out = out[0]
    res = {"y": np.asarray(cells["y"], dtype=np.float64), "x": np.asarray(cells["x"], dtype=np.float64), "meta": _meta(cells, o)}
    host = None if return_tensors else out.cpu().numpy()
    for k, name in enumerate(QUANTITIES):
        if return_tensors:
            res[name] = out[..., k]
        else:
            res[name] = host[..., k].astype(np.int64) if name in COUNTS else np.ascontiguousarray(host[..., k])
    return res


# ------------------------------------------------------------------------------------------------------------------ lattice
def _first_peak(profile: np.ndarray) -> float:
    """Lag of the first local maximum after the first minimum of an autocorrelation profile (lag 0 first), refined by the
    parabola through it and its neighbours.  The flat floor between two lattice peaks holds rounding ripple, so the minimum
    counts once the profile has fallen below half height (between its lowest value and lag 0) and the maximum once it is back
    above it."""
    n = profile.size
    half = 0.5 * (profile[0] + profile.min())
    k = 1
    while k + 1 < n and profile[k] >= half:
        k += 1
    while k + 1 < n and profile[k] <= half:
        k += 1
    while k + 1 < n and profile[k + 1] >= profile[k]:
        k += 1
    if k < 2 or k + 1 >= n:
        raise ValueError("no lattice period found in the reference's autocorrelation; pass pitch=")
    a, b, c = profile[k - 1], profile[k], profile[k + 1]
    den = a - 2.0 * b + c
    return float(k + (0.5 * (a - c) / den if den < 0.0 else 0.0))


def _estimate_pitch(reference) -> tuple[float, float]:
    from .corr import autocorr2d

    ac, _, _ = autocorr2d(reference, remove_mean=True, normalize="peak")
    ny, nx = ac.shape
    return _first_peak(ac[ny // 2:, nx // 2]), _first_peak(ac[ny // 2, nx // 2:])


def _good_spots(s: dict) -> np.ndarray:
    """Cells of a reference pass that hold a spot: flux, no saturation, and a height of at least a quarter of the typical one."""
    height = s["peak"] - s["background"]
    ok = np.isfinite(s["cy"]) & np.isfinite(s["cx"]) & (s["flux"] > 0) & (s["n_saturated"] == 0) & np.isfinite(height)
    if not ok.any():
        raise ValueError("the reference holds no spot")
    return ok & (height >= 0.25 * np.percentile(height[ok], 90.0))


def _circular_origin(pos: np.ndarray, weight: np.ndarray, p: float) -> float:
    """Origin in [-0.5, p - 0.5) that puts spots at `pos` (mod p) at the cell centres."""
    ang = 2.0 * np.pi * np.mod(pos, p) / p
    s = np.arctan2(np.sum(weight * np.sin(ang)), np.sum(weight * np.cos(ang))) * p / (2.0 * np.pi)
    return float(np.mod(s + 0.5 - 0.5 * p + 0.5, p) - 0.5)


def hartmann_lattice(reference, *, pitch=None, rotation_limit: float = 0.25, **spot_options) -> dict:
    """Pitch, origin and rotation of the spot lattice of a reference frame (H, W).

    ``pitch=None`` takes a first estimate from the frame's autocorrelation (``autocorr2d``): the first maximum after the first
    minimum along the central row and column.  One ``spot_centroids`` pass on cells of that pitch from origin (0, 0) gives each
    cell about one spot maximum; the circular mean of their positions modulo the pitch centres the cells on the spots, a second
    pass measures the centroids, and a least-squares fit of them to ``origin + (i + 0.5) pitch - 0.5`` with cross terms gives
    the final pitch, origin and the lattice's rotation.  ``spot_options`` go to ``spot_centroids``.
    Returns a ``hartmann_cells`` dict plus "rotation" in radians (cells stay axis-aligned).  ValueError for a rotation that
    carries a spot across more than ``rotation_limit`` of a pitch over the frame, or a reference without a lattice."""
    rs = _check_frames(reference, "reference", ndims=(2,))
    if not (_is_number(rotation_limit) and rotation_limit > 0.0):
        raise ValueError(f"rotation_limit must be > 0, got {rotation_limit!r}")
    if "return_tensors" in spot_options:
        raise ValueError("hartmann_lattice works on the host maps: return_tensors is not an option here")
    if pitch is not None:
        py, px = _real_pair(pitch, "pitch")
        if py <= 0.0 or px <= 0.0:
            raise ValueError(f"pitch must be > 0, got {pitch!r}")
        hartmann_cells(rs, (py, px))     # its errors before any device call
    _spot_options((1.0, 1.0), **{**dict(background="border", threshold=0.1, method="cog", sigma=None, iterations=8, saturation=None),
                                 **spot_options})
    if pitch is None:
        py, px = _estimate_pitch(reference)
    # first pass: whatever the origin, a cell of the right pitch holds about one spot maximum
    first = spot_centroids(reference, hartmann_cells(rs, (py, px)), **spot_options)
    ok = _good_spots(first)
    wgt = np.where(ok, first["peak"] - first["background"], 0.0)
    oy = _circular_origin(np.where(ok, first["peak_y"], 0.0), wgt, py)
    ox = _circular_origin(np.where(ok, first["peak_x"], 0.0), wgt, px)
    # second pass on centred cells, then the affine fit y = Y0 + A i + B j, x = X0 + C i + D j
    cells = hartmann_cells(rs, (py, px), (oy, ox))
    s = spot_centroids(reference, cells, **spot_options)
    ok = _good_spots(s)
    if ok.sum() < 3 or np.unique(np.nonzero(ok)[0]).size < 2 or np.unique(np.nonzero(ok)[1]).size < 2:
        raise ValueError("the reference holds too few spots for a lattice fit")
    gy, gx = cells["shape"]
    ii, jj = np.meshgrid(np.arange(gy, dtype=np.float64), np.arange(gx, dtype=np.float64), indexing="ij")
    ic, jc = 0.5 * (gy - 1), 0.5 * (gx - 1)
    A = np.stack([np.ones(int(ok.sum())), ii[ok] - ic, jj[ok] - jc], axis=1)
    (Y0, Ay, By), _, _, _ = np.linalg.lstsq(A, s["cy"][ok], rcond=None)
    (X0, Cx, Dx), _, _, _ = np.linalg.lstsq(A, s["cx"][ok], rcond=None)
    if not (Ay > 0.0 and Dx > 0.0):
        raise ValueError("the lattice fit gave a non-positive pitch")
    rotation = 0.5 * (np.arctan2(By, Dx) + np.arctan2(-Cx, Ay))
    if abs(rotation) * max(rs) > rotation_limit * min(Ay, Dx):
        raise ValueError(f"the lattice is rotated by {rotation:.3g} rad: more than {rotation_limit} of a pitch over the frame")
    # (Y0, X0) is the lattice at the grid centre; cell 0 of the second pass begins half a pitch before its spot
    fy = Y0 - ic * Ay - 0.5 * Ay + 0.5
    fx = X0 - jc * Dx - 0.5 * Dx + 0.5
    out = hartmann_cells(rs, (float(Ay), float(Dx)), (float(np.mod(fy + 0.5, Ay) - 0.5), float(np.mod(fx + 0.5, Dx) - 0.5)))
    out["rotation"] = float(rotation)
    return out


# ------------------------------------------------------------------------------------------------------------- displacement
def hartmann_displacement(reference, images, *, cells=None, pitch=None, min_snr: float = 3.0, background="border", threshold=0.1,
                          method="cog", sigma=None, iterations=8, saturation=None, return_tensors: bool = False) -> dict:
    """Spot shifts of ``images`` against ``reference`` in the ``displacement_map`` layout.

    ``reference``: ``None`` (absolute mode: shifts against the nominal positions of ``cells``, which is then required), (H, W),
    or (T, H, W) paired frame by frame with (T, H, W) ``images``.  ``cells=None`` calls ``hartmann_lattice(reference, pitch=pitch)``
    on the reference (its first frame if it is a stack).  The spot options are those of ``spot_centroids``.
    Returns {"dy", "dx": image centroid minus reference centroid in px, NaN where not valid; "y", "x": nominal positions;
    "peak": spot height ``peak - background`` over the largest valid one of its frame, in [0, 1], 0 where not valid;
    "snr": ``(peak - background) / max(noise, 2**-24 max(|peak|, |background|, 1e-30))`` of the image spot; "valid": in image and
    reference ``flux > 0``, ``n_saturated == 0`` and ``snr >= min_snr``; "transmission": flux over the reference's;
    "dark_field": ``var_y + var_x`` less the reference's, px^2 (spot broadening); "meta"}.  In absolute mode "transmission" and
    "dark_field" are NaN (there is nothing to compare with).  Maps are float64 (gy, gx) or (T, gy, gx), "valid" bool; device
    tensors with ``return_tensors=True``.  ``wavefront_from_displacement(m, ..., weights="peak", mask=m["valid"])`` takes it as it is."""
    ims = _check_frames(images, "images")
    if reference is None:
        if cells is None:
            raise ValueError("absolute mode (reference=None) needs cells")
    else:
        rs = _check_frames(reference, "reference")
        if rs[-2:] != ims[-2:]:
            raise ValueError(f"reference frames {rs[-2:]} and image frames {ims[-2:]} differ in shape")
        if len(rs) == 3 and (len(ims) != 3 or rs[0] != ims[0]):
            raise ValueError(f"a (T, H, W) reference needs (T, H, W) images with the same T, got {rs} and {ims}")
    if not _is_number(min_snr) or np.isnan(min_snr):
        raise ValueError(f"min_snr must be a number, got {min_snr!r}")
    opts = dict(background=background, threshold=threshold, method=method, sigma=sigma, iterations=iterations, saturation=saturation)
    if cells is None:
        _spot_options((1.0, 1.0), **opts)
        cells = hartmann_lattice(reference if len(rs) == 2 else reference[0], pitch=pitch, **opts)
    ye, xe = _check_cells(cells, ims[-2:])
    o = _spot_options(cells["pitch"], **opts)
    torch = _ffi.require_gpu()

    def measure(frames):
        s = _centroids_device(frames, ye, xe, o)
        q = {name: s[..., k] for k, name in enumerate(QUANTITIES)}
        height = q["peak"] - q["background"]
        floor = 2.0 ** -24 * torch.clamp(torch.maximum(q["peak"].abs(), q["background"].abs()), min=1e-30)
        q["height"] = height
        q["snr"] = height / torch.maximum(q["noise"], floor)
        q["ok"] = (q["flux"] > 0) & (q["n_saturated"] == 0) & (q["snr"] >= float(min_snr))
        return q

    S = measure(images)
    nan = torch.full_like(S["cy"], float("nan"))
    if reference is None:
        valid = S["ok"]
        ry = torch.as_tensor(np.asarray(cells["y"], dtype=np.float64), device=nan.device)[None, :, None]
        rx = torch.as_tensor(np.asarray(cells["x"], dtype=np.float64), device=nan.device)[None, None, :]
        transmission, dark = nan, nan.clone()
    else:
        R = measure(reference)
        valid = S["ok"] & R["ok"]
        ry, rx = R["cy"], R["cx"]
        transmission = torch.where(valid, S["flux"] / R["flux"], nan)
        dark = torch.where(valid, (S["var_y"] + S["var_x"]) - (R["var_y"] + R["var_x"]), nan)
    height = torch.where(valid, S["height"], torch.zeros_like(nan))
    top = height.amax(dim=(-2, -1), keepdim=True)
    res = {"dy": torch.where(valid, S["cy"] - ry, nan), "dx": torch.where(valid, S["cx"] - rx, nan),
           "peak": torch.where(top > 0, height / top, torch.zeros_like(nan)),
           "snr": S["snr"], "valid": valid, "transmission": transmission, "dark_field": dark}
    if len(ims) == 2:
        res = {k: v[0] for k, v in res.items()}
    if not return_tensors:
        res = {k: v.cpu().numpy() for k, v in res.items()}
    res.update({"y": np.asarray(cells["y"], dtype=np.float64), "x": np.asarray(cells["x"], dtype=np.float64),
                "meta": {**_meta(cells, o), "min_snr": float(min_snr), "absolute": reference is None,
                         "rotation": cells.get("rotation")}})
    return res
