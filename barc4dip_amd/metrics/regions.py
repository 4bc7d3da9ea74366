"""Per-region measurements of a label map on the device (``b4d_region_properties``): area, bounding box,
centroids, sums, extrema, flux-weighted centroid and second moments of every region of every frame, and ``find_spots``, which
thresholds, labels, measures and filters in one call.  There is no host fallback.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .. import _frames
from ..geometry import labels as L

COLUMNS = L.COLUMNS
INTEGER_COLUMNS = L.INTEGER_COLUMNS


def _check_values(background, saturation) -> tuple[float, float]:
    if not L._is_number(background) or not np.isfinite(background):
        raise ValueError(f"background must be a finite number, got {background!r}")
    if saturation is None:
        saturation = np.inf
    elif not L._is_number(saturation) or np.isnan(saturation):
        raise ValueError(f"saturation must be None or a number, got {saturation!r}")
    return float(background), float(saturation)


def _table_dict(table, n: np.ndarray, return_tensors: bool, rows=None, labels_of_rows=None) -> dict:
    """The dict of flat columns from a (rows, 20) float64 device tensor; n: regions per frame."""
    frame = np.repeat(np.arange(n.size, dtype=np.int64), n)
    label = (np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n) + 1) if labels_of_rows is None else labels_of_rows
    res = {}
    if return_tensors:
        torch = _ffi.require_gpu()
        for k, name in enumerate(COLUMNS):
            res[name] = table[:, k].to(torch.int64) if name in INTEGER_COLUMNS else table[:, k]
    else:
        host = table.cpu().numpy()
        for k, name in enumerate(COLUMNS):
            res[name] = host[:, k].astype(np.int64) if name in INTEGER_COLUMNS else np.ascontiguousarray(host[:, k])
    res["frame"], res["label"], res["n"] = frame, label, n
    return res


def region_properties(labels, images=None, *, background: float = 0.0, saturation=None, return_tensors: bool = False) -> dict:
    """Measure every region of a label map.

    ``labels``: (H, W) or (T, H, W) integers >= 0, NumPy or tensor; 0 is no region.  They may come from ``label_regions`` or from
    anywhere else (the rings of a two-time analysis ...): regions need not be connected, and a number without a pixel gives a row
    of area 0.  ``images``: frames of the same shape, or ``None`` for the geometry alone (the value columns are then NaN).
    With ``w = max(v - background, 0)`` per pixel; NaN pixels take no part in any value column and are counted in ``n_nan``;
    ``saturation``: pixels at or above it are counted in ``n_saturated`` (``None``: off).

    Returns a dict of flat arrays with one entry per region of every frame, in frame order, label order within a frame:
    ``area``, ``y0``, ``y1``, ``x0``, ``x1`` (the half-open box), ``max_y``, ``max_x`` (where ``max`` is, first occurrence in
    raster order), ``n_nan``, ``n_saturated``: int64; ``cy``, ``cx`` (geometric centroid), ``sum``, ``min``, ``max``, ``flux``
    (sum of w), ``wcy``, ``wcx`` (w-weighted centroid, NaN where flux is not > 0), ``var_y``, ``var_x``, ``cov_yx`` (w-weighted
    second moments about it): float64; and ``frame``, ``label`` (int64) and ``n`` (T,), the regions per frame.  Integer columns are
    exact and every column has the same bits call after call, for a frame alone and in any stack.  With ``return_tensors=True``
    the twenty columns are device tensors.  Sizing the table needs the largest label of every frame: the one synchronisation."""
    ls = L._shape(labels)
    if images is not None:
        ims = L._check_stack_shape(images, "images")
        if tuple(ims) != tuple(ls):
            raise ValueError(f"labels {ls} and images {ims} must have the same shape")
    bg, sat = _check_values(background, saturation)
    labels_t, _ = L._label_tensor(labels)
    img = None
    if images is not None:
        img, T, H, W = _frames.frame_stack(images)
        img = img.reshape(T, H, W)
    n = L.count_labels(labels_t)
    return _table_dict(L.properties_device(labels_t, img, n, bg, sat), n, return_tensors)


def find_spots(images, threshold, *, connectivity: int = 2, min_area=1, max_area=None, clear_border: bool = False,
               background: float = 0.0, saturation=None, return_labels: bool = False):
    """Threshold, label, measure and filter in one call: the blobs of ``images > threshold`` with their centroids and fluxes.

    ``images``, ``threshold`` (a number, a (T,) array or a hysteresis pair) and ``connectivity`` as in ``label_regions``;
    ``min_area``, ``max_area``, ``clear_border`` as in ``select_regions``; ``background``, ``saturation`` as in
    ``region_properties``.  Returns the ``region_properties`` dict of the regions that are kept, renumbered 1 .. n' per frame;
    with ``return_labels=True`` the pair (dict, labels) with the int32 label map of the kept regions."""
    s = L._check_stack_shape(images, "images")
    conn = L._check_connectivity(connectivity)
    low, high = L._check_threshold(threshold, s[0] if len(s) == 3 else 1)
    bg, sat = _check_values(background, saturation)
    L._check_select(None, min_area, max_area, clear_border, None, None)
    img, T, H, W = _frames.frame_stack(images)
    img = img.reshape(T, H, W)
    labels_t, n_dev = L.label_device(img, low, None, conn)
    n = L.read_counts(n_dev)
    table = L.properties_device(labels_t, img, n, bg, sat)
    host = table.cpu().numpy()
    col = {k: host[:, COLUMNS.index(k)] for k in ("area", "y0", "y1", "x0", "x1", "max")}
    ok = L.select_mask(col["area"].astype(np.int64), col["y0"], col["y1"], col["x0"], col["x1"], n, (H, W),
                       None if high is None else col["max"] > high, min_area, max_area, bool(clear_border), None)
    remap, kept = L.renumber(ok, n)
    rows = np.flatnonzero(ok)
    res = _table_dict(table[_ffi.require_gpu().from_numpy(rows).to(table.device)], kept, False)
    if not return_labels:
        return res
    lab = L.relabel_device(labels_t, n, remap)
    return res, (lab[0] if len(s) == 2 else lab).cpu().numpy()
