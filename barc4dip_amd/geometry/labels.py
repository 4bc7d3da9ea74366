"""Connected-component labelling on the device: which pixels of a frame belong together (``b4d_label_regions``, ``b4d_relabel``;
DESIGN.md section 32).

``label_regions`` numbers the connected regions of a thresholded frame or of a mask exactly as ``scipy.ndimage.label`` does,
``select_regions`` keeps some of them and renumbers, ``largest_region`` is the one-liner for the masks of the wavefront chain.
The measurements of the regions are in ``barc4dip_amd.metrics.regions``.  There is no host fallback.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .. import _frames

# what the kernels are built with (csrc/b4d_label.hpp): the tile of the first pass (rows, columns), the pixels per block of the
# numbering scan, the box area above which a region is measured by a workgroup instead of a wave
TILE = (32, 64)
SCAN_BLOCK = 2048
WAVE_AREA = 4096
ELOOP = -5

# columns of b4d_region_properties, in order
COLUMNS = ("area", "y0", "y1", "x0", "x1", "cy", "cx", "sum", "min", "max", "max_y", "max_x", "flux", "wcy", "wcx", "var_y", "var_x",
           "cov_yx", "n_nan", "n_saturated")
INTEGER_COLUMNS = ("area", "y0", "y1", "x0", "x1", "max_y", "max_x", "n_nan", "n_saturated")


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _shape(a) -> tuple:
    return tuple(int(s) for s in a.shape) if hasattr(a, "shape") else np.shape(a)


def _is_complex(a) -> bool:
    return bool(a.is_complex()) if D.is_tensor(a) else np.iscomplexobj(a)


def _check_stack_shape(a, name: str) -> tuple:
    s = _shape(a)
    if len(s) not in (2, 3):
        raise ValueError(f"{name} must be (H, W) or (T, H, W); got shape {s}")
    if 0 in s:
        raise ValueError(f"{name} must not be empty; got shape {s}")
    if _is_complex(a):
        raise NotImplementedError(f"complex {name} is not supported (real frames only).")
    return s


def _check_connectivity(connectivity) -> int:
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (edges) or 2 (edges and corners), got {connectivity!r}")
    return int(connectivity)


def _check_threshold(threshold, frames: int):
    """(low (T,) float32, high or None) of a number, a (T,) array, or a (low, high) pair of numbers (a tuple or a list)."""
    if isinstance(threshold, (tuple, list)) and len(threshold) == 2 and all(_is_number(v) for v in threshold):
        low, high = float(threshold[0]), float(threshold[1])
        if np.isnan(low) or np.isnan(high):
            raise ValueError(f"threshold must not be NaN, got {threshold!r}")
        if low > high:
            raise ValueError(f"hysteresis thresholds must be (low, high) with low <= high, got {threshold!r}")
        return np.full(frames, low, dtype=np.float32), high
    if _is_number(threshold):
        if np.isnan(threshold):
            raise ValueError("threshold must not be NaN")
        return np.full(frames, float(threshold), dtype=np.float32), None
    if threshold is None or isinstance(threshold, (str, bool, np.bool_)) or D.is_tensor(threshold):
        raise ValueError(f"threshold must be a number, a (T,) array or a (low, high) pair, got {threshold!r}")
    t = np.asarray(threshold)
    if t.dtype.kind not in "iuf" or t.ndim != 1:
        raise ValueError(f"threshold must be a number, a (T,) array or a (low, high) pair, got {threshold!r}")
    if t.shape != (frames,):
        raise ValueError(f"a threshold per frame must have shape ({frames},), got {t.shape}")
    if np.isnan(t.astype(np.float64)).any():
        raise ValueError("threshold must not be NaN")
    return np.ascontiguousarray(t, dtype=np.float32), None


def _mask_tensor(mask):
    """(T, H, W) uint8 device tensor of a bool / uint8 mask."""
    torch = _ffi.require_gpu()
    if D.is_tensor(mask):
        t = mask.to(device="cuda")
        t = t.to(torch.uint8) if t.dtype == torch.bool else t
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(mask), dtype=np.uint8)).to("cuda")
    return t.reshape((-1,) + tuple(t.shape[-2:])).contiguous()


def _check_mask(mask) -> tuple:
    s = _check_stack_shape(mask, "mask")
    if D.is_tensor(mask):
        import torch

        ok = mask.dtype in (torch.bool, torch.uint8)
    else:
        ok = np.asarray(mask).dtype in (np.dtype(bool), np.dtype(np.uint8))
    if not ok:
        raise ValueError("mask must be bool or uint8")
    return s


def read_counts(n_dev) -> np.ndarray:
    """The region counts of a call as int64 on the host: the one synchronisation of the labelling.  B4DError for a call whose
    kernels reached a loop bound (b4d.h: B4D_ELOOP)."""
    n = n_dev.cpu().numpy().astype(np.int64)
    if (n < 0).any():
        raise _ffi.B4DError(f"b4d error {ELOOP}: b4d_label_regions reached a loop bound of its union-find (the label array was "
                            "modified while it ran, or device memory is corrupt)")
    return n


def label_device(frames_t, thresholds, mask_t, connectivity: int):
    """b4d_label_regions on device tensors: frames_t (T, H, W) float32 with thresholds (T,) float32 on the host, or mask_t
    (T, H, W) uint8.  Returns (labels (T, H, W) int32, n (T,) int32), both on the device; nothing is read back."""
    torch = _ffi.require_gpu()
    src = frames_t if mask_t is None else mask_t
    T, H, W = (int(s) for s in src.shape)
    labels = torch.empty((T, H, W), dtype=torch.int32, device=src.device)
    n = torch.empty((T,), dtype=torch.int32, device=src.device)
    thr = None if mask_t is not None else torch.from_numpy(thresholds).to(src.device)
    _ffi.check(_ffi.lib().b4d_label_regions(
        D.ptr(frames_t) if mask_t is None else None, D.ptr(thr) if thr is not None else None, D.ptr(mask_t) if mask_t is not None else None,
        T, H, W, int(connectivity), D.ptr(labels), D.ptr(n), _ffi.stream_ptr()))
    return labels, n


def offsets_of(n: np.ndarray) -> np.ndarray:
    """HOST int32 (T + 1,) row offsets of per-frame region counts."""
    off = np.zeros(n.size + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    if off[-1] >= 2 ** 31:
        raise NotImplementedError(f"{int(off[-1])} regions in one call: the table is indexed with 32 bits")
    return np.ascontiguousarray(off, dtype=np.int32)


def properties_device(labels_t, frames_t, n: np.ndarray, background: float = 0.0, saturation: float = np.inf):
    """b4d_region_properties: (sum(n), 20) float64 device tensor for labels_t (T, H, W) int32, frames_t (T, H, W) float32 or None."""
    torch = _ffi.require_gpu()
    T, H, W = (int(s) for s in labels_t.shape)
    off = offsets_of(n)
    out = torch.empty((int(off[-1]), len(COLUMNS)), dtype=torch.float64, device=labels_t.device)
    _ffi.check(_ffi.lib().b4d_region_properties(
        D.ptr(frames_t) if frames_t is not None else None, D.ptr(labels_t), T, H, W, off.ctypes.data_as(_ffi.C.c_void_p),
        float(background), float(saturation), D.ptr(out) if off[-1] else None, _ffi.stream_ptr()))
    return out


def relabel_device(labels_t, n: np.ndarray, table: np.ndarray):
    """b4d_relabel: labels_t through the flat HOST table (sum(n),) old label -> new label (0 drops), a new device tensor."""
    torch = _ffi.require_gpu()
    T, H, W = (int(s) for s in labels_t.shape)
    off = offsets_of(n)
    out = torch.empty_like(labels_t)
    tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(labels_t.device) if off[-1] else None
    _ffi.check(_ffi.lib().b4d_relabel(D.ptr(labels_t), T, H, W, off.ctypes.data_as(_ffi.C.c_void_p),
                                      D.ptr(tab) if tab is not None else None, D.ptr(out), _ffi.stream_ptr()))
    return out


def renumber(keep: np.ndarray, n: np.ndarray):
    """(table, n'): the kept regions of every frame renumbered 1 .. n' in their old order; keep is flat over sum(n) regions."""
    keep = np.asarray(keep, dtype=bool)
    frame = np.repeat(np.arange(n.size), n)
    new_n = np.bincount(frame[keep], minlength=n.size).astype(np.int64)
    rank = np.cumsum(keep) - np.repeat(np.concatenate(([0], np.cumsum(new_n)[:-1])), n)
    return np.where(keep, rank, 0).astype(np.int32), new_n


def _result(labels_t, n: np.ndarray, squeeze: bool, return_tensors: bool):
    lab = labels_t[0] if squeeze else labels_t
    return (lab if return_tensors else lab.cpu().numpy()), (int(n[0]) if squeeze else n)


def label_regions(images=None, threshold=None, *, mask=None, connectivity: int = 1, return_tensors: bool = False):
    """Label the connected regions of ``images > threshold`` or of ``mask``.

    ``images``: (H, W) or (T, H, W), a NumPy array of any real dtype or a ROCm tensor, with ``threshold``: a number, a (T,) array
    (one per frame) or a ``(low, high)`` pair given as a tuple or a list (hysteresis: a region of ``v > low`` is kept only if its
    maximum is ``> high``).  The comparison is strict and made on the float32 frames and thresholds: a NaN pixel is background,
    ``+inf`` is foreground.  Or ``mask``: bool or uint8, non-zero is foreground.  Exactly one of ``images`` and ``mask``.
    ``connectivity``: 1 (pixels that share an edge) or 2 (an edge or a corner).

    Returns ``(labels, n)``: ``labels`` int32 of the input's shape, 0 on the background and 1 .. n on the regions, numbered per
    frame in the raster order of each region's first pixel, which is what ``scipy.ndimage.label`` returns; ``n`` a Python int, or
    an int64 (T,) array for a stack.  With ``return_tensors=True`` ``labels`` stays on the device.  Reading ``n`` back is the one
    synchronisation of the call (it sizes every table that follows)."""
    if (images is None) == (mask is None):
        raise ValueError("exactly one of images and mask must be given")
    conn = _check_connectivity(connectivity)
    if mask is not None:
        if threshold is not None:
            raise ValueError("threshold goes with images, not with mask")
        s = _check_mask(mask)
        labels_t, n_dev = label_device(None, None, _mask_tensor(mask), conn)
        return _result(labels_t, read_counts(n_dev), len(s) == 2, return_tensors)
    s = _check_stack_shape(images, "images")
    low, high = _check_threshold(threshold, s[0] if len(s) == 3 else 1)
    img, T, H, W = _frames.frame_stack(images)
    img = img.reshape(T, H, W)
    labels_t, n_dev = label_device(img, low, None, conn)
    n = read_counts(n_dev)
    if high is not None:
        top = properties_device(labels_t, img, n)[:, COLUMNS.index("max")].cpu().numpy()
        table, kept = renumber(top > high, n)      # dropping regions keeps the raster order of the others
        labels_t, n = relabel_device(labels_t, n, table), kept
    return _result(labels_t, n, len(s) == 2, return_tensors)


def _label_tensor(labels, name: str = "labels"):
    """((T, H, W) int32 device tensor, squeeze) of an integer label map; ValueError for negative labels."""
    s = _shape(labels)
    if len(s) not in (2, 3):
        raise ValueError(f"{name} must be (H, W) or (T, H, W); got shape {s}")
    if 0 in s:
        raise ValueError(f"{name} must not be empty; got shape {s}")
    if D.is_tensor(labels):
        import torch

        if labels.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool):
            raise ValueError(f"{name} must be integers, got {labels.dtype}")
        torch = _ffi.require_gpu()
        t = labels.to(device="cuda")
        if int(t.min()) < 0:
            raise ValueError(f"{name} must be >= 0")
        if int(t.max()) >= 2 ** 31:
            raise ValueError(f"{name} must be below 2^31")
        t = t.to(torch.int32)
    else:
        a = np.asarray(labels)
        if a.dtype.kind not in "iub":
            raise ValueError(f"{name} must be integers, got dtype {a.dtype}")
        if a.dtype.kind == "i" and a.min() < 0:
            raise ValueError(f"{name} must be >= 0")
        if a.max() >= 2 ** 31:
            raise ValueError(f"{name} must be below 2^31")
        torch = _ffi.require_gpu()
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda")
    return t.reshape((-1,) + tuple(t.shape[-2:])).contiguous(), len(s) == 2


def count_labels(labels_t) -> np.ndarray:
    """The largest label of every frame of a (T, H, W) device tensor, int64 on the host (a synchronisation)."""
    return labels_t.reshape(labels_t.shape[0], -1).amax(dim=1).cpu().numpy().astype(np.int64)


def _check_select(keep, min_area, max_area, clear_border, largest, properties):
    for name, v in (("min_area", min_area), ("max_area", max_area)):
        if v is not None and (not _is_number(v) or np.isnan(v)):
            raise ValueError(f"{name} must be None or a number, got {v!r}")
    if not isinstance(clear_border, (bool, np.bool_)):
        raise ValueError(f"clear_border must be a bool, got {clear_border!r}")
    if largest is not None and (isinstance(largest, (bool, np.bool_)) or not isinstance(largest, (int, np.integer)) or largest < 0):
        raise ValueError(f"largest must be None or an integer >= 0, got {largest!r}")
    if keep is not None:
        k = np.asarray(keep)
        if k.dtype != np.dtype(bool) or k.ndim != 1:
            raise ValueError("keep must be a flat bool table, one entry per region")
    if properties is not None and (not isinstance(properties, dict) or any(k not in properties for k in ("area", "y0", "y1", "x0", "x1", "n"))):
        raise ValueError("properties must be a region_properties dict (area, y0, y1, x0, x1, n)")


def select_mask(area, y0, y1, x0, x1, n, shape, keep=None, min_area=None, max_area=None, clear_border=False, largest=None) -> np.ndarray:
    """The flat bool table of the regions that pass every condition (host arithmetic on the table's columns)."""
    H, W = shape
    ok = np.ones(area.size, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    if ok.shape != area.shape:
        raise ValueError(f"keep must have one entry per region ({area.size}), got {ok.size}")
    if min_area is not None:
        ok &= area >= min_area
    if max_area is not None:
        ok &= area <= max_area
    if clear_border:
        ok &= (y0 > 0) & (x0 > 0) & (y1 < H) & (x1 < W)
    ok &= area > 0
    if largest is not None:
        first = 0
        for cnt in n:
            idx = first + np.flatnonzero(ok[first:first + cnt])
            order = idx[np.argsort(-area[idx], kind="stable")]     # stable: ties to the lower label
            ok[order[int(largest):]] = False
            first += int(cnt)
    return ok


def select_regions(labels, keep=None, *, min_area=None, max_area=None, clear_border: bool = False, largest=None, properties=None,
                   return_tensors: bool = False):
    """Keep some regions of a label map and renumber them 1 .. n' in their old order.

    ``labels``: (H, W) or (T, H, W) integers >= 0, NumPy or tensor (from ``label_regions`` or anywhere else).  A region is kept
    if it passes every condition given: ``keep`` (a flat bool table, one entry per region of every frame in frame order),
    ``min_area <= area <= max_area``, ``clear_border`` (its box touches no frame edge), and, among those, ``largest=k``: the k
    largest by area per frame, ties to the lower label.  ``properties``: a ``region_properties`` dict of ``labels`` if one is at
    hand (otherwise the geometry is measured here).  Returns ``(labels, n)`` as ``label_regions`` does."""
    _check_select(keep, min_area, max_area, clear_border, largest, properties)
    labels_t, squeeze = _label_tensor(labels)
    H, W = int(labels_t.shape[1]), int(labels_t.shape[2])
    if properties is None:
        n = count_labels(labels_t)
        tab = properties_device(labels_t, None, n).cpu().numpy()
        cols = {k: tab[:, COLUMNS.index(k)].astype(np.int64) for k in ("area", "y0", "y1", "x0", "x1")}
    else:
        n = np.atleast_1d(np.asarray(properties["n"], dtype=np.int64))
        if n.size != labels_t.shape[0]:
            raise ValueError(f"properties hold {n.size} frames, labels {int(labels_t.shape[0])}")
        cols = {k: np.asarray(properties[k], dtype=np.int64) for k in ("area", "y0", "y1", "x0", "x1")}
        if any(c.shape != (int(n.sum()),) for c in cols.values()):
            raise ValueError("properties do not hold one entry per region")
    ok = select_mask(cols["area"], cols["y0"], cols["y1"], cols["x0"], cols["x1"], n, (H, W), keep, min_area, max_area,
                     bool(clear_border), largest)
    table, new_n = renumber(ok, n)
    return _result(relabel_device(labels_t, n, table), new_n, squeeze, return_tensors)


def largest_region(mask, connectivity: int = 1):
    """The largest connected region of ``mask`` ((H, W) or (T, H, W), bool or uint8) as a bool mask of the same shape and kind
    (NumPy in, NumPy out; tensor in, tensor out); ties go to the region that comes first in raster order, an empty mask stays
    empty.  For ``wavefront_from_displacement(mask=...)`` and ``phase_unwrap``, which level disconnected pieces instead of
    measuring them."""
    conn = _check_connectivity(connectivity)
    s = _check_mask(mask)
    labels_t, n_dev = label_device(None, None, _mask_tensor(mask), conn)
    n = read_counts(n_dev)
    area = properties_device(labels_t, None, n)[:, 0].cpu().numpy().astype(np.int64)
    ok = np.zeros(area.size, dtype=bool)
    first = 0
    for cnt in n:
        if cnt:
            ok[first + int(np.argmax(area[first:first + cnt]))] = True      # argmax: the first of equals
        first += int(cnt)
    table, _ = renumber(ok, n)
    out = relabel_device(labels_t, n, table) > 0
    out = out[0] if len(s) == 2 else out
    return out if D.is_tensor(mask) else out.cpu().numpy()
