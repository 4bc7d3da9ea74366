"""Argument checks shared by the metrics that work on the regions of a label map (twotime.py, multitau.py)."""
from __future__ import annotations

import numpy as np

from .. import _device as D

MAX_REGIONS = 64        # RG_MAX_R, csrc/b4d_regions.hpp


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if D.is_tensor(a) else np.asarray(a)


def stack_shape(shape, is_complex: bool, who: str):
    """(T, H, W) of a real, non-empty stack of at least two frames; ``who`` names the caller in the last message."""
    if is_complex:
        raise NotImplementedError("complex input is not supported by the HIP path (real frames only).")
    if len(shape) != 3 or 0 in shape:
        raise ValueError(f"images must be a non-empty (T, H, W) stack, got shape {tuple(shape)}")
    if shape[0] < 2:
        raise ValueError(f"{who} needs at least two frames")
    return tuple(shape)


def region_map(labels, mask, H: int, W: int):
    """``labels`` or ``mask`` checked against the frame shape.  Returns (host label map as contiguous int32 or None, R)."""
    if labels is not None and mask is not None:
        raise ValueError("pass labels or mask, not both")
    lab, R = None, 1
    if labels is not None:
        lab = _host(labels)
        if lab.shape != (H, W):
            raise ValueError(f"labels must have the frame shape {(H, W)}, got {lab.shape}")
        if lab.dtype.kind not in "iu":
            raise ValueError(f"labels must be an integer map, got dtype {lab.dtype}")
        if lab.min() < 0:
            raise ValueError("labels must not be negative (0 = not used, 1 .. R = regions)")
        R = int(lab.max())
        if R < 1:
            raise ValueError("labels names no region (all zero)")
    elif mask is not None:
        m = _host(mask)
        if m.shape != (H, W):
            raise ValueError(f"mask must have the frame shape {(H, W)}, got {m.shape}")
        if m.dtype.kind not in "biu":
            raise ValueError(f"mask must be a bool map, got dtype {m.dtype}")
        lab = m.astype(bool)
    return (None if lab is None else np.ascontiguousarray(lab, dtype=np.int32)), R
