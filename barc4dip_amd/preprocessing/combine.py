"""Combine the frames of a stack into one frame, and reject zingers along the frame axis (csrc/b4d_torder.hip through
barc4dip_amd.metrics.order).

``combine_frames`` reduces darks, flats or a speckle stack ``(T, H, W)`` to a 2-D float32 frame -- by the per-pixel median, the
plain mean or the mean of the samples that survive an outlier test -- that ``flat_field_correction(flats=..., darks=...)`` takes as
it is.  ``remove_zingers`` applies the same test sample by sample and replaces a rejected sample by its pixel's median over T:
where the spatial ``remove_outliers`` cannot tell a zinger from a speckle grain, the other frames can.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from ..metrics import order
from .normalize import _reduce_stack

_COMBINE = ("median", "mean", "robust")


def combine_frames(stack, method: str = "median", **kw):
    """One (H, W) float32 frame from a stack (T, H, W).
      ``"median"``: ``metrics.temporal_median`` (keywords ``ignore_nan``, ``return_tensors``, ``max_bytes``);
      ``"mean"``  : NumPy's float32 mean along axis 0, as ``flat_field_correction`` reduces a stack itself (``return_tensors``);
      ``"robust"``: ``metrics.temporal_robust_mean`` (keywords ``threshold``, ``scale``, ``polarity``, ``min_scale``, ...)."""
    if method not in _COMBINE:
        raise ValueError(f"Invalid method: {method!r} (expected one of {list(_COMBINE)})")
    if method == "median":
        return order.temporal_median(stack, **kw)
    if method == "robust":
        if kw.get("return_info") or kw.get("return_mask"):
            raise ValueError("combine_frames returns one frame; call metrics.temporal_robust_mean for the info")
        return order.temporal_robust_mean(stack, **kw)
    return_tensors = bool(kw.pop("return_tensors", False))
    if kw:
        raise TypeError(f"combine_frames(method='mean') got unexpected keywords {sorted(kw)}")
    stack, _ = order._source(stack)
    out = _reduce_stack(stack if D.is_tensor(stack) else np.asarray(stack))
    return out if return_tensors else D.to_host(out)


def remove_zingers(stack, *, threshold: float = 5.0, scale: str = "mad", polarity: str = "hot", min_scale: float = 0.0,
                   return_mask: bool = False, return_tensors: bool = False, max_bytes: int = order.DEFAULT_MAX_BYTES):
    """The stack (T, H, W) as float32 with every sample that fails the outlier test of ``metrics.temporal_robust_mean`` (by
    default: hotter than 5 scaled MADs above its pixel's median over T; a non-finite sample always) replaced by that median.
    ``return_mask`` adds ``{"mask": (T, H, W) bool, "count": (T,) int64 replaced samples per frame}``."""
    kind, thr, floor_, pol = order._robust_args(threshold, scale, polarity, min_scale)
    stack, shape = order._source(stack)
    order.row_bands(shape, max_bytes)

    def fn(t):
        res = order.run_robust_mean(t, kind, thr, floor_, pol, want_mask=return_mask, want_cleaned=True)
        return res[5], res[4]

    cleaned, rej = order.over_bands(stack, shape, max_bytes, fn, return_tensors)
    if not return_mask:
        return cleaned
    if return_tensors:
        torch = _ffi.require_gpu()
        mask = rej.to(torch.bool)
        return cleaned, {"mask": mask, "count": mask.sum(dim=(1, 2))}
    mask = rej.astype(bool)
    return cleaned, {"mask": mask, "count": np.count_nonzero(mask, axis=(1, 2)).astype(np.int64)}
