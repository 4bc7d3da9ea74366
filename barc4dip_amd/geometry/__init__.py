from __future__ import annotations

from . import labels, masks, roi
from .labels import label_regions, largest_region, select_regions
from .masks import pad_to_square
from .roi import embed_roi, odd_size, roi_grid_3x3, roi_slices

__all__ = ["masks", "roi", "pad_to_square", "embed_roi", "odd_size", "roi_grid_3x3", "roi_slices", "labels", "label_regions",
           "select_regions", "largest_region"]
