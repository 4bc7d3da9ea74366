"""GPU drop-in for ``barc4dip.utils.range`` and ``barc4dip.utils.dtype``: display / scaling bounds and the uint16 conversion."""
from __future__ import annotations

from . import dtype, range  # noqa: A004 - the reference's module name
from .dtype import round_uint16_bounds, to_uint16
from .range import filtered_minmax_range, filtered_minmax_range_streaming, percentile_minmax_range

__all__ = ["dtype", "range", "filtered_minmax_range", "filtered_minmax_range_streaming", "percentile_minmax_range",
           "round_uint16_bounds", "to_uint16"]
