"""What the filters over a frame ``(H, W)`` or a stack ``(T, H, W)`` share on the Python side (preprocessing/rank.py, smooth.py,
distortion.py, metrics/contrast.py, utils/range.py, dtype.py): the border-mode codes of csrc/b4d_tile.hpp, the frames as a float32
device tensor, and scalar-or-pair arguments.  Argument errors come before the device is asked for."""
from __future__ import annotations

import numpy as np

from . import _device as D

# scipy.ndimage's border modes -> MODE_* of csrc/b4d_tile.hpp
MODES = {"nearest": 0, "reflect": 1, "mirror": 2, "constant": 3, "grid-constant": 3, "wrap": 4, "grid-wrap": 4}


def mode_code(mode) -> int:
    """The code of border mode `mode`."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"Invalid mode: {mode!r} (expected one of {sorted(MODES)})")
    return MODES[mode]


def frame_stack(images):
    """float32 device tensor of `images` ((H, W) or (T, H, W), no empty side) and its (batch, ny, nx)."""
    shape = tuple(images.shape) if hasattr(images, "shape") else np.shape(images)
    if len(shape) not in (2, 3):
        raise ValueError(f"images must be (H, W) or (T, H, W); got shape {shape}")
    if 0 in shape:
        raise ValueError(f"images must not be empty; got shape {shape}")
    t, _, _ = D.to_device_f32(images, ndim=(2, 3))
    return t, (int(shape[0]) if len(shape) == 3 else 1), int(shape[-2]), int(shape[-1])


def pair(value, name, kind=float):
    """(y, x) of a scalar or a pair; kind=int takes whole numbers only."""
    try:
        y, x = (value, value) if np.ndim(value) == 0 else value
        if kind is int and (int(y) != y or int(x) != x):
            raise TypeError
        return kind(y), kind(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a scalar or a pair (y, x); got {value!r}") from None


def window(size, max_size: int) -> tuple[int, int]:
    """(size_y, size_x) of an int or a pair, each in 1 .. max_size."""
    try:
        sy, sx = pair(size, "size", int)
    except ValueError:
        raise ValueError(f"size must be an int or a pair (size_y, size_x) of ints; got {size!r}") from None
    if not (1 <= sy <= max_size and 1 <= sx <= max_size):
        raise ValueError(f"window sizes must be in 1 .. {max_size}; got {(sy, sx)}")
    return sy, sx
