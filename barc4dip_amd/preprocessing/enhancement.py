"""GPU drop-in for ``barc4dip.preprocessing.enhancement`` (csrc/b4d_enhance.hip): contrast-limited adaptive
histogram equalisation (CLAHE) by the rule of OpenCV's CPU implementation, and global histogram equalisation by the rule of
``cv2.equalizeHist``, on ``uint8`` / ``uint16`` frames and -- which OpenCV cannot take -- on float32 frames at 2 .. 65536 levels.

Frames ``(H, W)`` or stacks ``(T, H, W)``, NumPy arrays or device tensors.  ``uint8`` gives 256 levels and a ``uint8`` result,
``uint16`` 65536 levels and a ``uint16`` result; every other dtype is taken as float32 and quantised to ``levels`` bins over
``value_range`` (default: each frame's own minimum and maximum), the result being float32 in that range.  NaN pixels take no part
in any histogram and stay NaN.  Nothing in the computation is a float reduction: the result is specified to the bit
(include/b4d.h) and a frame gives the same bits alone and inside any batch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import MODES, frame_stack
from . import rank as R

MAX_LEVELS = 65536
MAX_TILES = 4096
MAX_TILE_AREA = 1 << 24
WORKSPACE_BYTES = 256 << 20      # counts and tables of one chunk of frames
MAX_CHUNK = 65535                # frames per call of the C entry points
_NULL = C.c_void_p(0)


# ------------------------------------------------------------------------------------------------- arguments (no device)
def _shape(a) -> tuple:
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _integer_levels(image):
    """(levels, NumPy dtype) of uint8 / uint16 input, (None, None) for anything else."""
    name = str(getattr(image, "dtype", "")).replace("torch.", "")
    return {"uint8": (256, np.uint8), "uint16": (65536, np.uint16)}.get(name, (None, None))


def tile_geometry(ny: int, nx: int, tile_grid_size) -> tuple[int, int, int, int]:
    """(tiles_x, tiles_y, tile height, tile width) of a frame under ``tile_grid_size = (tiles along x, tiles along y)``; an axis
    that its tile count does not divide is extended by reflected pixels to the next multiple.  ValueError outside the limits."""
    try:
        tx, ty = tile_grid_size
        if int(tx) != tx or int(ty) != ty:
            raise TypeError
        tx, ty = int(tx), int(ty)
    except (TypeError, ValueError):
        raise ValueError(f"tile_grid_size must be a pair of ints (tiles along x, tiles along y); got {tile_grid_size!r}") from None
    if tx < 1 or ty < 1:
        raise ValueError(f"tile_grid_size needs at least one tile per axis; got {(tx, ty)}")
    if tx * ty > MAX_TILES:
        raise ValueError(f"at most {MAX_TILES} tiles; got {tx} x {ty}")
    sides = []
    for side, tiles, name in ((ny, ty, "rows"), (nx, tx, "columns")):
        pad = (tiles - side % tiles) % tiles
        if pad > side - 1:
            raise ValueError(f"{tiles} tiles over {side} {name} would extend the frame by {pad} reflected {name}, more than the "
                             f"{side - 1} it can give")
        sides.append((side + pad) // tiles)
    if sides[0] * sides[1] > MAX_TILE_AREA:
        raise ValueError(f"a tile of {sides[0]} x {sides[1]} pixels exceeds {MAX_TILE_AREA}; use more tiles")
    return tx, ty, sides[0], sides[1]


class _Spec:
    """What a call fixes before the device is asked for: shape, levels, integer dtype (or None) and the given value range."""

    def __init__(self, image, levels, value_range, tile_grid_size):
        shape = _shape(image)
        if len(shape) not in (2, 3):
            raise ValueError(f"images must be (H, W) or (T, H, W); got shape {shape}")
        if 0 in shape:
            raise ValueError(f"images must not be empty; got shape {shape}")
        self.squeeze = len(shape) == 2
        self.batch, self.ny, self.nx = (1 if self.squeeze else int(shape[0])), int(shape[-2]), int(shape[-1])
        if self.ny * self.nx >= 1 << 31:
            raise ValueError(f"frames of {self.ny} x {self.nx} pixels are beyond 2^31")
        self.tx, self.ty, self.th, self.tw = tile_geometry(self.ny, self.nx, tile_grid_size)
        implied, self.int_dtype = _integer_levels(image)
        if implied is not None:
            if levels not in (None, implied) or value_range is not None:
                raise ValueError(f"{np.dtype(self.int_dtype).name} input has {implied} levels over [0, {implied}); levels and value_range "
                                 "are for float input")
            self.levels, self.range = implied, None
            return
        self.levels = MAX_LEVELS if levels is None else levels
        if isinstance(self.levels, bool) or int(self.levels) != self.levels or not 2 <= self.levels <= MAX_LEVELS:
            raise ValueError(f"levels must be an int in 2 .. {MAX_LEVELS}; got {levels!r}")
        self.levels = int(self.levels)
        self.range = None
        if value_range is not None:
            try:
                lo, hi = (np.float32(v) for v in value_range)
            except (TypeError, ValueError):
                raise ValueError(f"value_range must be a pair (lo, hi); got {value_range!r}") from None
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise ValueError(f"value_range must be finite with lo <= hi; got {value_range!r}")
            self.range = (lo, hi)


def _check_clip(clip_limit) -> float:
    c = float(clip_limit)
    if not c >= 0.0:
        raise ValueError(f"clip_limit must be >= 0 (0: no clipping); got {clip_limit!r}")
    return c


def quantiser(lo, hi, levels: int) -> np.ndarray:
    """The (n, 4) float32 rows {lo, s, inv, 0} of b4d.h for float32 bounds lo, hi: s = float32(L / (hi - lo)) and
    inv = float32((hi - lo) / (L - 1)) with the difference in float64; s = 0 (frame left unchanged) where the bounds are not
    finite or not lo < hi."""
    lo = np.atleast_1d(np.asarray(lo, dtype=np.float32))
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float32))
    q = np.zeros((lo.size, 4), dtype=np.float32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(lo) & np.isfinite(hi) & (lo < hi)
        span = np.where(ok, hi.astype(np.float64) - lo.astype(np.float64), 1.0)
        q[:, 0] = np.where(ok, lo, 0.0)
        q[:, 1] = np.where(ok, (levels / span).astype(np.float32), 0.0)
        q[:, 2] = np.where(ok, (span / (levels - 1)).astype(np.float32), 0.0)
    return q


# ------------------------------------------------------------------------------------------------- device calls
def _qparams(spec: _Spec, t):
    """(batch, 4) float32 device tensor of quantiser rows and the host arrays (lo, hi) of every frame."""
    torch = _ffi.require_gpu()
    if spec.int_dtype is not None:
        lo = np.zeros(spec.batch, dtype=np.float32)
        hi = np.full(spec.batch, spec.levels, dtype=np.float32)
        q = np.tile(np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32), (spec.batch, 1))
    else:
        if spec.range is not None:
            lo = np.full(spec.batch, spec.range[0], dtype=np.float32)
            hi = np.full(spec.batch, spec.range[1], dtype=np.float32)
        else:   # each frame's own bounds: the range-only 1 x 1 rank filter (integer min / max on ordered keys, NaN skipped)
            _, mm = R.run_rank_filter(t, spec.batch, spec.ny, spec.nx, 1, 1, 0, MODES["reflect"], 0.0, want_out=False, want_range=True)
            mm = mm.cpu().numpy()
            lo, hi = mm[:, 0].copy(), mm[:, 1].copy()
        q = quantiser(lo, hi, spec.levels)
    return torch.from_numpy(q).to(t.device), lo, hi


def _chunk_frames(spec: _Spec, tables: bool) -> int:
    per_frame = spec.tx * spec.ty * (spec.levels * (6 if tables else 4) + 4)
    return max(1, min(spec.batch, MAX_CHUNK, WORKSPACE_BYTES // per_frame))


def run_tile_histogram(t, q, batch, spec: _Spec, tx, ty, counts, n_valid):
    _ffi.check(_ffi.lib().b4d_tile_histogram(D.ptr(t), batch, spec.ny, spec.nx, tx, ty, spec.levels, D.ptr(q), D.ptr(counts), D.ptr(n_valid),
                                             _ffi.stream_ptr()))


def _equalise(image, spec: _Spec, clip_limit: float, mode: int, return_tensors: bool):
    torch = _ffi.require_gpu()
    t, _, _, _ = frame_stack(image)
    t = t.reshape(spec.batch, spec.ny, spec.nx)
    q, _, _ = _qparams(spec, t)
    tx, ty = (spec.tx, spec.ty) if mode == 0 else (1, 1)
    tiles, L = tx * ty, spec.levels
    chunk = _chunk_frames(spec, True) if mode == 0 else max(1, min(spec.batch, MAX_CHUNK, WORKSPACE_BYTES // (6 * L + 8)))
    dev = t.device
    counts = torch.empty((chunk, tiles, L), dtype=torch.int32, device=dev)
    n_valid = torch.empty((chunk, tiles), dtype=torch.int32, device=dev)
    lut = torch.empty((chunk, tiles, L), dtype=torch.int16, device=dev)
    unchanged = torch.empty((chunk,), dtype=torch.int32, device=dev) if mode == 1 else None
    out = torch.empty_like(t)
    flags = (0 if spec.int_dtype is not None else 1) | (2 if mode == 1 else 0)
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    for a in range(0, spec.batch, chunk):
        n = min(chunk, spec.batch - a)
        run_tile_histogram(t[a:a + n], q[a:a + n], n, spec, tx, ty, counts, n_valid)
        _ffi.check(lib.b4d_equalize_lut(D.ptr(counts), D.ptr(n_valid), n, tiles, L, float(clip_limit), mode, D.ptr(lut),
                                        D.ptr(unchanged) if mode == 1 else _NULL, st))
        _ffi.check(lib.b4d_lut_apply(D.ptr(t[a:a + n]), n, spec.ny, spec.nx, tx, ty, L, D.ptr(q[a:a + n]), D.ptr(lut),
                                     D.ptr(unchanged) if mode == 1 else _NULL, flags, D.ptr(out[a:a + n]), st))
    if spec.squeeze:
        out = out[0]
    if return_tensors:
        return out
    return D.to_host(out) if spec.int_dtype is None else D.to_host(out).astype(spec.int_dtype)


# ------------------------------------------------------------------------------------------------- public
def clahe(image, clip_limit: float = 2.0, tile_grid_size=(8, 8), *, levels=None, value_range=None, return_tensors: bool = False):
    """Contrast-limited adaptive histogram equalisation of every frame, by the rule of ``cv2.createCLAHE(clip_limit,
    tile_grid_size).apply``: a histogram per tile, clipped at ``clip_limit`` times the mean bin count with the excess spread over
    all bins, a table per tile, and every pixel interpolated between the tables of the four nearest tiles.

    ``tile_grid_size`` is OpenCV's ``(tiles along x, tiles along y)``; an axis that its tile count does not divide is extended by
    reflected pixels.  ``clip_limit=0`` does not clip.  Float input: ``levels`` bins (default 65536) over ``value_range=(lo, hi)``,
    by default each frame's own minimum and maximum; pixels outside take the end bins; a frame with ``lo == hi`` or without finite
    bounds (no pixel that is not NaN, or an infinite one) comes back unchanged.

    Returns the frames in the input's integer dtype, or float32; with ``return_tensors=True`` the float32 device tensor (whole-number
    levels for integer input)."""
    clip = _check_clip(clip_limit)
    spec = _Spec(image, levels, value_range, tile_grid_size)
    return _equalise(image, spec, clip, 0, return_tensors)


def equalize_hist(image, *, levels=None, value_range=None, return_tensors: bool = False):
    """Global histogram equalisation of every frame by the rule of ``cv2.equalizeHist`` at ``levels`` levels: the table is the
    cumulative histogram behind the first occupied bin, scaled to ``levels - 1``.  A frame whose valid pixels all fall into one bin
    comes back unchanged.  Arguments and returns as for ``clahe``."""
    spec = _Spec(image, levels, value_range, (1, 1))
    return _equalise(image, spec, 0.0, 1, return_tensors)


def frame_histogram(images, levels=None, value_range=None, *, tile_grid_size=(1, 1)) -> dict:
    """Histograms of every frame, or of every tile of ``tile_grid_size`` (tiles along x, tiles along y), with the quantiser and the
    tiles of ``clahe`` (reflected padding counted).  Returns ``{"counts": (T, ty, tx, L) int64, "n_valid": (T, ty, tx) int64,
    "lo": (T,) float32, "hi": (T,) float32}`` without the leading axis for a single frame.  For ``uint8`` / ``uint16`` frames and
    one tile, ``counts`` is ``np.bincount(frame.ravel(), minlength=L)``."""
    spec = _Spec(images, levels, value_range, tile_grid_size)
    torch = _ffi.require_gpu()
    t, _, _, _ = frame_stack(images)
    t = t.reshape(spec.batch, spec.ny, spec.nx)
    q, lo, hi = _qparams(spec, t)
    tiles, L = spec.tx * spec.ty, spec.levels
    chunk = _chunk_frames(spec, False)
    counts = torch.empty((chunk, tiles, L), dtype=torch.int32, device=t.device)
    n_valid = torch.empty((chunk, tiles), dtype=torch.int32, device=t.device)
    hc = np.empty((spec.batch, spec.ty, spec.tx, L), dtype=np.int64)
    hn = np.empty((spec.batch, spec.ty, spec.tx), dtype=np.int64)
    for a in range(0, spec.batch, chunk):
        n = min(chunk, spec.batch - a)
        run_tile_histogram(t[a:a + n], q[a:a + n], n, spec, spec.tx, spec.ty, counts, n_valid)
        hc[a:a + n] = counts[:n].cpu().numpy().reshape(n, spec.ty, spec.tx, L)
        hn[a:a + n] = n_valid[:n].cpu().numpy().reshape(n, spec.ty, spec.tx)
    out = {"counts": hc, "n_valid": hn, "lo": lo, "hi": hi}
    return {k: v[0] for k, v in out.items()} if spec.squeeze else out
