"""NumPy model of barc4dip_amd.preprocessing.enhancement, written from the rule in include/b4d.h -- not a port
of any implementation.  Where the rule says float32 every operation is one np.float32 operation; counts are integer arrays.

Deviations of the library from the plain statement of the rule, repeated here as the header states them:
  * the quantiser clamps the floored float32 product before it becomes an integer (+-Inf take the end bins, a NaN product bin 0);
  * a clip level at or above n is n (nothing exceeds it), so that a huge clip_limit needs no wide integer;
  * float input without a given value_range takes each frame's nanmin / nanmax; a frame whose bounds are not finite, or equal,
    comes back unchanged (so does a frame that holds an infinite pixel).

clahe() and equalize_hist() return (result, branches): the set of branch names the call reached, from
  "excess0" "excess+"  "batch0" "batch+"  "residual0" "step1" "step>1"  "pad_only_tile" "empty_tile".
"""
from __future__ import annotations

import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- quantiser
def frame_range(frame):
    """(lo, hi) float32 of a float frame by default: its minimum and maximum over the pixels that are not NaN (NaN if none)."""
    a = np.asarray(frame, dtype=F)
    ok = ~np.isnan(a)
    return (F(a[ok].min()), F(a[ok].max())) if ok.any() else (F(np.nan), F(np.nan))


def usable(lo, hi) -> bool:
    return bool(np.isfinite(lo) and np.isfinite(hi) and lo < hi)


def quantiser(lo, hi, L):
    """(s, inv) float32 for float32 bounds: the difference in float64, one rounding each."""
    span = np.float64(F(hi)) - np.float64(F(lo))
    return F(np.float64(L) / span), F(span / np.float64(L - 1))


def bins(frame, lo, s, L):
    """Bin of every pixel (int64), -1 for NaN."""
    a = np.asarray(frame, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((a - F(lo)) * F(s))          # two float32 operations
    b = np.where(f > 0, np.minimum(f, F(L - 1)), F(0)).astype(np.int64)     # clamp as float, then convert; NaN product -> 0
    return np.where(np.isnan(a), -1, b)


# ---------------------------------------------------------------------------------------------------------------- tiles
def geometry(ny, nx, grid):
    """(tx, ty, th, tw, pad_y, pad_x) for grid = (tiles along x, tiles along y)."""
    tx, ty = int(grid[0]), int(grid[1])
    pad_y, pad_x = (ty - ny % ty) % ty, (tx - nx % tx) % tx
    assert pad_y <= ny - 1 and pad_x <= nx - 1
    return tx, ty, (ny + pad_y) // ty, (nx + pad_x) // tx, pad_y, pad_x


def extend(a, pad_y, pad_x):
    """a extended at the bottom and the right by reflection without repeating the edge: row y >= H is row 2 (H - 1) - y."""
    ny, nx = a.shape
    ys = np.arange(ny + pad_y)
    xs = np.arange(nx + pad_x)
    ys = np.where(ys < ny, ys, 2 * (ny - 1) - ys)
    xs = np.where(xs < nx, xs, 2 * (nx - 1) - xs)
    return a[np.ix_(ys, xs)]


def tile_counts(binned, grid, L):
    """counts (ty, tx, L) int64 and n_valid (ty, tx) int64 of a binned frame (-1: no bin), reflected padding counted; plus the set
    {"pad_only_tile"} if a tile lies wholly in the padding."""
    ny, nx = binned.shape
    tx, ty, th, tw, pad_y, pad_x = geometry(ny, nx, grid)
    ext = extend(binned, pad_y, pad_x)
    counts = np.zeros((ty, tx, L), dtype=np.int64)
    n_valid = np.zeros((ty, tx), dtype=np.int64)
    seen = set()
    for j in range(ty):
        for i in range(tx):
            t = ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel()
            t = t[t >= 0]
            counts[j, i] = np.bincount(t, minlength=L)
            n_valid[j, i] = t.size
            if j * th >= ny or i * tw >= nx:
                seen.add("pad_only_tile")
    return counts, n_valid, seen


# ---------------------------------------------------------------------------------------------------------------- tables
def clahe_table(h, n, L, clip_limit, seen):
    """The CLAHE table (int64, L entries) of one tile's counts h with n valid pixels; adds the branches reached to `seen`."""
    if n == 0:
        seen.add("empty_tile")
        return np.arange(L, dtype=np.int64)
    h = h.astype(np.int64).copy()
    if clip_limit != 0:
        c = np.float64(clip_limit) * np.float64(n) / np.float64(L)
        clip = int(n) if c >= n else max(int(c), 1)
        excess = int(np.maximum(h - clip, 0).sum())
        h = np.minimum(h, clip)
        batch, residual = excess // L, excess % L
        seen.add("excess+" if excess else "excess0")
        seen.add("batch+" if batch else "batch0")
        h += batch
        if residual > 0:
            step = max(L // residual, 1)
            seen.add("step1" if step == 1 else "step>1")
            h[np.arange(residual) * step] += 1
        else:
            seen.add("residual0")
    assert h.sum() == n
    scale = F(L - 1) / F(n)
    return np.clip(np.rint(np.cumsum(h).astype(F) * scale), 0, L - 1).astype(np.int64)


def equalize_table(h, n, L):
    """(table, unchanged) by the equalize_hist rule."""
    if n == 0:
        return np.arange(L, dtype=np.int64), True
    i0 = int(np.flatnonzero(h)[0])
    if h[i0] == n:
        return np.arange(L, dtype=np.int64), True
    scale = F(L - 1) / F(n - h[i0])
    g = h.astype(np.int64).copy()
    g[:i0 + 1] = 0
    return np.clip(np.rint(np.cumsum(g).astype(F) * scale), 0, L - 1).astype(np.int64), False


# ---------------------------------------------------------------------------------------------------------------- interpolation
def axis_terms(n, tile, tiles):
    """(t0, t1, a, a1) of the pixels 0 .. n - 1 along an axis with `tiles` tiles of `tile` pixels."""
    inv = F(1.0) / F(tile)
    f = np.arange(n).astype(F) * inv - F(0.5)
    fl = np.floor(f)
    t = fl.astype(np.int64)
    a = f - fl
    return np.maximum(t, 0), np.minimum(t + 1, tiles - 1), a.astype(F), (F(1.0) - a).astype(F)


def interpolate(binned, tables, th, tw):
    """res (float32) of every pixel with a bin from tables (ty, tx, L); pixels without a bin give 0."""
    ny, nx = binned.shape
    ty, tx, _ = tables.shape
    r0, r1, ya, ya1 = axis_terms(ny, th, ty)
    c0, c1, xa, xa1 = axis_terms(nx, tw, tx)
    b = np.maximum(binned, 0)
    R0, R1, YA, YA1 = r0[:, None], r1[:, None], ya[:, None], ya1[:, None]
    C0, C1, XA, XA1 = c0[None, :], c1[None, :], xa[None, :], xa1[None, :]
    v11, v12 = tables[R0, C0, b].astype(F), tables[R0, C1, b].astype(F)
    v21, v22 = tables[R1, C0, b].astype(F), tables[R1, C1, b].astype(F)
    up = v11 * XA1 + v12 * XA          # every product and sum one float32 operation
    dn = v21 * XA1 + v22 * XA
    return (up * YA1 + dn * YA).astype(F)


# ---------------------------------------------------------------------------------------------------------------- public
def _setup(frame, levels, value_range):
    """(float32 frame, integer dtype or None, L, lo, hi) of one frame."""
    frame = np.asarray(frame)
    if frame.dtype in (np.uint8, np.uint16):
        L = 256 if frame.dtype == np.uint8 else 65536
        if levels is not None:      # the hand example: whole-number pixels at another depth
            L = levels
        return frame.astype(F), frame.dtype, L, F(0), F(L)
    a = frame.astype(F)
    lo, hi = frame_range(a) if value_range is None else (F(value_range[0]), F(value_range[1]))
    return a, None, (65536 if levels is None else levels), lo, hi


def _epilogue(a, binned, res, int_dtype, L, lo, inv):
    if int_dtype is not None:
        return np.clip(np.rint(res), 0, L - 1).astype(int_dtype)
    out = (res * inv + lo).astype(F)
    return np.where(binned < 0, a, out)


def frame_histogram(frame, grid=(1, 1), *, levels=None, value_range=None):
    """(counts (ty, tx, L), n_valid (ty, tx), branches) of one frame."""
    a, int_dtype, L, lo, hi = _setup(frame, levels, value_range)
    s = F(1) if int_dtype is not None else (quantiser(lo, hi, L)[0] if usable(lo, hi) else F(0))
    return tile_counts(bins(a, lo, s, L), grid, L)


def clahe(frame, clip_limit=2.0, grid=(8, 8), *, levels=None, value_range=None):
    """(result, branches) of one frame (H, W): uint8 / uint16 in their dtype, anything else float32."""
    a, int_dtype, L, lo, hi = _setup(frame, levels, value_range)
    if int_dtype is None and not usable(lo, hi):
        return a, set()
    s, inv = (F(1), F(1)) if int_dtype is not None else quantiser(lo, hi, L)
    binned = bins(a, lo, s, L)
    counts, n_valid, seen = tile_counts(binned, grid, L)
    tx, ty, th, tw, _, _ = geometry(a.shape[0], a.shape[1], grid)
    tables = np.stack([np.stack([clahe_table(counts[j, i], n_valid[j, i], L, clip_limit, seen) for i in range(tx)]) for j in range(ty)])
    assert np.all(np.diff(tables, axis=-1) >= 0) and tables.min() >= 0 and tables.max() <= L - 1
    return _epilogue(a, binned, interpolate(binned, tables, th, tw), int_dtype, L, lo, inv), seen


def equalize_hist(frame, *, levels=None, value_range=None):
    """(result, unchanged) of one frame."""
    a, int_dtype, L, lo, hi = _setup(frame, levels, value_range)
    same = frame.copy() if int_dtype is not None else a
    if int_dtype is None and not usable(lo, hi):
        return same, True
    s, inv = (F(1), F(1)) if int_dtype is not None else quantiser(lo, hi, L)
    binned = bins(a, lo, s, L)
    counts, n_valid, _ = tile_counts(binned, (1, 1), L)
    table, unchanged = equalize_table(counts[0, 0], n_valid[0, 0], L)
    if unchanged:
        return same, True
    res = table[np.maximum(binned, 0)].astype(F)          # lut[bin] directly, not through the four-table formula
    return _epilogue(a, binned, res, int_dtype, L, lo, inv), False


# ---------------------------------------------------------------------------------------------------------------- the GPU cases
def case_data():
    """The inputs of tests/test_gpu_enhancement.py, from one generator (seed 29), by name."""
    rng = np.random.default_rng(29)
    d = {}
    d["u8"] = np.minimum(rng.poisson(40, (3, 70, 150)), 255).astype(np.uint8)
    d["u8_exact"] = np.ascontiguousarray(d["u8"][:, :64, :96])
    d["u8_tiny"] = rng.integers(0, 256, (2, 9, 13)).astype(np.uint8)
    d["u16"] = rng.poisson(40000, (1, 70, 150)).astype(np.uint16)
    d["u16_dense"] = rng.poisson(30, (1, 256, 256)).astype(np.uint16)
    d["u8_const"] = np.full((1, 16, 16), 7, dtype=np.uint8)
    f = rng.normal(0.5, 0.1, (2, 70, 150)).astype(np.float32)
    f[:, :30, :45] = np.nan          # all of tile (0, 0) (24 x 38 under grid (4, 3)) and part of its neighbours
    d["f32"] = f
    flat = np.full((2, 32, 48), 3.25, dtype=np.float32)
    flat[1] = np.nan
    d["f32_flat"] = flat
    return d


# name -> (data key, keyword arguments of clahe, branches the call must reach)
CLAHE_CASES = {
    "u8_clip2": ("u8", dict(clip_limit=2.0, tile_grid_size=(4, 3)), {"excess+", "batch+", "step1"}),
    "u8_clip40": ("u8", dict(clip_limit=40.0, tile_grid_size=(4, 3)), {"excess0", "batch0", "residual0"}),
    "u8_clip001": ("u8", dict(clip_limit=0.01, tile_grid_size=(4, 3)), {"excess+", "batch+", "step>1"}),
    "u8_noclip": ("u8", dict(clip_limit=0, tile_grid_size=(4, 3)), set()),
    "u8_exact": ("u8_exact", dict(clip_limit=2.0, tile_grid_size=(8, 8)), {"excess+"}),
    "u8_tiny": ("u8_tiny", dict(clip_limit=2.0, tile_grid_size=(8, 8)), {"pad_only_tile"}),
    "u16_slices": ("u16", dict(clip_limit=2.0, tile_grid_size=(4, 3)), {"excess+", "batch0"}),
    "u16_dense_clip1": ("u16_dense", dict(clip_limit=1.0, tile_grid_size=(1, 1)), {"excess+", "step1"}),
    "u16_dense_clip100": ("u16_dense", dict(clip_limit=100.0, tile_grid_size=(1, 1)), {"excess+"}),
    "u8_const": ("u8_const", dict(clip_limit=2.0, tile_grid_size=(2, 2)), {"excess+"}),
    "f32_auto": ("f32", dict(clip_limit=2.0, tile_grid_size=(4, 3), levels=1024), {"empty_tile", "excess+"}),
    "f32_range": ("f32", dict(clip_limit=2.0, tile_grid_size=(4, 3), levels=1024, value_range=(0.2, 0.8)), {"empty_tile", "excess+"}),
    "f32_flat": ("f32_flat", dict(), set()),
}


def clahe_stack(stack, clip_limit=2.0, tile_grid_size=(8, 8), *, levels=None, value_range=None):
    """(results (T, H, W), union of the branches) of a stack, frame by frame."""
    outs, seen = [], set()
    for fr in stack:
        o, s = clahe(fr, clip_limit, tile_grid_size, levels=levels, value_range=value_range)
        outs.append(o)
        seen |= s
    return np.stack(outs), seen


def equalize_stack(stack, *, levels=None, value_range=None):
    res = [equalize_hist(fr, levels=levels, value_range=value_range) for fr in stack]
    return np.stack([r[0] for r in res]), [r[1] for r in res]
