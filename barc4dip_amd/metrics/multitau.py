"""Multi-tau correlation of long and streamed stacks of speckle frames: g2 at quasi-logarithmic delays in one pass.

``multi_tau_correlation`` gives, per region of a label map, the intensity correlation g2(tau) at the delays of a multi-tau
correlator: level 0 is the stack itself, every further level the pairwise average of the one below, and each level contributes
``lags_per_level`` (level 0) or half as many (above) delays.  The definitions are those of ``include/b4d.h`` (b4d_multi_tau_*);
the state per pixel is fixed, so the stack may be of any length and may be streamed from a memory-mapped file (DESIGN.md
section 21).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from ._regions import MAX_REGIONS, region_map, stack_shape

LAGS_PER_LEVEL = (8, 16, 32)
MAX_LEVELS = 24


def lag_table(T: int, lags_per_level: int = 16, max_level: int | None = None):
    """(lags, level, n_pairs, n_levels) of a stack of T frames: int64 arrays of the delays in frames, their levels and the
    number T_l - j of frame pairs behind each, and the number of levels in use.  The table is b4d_multi_tau_lags' (host only)."""
    lib = _ffi.lib()
    cap = -1 if max_level is None else int(max_level)
    n = int(lib.b4d_multi_tau_lags(int(T), int(lags_per_level), cap, None, None, None, None))
    _ffi.check(min(n, 0))
    lags, level, pairs = np.empty(n, np.int64), np.empty(n, np.int32), np.empty(n, np.int64)
    nl = C.c_int(0)
    lib.b4d_multi_tau_lags(int(T), int(lags_per_level), cap, lags.ctypes.data_as(C.c_void_p), level.ctypes.data_as(C.c_void_p),
                           pairs.ctypes.data_as(C.c_void_p), C.c_void_p(C.addressof(nl)))
    return lags, level.astype(np.int64), pairs, int(nl.value)


def _is_streamed(images) -> bool:
    """Memory-mapped arrays and other sliceable host sources (h5py datasets) are streamed; tensors and plain arrays are resident."""
    if D.is_tensor(images):
        return False
    if isinstance(images, np.memmap):
        return True
    return not isinstance(images, (np.ndarray, list, tuple)) and all(hasattr(images, a) for a in ("shape", "dtype", "__getitem__"))


def _check(images, labels, mask, lags_per_level, max_level, chunk_frames):
    """Every argument error, before the GPU is touched.  Returns (images, streamed, dtype kind, T, H, W, int32 label map or None,
    R, m, max_level or None)."""
    streamed = _is_streamed(images)
    if D.is_tensor(images):
        shape, kind = tuple(int(s) for s in images.shape), ("c" if images.is_complex() else "f" if images.is_floating_point() else "i")
    else:
        if not streamed:
            images = np.asarray(images)
        shape, kind = tuple(int(s) for s in images.shape), np.dtype(images.dtype).kind
    T, H, W = stack_shape(shape, kind == "c", "multi_tau_correlation")
    if isinstance(lags_per_level, bool) or lags_per_level not in LAGS_PER_LEVEL:
        raise ValueError(f"lags_per_level must be one of {LAGS_PER_LEVEL}, got {lags_per_level!r}")
    if max_level is not None and (isinstance(max_level, bool) or int(max_level) != max_level or int(max_level) < 0):
        raise ValueError(f"max_level must be an integer >= 0 or None, got {max_level!r}")
    if isinstance(chunk_frames, bool) or int(chunk_frames) != chunk_frames or int(chunk_frames) < 1:
        raise ValueError(f"chunk_frames must be an integer >= 1, got {chunk_frames!r}")
    lab, R = region_map(labels, mask, H, W)
    if R > MAX_REGIONS or H * W >= 2 ** 31 or T >= 2 ** 31:
        raise NotImplementedError(f"multi_tau_correlation: at most {MAX_REGIONS} regions, fewer than 2^31 pixels per frame and fewer "
                                  f"than 2^31 frames (got T = {T}, R = {R}, {H} x {W})")
    return images, streamed, kind, T, H, W, lab, R, int(lags_per_level), (None if max_level is None else int(max_level))


def multi_tau_correlation(images, labels=None, mask=None, lags_per_level: int = 16, max_level: int | None = None,
                          chunk_frames: int = 256, return_tensors: bool = False) -> dict:
    """Multi-tau intensity correlation g2(tau) of a stack of frames of any length, in one pass and with a fixed state per pixel.

    images: (T, H, W), T >= 2: a ROCm tensor or a NumPy array (taken to the device whole and cut there into pieces of
            ``chunk_frames``), or a sliceable host source that ``ingest.iter_device_chunks`` accepts -- a memory-mapped .npy file,
            an h5py dataset -- which is streamed through two pinned buffers in pieces of ``chunk_frames``.  Both ways issue the
            same sequence of pushes, so the same ``chunk_frames`` gives the same bits.
    labels: (H, W) integer map, 0 = pixel not used, 1 .. R = regions (R = its largest value, at most 64).
    mask:   (H, W) bool map of the one region; with neither, all pixels form it.  A pixel that is NaN or +-Inf in any frame takes
            no part.  Float sources are scanned for such pixels before the first frame is correlated: a STREAMED FLOAT SOURCE IS
            THEREFORE READ TWICE.  Integer sources skip the scan.
    lags_per_level: m, one of 8, 16, 32.  Level 0 (the frames themselves) gives the delays 0 .. m - 1; level l >= 1 (frames
            averaged pairwise l times, in float32) gives j 2^l for j = m/2 .. m - 1, while it has at least m/2 + 1 frames.
    max_level: the last level used (default: all that T fills; more than 24 levels are not supported).

    Returns a dict; with ``labels`` the float arrays have a leading R axis, otherwise not:
      ``lags``, ``level``, ``n_pairs`` (n_lags,) int64: the delay in frames, its level l, and n = T_l - j frame pairs behind it;
      ``g2`` (n_lags,) float64 = <I(t) I(t + tau)> / (<I(t)> <I(t + tau)>) over the region's pixels and the n pairs, each mean
            over exactly the frames that enter the product (the symmetric normalisation);
      ``g2_err`` (n_lags,) float64: the standard error of the mean product over pixels and pairs as if the products were
            independent, over the same denominator.  Neighbouring frames and pixels are correlated, so this is a LOWER BOUND
            on the real error;
      ``mean`` float64: the region's mean over all T frames; ``n_pixels`` int64;
      ``meta`` {lags_per_level, n_levels, n_regions, n_frames, chunk_frames}.
    A quotient whose denominator is not above 0 is NaN (an all-zero region); a region without pixels is NaN with n_pixels 0.
    The same bits from run to run, and for a region alone under ``mask`` as among others under ``labels``.  Arrays are NumPy
    unless ``return_tensors``.  Argument errors are raised before the GPU is touched; size limits are NotImplementedError."""
    images, streamed, kind, T, H, W, lab, R, m, cap = _check(images, labels, mask, lags_per_level, max_level, chunk_frames)
    lags, level, pairs, L = lag_table(T, m, cap)
    torch = _ffi.require_gpu()
    lib, st = _ffi.lib(), _ffi.stream_ptr()
    npix, chunk = H * W, max(1, min(int(chunk_frames), T))
    dev = torch.device("cuda", torch.cuda.current_device())
    nbytes = int(lib.b4d_multi_tau_workspace_bytes(npix, R, m, L, chunk))
    if nbytes == 0:
        raise NotImplementedError(f"multi_tau_correlation: no native path for {H} x {W}, {R} regions, {L} levels")

    if streamed:
        from ..ingest import iter_device_chunks

        chunks = lambda: iter_device_chunks(images, chunk)  # noqa: E731
    else:
        x = D.to_device_f32(images, ndim=(3,))[0]
        chunks = lambda: (x[a:a + chunk] for a in range(0, T, chunk))  # noqa: E731

    bad = None
    if kind == "f":
        bad = torch.zeros(npix, dtype=torch.uint8, device=dev)
        for part in chunks():
            _ffi.check(lib.b4d_multi_tau_scan(D.ptr(part), int(part.shape[0]), npix, D.ptr(bad), st))
    lab_dev = torch.from_numpy(lab.reshape(-1)).to(dev) if lab is not None else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _ffi.check(lib.b4d_multi_tau_init(D.ptr(lab_dev) if lab_dev is not None else None, D.ptr(bad) if bad is not None else None,
                                      npix, R, m, L, chunk, D.ptr(ws), st))
    t0 = 0
    for part in chunks():
        n = int(part.shape[0])
        _ffi.check(lib.b4d_multi_tau_push(D.ptr(part), t0, n, npix, R, m, L, chunk, D.ptr(ws), st))
        t0 += n
    assert t0 == T
    n_lags = len(lags)
    g2 = torch.empty((R, n_lags), dtype=torch.float64, device=dev)
    g2e = torch.empty((R, n_lags), dtype=torch.float64, device=dev)
    mean = torch.empty((R,), dtype=torch.float64, device=dev)
    npx = torch.empty((R,), dtype=torch.int64, device=dev)
    _ffi.check(lib.b4d_multi_tau_finish(T, npix, R, m, L, chunk, D.ptr(ws), D.ptr(g2), D.ptr(g2e), D.ptr(mean), D.ptr(npx), st))
    out = {"g2": g2, "g2_err": g2e, "mean": mean, "n_pixels": npx}
    if labels is None:
        out = {k: v[0] for k, v in out.items()}
    if return_tensors:
        out.update({"lags": torch.from_numpy(lags).to(dev), "level": torch.from_numpy(level).to(dev),
                    "n_pairs": torch.from_numpy(pairs).to(dev)})
    else:
        out = {k: v.cpu().numpy() for k, v in out.items()}
        out.update({"lags": lags, "level": level, "n_pairs": pairs})
    out["meta"] = {"lags_per_level": m, "n_levels": L, "n_regions": R, "n_frames": T, "chunk_frames": chunk}
    return out
