"""How close frames are to a reference frame, on the GPU (csrc/b4d_perceptual.hip): structural similarity
(SSIM, Wang et al. 2004, as ``skimage.metrics.structural_similarity`` forms it), multi-scale SSIM (Wang, Simoncelli & Bovik 2003)
and the error metrics MSE / RMSE / MAE / PSNR / NRMSE.

Pairing: a ``reference`` frame ``(H, W)`` goes with ``images`` ``(H, W)`` or with every frame of ``(T, H, W)``; a ``reference``
stack ``(T, H, W)`` goes with ``images`` ``(T, H, W)`` frame by frame.  Scores are float64 NumPy arrays of shape ``(T,)``, 0-d for a
2-D ``images``.  Device tensors stay on the device; nothing of frame size comes back unless the maps are asked for.

The window sums are float64 (on 16-bit detector levels float32 sums move the SSIM map by up to 1e-2), and the per-frame means are
reduced on the device from the float64 values in a fixed order: a frame scores the same bits alone and inside any batch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _ffi
from .._frames import frame_stack, mode_code, pair, window as size_pair
from ..preprocessing.smooth import gaussian_taps

MAX_SIZE = 63
MAX_HALF_WIDTH = 31
LDS_LIMIT = 160 * 1024
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_NULL = C.c_void_p(0)


def lds_bytes(size_y: int, size_x: int) -> int:
    """LDS of one workgroup of b4d_ssim for a size_y x size_x window (include/b4d.h); a window is supported up to LDS_LIMIT."""
    rows = 31 + size_y
    up4 = lambda n: (n + 3) & ~3  # noqa: E731
    return 8 * up4(rows * up4(31 + size_x)) + 1280 * rows + 128


# ------------------------------------------------------------------------------------------------- arguments (no device)
def _shape(a) -> tuple:
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _pairing(reference, images):
    """(batch, ny, nx, paired) of a reference / images pair; ValueError for anything but the three pairings."""
    rs, xs = _shape(reference), _shape(images)
    ok = (len(rs) == 2 and len(xs) in (2, 3) and xs[-2:] == rs) or (len(rs) == 3 and xs == rs)
    if not ok:
        raise ValueError(f"reference (H, W) goes with images (H, W) or (T, H, W), reference (T, H, W) with images (T, H, W); "
                         f"got reference {rs} and images {xs}")
    if 0 in xs:
        raise ValueError(f"images must not be empty; got shape {xs}")
    return (int(xs[0]) if len(xs) == 3 else 1), int(xs[-2]), int(xs[-1]), len(rs) == 3


class _Window:
    """Sizes, float64 taps (None: box) and cov_norm of the SSIM window."""

    def __init__(self, window, sigma, truncate, size, sample_covariance):
        if window not in ("gaussian", "box"):
            raise ValueError(f"window must be 'gaussian' or 'box'; got {window!r}")
        if window == "gaussian":
            if sample_covariance:
                raise ValueError("sample_covariance=True goes with window='box' only (scikit-image's Gaussian window uses the population covariance)")
            gy, gx = pair(sigma, "sigma")
            self.wy = gaussian_taps(gy, 0, truncate, max_half_width=MAX_HALF_WIDTH)
            self.wx = gaussian_taps(gx, 0, truncate, max_half_width=MAX_HALF_WIDTH)
            self.sy, self.sx = int(self.wy.size), int(self.wx.size)
            self.cov_norm = 1.0
        else:
            self.sy, self.sx = size_pair(size, MAX_SIZE)
            self.wy = self.wx = None
            n = self.sy * self.sx
            if sample_covariance and n < 2:
                raise ValueError("sample_covariance=True needs a window of more than one pixel")
            self.cov_norm = n / (n - 1.0) if sample_covariance else 1.0
        if lds_bytes(self.sy, self.sx) > LDS_LIMIT:
            raise ValueError(f"a {self.sy} x {self.sx} window needs {lds_bytes(self.sy, self.sx)} bytes of LDS, more than {LDS_LIMIT} "
                             "(every window up to 52 x 52 fits)")

    def crop(self, crop_border: bool):
        return ((self.sy - 1) // 2, (self.sx - 1) // 2) if crop_border else (0, 0)


def _check_constants(K1, K2):
    K1, K2 = float(K1), float(K2)
    if not (K1 > 0.0 and K2 > 0.0):
        raise ValueError(f"K1 and K2 must be > 0; got {K1!r}, {K2!r}")
    return K1, K2


def _check_range(data_range):
    """float(data_range), or None where it is to be taken from the reference."""
    if data_range is None:
        return None
    L = float(data_range)
    if not (L > 0.0 and np.isfinite(L)):
        raise ValueError(f"data_range must be finite and > 0; got {data_range!r}")
    return L


def _check_region(ny, nx, win, crop, what="the frames"):
    if ny - 2 * crop[0] < 1 or nx - 2 * crop[1] < 1:
        raise ValueError(f"{what} ({ny} x {nx}) are smaller than the {win.sy} x {win.sx} window, so crop_border=True leaves nothing to "
                         "average over; pass crop_border=False")


def ms_ssim_min_side(size: int, scales: int) -> int:
    """Smallest frame side whose `scales`-th level (scales - 1 halvings, each dropping an odd row) still holds a window of `size`."""
    return int(size) << (int(scales) - 1)


# ------------------------------------------------------------------------------------------------- device calls
def _load(reference, images):
    """Both as float32 device tensors (the pairing has been checked)."""
    return frame_stack(reference)[0], frame_stack(images)[0]


def run_pair_errors(r, ref_stride, x, batch, ny, nx):
    """b4d_pair_errors on float32 device tensors: the (batch, 8) float64 device tensor of sum (x - r)^2, sum |x - r|, max |x - r|,
    sum r^2, sum r, min r, max r, sum x."""
    torch = _ffi.require_gpu()
    out = torch.empty((batch, 8), dtype=torch.float64, device=x.device)
    _ffi.check(_ffi.lib().b4d_pair_errors(D.ptr(r), int(ref_stride), D.ptr(x), batch, ny, nx, D.ptr(out), _ffi.stream_ptr()))
    return out


def run_ssim(r, ref_stride, x, batch, ny, nx, win, mode, cval, c1, c2, crop, *, maps=False, means=True):
    """b4d_ssim on float32 device tensors; returns (means (batch, 2) float64 or None, ssim_map or None, cs_map or None)."""
    torch = _ffi.require_gpu()
    m = torch.empty((batch, 2), dtype=torch.float64, device=x.device) if means else None
    sm = torch.empty((batch, ny, nx), dtype=torch.float32, device=x.device) if maps else None
    cm = torch.empty((batch, ny, nx), dtype=torch.float32, device=x.device) if maps else None
    p = lambda t: D.ptr(t) if t is not None else _NULL  # noqa: E731
    taps = lambda w: w.ctypes.data_as(C.c_void_p) if w is not None else _NULL  # noqa: E731
    _ffi.check(_ffi.lib().b4d_ssim(D.ptr(r), int(ref_stride), D.ptr(x), batch, ny, nx, win.sy, win.sx, taps(win.wy), taps(win.wx), int(mode),
                                   float(cval), float(c1), float(c2), float(win.cov_norm), int(crop[0]), int(crop[1]), p(sm), p(cm), p(m),
                                   _ffi.stream_ptr()))
    return m, sm, cm


def run_pool2(t, batch, ny, nx):
    """b4d_pool2 on a float32 device tensor (batch, ny, nx): the (batch, ny // 2, nx // 2) means of 2 x 2 blocks."""
    torch = _ffi.require_gpu()
    out = torch.empty((batch, ny // 2, nx // 2), dtype=torch.float32, device=t.device)
    _ffi.check(_ffi.lib().b4d_pool2(D.ptr(t), batch, ny, nx, D.ptr(out), _ffi.stream_ptr()))
    return out


def _reference_range(r, ny, nx) -> float:
    """max - min over all reference frames, from b4d_pair_errors of the reference with itself."""
    n = int(r.shape[0]) if r.ndim == 3 else 1
    return _range_of(run_pair_errors(r, ny * nx, r, n, ny, nx).cpu().numpy())


def _range_of(e) -> float:
    """max r - min r over the rows of b4d_pair_errors (np.max / np.min: a NaN row makes it NaN, which is refused)."""
    L = float(np.max(e[:, 6]) - np.min(e[:, 5]))
    if not L > 0.0:
        raise ValueError(f"data_range=None needs a reference with max > min (got max - min = {L!r}); pass data_range")
    return L


def _scores(t, squeeze):
    a = np.asarray(t, dtype=np.float64)
    return a.reshape(a.shape[1:]) if squeeze else a


# ------------------------------------------------------------------------------------------------- public
def ssim(reference, images, *, data_range=None, window: str = "gaussian", sigma=1.5, truncate: float = 3.5, size=7,
         sample_covariance: bool = False, K1: float = 0.01, K2: float = 0.03, mode: str = "reflect", cval: float = 0.0,
         crop_border: bool = True, full: bool = False, return_tensors: bool = False):
    """Mean structural similarity of every frame of ``images`` to its reference frame.

    ``window="gaussian"`` (default): weights ``gaussian_taps(sigma, 0, truncate)``; the defaults are the 11-tap window of Wang et al.
    and of scikit-image's ``gaussian_weights=True``.  ``window="box"``: ``size`` (int or pair ``(y, x)``) equal weights, with
    ``sample_covariance=True`` the N / (N - 1) covariances that are scikit-image's default for that window.
    ``c1 = (K1 L)^2``, ``c2 = (K2 L)^2`` with ``L = data_range``; ``None`` takes max - min over all reference frames.
    ``crop_border=True`` averages over the interior that scikit-image averages over ((n - 1) // 2 pixels cropped per side);
    the frames are padded by ``mode`` / ``cval`` in two dimensions (scikit-image: "reflect").

    Returns the float64 scores; with ``full=True`` a dict ``{"ssim", "cs", "ssim_map", "cs_map"}`` (cs: the contrast-structure
    factor; maps float32, tensors with ``return_tensors=True``).  A NaN poisons its footprint in the maps and its frame's scores."""
    win = _Window(window, sigma, truncate, size, sample_covariance)
    K1, K2 = _check_constants(K1, K2)
    L = _check_range(data_range)
    m = mode_code(mode)
    batch, ny, nx, paired = _pairing(reference, images)
    crop = win.crop(crop_border)
    _check_region(ny, nx, win, crop)
    r, x = _load(reference, images)
    if L is None:
        L = _reference_range(r, ny, nx)
    means, sm, cm = run_ssim(r, ny * nx if paired else 0, x, batch, ny, nx, win, m, cval, (K1 * L) ** 2, (K2 * L) ** 2, crop, maps=full)
    squeeze = len(_shape(images)) == 2
    if return_tensors:
        score = lambda k: means[0, k] if squeeze else means[:, k]  # noqa: E731
        shape = lambda t: t[0] if squeeze else t  # noqa: E731
        return {"ssim": score(0), "cs": score(1), "ssim_map": shape(sm), "cs_map": shape(cm)} if full else score(0)
    h = means.cpu().numpy()
    if not full:
        return _scores(h[:, 0], squeeze)
    return {"ssim": _scores(h[:, 0], squeeze), "cs": _scores(h[:, 1], squeeze), "ssim_map": _scores_map(sm, squeeze), "cs_map": _scores_map(cm, squeeze)}


def _scores_map(t, squeeze):
    a = D.to_host(t)
    return a[0] if squeeze else a


def ms_ssim(reference, images, *, weights=MS_SSIM_WEIGHTS, data_range=None, window: str = "gaussian", sigma=1.5, truncate: float = 3.5,
            size=7, sample_covariance: bool = False, K1: float = 0.01, K2: float = 0.03, mode: str = "reflect", cval: float = 0.0,
            crop_border: bool = True, full: bool = False):
    """Multi-scale SSIM: at each of ``len(weights)`` scales the mean cs and mean ssim of the current pair, then both frames are
    halved by 2 x 2 means (a trailing odd row or column is dropped).  The score is
    ``prod_{s < last} max(cs_s, 0)^w_s * max(ssim_last, 0)^w_last``; ``data_range`` and ``crop_border`` are those of every scale.
    The coarsest scale must still hold the window: sides of at least ``size * 2^(len(weights) - 1)`` (176 for the defaults).

    Returns the float64 scores; with ``full=True`` ``{"ms_ssim", "ssim", "cs"}`` with the per-scale means as ``(T, S)`` arrays."""
    win = _Window(window, sigma, truncate, size, sample_covariance)
    K1, K2 = _check_constants(K1, K2)
    L = _check_range(data_range)
    m = mode_code(mode)
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size < 1 or not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError(f"weights must be a 1-D sequence of finite values >= 0; got {weights!r}")
    S = int(w.size)
    batch, ny, nx, paired = _pairing(reference, images)
    need_y, need_x = ms_ssim_min_side(win.sy, S), ms_ssim_min_side(win.sx, S)
    if ny < need_y or nx < need_x:
        raise ValueError(f"{S} scales of a {win.sy} x {win.sx} window need frames of at least {need_y} x {need_x}; got {ny} x {nx}")
    crop = win.crop(crop_border)
    r, x = _load(reference, images)
    if L is None:
        L = _reference_range(r, ny, nx)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    nref = batch if paired else 1
    r = r.reshape(nref, ny, nx)
    x = x.reshape(batch, ny, nx)
    per_scale = []
    for s in range(S):
        means, _, _ = run_ssim(r, ny * nx if paired else 0, x, batch, ny, nx, win, m, cval, c1, c2, crop)
        per_scale.append(means)
        if s + 1 < S:
            r, x = run_pool2(r, nref, ny, nx), run_pool2(x, batch, ny, nx)
            ny, nx = ny // 2, nx // 2
    h = np.stack([p.cpu().numpy() for p in per_scale], axis=1)      # (T, S, 2)
    ss, cs = h[:, :, 0], h[:, :, 1]
    with np.errstate(invalid="ignore"):
        factors = np.maximum(np.concatenate([cs[:, :-1], ss[:, -1:]], axis=1), 0.0)      # (np.maximum: a NaN stays)
        score = np.prod(factors ** w[None, :], axis=1)
    squeeze = len(_shape(images)) == 2
    if not full:
        return _scores(score, squeeze)
    return {"ms_ssim": _scores(score, squeeze), "ssim": _scores(ss, squeeze), "cs": _scores(cs, squeeze)}


def frame_errors(reference, images, *, data_range=None) -> dict:
    """``{"mse", "rmse", "mae", "max_abs", "psnr", "nrmse"}`` of every frame against its reference frame, from one pass over both
    (float64 sums): ``psnr = 10 log10(L^2 / mse)`` with ``L = data_range`` (``None``: max - min over all reference frames), ``inf``
    where ``mse`` is 0; ``nrmse = rmse / sqrt(mean r^2)`` (the Euclidean normalisation)."""
    L = _check_range(data_range)
    e, npix, squeeze = _errors(reference, images)
    out = _error_metrics(e, npix, _range_of(e) if L is None else L)
    return {k: _scores(v, squeeze) for k, v in out.items()}


def _errors(reference, images):
    """The (T, 8) sums of b4d_pair_errors on the host, the pixel count and whether `images` is one frame."""
    batch, ny, nx, paired = _pairing(reference, images)
    r, x = _load(reference, images)
    e = run_pair_errors(r, ny * nx if paired else 0, x, batch, ny, nx).cpu().numpy()
    return e, ny * nx, len(_shape(images)) == 2


def _error_metrics(e, npix, L):
    with np.errstate(divide="ignore", invalid="ignore"):
        mse_ = e[:, 0] / npix
        rmse = np.sqrt(mse_)
        return {"mse": mse_, "rmse": rmse, "mae": e[:, 1] / npix, "max_abs": e[:, 2].copy(),
                "psnr": np.where(mse_ == 0.0, np.inf, 10.0 * np.log10((L * L) / mse_)), "nrmse": rmse / np.sqrt(e[:, 3] / npix)}


def mse(reference, images):
    """Mean squared error of every frame against its reference frame."""
    e, npix, squeeze = _errors(reference, images)
    return _scores(e[:, 0] / npix, squeeze)


def psnr(reference, images, *, data_range=None):
    """Peak signal-to-noise ratio in dB, ``10 log10(data_range^2 / mse)``; ``data_range=None``: max - min of the reference frames."""
    return frame_errors(reference, images, data_range=data_range)["psnr"]


def nrmse(reference, images, *, normalization: str = "euclidean"):
    """Normalised root-mean-square error, scikit-image's three normalisations by the reference frame: ``"euclidean"``
    ``sqrt(mean r^2)``, ``"min-max"`` ``max r - min r``, ``"mean"`` ``mean r``."""
    if normalization not in ("euclidean", "min-max", "mean"):
        raise ValueError(f"normalization must be 'euclidean', 'min-max' or 'mean'; got {normalization!r}")
    e, npix, squeeze = _errors(reference, images)
    with np.errstate(divide="ignore", invalid="ignore"):
        rmse = np.sqrt(e[:, 0] / npix)
        den = {"euclidean": np.sqrt(e[:, 3] / npix), "min-max": e[:, 6] - e[:, 5], "mean": e[:, 4] / npix}[normalization]
        return _scores(rmse / den, squeeze)
