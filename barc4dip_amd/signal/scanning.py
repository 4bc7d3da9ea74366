"""Speckle scanning at detector resolution (``b4d_speckle_scan``): speckle-vector tracking, "UMPA".

The same N diffuser positions are recorded once without and once with the sample; every detector pixel is analysed with a window
of a few pixels, pooled over the positions.  Reference scan ``R[n]`` (N, H, W), sample scan ``S[n]`` (N, H, W), odd window
``(wy, wx)``, search ``(sy, sx)``, weights ``g[n] >= 0`` per position and a taper per axis (``"flat"``, or ``"hann"``: the
half-sample Hann of ``speckle_contrast``) give the pooled weights

    w[n, j, i] = g[n] h_wy[j] h_wx[i] / (sum g  sum h_wy  sum h_wx).

For pixel p and candidate shift u, ``|uy| <= sy``, ``|ux| <= sx``, the reference window is centred on p and the sample window on
p + u -- the convention of ``displacement_map`` and ``correct_distortion``: the sample displaced by the tracked shift matches the
reference.  With the weighted means Rm, Sm(u), variances VR, VS(u) and covariance C(u), all pooled over n and the window,

    rho(u) = C(u) / sqrt(VR VS(u)),

undefined when ``VR <= 1e-12 Rm^2`` or ``VS(u) <= 1e-12 Sm(u)^2`` (a constant patch).  The integer peak u* is the defined
candidate of largest rho, the first in row-major order among equals; this minimises the UMPA least-squares residual of
``r = a s + b`` with the reference window held fixed.  Each axis then adds the parabola step ``0.5 (a - c) / (a - 2 b + c)``
through rho at u* - e, u*, u* + e, clipped to +-0.5 and 0 when the parabola has no maximum, when a neighbour is undefined or when
u* lies on the border of the search range (the pixel's ``edge`` flag).  At the integer peak:

    transmission = Sm(u*) / Rm        dark_field = C(u*) / (VR transmission)        correlation = rho(u*)

(``dark_field`` is the ``dark_field_fit`` of ``speckle_contrast``).  A pixel is NaN in all planes, and neither valid nor edge,
when its margin ``(wy // 2 + sy, wx // 2 + sx)`` leaves the frame, when a reference value of its window or a sample value of its
window grown by the search is not finite in a position of weight above 0, or when no candidate is defined.  A position of weight
0 is never read.  Everything runs on the device in float64 sums; there is no host fallback.
"""
from __future__ import annotations

import numpy as np

from .. import _device as D
from .. import _ffi
from .displacement import _shape

MAX_WINDOW = 31
MAX_SEARCH = 16
MAX_POSITIONS = 4096
TAPERS = ("flat", "hann")
PLANES = ("dy", "dx", "correlation", "transmission", "dark_field")


def _int_pair(v, name: str, low: int) -> tuple[int, int]:
    if isinstance(v, str) or np.ndim(v) > 1 or (np.ndim(v) == 1 and len(v) != 2):
        raise ValueError(f"{name} must be an int or a (y, x) pair, got {v!r}")
    pair = tuple(v) if np.ndim(v) == 1 else (v, v)
    out = []
    for a in pair:
        try:
            ok = not isinstance(a, (bool, np.bool_)) and int(a) == a
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"{name} must hold integers, got {v!r}")
        out.append(int(a))
    if min(out) < low:
        raise ValueError(f"{name} must be >= {low} per axis, got {v!r}")
    return out[0], out[1]


def _check(reference, sample, window, search, taper, weights, min_correlation):
    """Everything that can be wrong with the arguments, on the host.  Returns (sample shape, window, search, taper code,
    weights as float64 (N,), min_correlation)."""
    for name, a in (("reference", reference), ("sample", sample)):
        if (a.is_complex() if D.is_tensor(a) else np.asarray(a).dtype.kind not in "buif"):
            raise ValueError(f"{name} must be a real array")
    rs, ss = _shape(reference), _shape(sample)
    if len(rs) != 3 or len(ss) not in (3, 4):
        raise ValueError(f"reference must be (N, H, W) and sample (N, H, W) or (M, N, H, W), got {rs} and {ss}")
    if 0 in rs or 0 in ss:
        raise ValueError("empty reference or sample")
    if rs[-2:] != ss[-2:]:
        raise ValueError(f"reference frames {rs[-2:]} and sample frames {ss[-2:]} differ in shape")
    if rs[0] != ss[-3]:
        raise ValueError(f"reference has {rs[0]} positions, sample {ss[-3]}")
    wy, wx = _int_pair(window, "window", 1)
    if wy % 2 == 0 or wx % 2 == 0:
        raise ValueError(f"window sides must be odd, got {window!r}")
    sy, sx = _int_pair(search, "search", 0)
    if not isinstance(taper, str) or taper not in TAPERS:
        raise ValueError(f"taper must be one of {TAPERS}, got {taper!r}")
    N, (H, W) = rs[0], rs[-2:]
    if weights is None:
        g = np.ones(N)
    else:
        if isinstance(weights, str):
            raise ValueError(f"weights must be None or {N} numbers, got {weights!r}")
        try:
            g = np.array(weights.cpu() if D.is_tensor(weights) else weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"weights must be None or {N} numbers, got {weights!r}") from None
        if g.shape != (N,):
            raise ValueError(f"weights must have one entry per position ({N},), got shape {g.shape}")
        if not np.all(np.isfinite(g)) or np.any(g < 0.0) or not np.any(g > 0.0):
            raise ValueError("weights must be finite, >= 0 and not all 0")
    if min_correlation is not None:
        bad = isinstance(min_correlation, (bool, str)) or np.ndim(min_correlation) != 0
        if not bad:
            try:
                min_correlation = float(min_correlation)
            except (TypeError, ValueError):
                bad = True
        if bad or not -1.0 <= min_correlation <= 1.0:
            raise ValueError(f"min_correlation must be None or a number in [-1, 1], got {min_correlation!r}")
    if wy > MAX_WINDOW or wx > MAX_WINDOW:
        raise NotImplementedError(f"window {(wy, wx)} exceeds the kernel's limit of {MAX_WINDOW} px per axis")
    if sy > MAX_SEARCH or sx > MAX_SEARCH:
        raise NotImplementedError(f"search {(sy, sx)} exceeds the kernel's limit of {MAX_SEARCH} px per axis")
    if N > MAX_POSITIONS:
        raise NotImplementedError(f"{N} positions exceed the kernel's limit of {MAX_POSITIONS}")
    if H < wy + 2 * sy or W < wx + 2 * sx:
        raise ValueError(f"a {(wy, wx)} window searched +-{(sy, sx)} px does not fit in a {(H, W)} frame")
    return ss, (wy, wx), (sy, sx), TAPERS.index(taper), g, min_correlation


def speckle_scan(reference, sample, *, window=5, search=4, taper: str = "hann", subpixel: bool = True, weights=None,
                 min_correlation=None, return_tensors: bool = False) -> dict:
    """Differential phase, transmission and dark field at every detector pixel from a stepped-diffuser scan.

    reference (N, H, W): the N diffuser positions without the sample; sample (N, H, W), or (M, N, H, W) for M scans against the
    one reference.  NumPy arrays of any real dtype or ROCm tensors.  ``window`` (odd) and ``search`` (>= 0): int or (y, x).
    ``taper``: "flat" or "hann".  ``weights``: one number >= 0 per position (default all 1; a position of weight 0 is never
    read).  ``subpixel=False`` keeps the integer peak.  Formulas in the module docstring.
    Returns {"dy", "dx", "correlation", "transmission", "dark_field": float64 (H, W) or (M, H, W), NaN where the pixel has no
    result; "peak": the correlation plane (for ``weights="peak"`` downstream); "edge": bool, the peak lies on the border of the
    search range; "valid": bool, the pixel has a result and, with ``min_correlation`` (a number in [-1, 1]),
    ``correlation >= min_correlation``; "y", "x": pixel coordinates (float64); "meta"}, so that
    ``wavefront_from_displacement(m, ..., mask=m["valid"])`` and ``correct_distortion(frame, m)`` take it as it is.  Device
    tensors with ``return_tensors=True``.  A scan gives the same bits alone and inside any batch.
    ValueError for bad shapes, a position count that differs, an even or non-positive window, a negative search, bad weights,
    a frame smaller than window + 2 search, a bad ``taper`` or ``min_correlation``; NotImplementedError for a window beyond
    31, a search beyond 16 px or more than 4096 positions -- all raised before the GPU is touched."""
    ss, (wy, wx), (sy, sx), tap, g, min_correlation = _check(reference, sample, window, search, taper, weights, min_correlation)
    torch = _ffi.require_gpu()
    ref, _, _ = D.to_device_f32(reference, ndim=(3,))
    smp, _, _ = D.to_device_f32(sample, ndim=(3, 4))
    N, H, W = (int(s) for s in ref.shape)
    M = 1 if len(ss) == 3 else int(ss[0])
    gd = torch.from_numpy(g).to(ref.device)
    out = torch.empty((M, 6, H, W), dtype=torch.float64, device=ref.device)
    _ffi.check(_ffi.lib().b4d_speckle_scan(D.ptr(ref), D.ptr(smp), M, N, H, W, wy, wx, sy, sx, D.ptr(gd), tap, int(bool(subpixel)),
                                           D.ptr(out), _ffi.stream_ptr()))
    if len(ss) == 3:
        out = out[0]
    res = {name: out[..., k, :, :] for k, name in enumerate(PLANES)}
    flags = out[..., 5, :, :]
    res["peak"] = res["correlation"]
    res["edge"] = flags >= 2.0
    valid = flags >= 1.0
    if min_correlation is not None:
        valid = valid & (res["correlation"] >= min_correlation)
    res["valid"] = valid
    if not return_tensors:
        host = out.cpu().numpy()
        res = {k: (host[..., PLANES.index("correlation" if k == "peak" else k), :, :] if k in PLANES or k == "peak"
                   else v.cpu().numpy()) for k, v in res.items()}
    res.update({"y": np.arange(H, dtype=np.float64), "x": np.arange(W, dtype=np.float64),
                "meta": {"window": (wy, wx), "step": (1, 1), "search": (sy, sx), "taper": taper, "subpixel": bool(subpixel),
                         "n_positions": N, "min_correlation": min_correlation}})
    return res
