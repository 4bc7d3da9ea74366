"""NumPy restatement of barc4dip_amd.metrics.order / csrc/b4d_torder.hip (per-pixel order statistics along the frame axis of a
stack): sort-based quantiles with the five methods and two NaN policies, and the robust mean with its float32 rejection rules.
Written from the formulas of the module docstring; the product never imports it.

A stack is (T, ...) and is cast to float32 first.  Per pixel the samples are sorted in np.sort's order (NaN last).  With s[0..n)
the sorted samples taking part and h = q (n - 1) in float64, a method gives an index i and a fraction g; g == 0 gives s[i]
itself, otherwise float32(a + (b - a) g) with a, b = float64(s[i]), float64(s[i + 1]) and every operation rounded once."""
import numpy as np

METHODS = ("linear", "lower", "higher", "nearest", "midpoint")
SCALES = ("absolute", "mad", "poisson")
POLARITIES = ("both", "hot", "dead")


def quantile_position(q, n, method):
    """(i, g) for the fraction q and the integer array n of samples taking part; n < 1 gives (0, 0)."""
    n = np.asarray(n, dtype=np.int64)
    h = np.float64(q) * np.maximum(n - 1, 0).astype(np.float64)
    fl = np.floor(h)
    if method == "higher":
        i = np.ceil(h)
    elif method == "nearest":
        i = np.rint(h)            # half to even
    elif method in ("linear", "lower", "midpoint"):
        i = fl
    else:
        raise ValueError(method)
    g = np.zeros_like(h)
    if method == "linear":
        g = h - fl
    if method == "midpoint":
        g = np.where(h > fl, 0.5, 0.0)
    return i.astype(np.int64), g


def quantiles(stack, fractions, method="linear", ignore_nan=False):
    """((Q, ...) float32 quantiles along axis 0, (...) int count of non-NaN samples)."""
    x = np.asarray(stack).astype(np.float32)
    T = x.shape[0]
    s = np.sort(x, axis=0)
    nv = np.count_nonzero(~np.isnan(x), axis=0)
    n = nv if ignore_nan else np.full_like(nv, T)
    out = []
    with np.errstate(all="ignore"):
        for q in np.atleast_1d(np.asarray(fractions, dtype=np.float64)):
            i, g = quantile_position(q, n, method)
            a = np.take_along_axis(s, i[None], axis=0)[0]
            b = np.take_along_axis(s, np.minimum(i + 1, T - 1)[None], axis=0)[0]
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            d = b64 - a64
            p = d * g
            r = np.where(g == 0.0, a, (a64 + p).astype(np.float32))
            bad = (n < 1) | (nv < T if not ignore_nan else False)
            out.append(np.where(bad, np.float32(np.nan), r).astype(np.float32))
    return np.stack(out), nv


def percentile(stack, q, method="linear", ignore_nan=False):
    """np.percentile's calling convention: q in percent, scalar -> (...), sequence -> (Q, ...)."""
    res, _ = quantiles(stack, np.asarray(q, dtype=np.float64) / 100.0, method, ignore_nan)
    return res[0] if np.ndim(q) == 0 else res


def median(stack, ignore_nan=False):
    return quantiles(stack, [0.5], "midpoint", ignore_nan)[0][0]


def outlier_rule(x, med, mad, threshold=5.0, scale="mad", polarity="both", min_scale=0.0):
    """(rhs, rejected) of the outlier rule (csrc/b4d_keys.hpp: outlier_rhs, outlier_rejected) for float32 samples x against the
    median med of their neighbourhood -- a window (remove_outliers) or the frames of a stack (robust_mean) -- and, for
    scale="mad" only, its MAD (a callable is evaluated only then).  Every float32 operation is rounded on its own; x, med and mad
    broadcast, rhs has the shape of med."""
    x, med = np.asarray(x), np.asarray(med)
    assert x.dtype == np.float32 and med.dtype == np.float32
    thr, floor_ = np.float32(threshold), np.float32(min_scale)

    def floored(s):      # np.maximum(s, floor_) with the tie -0 / +0 pinned (NumPy returns either operand): s unless s < floor_
        return np.where(s < floor_, floor_, s)

    with np.errstate(all="ignore"):
        d = x - med
        if scale == "absolute":
            rhs = np.full_like(med, thr)
            out = np.abs(d) > rhs
        elif scale == "mad":
            mad = np.asarray(mad() if callable(mad) else mad)
            assert mad.dtype == np.float32
            rhs = thr * floored(np.float32(1.4826) * mad)
            out = np.abs(d) > rhs
        elif scale == "poisson":
            rhs = (thr * thr) * floored(med)
            out = d * d > rhs
        else:
            raise ValueError(scale)
        if polarity == "hot":
            out &= d > 0
        elif polarity == "dead":
            out &= d < 0
        elif polarity != "both":
            raise ValueError(polarity)
        out |= ~np.isfinite(x)          # last: a sample that is not finite is always an outlier
    assert d.dtype == np.float32 and rhs.dtype == np.float32
    return rhs, out


def robust_mean(stack, threshold=5.0, scale="mad", polarity="both", min_scale=0.0):
    """{"mean", "median", "scale", "n_kept", "rejected", "cleaned"} in the float32 operation order of the kernels."""
    x = np.asarray(stack).astype(np.float32)
    x = np.where(np.isfinite(x), x, np.float32(np.nan)).astype(np.float32)
    with np.errstate(all="ignore"):
        med = median(x, ignore_nan=True)
        rhs, out = outlier_rule(x, med, lambda: median(np.abs(x - med[None]), ignore_nan=True), threshold, scale, polarity, min_scale)
        n_kept = np.count_nonzero(~out, axis=0)
        total = np.sum(np.where(out, 0.0, x.astype(np.float64)), axis=0)
        mean = np.where(n_kept > 0, total / np.maximum(n_kept, 1), np.nan).astype(np.float32)
    assert rhs.dtype == np.float32
    return {"mean": mean, "median": med, "scale": rhs.astype(np.float32), "n_kept": n_kept, "rejected": out,
            "cleaned": np.where(out, med[None], x).astype(np.float32)}


def ulp_distance(a, b):
    """Distance in float32 ulps between arrays of the same sign pattern (NaN pairs count 0)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.where(both_nan, 0, np.abs(ia - ib))


# ------------------------------------------------------------------------------------------------ inputs shared by both tiers
def counts_stack(T, shape, seed=0, lam=6.0, fractional=True):
    """Positive data with many ties: Poisson counts + 1, a fifth of them with a fractional part."""
    rng = np.random.default_rng(seed)
    x = rng.poisson(lam, (T,) + tuple(shape)).astype(np.float32) + np.float32(1)
    if fractional:
        frac = (rng.integers(1, 8, x.shape) / 8.0).astype(np.float32)
        x = np.where(rng.random(x.shape) < 0.2, x + frac, x).astype(np.float32)
    return x


def zinger_stack(T, shape, seed=0, lam=400.0):
    """Poisson(lam) stack with planted zingers (x 6) and dead samples (0): (stack, hot mask, dead mask), at most one in ten samples
    of a pixel and never the same sample twice."""
    rng = np.random.default_rng(seed)
    x = rng.poisson(lam, (T,) + tuple(shape)).astype(np.float32)
    hot = np.zeros(x.shape, bool)
    dead = np.zeros(x.shape, bool)
    flat_hot, flat_dead = hot.reshape(T, -1), dead.reshape(T, -1)
    npix = flat_hot.shape[1]
    k = max(1, T // 10) if T >= 5 else 0
    for p in range(npix):
        if k and p % 3 != 2:
            idx = rng.choice(T, min(T, 2 * k), replace=False)
            flat_hot[idx[:k], p] = p % 3 == 0
            flat_dead[idx[:k], p] = p % 3 == 1
    x[hot] = np.float32(6 * lam)
    x[dead] = np.float32(0)
    return x, hot, dead
