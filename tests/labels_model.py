"""Host model of barc4dip_amd.geometry.labels and barc4dip_amd.metrics.regions, and the cases of their tests.

Labels: ``scipy.ndimage.label``.  Columns: plain float64 NumPy over the pixels of each region in raster order (``np.bincount`` sums,
``np.minimum.at`` / ``np.maximum.at``, first occurrences by ``np.unique``); tests/test_labels_host.py holds it against
``scipy.ndimage`` one function at a time.  The generators place their features on the seams of whatever tile the kernels use
(``labels.TILE``)."""
import numpy as np
from scipy import ndimage

EPS = 2.0 ** -53


def structure(connectivity):
    return ndimage.generate_binary_structure(2, connectivity)


def label(mask, connectivity):
    """(labels int32, n) of a 2-D mask."""
    lab, n = ndimage.label(np.asarray(mask) != 0, structure(connectivity))
    return lab.astype(np.int32), int(n)


def threshold_mask(image, threshold):
    """Foreground of the device rule: float32 pixels strictly above the float32 threshold (NaN: background)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(image, dtype=np.float32) > np.float32(threshold)


def relabel_kept(lab, keep):
    """lab with the regions k + 1 where keep[k] renumbered 1 .. in their old order, the others 0."""
    keep = np.asarray(keep, dtype=bool)
    table = np.concatenate(([0], np.where(keep, np.cumsum(keep), 0))).astype(np.int32)
    return table[lab], int(keep.sum())


def hysteresis(image, low, high, connectivity):
    lab, n = label(threshold_mask(image, low), connectivity)
    if n == 0:
        return lab, 0
    top = ndimage.maximum(np.asarray(image, dtype=np.float32), lab, index=np.arange(1, n + 1))
    return relabel_kept(lab, top > high)


def select(lab, keep=None, min_area=None, max_area=None, clear_border=False, largest=None):
    """select_regions on one frame, written with scipy.ndimage."""
    n = int(lab.max())
    H, W = lab.shape
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    ok = np.ones(n, dtype=bool) if keep is None else np.array(keep, dtype=bool)
    if min_area is not None:
        ok &= area >= min_area
    if max_area is not None:
        ok &= area <= max_area
    if clear_border:
        for k, sl in enumerate(ndimage.find_objects(lab, max_label=n)):
            if sl is not None and (sl[0].start == 0 or sl[1].start == 0 or sl[0].stop == H or sl[1].stop == W):
                ok[k] = False
    ok &= area > 0
    if largest is not None:
        cand = [k for k in range(n) if ok[k]]
        cand.sort(key=lambda k: (-area[k], k))
        ok[:] = False
        ok[cand[:largest]] = True
    return relabel_kept(lab, ok)


COLUMNS = ("area", "y0", "y1", "x0", "x1", "cy", "cx", "sum", "min", "max", "max_y", "max_x", "flux", "wcy", "wcx", "var_y", "var_x",
           "cov_yx", "n_nan", "n_saturated")
INTEGER_COLUMNS = ("area", "y0", "y1", "x0", "x1", "max_y", "max_x", "n_nan", "n_saturated")


def properties(lab, image=None, background=0.0, saturation=None, n=None):
    """The columns of one frame, plus "abs_sum" (the sum of |v|, for the bound of `sum`) and "side" (the longer box side)."""
    lab = np.asarray(lab)
    n = int(lab.max()) if n is None else int(n)
    yy, xx = np.nonzero((lab >= 1) & (lab <= n))          # raster order
    l = lab[yy, xx].astype(np.int64) - 1
    cnt = lambda idx, w=None: np.bincount(idx, weights=w, minlength=n)  # noqa: E731
    area = cnt(l).astype(np.int64)
    some = area > 0
    big = np.iinfo(np.int64).max
    y0, x0 = np.full(n, big), np.full(n, big)
    y1, x1 = np.full(n, -1), np.full(n, -1)
    np.minimum.at(y0, l, yy)
    np.minimum.at(x0, l, xx)
    np.maximum.at(y1, l, yy)
    np.maximum.at(x1, l, xx)
    y0, x0, y1, x1 = (np.where(some, a, b) for a, b in ((y0, 0), (x0, 0), (y1 + 1, 0), (x1 + 1, 0)))
    r, c = yy - y0[l], xx - x0[l]
    nan = np.full(n, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"area": area, "y0": y0, "y1": y1, "x0": x0, "x1": x1,
               "cy": np.where(some, y0 + cnt(l, r) / area, np.nan), "cx": np.where(some, x0 + cnt(l, c) / area, np.nan)}
    out["side"] = np.maximum(np.maximum(y1 - y0, x1 - x0), 1)
    zero = np.zeros(n, dtype=np.int64)
    if image is None:
        out.update({k: nan for k in ("sum", "min", "max", "flux", "wcy", "wcx", "var_y", "var_x", "cov_yx")})
        out.update(max_y=zero - 1, max_x=zero - 1, n_nan=zero, n_saturated=zero, abs_sum=np.zeros(n))
        return out
    v = np.asarray(image, dtype=np.float32)[yy, xx].astype(np.float64)
    ok = ~np.isnan(v)
    out["n_nan"] = cnt(l[~ok]).astype(np.int64)
    l, v, r, c, py, px = l[ok], v[ok], r[ok], c[ok], yy[ok], xx[ok]
    valued = cnt(l) > 0
    out["sum"], out["abs_sum"] = cnt(l, v), cnt(l, np.abs(v))
    mn, mx = np.full(n, np.inf), np.full(n, -np.inf)
    np.minimum.at(mn, l, v)
    np.maximum.at(mx, l, v)
    out["min"], out["max"] = np.where(valued, mn, np.nan), np.where(valued, mx, np.nan)
    hit = np.flatnonzero(v == mx[l])
    who, first = np.unique(l[hit], return_index=True)     # the first hit of every label: pixels are in raster order
    out["max_y"], out["max_x"] = zero - 1, zero - 1
    out["max_y"][who], out["max_x"][who] = py[hit[first]], px[hit[first]]
    out["n_saturated"] = zero if saturation is None or np.isinf(saturation) else cnt(l[v >= saturation]).astype(np.int64)
    w = np.maximum(v - background, 0.0)
    flux = cnt(l, w)
    out["flux"] = flux
    lit = valued & (flux > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        wr, wc = np.where(lit, cnt(l, w * r) / flux, np.nan), np.where(lit, cnt(l, w * c) / flux, np.nan)
        ey, ex = r - wr[l], c - wc[l]
        use = w > 0
        out["wcy"], out["wcx"] = y0 + wr, x0 + wc
        out["var_y"] = np.where(lit, cnt(l[use], (w * ey * ey)[use]) / flux, np.nan)
        out["var_x"] = np.where(lit, cnt(l[use], (w * ex * ex)[use]) / flux, np.nan)
        out["cov_yx"] = np.where(lit, cnt(l[use], (w * ey * ex)[use]) / flux, np.nan)
    return out


def stack_properties(labs, images=None, **kw):
    """The flat table of a stack: the frames' columns one after another, with frame, label and n."""
    per = [properties(labs[t], None if images is None else images[t], **kw) for t in range(len(labs))]
    out = {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    out["n"] = np.array([p["area"].size for p in per], dtype=np.int64)
    out["frame"] = np.repeat(np.arange(len(labs)), out["n"])
    out["label"] = np.concatenate([np.arange(1, m + 1) for m in out["n"]]).astype(np.int64) if len(per) else np.zeros(0, np.int64)
    return out


def compare_properties(got, want, observe=None, tag=""):
    """Assert the contract of the columns: integer columns, min, max and every NaN pattern exact; float sums within
    2 n 2^-53 sum|terms|; centroids within 4 n 2^-53 L px; moments within 4 n 2^-53 L^2.  n: the region's area, L: its longer
    box side.  Returns the worst ratio of difference to bound per kind."""
    for k in INTEGER_COLUMNS + ("min", "max"):
        assert np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), equal_nan=True), (tag, k)
    n, L = want["area"].astype(np.float64), want["side"].astype(np.float64)
    worst = {}

    def within(kind, keys, bound):
        ratio = 0.0
        for k in keys:
            g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, k, "NaN pattern")
            live = ~np.isnan(w)
            b = bound(k)[live]
            d = np.abs(g[live] - w[live])
            assert np.all(d <= b), (tag, k, float(np.max(d - b)))
            if d.size:
                ratio = max(ratio, float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), 0.0))))
        worst[kind] = ratio
        if observe is not None:
            observe(f"regions_{kind}_ratio", ratio, 1.0)

    within("sum", ("sum", "flux"), lambda k: 2.0 * n * EPS * (want["abs_sum"] if k == "sum" else want["flux"]))
    within("centroid", ("cy", "cx", "wcy", "wcx"), lambda k: 4.0 * n * EPS * L)
    within("moment", ("var_y", "var_x", "cov_yx"), lambda k: 4.0 * n * EPS * L * L)
    return worst


# ---------------------------------------------------------------------------------------------------------------------- cases
DENSITIES = (0.3, 0.407, 0.593, 0.8)      # 0.407 and 0.593: the site-percolation thresholds of connectivity 2 and 1


def shapes(tile):
    ty, tx = tile
    return ((1, 1), (1, tx + 3), (ty + 3, 1), (2 * ty + 1, 2 * tx + 1), (200, 333))


def random_mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def checkerboard(shape):
    y, x = np.indices(shape)
    return (y + x) % 2 == 0


def corner_pairs(tile):
    """Two masks of 2 x 2 tiles: the pixels (ty - 1, tx - 1), (ty, tx), and the pixels (ty - 1, tx), (ty, tx - 1)."""
    ty, tx = tile
    a, b = np.zeros((2 * ty, 2 * tx), bool), np.zeros((2 * ty, 2 * tx), bool)
    a[ty - 1, tx - 1] = a[ty, tx] = True
    b[ty - 1, tx] = b[ty, tx - 1] = True
    return a, b


def serpentine(shape):
    """Full rows 0, 2, 4, .. joined at alternating ends: one region whose chain is about H W / 2 long."""
    H, W = shape
    m = np.zeros(shape, bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def spiral(shape):
    """A square spiral one pixel wide with one pixel between its turns."""
    H, W = shape
    m = np.zeros(shape, bool)
    y = x = d = 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[0, 0] = True
    turns = 0
    while turns < 2:
        dy, dx = step[d]
        ny_, nx_ = y + dy, x + dx
        by, bx = ny_ + dy, nx_ + dx
        free = 0 <= ny_ < H and 0 <= nx_ < W and not m[ny_, nx_] and not (0 <= by < H and 0 <= bx < W and m[by, bx])
        if free:
            y, x, turns = ny_, nx_, 0
            m[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def comb(shape):
    """Upside down: teeth in every other column from row 0 down, joined only by the last row."""
    m = np.zeros(shape, bool)
    m[:, 0::2] = True
    m[-1] = True
    return m


def smooth_frame(shape, seed, signed=False):
    """Smooth float32 frame: positive (80 .. 320), or of both signs."""
    H, W = shape
    y, x = np.indices(shape, dtype=np.float64)
    rng = np.random.default_rng(seed)
    f = 200.0 + 100.0 * np.sin(y / 7.0 + 0.3) * np.cos(x / 5.0) + 20.0 * rng.random(shape)
    if signed:
        f = (f - 200.0) * (1.0 + rng.random(shape))
    return f.astype(np.float32)


def sprinkle(frame, seed, saturation=4095.0):
    """frame with 3 % NaN pixels and 3 % pixels at `saturation`."""
    rng = np.random.default_rng(seed)
    u = rng.random(frame.shape)
    f = frame.copy()
    f[u < 0.03] = np.nan
    f[u > 0.97] = saturation
    return f
