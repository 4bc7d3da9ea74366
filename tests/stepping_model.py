"""Float64 NumPy restatement of barc4dip_amd.signal.stepping (phase-stepping analysis of grating scans): the masked per-pixel
least-squares fit with its validity rule, the sample-against-reference formulas and the step self-calibration iteration.
Written from the formulas of the module docstring; the product never imports it.

Model: I_t = a0 + sum_k (c_k cos k phi_t + s_k sin k phi_t), coefficient order (a0, c_1, s_1, c_2, s_2), a_k = hypot(c_k, s_k),
phi_k = atan2(-s_k, c_k)."""
import numpy as np

PIVOT_RTOL = 1e-10


def uniform_steps(T, periods=1.0):
    return 2.0 * np.pi * float(periods) * np.arange(T, dtype=np.float64) / T


def basis(steps, K):
    """(T, 2K + 1) float64: columns 1, cos phi, sin phi, cos 2 phi, sin 2 phi."""
    p = np.asarray(steps, dtype=np.float64)
    cols = [np.ones_like(p)]
    for k in range(1, K + 1):
        cols += [np.cos(k * p), np.sin(k * p)]
    return np.stack(cols, axis=1)


def cholesky_solve(A, b):
    """x of A x = b by Cholesky, or None if a pivot is not above PIVOT_RTOL times the largest diagonal entry of A."""
    M = A.shape[0]
    L = np.zeros_like(A)
    floor = PIVOT_RTOL * np.max(np.diag(A))
    for j in range(M):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > floor:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, M):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(M)
    for i in range(M):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(M)
    for i in range(M - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def dropped(stack, saturation=None):
    I = np.asarray(stack, dtype=np.float64)
    drop = ~np.isfinite(I)
    if saturation is not None:
        with np.errstate(invalid="ignore"):
            drop |= I >= float(saturation)
    return drop


def fit(stack, steps, K=1, saturation=None):
    """Masked least-squares fit of a (T, ...) stack.  Returns {"coeff": (M, ...), "residual", "n_samples", "valid", "mean",
    "amplitude", "phase", "visibility": (K, ...)}; everything of an invalid pixel is NaN."""
    I = np.asarray(stack, dtype=np.float64)
    T = I.shape[0]
    shape = I.shape[1:]
    I = I.reshape(T, -1)
    B = basis(steps, K)
    M = B.shape[1]
    drop = dropped(I, saturation)
    Ik = np.where(drop, 0.0, I)
    b = B.T @ Ik                                    # (M, P)
    sii = np.sum(Ik * Ik, axis=0)
    nk = T - drop.sum(axis=0)
    G = B.T @ B
    coeff = np.full((M, I.shape[1]), np.nan)
    clean = ~drop.any(axis=0)
    x0 = cholesky_solve(G, np.zeros(M))
    if x0 is not None and T >= M:
        coeff[:, clean] = np.linalg.solve(G, b[:, clean])
    for p in np.nonzero(~clean)[0]:
        if nk[p] < M:
            continue
        kept = ~drop[:, p]
        A = B[kept].T @ B[kept]
        x = cholesky_solve(A, b[:, p])
        if x is not None:
            coeff[:, p] = x
    valid = ~np.isnan(coeff[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.sqrt(np.maximum(sii - np.sum(b * coeff, axis=0), 0.0) / nk)
    res[~valid] = np.nan
    out = {"coeff": coeff.reshape((M,) + shape), "residual": res.reshape(shape), "n_samples": nk.reshape(shape),
           "valid": valid.reshape(shape)}
    out.update(derived(out["coeff"]))
    return out


def derived(coeff):
    """mean, amplitude, phase, visibility of a coefficient array (M, ...)."""
    c = np.asarray(coeff, dtype=np.float64)
    K = (c.shape[0] - 1) // 2
    a0 = c[0]
    amp = np.stack([np.hypot(c[2 * k + 1], c[2 * k + 2]) for k in range(K)])
    ph = np.stack([np.arctan2(-c[2 * k + 2], c[2 * k + 1]) for k in range(K)])
    with np.errstate(invalid="ignore", divide="ignore"):
        vis = amp / a0
    return {"mean": a0, "amplitude": amp, "phase": ph, "visibility": vis}


def wrap(d):
    """Wrap to (-pi, pi]."""
    d = np.asarray(d, dtype=np.float64)
    w = d - 2.0 * np.pi * np.ceil((d - np.pi) / (2.0 * np.pi))
    return w


def compare(coeff_s, coeff_r):
    """Sample against reference coefficient arrays (M, ...): transmission, dpc, visibility (sample), visibility_ref,
    dark_field, valid (K, ...)."""
    s, r = derived(coeff_s), derived(coeff_r)
    with np.errstate(invalid="ignore", divide="ignore"):
        trans = s["mean"] / r["mean"]
        dark = s["visibility"] / r["visibility"]
    dpc = wrap(s["phase"] - r["phase"])
    ok = ~np.isnan(s["mean"]) & ~np.isnan(r["mean"]) & (s["mean"] > 0) & (r["mean"] > 0)
    valid = ok[None] & (r["amplitude"] > 0)
    return {"transmission": trans, "dpc": dpc, "visibility": s["visibility"], "visibility_ref": r["visibility"], "dark_field": dark,
            "valid": valid}


def calibrate_iteration(stack, delta, saturation=None):
    """One iteration of the step self-calibration on a (T, ...) stack with the current step phases `delta` (T,).
    Returns (new delta, change, dose g_t, modulation m_t), or None if the fit with `delta` is singular."""
    I = np.asarray(stack, dtype=np.float64)
    T = I.shape[0]
    I = I.reshape(T, -1)
    B = basis(delta, 1)
    G = B.T @ B
    if cholesky_solve(G, np.zeros(3)) is None:
        return None
    use = ~dropped(I, saturation).any(axis=0)
    Iu = I[:, use]
    X = np.linalg.solve(G, B.T @ Iu)                # (3, P): a0, c, s
    N = X @ X.T
    R = X @ Iu.T                                    # (3, T)
    guv = np.linalg.solve(N, R)                     # rows g, u, v
    g, u, v = guv
    raw = np.arctan2(v, u) - np.arctan2(v[0], u[0])
    new = delta + wrap(raw - delta)
    return new, float(np.max(np.abs(new - delta))), g, np.hypot(u, v)


def calibrate(stack, steps, saturation=None, tol=1e-9, max_iter=200):
    """Iterate to `tol`.  Returns (steps, {"iterations", "change", "converged", "dose", "modulation"}); the returned steps keep
    steps[0]."""
    s0 = np.asarray(steps, dtype=np.float64)
    delta = s0 - s0[0]
    change, g, m, it = np.inf, None, None, 0
    while it < max_iter:
        r = calibrate_iteration(stack, delta, saturation)
        if r is None:
            break
        delta, change, g, m = r
        it += 1
        if change <= tol:
            break
    return delta + s0[0], {"iterations": it, "change": change, "converged": bool(change <= tol), "dose": g, "modulation": m}


def calibration_fringes(T, H, W, steps, K=1):
    """The issue's noise-free calibration fringes, float32: a0 = 1000 (1 + 0.3 cos(x/17) sin(y/11)), visibility
    0.3 + 0.1 sin(x/13), phase 2 pi (x/9.7 + 0.002 (y - H/2)^2) + 0.3 sin(y/5)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a0 = 1000.0 * (1.0 + 0.3 * np.cos(x / 17.0) * np.sin(y / 11.0))
    vis = 0.3 + 0.1 * np.sin(x / 13.0)
    ph = 2.0 * np.pi * (x / 9.7 + 0.002 * (y - H / 2.0) ** 2) + 0.3 * np.sin(y / 5.0)
    p = np.asarray(steps, dtype=np.float64)[:, None, None]
    I = a0 * (1.0 + vis * np.cos(p + ph))
    return I.astype(np.float32), a0, vis, ph

