"""NumPy model of the "ysplit" route of the PSD + autocorrelation pipeline (b4d_fft2d.hpp): one radix-2 stage of the
column transform is done by the row passes.  The model follows the kernels' index maps one to one -- row pairing (p, p + h)
in K1, the [parity][tile][n][c] workspace, the ky = 2k + parity PSD rows and their mirrors in K2, rows 0 .. h/2 kept in
place, the combine and the row ownership of K3 -- and is compared against np.fft.  Untouched workspace / output cells are
NaN, so a read of a row nobody wrote, or an output row nobody owns, shows in the result."""
import numpy as np
import pytest


def _k1(x, ctw):
    """rows p and p + h ride one complex transform; a' = A + B -> parity 0, b' = (A - B) w^p -> parity 1"""
    ny, nx = x.shape
    h, nxh = ny // 2, nx // 2
    w = np.exp(-2j * np.pi * np.arange(ny) / ny)
    spec = np.full((2, nxh // ctw, h, ctw), np.nan + 0j)
    nyq = np.full(ny, np.nan)
    for p in range(h):
        z = np.fft.fft(x[p] + 1j * x[p + h])
        zr = np.conj(z[(-np.arange(nxh)) % nx])
        A, B = 0.5 * (z[:nxh] + zr), -0.5j * (z[:nxh] - zr)
        A[0], B[0] = z[0].real, z[0].imag
        nyq[p], nyq[p + h] = z[nxh].real, z[nxh].imag
        for k in range(nxh):
            spec[0, k // ctw, p, k % ctw] = A[k] + B[k]
            spec[1, k // ctw, p, k % ctw] = (A[k] - B[k]) * w[p]
    return spec, nyq


def _k2(spec, ny, nx, scale, remove_mean, psd, psd_hits):
    """per (parity, tile): h-point forward transform = F(2k + parity), PSD rows + mirrors, inverse of the power columns in
    pairs, rows 0 .. h/2 back in place"""
    h = ny // 2
    _, ntp, _, ctw = spec.shape
    out = np.full_like(spec, np.nan)
    for par in range(2):
        for ct in range(ntp):
            P = np.abs(np.fft.fft(spec[par, ct], axis=0)) ** 2
            for k in range(h):
                ky = 2 * k + par
                for c in range(ctw):
                    kx = ct * ctw + c
                    rd, rm = (ky + ny // 2) % ny, (ny // 2 - ky) % ny
                    psd[rd, nx // 2 + kx] = P[k, c] * scale
                    psd_hits[rd, nx // 2 + kx] += 1
                    if kx >= 1:
                        psd[rm, nx // 2 - kx] = P[k, c] * scale
                        psd_hits[rm, nx // 2 - kx] += 1
            if remove_mean and par == 0 and ct == 0:
                P[0, 0] = 0.0
            for c in range(0, ctw, 2):   # two real power columns per complex inverse transform
                V = np.fft.ifft(P[:, c] + 1j * P[:, c + 1]) * h
                Vr = np.conj(V[(-np.arange(h)) % h])
                Ga, Gb = 0.5 * (V + Vr), -0.5j * (V - Vr)
                out[par, ct, : h // 2 + 1, c] = Ga[: h // 2 + 1]
                out[par, ct, : h // 2 + 1, c + 1] = Gb[: h // 2 + 1]
    return out


def _k_nyq(nyq, ny, nx, scale, psd, psd_hits):
    P = np.abs(np.fft.fft(nyq)) ** 2
    for ky in range(ny):
        psd[(ky + ny // 2) % ny, 0] = P[ky] * scale
        psd_hits[(ky + ny // 2) % ny, 0] += 1
    return np.real(np.fft.ifft(P) * ny)


def _k3(g, gnyq, ny, nx):
    """transform y in [0, h/2]: Ga = E + conj(w^y) O = G(y), Gb = conj(E - conj(w^y) O) = G(h - y); each output row once"""
    h, nxh = ny // 2, nx // 2
    w = np.exp(-2j * np.pi * np.arange(ny) / ny)
    out = np.full((ny, nx), np.nan)
    hits = np.zeros(ny, dtype=int)
    ctw = g.shape[3]
    xs = np.arange(nx)
    c, cm = (xs + nx // 2) % nx, (nx // 2 - xs) % nx
    for y in range(h // 2 + 1):
        E = np.array([g[0, k // ctw, y, k % ctw] for k in range(nxh)])
        O = np.array([g[1, k // ctw, y, k % ctw] for k in range(nxh)])
        t = np.conj(w[y]) * O
        Ga, Gb = E + t, np.conj(E - t)
        Z = np.zeros(nx, dtype=complex)
        Z[:nxh] = Ga + 1j * Gb
        Z[0] = Ga[0].real + 1j * Gb[0].real
        Z[nxh] = gnyq[y] + 1j * gnyq[h - y]
        Z[nx - np.arange(1, nxh)] = np.conj(Ga[1:]) + 1j * np.conj(Gb[1:])
        z = np.fft.ifft(Z) * nx
        r0, r1 = z.real / (nx * ny), z.imag / (nx * ny)
        ya, yb = y, h - y
        out[(ya + h) % ny, c] = r0
        hits[(ya + h) % ny] += 1
        if 1 <= y:   # point mirror of row y: row -y (y = h/2 included: its mirror is row -h/2)
            out[(h - ya) % ny, cm] = r0
            hits[(h - ya) % ny] += 1
        if y < h // 2:   # y = h/2: Gb is the same row as Ga
            out[(yb + h) % ny, c] = r1
            hits[(yb + h) % ny] += 1
            if y >= 1:   # row h is its own mirror
                out[(h - yb) % ny, cm] = r1
                hits[(h - yb) % ny] += 1
    return out, hits


def _model(x, ctw, remove_mean):
    ny, nx = x.shape
    scale = 1.0 / (nx * ny)
    psd = np.full((ny, nx), np.nan)
    psd_hits = np.zeros((ny, nx), dtype=int)
    spec, nyq = _k1(x, ctw)
    assert not np.isnan(spec).any() and not np.isnan(nyq).any()
    g = _k2(spec, ny, nx, scale, remove_mean, psd, psd_hits)
    gnyq = _k_nyq(nyq, ny, nx, scale, psd, psd_hits)
    ac, hits = _k3(g, gnyq, ny, nx)
    return psd, psd_hits, ac, hits


def _reference(x, remove_mean):
    ny, nx = x.shape
    P = np.abs(np.fft.fft2(x)) ** 2
    psd = np.fft.fftshift(P) / (nx * ny)
    if remove_mean:
        P = P.copy()
        P[0, 0] = 0.0
    return psd, np.fft.fftshift(np.real(np.fft.ifft2(P)))


SHAPES = [(8, 4, 2), (8, 8, 2), (8, 8, 4), (16, 4, 2), (16, 16, 4), (16, 32, 16), (64, 8, 4), (64, 32, 8), (64, 32, 16),
          (2048, 64, 32), (2048, 64, 16)]


@pytest.mark.parametrize("remove_mean", [False, True])
@pytest.mark.parametrize("ny,nx,ctw", SHAPES)
def test_ysplit_model_matches_fft(ny, nx, ctw, remove_mean):
    rng = np.random.default_rng(ny * 131 + nx * 7 + ctw)
    x = rng.random((ny, nx)) + 0.25
    psd, psd_hits, ac, hits = _model(x, ctw, remove_mean)
    ref_p, ref_a = _reference(x, remove_mean)
    # every PSD element and every autocorrelation row is written exactly once
    assert np.all(psd_hits == 1), np.argwhere(psd_hits != 1)[:8]
    assert np.all(hits == 1), np.flatnonzero(hits != 1)[:8]
    assert not np.isnan(psd).any() and not np.isnan(ac).any()
    assert np.max(np.abs(psd - ref_p)) <= 1e-12 * np.max(np.abs(ref_p))
    assert np.max(np.abs(ac - ref_a)) <= 1e-12 * np.max(np.abs(ref_a))
    # zero lag (the first value of the y = 0 transform: what the C2R_PEAK pre-pass reads) lands at the centre
    assert int(np.argmax(ac)) == (ny // 2) * nx + nx // 2
