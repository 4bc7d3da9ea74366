"""Every FFT route bin by bin, on frames without a DC term.

The other transform tests compare normwise, max|got - ref| <= 1e-5 max|ref|, on frames with a large mean: there max|ref| is the DC
bin, 4e3 .. 2e4 times a typical |F| and 1e7 .. 3e8 times a typical PSD bin, so a wrong twiddle, two swapped bins or a PSD store one
column off all pass.  Here the same metric and the same bar run on frames whose largest bin is a typical bin:

  noise0, noise1   white noise, float64 mean removed: max|F| / rms|F| ~ 3.3, max P / median P ~ 16, DC ~ 1e-6 of the maximum
  imp00, imp11,    one 1.0 at (0, 0), (1, 1), (ny - 1, nx // 2 + 1): |F| = 1 in every bin and a phase that no two bins share
  impedge          (closed form exp(-2 pi i (ky y0 / ny + kx x0 / nx)))
  marker           cosines of amplitudes 1..7 at the axis, Nyquist and near-Nyquist bins: a dozen bins hold all the power
  rowconst         x[y, :] = g[y]: all the power in the kx = 0 column
  colconst         x[:, x] = h[x]: all the power in the ky = 0 row

Eight frames go through one *_stack call (the frame-per-XCD tile order of the power-of-two column pass); the prefixes [:1] and [:3]
(the other order) must give the same bits.  The reference is the float64 oracle of the float32 frame.  Every deviation goes through
observe() as bins.<route>.<ny>x<nx>.<entry>.<frame kind> with the bar TOL; the float32 NumPy transform of the same frame is printed
next to it.  ROUTES names, per shape, the flag bits b4d_size_route must report: the thinnest frame that runs each kernel instantiation.

This module imports without a GPU: tests/test_spectrum_bins_host.py runs its frame builder and checker on the CPU.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5   # the project's bar for float32 transforms against the float64 oracle

# B4D_ROUTE_* of include/b4d.h (the host test holds these against the header)
POW2, PARITY, WMR, FUSED, DFTMAT, PMROWS, BLUESTEIN_Y, BLUESTEIN_X = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80

KINDS = ("noise0", "noise1", "imp00", "imp11", "impedge", "marker", "rowconst", "colconst")
OPTION_DEFAULTS = {"ysplit": 1, "row16": 1, "colsets": 1}

# the lengths of B4D_WMR_LENGTHS (csrc/b4d_wiener_mr.hip), a literal copy: the host test holds it against the source
WMR_LENGTHS = (4104, 4096, 3840, 3648, 3200, 3072, 3000, 2592, 2560, 2448, 2400, 2304, 2160, 2048, 1944, 1936, 1920, 1600, 1536, 1440,
               1280, 1216, 1200, 1080, 1024, 1000, 960, 800, 768, 720, 640, 600, 576, 540, 520, 512, 480, 264, 228, 171, 170)
# the lengths test_fused_transform_factorisations names, one per small-DFT variant of the fused row transform
FUSED_LENGTHS = (1072, 536, 1197, 640, 1540, 1326, 8192, 3024, 2056)


def _routes():
    """(route name, shape, expected b4d_size_route, options, frame kinds)"""
    out = []
    for ny in (64, 128, 256, 512, 1024, 4096):    # every column instantiation ((2048, 64): the parity cases below)
        out.append(("pow2", (ny, 64), POW2, {}, KINDS))
    for nx in (128, 256, 512, 1024, 2048, 4096):  # every row instantiation
        out.append(("pow2", (64, nx), POW2, {}, KINDS))
    for shape in ((2048, 64), (2048, 128)):
        for name, opts in (("parity_ysplit0", {"ysplit": 0}), ("parity_row16_0", {"ysplit": 1, "row16": 0}),
                           ("parity_colsets0", {"row16": 1, "colsets": 0}), ("parity", {})):
            out.append((name, shape, POW2 | PARITY, opts, KINDS))
    out.append(("parity", (2048, 2048), POW2 | PARITY, {}, ("noise0", "marker", "imp11")))   # the benchmark's own instantiations
    out.append(("parity", (2048, 4096), POW2 | PARITY, {}, ("noise0", "marker")))            # the one nx without column sets
    for shape in ((2, 3), (33, 45), (97, 512), (512, 101), (227, 227)):
        out.append(("dftmat", shape, DFTMAT, {}, KINDS))
    for shape in ((228, 228), (171, 170), (170, 228), (228, 171)):   # (the last: 171 as a row length too)
        out.append(("wmr", shape, WMR, {}, KINDS))
    for L in WMR_LENGTHS:
        if L not in (228, 171, 170):
            out.append(("wmr", (L, 170), WMR, {}, KINDS))
            out.append(("wmr", (171, L), WMR, {}, KINDS))
    for L in FUSED_LENGTHS:
        out.append(("fused", (6, L), FUSED, {}, KINDS))
        out.append(("fused", (L, 5), FUSED, {}, KINDS))
    out.append(("bluestein", (1042, 6), PMROWS | BLUESTEIN_Y, {}, KINDS))
    out.append(("bluestein", (5, 1031), PMROWS | BLUESTEIN_X, {}, KINDS))
    out.append(("bluestein", (4093, 6), PMROWS | BLUESTEIN_Y, {}, KINDS))
    out.append(("bluestein", (1042, 1031), PMROWS | BLUESTEIN_Y | BLUESTEIN_X, {}, KINDS))
    return out


ROUTES = _routes()
# complex frames run the engines of b4d_plan_create_general, one shape per branch of its 2-D transform: DFT matrices (a power-of-two
# size as well, and a mixed-radix plan, which keeps its matrices for these entry points) and row transforms per axis, fused and
# Bluestein.  The flags are those of the real-input plan of the shape.
C2C_ROUTES = [((64, 64), POW2), ((97, 512), DFTMAT), ((228, 228), WMR), ((6, 1072), FUSED), ((1042, 6), PMROWS | BLUESTEIN_Y)]


def case_id(case):
    name, (ny, nx) = case[0], case[1]
    return f"{name}-{ny}x{nx}"


# ------------------------------------------------------------------------------------------------------------------ the frames
def marker_bins(shape, hermitian=True):
    """[(ky, kx, amplitude)] of the marker frame: (0, 1), (1, 0), the three Nyquist bins and two bins next to the Nyquist corner,
    amplitudes 1..7 in that order.  Nyquist markers of an odd side are dropped, indices are reduced modulo the side, the DC bin and
    repeats (for a real frame: of a bin or of its mirror) are dropped, so that tiny sides keep distinct bins."""
    ny, nx = shape
    want = [(0, 1, True), (1, 0, True), (ny // 2, 0, ny % 2 == 0), (0, nx // 2, nx % 2 == 0),
            (ny // 2, nx // 2, ny % 2 == 0 and nx % 2 == 0), (ny // 2 - 1, nx // 2 - 1, True), (-(ny // 2 - 1), nx // 2 - 1, True)]
    seen, out = {(0, 0)}, []
    for amp, (ky, kx, keep) in enumerate(want, start=1):
        k = (ky % ny, kx % nx)
        mirror = ((-ky) % ny, (-kx) % nx)
        if not keep or k in seen or (hermitian and mirror in seen):
            continue
        seen.add(k)
        out.append((k[0], k[1], float(amp)))
    return out


def _phase(shape, ky, kx):
    """2 pi (ky y / ny + kx x / nx) on the pixel grid, reduced in integers first"""
    ny, nx = shape
    y, x = np.arange(ny)[:, None], np.arange(nx)[None, :]
    return 2.0 * np.pi * (((ky * y) % ny) / ny + ((kx * x) % nx) / nx)


def impulse_site(shape, kind):
    ny, nx = shape
    return {"imp00": (0, 0), "imp11": (1, 1), "impedge": (ny - 1, nx // 2 + 1)}[kind]


def build_frame(shape, kind):
    """one float32 frame of `shape`; the noise is seeded by the shape and the kind alone"""
    ny, nx = shape
    rng = np.random.default_rng([ny, nx, KINDS.index(kind)])
    if kind.startswith("noise"):
        x = rng.standard_normal(shape)
        x -= x.mean()
    elif kind.startswith("imp"):
        x = np.zeros(shape)
        x[impulse_site(shape, kind)] = 1.0
    elif kind == "marker":
        x = np.zeros(shape)
        for ky, kx, amp in marker_bins(shape):
            x += amp * np.cos(_phase(shape, ky, kx))
    elif kind == "rowconst":
        g = rng.standard_normal(ny)
        x = np.repeat((g - g.mean())[:, None], nx, axis=1)
    elif kind == "colconst":
        h = rng.standard_normal(nx)
        x = np.repeat((h - h.mean())[None, :], ny, axis=0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def build_stack(shape, kinds=KINDS):
    st = np.stack([build_frame(shape, k) for k in kinds])
    st.setflags(write=False)
    return st


def build_complex_frame(shape):
    """zero-mean complex normal plus complex markers: each sits in ONE bin, which no real frame can give"""
    ny, nx = shape
    rng = np.random.default_rng([ny, nx, 99])
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    z -= z.mean()
    for ky, kx, amp in marker_bins(shape, hermitian=False):
        z += amp * np.exp(1j * _phase(shape, ky, kx))
    return z.astype(np.complex64)


# ------------------------------------------------------------------------------------------------------------------- the check
def nerr(got, ref):
    return float(np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref)))


def impulse_spectrum(shape, kind):
    """the exact shifted spectrum of an impulse frame"""
    ny, nx = shape
    y0, x0 = impulse_site(shape, kind)
    ky = np.fft.fftshift(np.arange(ny))[:, None]
    kx = np.fft.fftshift(np.arange(nx))[None, :]
    return np.exp(-2j * np.pi * (((ky * y0) % ny) / ny + ((kx * x0) % nx) / nx))


def reference(frame):
    """float64 oracle of a float32 frame: shifted spectrum, unscaled PSD, PSD with the default scale"""
    from oracle import signal_np as S

    x = np.asarray(frame, dtype=np.float64)
    ny, nx = x.shape
    raw = S.psd2d(x, scale=False)[0]
    # S.psd2d(x) is the same transform times (dx dy) / (nx ny) with unit steps: not computed a third time (the host test holds
    # this line against the oracle)
    return {"fft": S.fft2d(x)[0], "psd_raw": raw, "psd": raw * ((1.0 * 1.0) / (float(nx) * float(ny)))}


def float32_transform(frame):
    """the same three outputs from NumPy's float32 transform: the figure recorded next to every observed deviation"""
    from oracle import signal_np as S

    F = S.fft2d(np.asarray(frame, dtype=np.float32))[0]
    assert F.dtype == np.complex64
    P = (F.real * F.real + F.imag * F.imag).astype(np.float32)
    ny, nx = frame.shape
    return {"fft": F, "psd_raw": P, "psd": P * np.float32(1.0 / (float(nx) * float(ny)))}


def _bins_above(mag, ref_max):
    return set(map(tuple, np.argwhere(mag > 1e-3 * ref_max)))


def check_frame(kind, frame, got, ref=None, record=None):
    """Hold the outputs `got` ({"fft" | "psd_raw" | "psd": array} of ONE frame) against the oracle, every bin, nothing masked.

    Every figure is a deviation relative to the largest reference bin and goes to record(entry, value); without a recorder the
    bar TOL is asserted here.  Raises AssertionError on the first miss."""
    ref = ref or reference(frame)
    shape = frame.shape
    ny, nx = shape

    def rec(entry, value):
        if record is not None:
            record(entry, value)
        else:
            assert value <= TOL, f"{kind} {shape} {entry}: {value:.3e} > {TOL:.0e}"

    for entry in ("fft", "psd_raw", "psd"):
        if entry not in got:
            continue
        g, r = np.asarray(got[entry]), ref[entry]
        assert g.shape == r.shape and np.isfinite(g).all(), (kind, entry)
        rmax = float(np.max(np.abs(r)))
        rec(entry, nerr(g, r))
        if kind.startswith("imp"):
            if entry == "fft":
                rec("fft_closed", nerr(g, impulse_spectrum(shape, kind)))
            elif entry == "psd_raw":
                rec("psd_raw_unit", float(np.max(np.abs(g.astype(np.float64) - 1.0))))
        elif kind == "marker":
            have, want = _bins_above(np.abs(g), rmax), _bins_above(np.abs(r), rmax)
            assert have == want, f"{kind} {shape} {entry}: bins above 1e-3 of the maximum: extra {sorted(have - want)[:8]}, " \
                                 f"missing {sorted(want - have)[:8]}"
        elif kind in ("rowconst", "colconst"):
            off = np.abs(g).astype(np.float64)
            if kind == "rowconst":
                off[:, nx // 2] = 0.0     # the kx = 0 column of the shifted spectrum
            else:
                off[ny // 2, :] = 0.0     # the ky = 0 row
            rec(entry + "_off", float(off.max()) / rmax)


# ---------------------------------------------------------------------------------------------------------------- the GPU tests
@pytest.fixture(scope="module")
def gs():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from barc4dip_amd import _ffi, signal

    lib = _ffi.load_library()
    assert lib.b4d_missing_symbols == ()
    return signal


class options:
    """with options({...}): the calls inside take these b4d_set_option values; the defaults are back on the way out"""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        import barc4dip_amd

        for k, v in self.opts.items():
            barc4dip_amd.set_option(k, v)

    def __exit__(self, *exc):
        import barc4dip_amd

        for k, v in OPTION_DEFAULTS.items():
            barc4dip_amd.set_option(k, v)
        return False


class Recorder:
    """prints every figure with its float32 CPU counterpart, hands it to observe(), and keeps the misses for one assertion at the end"""

    def __init__(self, observe, prefix):
        self.observe, self.prefix, self.misses = observe, prefix, []

    def __call__(self, name, value, cpu32=None):
        full = f"{self.prefix}.{name}"
        print(f"{full}: {value:.3e}" + ("" if cpu32 is None else f"   (float32 NumPy: {cpu32:.3e})"))
        try:
            self.observe(full, value, TOL)
        except AssertionError as e:
            self.misses.append(str(e))


def size_route(ny, nx):
    from barc4dip_amd import _ffi

    return int(_ffi.load_library().b4d_size_route(int(ny), int(nx)))


@pytest.mark.parametrize("case", ROUTES, ids=case_id)
def test_bins_vs_oracle(gs, observe, case):
    from barc4dip_amd.signal.fft import fft2d_stack, psd2d_stack

    route, shape, flags, opts, kinds = case
    ny, nx = shape
    assert size_route(ny, nx) == flags, f"{shape}: b4d_size_route reports {size_route(ny, nx):#x}, the table expects {flags:#x}"
    stack = build_stack(shape, kinds)
    with options(opts):
        got = {"fft": fft2d_stack(stack), "psd_raw": psd2d_stack(stack, scale=False), "psd": psd2d_stack(stack)}
        joint_psd, ac = gs.psd_autocorr2d_stack(stack)
        # the shared column pass drops rows when an autocorrelation is asked for: the PSD must not notice
        np.testing.assert_array_equal(joint_psd, got["psd"])
        assert np.isfinite(ac).all()
        for n in (1, 3):    # the other tile order of the column pass, other launch groups: the same bits
            if n >= len(kinds):
                continue
            np.testing.assert_array_equal(fft2d_stack(stack[:n]), got["fft"][:n])
            np.testing.assert_array_equal(psd2d_stack(stack[:n], scale=False), got["psd_raw"][:n])
            np.testing.assert_array_equal(psd2d_stack(stack[:n]), got["psd"][:n])
            p, a = gs.psd_autocorr2d_stack(stack[:n])
            np.testing.assert_array_equal(p, got["psd"][:n])
            np.testing.assert_array_equal(a, ac[:n])
    rec = Recorder(observe, f"bins.{route}.{ny}x{nx}")
    for t, kind in enumerate(kinds):
        ref = reference(stack[t])
        f32 = float32_transform(stack[t])
        cpu = {e: nerr(f32[e], ref[e]) for e in ref}
        check_frame(kind, stack[t], {e: got[e][t] for e in got}, ref=ref,
                    record=lambda entry, v, kind=kind, cpu=cpu: rec(f"{entry}.{kind}", v, cpu.get(entry)))
    assert rec.misses == [], "\n".join(rec.misses)


@pytest.mark.parametrize("shape,flags", C2C_ROUTES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else None)
def test_complex_bins_vs_oracle(gs, observe, shape, flags):
    """fft2d of a complex frame and ifft2d, each against the oracle (not only as a round trip)"""
    from oracle import signal_np as S

    ny, nx = shape
    assert size_route(ny, nx) == flags
    z = build_complex_frame(shape)
    Fr = S.fft2d(z.astype(np.complex128))[0]
    assert len(_bins_above(np.abs(Fr), float(np.abs(Fr).max()))) >= len(marker_bins(shape, hermitian=False))
    rec = Recorder(observe, f"bins.c2c.{ny}x{nx}")
    F = gs.fft2d(z)[0]
    assert F.dtype == np.complex64 and F.shape == shape
    rec("fft2d.noise+marker", nerr(F, Fr), nerr(S.fft2d(z)[0], Fr))
    W = Fr.astype(np.complex64)                     # a shifted spectrum as the caller would hold it
    zr = S.ifft2d(W.astype(np.complex128))
    back = gs.fft.ifft2d(W)
    assert back.dtype == np.complex64 and back.shape == shape
    rec("ifft2d.noise+marker", nerr(back, zr), nerr(S.ifft2d(W), zr))
    assert rec.misses == [], "\n".join(rec.misses)
