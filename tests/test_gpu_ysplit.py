"""The "ysplit" route of the PSD + autocorrelation pipeline (2048-row frames: one radix-2 stage of the column transform is done
by the row passes, the column pass works on parity tiles -- b4d_fft2d.hpp) against the float64 oracle, next to the full-column
route on the same inputs.

The route depends on ny alone, so thin frames exercise every index map: (2048, 64) is one 32-column tile per parity, (2048, 128)
two tiles, with the PSD mirror straggler of the second crossing into the first.  Batches 1 and 3 take the per-XCD tile ranges of
the column pass, batch 8 the frame-per-XCD mapping."""
import numpy as np
import pytest

from barc4dip_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-5            # the project's bar for float32 transforms against the float64 oracle
YSPLIT_DEFAULT = 1    # what the library ships with ("ysplit" of b4d_set_option)
SHAPES = [(2048, 64), (2048, 128)]
BATCHES = [1, 3, 8]


def nerr(got, ref):
    return float(np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def gs():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from barc4dip_amd import _ffi, signal

    lib = _ffi.load_library()
    assert lib.b4d_missing_symbols == ()
    return signal


class route:
    """with route(v): calls inside take "ysplit" = v; the default is restored on the way out"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        import barc4dip_amd

        barc4dip_amd.set_option("ysplit", self.v)

    def __exit__(self, *exc):
        import barc4dip_amd

        barc4dip_amd.set_option("ysplit", YSPLIT_DEFAULT)
        return False


_FRAMES, _REFS = {}, {}


def frames_of(shape):
    """8 frames per shape, computed once and never modified (every batch is a prefix)"""
    if shape not in _FRAMES:
        ny, nx = shape
        st = np.stack([np.ascontiguousarray(synth.speckle_frame(ny, 4321 + 17 * t)[:, :nx]) for t in range(max(BATCHES))]).astype(np.float32)
        st.setflags(write=False)
        _FRAMES[shape] = st
    return _FRAMES[shape]


def reference(shape, t, rm, nm):
    """float64 oracle of frame t: (psd, autocorrelation), shared by every test that needs it"""
    from oracle import signal_np as S

    key = (shape, t, rm, nm)
    if key not in _REFS:
        x = frames_of(shape)[t].astype(np.float64)
        if ("psd", shape, t) not in _REFS:
            _REFS[("psd", shape, t)] = S.psd2d(x)[0]
        _REFS[key] = (_REFS[("psd", shape, t)], S.autocorr2d(x, remove_mean=rm, normalize=nm)[0])
    return _REFS[key]


def mirror(a):
    return np.roll(a[:, ::-1, ::-1], (1, 1), axis=(1, 2))


def check_against_oracle(psd, ac, shape, rm, nm, tag):
    ny, nx = shape
    for t in range(psd.shape[0]):
        rp, ra = reference(shape, t, rm, nm)
        ep, ea = nerr(psd[t], rp), nerr(ac[t], ra)
        print(f"{tag} {shape} frame {t} rm={rm} nm={nm}: psd nerr {ep:.3e}  autocorr nerr {ea:.3e}")
        assert ep < TOL and ea < TOL, (tag, t, ep, ea)
        if nm == "peak":
            assert ac[t, ny // 2, nx // 2] == 1.0
        assert int(np.argmax(ac[t])) == (ny // 2) * nx + nx // 2


@pytest.mark.parametrize("nm", ["peak", "none"])
@pytest.mark.parametrize("rm", [True, False])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_ysplit_psd_autocorr_vs_oracle(gs, shape, batch, rm, nm):
    ny, nx = shape
    st = frames_of(shape)[:batch]
    with route(1):
        psd, ac = gs.psd_autocorr2d_stack(st, remove_mean=rm, normalize=nm)
        # stack call == per-frame calls, bit for bit (first and last frame: the other batch sizes cover the rest)
        singles = [gs.psd_autocorr2d_stack(st[t:t + 1], remove_mean=rm, normalize=nm) for t in sorted({0, batch - 1})]
    assert psd.dtype == np.float32 and ac.dtype == np.float32 and psd.shape == (batch, ny, nx)
    check_against_oracle(psd, ac, shape, rm, nm, "ysplit=1")
    for t, (p1, a1) in zip(sorted({0, batch - 1}), singles):
        np.testing.assert_array_equal(p1[0], psd[t])
        np.testing.assert_array_equal(a1[0], ac[t])
    # the Hermitian mirror of the PSD is the SAME value stored twice; columns kx = 0 and kx = nx/2 come from transforms of their own
    mp = mirror(psd)
    keep = np.ones(nx, dtype=bool)
    keep[0] = keep[nx // 2] = False
    np.testing.assert_array_equal(mp[:, 1:][:, :, keep], psd[:, 1:][:, :, keep])
    assert float(np.max(np.abs(mirror(ac) - ac))) < 2e-6 * max(1.0, float(np.max(np.abs(ac))))
    # the full-column route on the same inputs meets the same bar
    with route(0):
        psd0, ac0 = gs.psd_autocorr2d_stack(st, remove_mean=rm, normalize=nm)
    check_against_oracle(psd0, ac0, shape, rm, nm, "ysplit=0")


@pytest.mark.parametrize("shape", SHAPES)
def test_ysplit_psd_only_and_autocorr_only(gs, shape):
    from barc4dip_amd.signal.corr import autocorr2d_stack
    from barc4dip_amd.signal.fft import psd2d_stack

    st = frames_of(shape)[:3]
    for v in (1, 0):
        with route(v):
            psd = psd2d_stack(st)
            ac = autocorr2d_stack(st)
            both = gs.psd_autocorr2d_stack(st)
        check_against_oracle(psd, ac, shape, True, "peak", f"ysplit={v} single-output calls")
        np.testing.assert_array_equal(psd, both[0])
        np.testing.assert_array_equal(ac, both[1])


def test_ysplit_constant_frame_stays_zero(gs):
    """a constant frame has no power left once the mean is removed: the autocorrelation is 0 everywhere, not NaN and not 1"""
    st = np.full((1, 2048, 64), 3.5, dtype=np.float32)
    for v in (1, 0):
        with route(v):
            psd, ac = gs.psd_autocorr2d_stack(st)
        assert np.all(ac == 0.0), v
        assert np.isfinite(psd).all()
        assert psd[0, 1024, 32] == pytest.approx(3.5 ** 2 * 2048 * 64, rel=1e-6)
        psd[0, 1024, 32] = 0.0
        assert np.all(psd == 0.0), v
