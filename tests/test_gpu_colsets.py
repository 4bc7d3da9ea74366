"""The "colsets" option of the parity-tile route (2048-row frames): between the forward row pass and the column pass a tile holds
rows n and n + 512 of ONE column in every 16 bytes ([n][e][cp][h]), so that the column pass has its first register set
complete after half of its loads (b4d_fft2d.hpp).  Only the placement of the data in the workspace and the order of independent
work change, so every output must equal the plain tiles' bit for bit; the launchers fall back as they do for "row16" when the
caller's pointers are not 16-byte aligned.

The route depends on ny alone: (2048, 64) is four lanes per transform (sixteen couples of transforms in two waves) and one 32-column
tile per parity, (2048, 128) two tiles, (2048, 2048) the benchmark's own instantiations of both kernels."""
import ctypes as C

import numpy as np
import pytest

from barc4dip_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-5             # the project's bar for float32 transforms against the float64 oracle
COLSETS_DEFAULT = 1    # what the library ships with ("colsets" of b4d_set_option)
THIN = [(2048, 64), (2048, 128)]
BATCHES = [1, 3, 8]    # 8: the XCD-interleaved tile order of the column pass; 1 and 3: the other
COMBOS = [(True, "peak"), (True, "none"), (False, "peak"), (False, "none")]


@pytest.fixture(scope="module")
def gs():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from barc4dip_amd import _ffi, signal

    lib = _ffi.load_library()
    assert lib.b4d_missing_symbols == ()
    return signal


class colsets:
    """with colsets(v): calls inside take "colsets" = v; the default is restored on the way out"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        import barc4dip_amd

        barc4dip_amd.set_option("colsets", self.v)

    def __exit__(self, *exc):
        import barc4dip_amd

        barc4dip_amd.set_option("colsets", COLSETS_DEFAULT)
        return False


_FRAMES = {}
_PLAIN = {}


def frames_of(shape):
    """the frames of a shape, computed once and never modified (every batch is a prefix)"""
    if shape not in _FRAMES:
        ny, nx = shape
        n = 3 if nx == 2048 else max(BATCHES)
        st = np.stack([np.ascontiguousarray(synth.speckle_frame(ny, 1543 + 7 * t)[:, :nx]) for t in range(n)]).astype(np.float32)
        st.setflags(write=False)
        _FRAMES[shape] = st
    return _FRAMES[shape]


def plain(gs, shape, batch, rm, nm):
    """PSD and autocorrelation through the plain tiles ("colsets" = 0), computed once per case"""
    key = (shape, batch, rm, nm)
    if key not in _PLAIN:
        with colsets(0):
            p, a = gs.psd_autocorr2d_stack(frames_of(shape)[:batch], remove_mean=rm, normalize=nm)
        p.setflags(write=False)
        a.setflags(write=False)
        _PLAIN[key] = (p, a)
    return _PLAIN[key]


@pytest.mark.parametrize("rm,nm", COMBOS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shape", THIN)
def test_colsets_equals_plain_thin(gs, shape, batch, rm, nm):
    p0, a0 = plain(gs, shape, batch, rm, nm)
    with colsets(1):
        p1, a1 = gs.psd_autocorr2d_stack(frames_of(shape)[:batch], remove_mean=rm, normalize=nm)
    assert np.isfinite(p1).all() and np.isfinite(a1).all()
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(a1, a0)


@pytest.mark.parametrize("rm,nm", COMBOS)
def test_colsets_equals_plain_2048(gs, rm, nm):
    shape = (2048, 2048)
    p0, a0 = plain(gs, shape, 3, rm, nm)
    with colsets(1):
        p1, a1 = gs.psd_autocorr2d_stack(frames_of(shape), remove_mean=rm, normalize=nm)
    assert np.isfinite(p1).all() and np.isfinite(a1).all()
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(a1, a0)


@pytest.mark.parametrize("shape", THIN)
def test_colsets_single_output_calls(gs, shape):
    """PSD only (the inverse row pass does not run, the column pass keeps every row) and autocorrelation only equal the joint call"""
    from barc4dip_amd.signal.corr import autocorr2d_stack
    from barc4dip_amd.signal.fft import psd2d_stack

    st = frames_of(shape)[:3]
    with colsets(1):
        psd = psd2d_stack(st)
        ac = autocorr2d_stack(st)
        both = gs.psd_autocorr2d_stack(st)
    np.testing.assert_array_equal(psd, both[0])
    np.testing.assert_array_equal(ac, both[1])


def test_colsets_vs_oracle(gs):
    from oracle import signal_np as S

    shape = (2048, 128)
    ny, nx = shape
    st = frames_of(shape)[:3]
    with colsets(1):
        psd, ac = gs.psd_autocorr2d_stack(st)
    for t in range(3):
        x = st[t].astype(np.float64)
        rp, ra = S.psd2d(x)[0], S.autocorr2d(x, remove_mean=True, normalize="peak")[0]
        ep = float(np.max(np.abs(psd[t] - rp)) / np.max(np.abs(rp)))
        ea = float(np.max(np.abs(ac[t] - ra)) / np.max(np.abs(ra)))
        print(f"colsets=1 {shape} frame {t}: psd nerr {ep:.3e}  autocorr nerr {ea:.3e}")
        assert ep < TOL and ea < TOL, (t, ep, ea)
        assert ac[t, ny // 2, nx // 2] == 1.0
        assert int(np.argmax(ac[t])) == (ny // 2) * nx + nx // 2


def test_colsets_constant_frame_stays_zero(gs):
    """a constant frame has no power left once the mean is removed: the autocorrelation is 0 everywhere, not NaN and not 1"""
    st = np.full((1, 2048, 64), 3.5, dtype=np.float32)
    with colsets(1):
        psd, ac = gs.psd_autocorr2d_stack(st)
    assert not np.isnan(ac).any()
    assert np.all(ac == 0.0)
    assert np.isfinite(psd).all()


def test_colsets_misaligned_pointers_give_the_same_bits():
    """frames, PSD and autocorrelation one float into a larger device buffer (4-byte alignment is all the C ABI asks for), in all
    eight combinations: the launchers route such calls as they do for "row16", and the results do not depend on it"""
    import torch

    from barc4dip_amd import _ffi

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    shape, batch = (2048, 64), 3
    ny, nx = shape
    n = batch * ny * nx
    lib = _ffi.lib()
    plan = _ffi.Plan(ny, nx, 8)
    src = torch.from_numpy(np.array(frames_of(shape)[:batch]).reshape(-1)).cuda()
    flags = _ffi.REMOVE_MEAN | _ffi.NORM_PEAK
    results = {}
    try:
        for cs, cases in ((0, [(0, 0, 0)]), (1, [(i, p, a) for i in (0, 1) for p in (0, 1) for a in (0, 1)])):
            with colsets(cs):
                for mis in cases:
                    bufs = [torch.zeros(n + 8, dtype=torch.float32, device="cuda") for _ in range(3)]
                    assert all(b.data_ptr() % 16 == 0 for b in bufs)
                    fin, psd, ac = (b[m:m + n] for b, m in zip(bufs, mis))
                    assert [v.data_ptr() % 16 for v in (fin, psd, ac)] == [4 * m for m in mis]
                    fin.copy_(src)
                    _ffi.check(lib.b4d_psd_autocorr2d(plan.handle, C.c_void_p(fin.data_ptr()), batch, C.c_void_p(psd.data_ptr()),
                                                      1.0 / (ny * nx), C.c_void_p(ac.data_ptr()), flags, _ffi.stream_ptr()))
                    torch.cuda.synchronize()
                    results[(cs,) + mis] = (psd.cpu().numpy(), ac.cpu().numpy())
                    # nothing outside the views was written
                    for b, m in zip(bufs[1:], mis[1:]):
                        assert float(b[:m].abs().sum()) == 0.0 and float(b[m + n:].abs().sum()) == 0.0
    finally:
        plan.close()
    p0, a0 = results[(0, 0, 0, 0)]
    assert np.isfinite(p0).all() and np.isfinite(a0).all() and a0.reshape(batch, ny, nx)[0, ny // 2, nx // 2] == 1.0
    for key, (p, a) in results.items():
        np.testing.assert_array_equal(p, p0, err_msg=str(key))
        np.testing.assert_array_equal(a, a0, err_msg=str(key))
