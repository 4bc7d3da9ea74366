"""The column pass on column-set tiles ("colsets" = 1, 2048-row frames) at every grid shape it decodes: it streams the direct half of
the PSD past L2 and takes the twiddles of its INVERSE transform from the two tables that the forward transform left in LDS
(b4d_fft2d.hpp, DESIGN.md §8.1 "colpf").  Both are routes only: the products are those of the plain tiles' kernel ("colsets" = 0,
twiddles from memory, cached stores), so PSD and autocorrelation must be equal bit for bit.

Plans are made with chunk = batch, so one launch fills the workspace to its last tile, and the calls go through the C ABI.  Batches
8 and 16 take the XCD-interleaved tile order of the column pass, 1, 3 and 9 the other; (2048, 64) is one tile per parity,
(2048, 128) two.  tests/test_gpu_colsets.py holds the (2048, 2048) case, the single-output calls and the misaligned pointers."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5             # the project's bar for float32 transforms against the float64 oracle
COLSETS_DEFAULT = 1    # what the library ships with ("colsets" of b4d_set_option)
SHAPES = [(2048, 64), (2048, 128)]
BATCHES = [1, 3, 8, 9, 16]
NMAX = max(BATCHES)

_FRAMES = {}
_OUT = {}


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


def frames_of(shape):
    """sixteen frames of a shape with a mean well above their spread, made once and never modified (every batch is a prefix)"""
    if shape not in _FRAMES:
        ny, nx = shape
        rng = np.random.default_rng(2048 + nx)
        st = (0.5 + rng.random((NMAX, ny, nx), dtype=np.float32)).astype(np.float32)
        st *= rng.random((NMAX, 1, 1), dtype=np.float32) + 0.5   # every frame its own level
        st.setflags(write=False)
        _FRAMES[shape] = st
    return _FRAMES[shape]


def run(shape, batch, flags, cs):
    """(psd, autocorr) of the first `batch` frames through b4d_psd_autocorr2d on a plan of exactly that chunk; once per case"""
    import torch

    from barc4dip_amd import _ffi

    key = (shape, batch, flags, cs)
    if key not in _OUT:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        ny, nx = shape
        lib = _ffi.lib()
        src = torch.from_numpy(np.array(frames_of(shape)[:batch])).cuda()
        psd = torch.full_like(src, float("nan"))
        ac = torch.full_like(src, float("nan"))
        plan = _ffi.Plan(ny, nx, batch)
        try:
            with colsets(cs):
                _ffi.check(lib.b4d_psd_autocorr2d(plan.handle, C.c_void_p(src.data_ptr()), batch, C.c_void_p(psd.data_ptr()),
                                                  1.0 / (ny * nx), C.c_void_p(ac.data_ptr()), flags, _ffi.stream_ptr()))
                torch.cuda.synchronize()
        finally:
            plan.close()
        p, a = psd.cpu().numpy(), ac.cpu().numpy()
        p.setflags(write=False)
        a.setflags(write=False)
        _OUT[key] = (p, a)
    return _OUT[key]


def flag_sets():
    from barc4dip_amd import _ffi

    return {"mean+peak": _ffi.REMOVE_MEAN | _ffi.NORM_PEAK, "none": 0}


@pytest.mark.parametrize("fl", ["mean+peak", "none"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_column_sets_equal_plain_tiles_at_every_grid(shape, batch, fl):
    flags = flag_sets()[fl]
    p0, a0 = run(shape, batch, flags, 0)
    p1, a1 = run(shape, batch, flags, 1)
    assert np.isfinite(p1).all() and np.isfinite(a1).all()   # every element written (the buffers start as NaN)
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(a1, a0)


@pytest.mark.parametrize("shape,batch,frame", [((2048, 64), 9, 8), ((2048, 128), 16, 15)])
def test_last_frame_of_a_batch_against_the_oracle(shape, batch, frame):
    """the last tiles of the launch: the ninth frame of nine (per-XCD tile ranges) and the sixteenth of sixteen (interleaved frames)"""
    from oracle import signal_np as S

    ny, nx = shape
    psd, ac = run(shape, batch, flag_sets()["mean+peak"], 1)
    x = frames_of(shape)[frame].astype(np.float64)
    rp, ra = S.psd2d(x)[0], S.autocorr2d(x, remove_mean=True, normalize="peak")[0]
    ep = float(np.max(np.abs(psd[frame] - rp)) / np.max(np.abs(rp)))
    ea = float(np.max(np.abs(ac[frame] - ra)) / np.max(np.abs(ra)))
    print(f"{shape} batch {batch} frame {frame}: psd nerr {ep:.3e}  autocorr nerr {ea:.3e}")
    assert ep < TOL and ea < TOL, (ep, ea)
    assert ac[frame, ny // 2, nx // 2] == 1.0
    assert int(np.argmax(ac[frame])) == (ny // 2) * nx + nx // 2
