"""CPU tier: the two dtype rules of the upload (_device.result_dtype, _device.staged_code) over every real NumPy dtype in both
byte orders, against NumPy's own FFT promotion; and the reference's own invariance to byte order, which the GPU tier's
representation tests (test_gpu_input_layouts.py) hold this library to."""
import importlib
import warnings

import numpy as np
import pytest

from barc4dip_amd import _device as D
from barc4dip_amd.signal import fft as F

# every numeric NumPy type code: bool, the integers, the floats and the complex types (long double included)
CODES = "?" + np.typecodes["AllInteger"] + np.typecodes["AllFloat"]
# b4d_to_f32's source codes by (kind, item size), restated from include/b4d.h
TO_F32_CODES = {("u", 1): 0, ("u", 2): 1, ("i", 2): 2, ("i", 4): 3, ("u", 4): 4, ("f", 4): 5, ("f", 8): 6}


def _dtypes():
    for c in CODES:
        for order in "<>":
            yield np.dtype(c).newbyteorder(order)


def _is_longdouble(dt):
    return dt.type in (np.longdouble, np.clongdouble) and np.dtype(np.longdouble).itemsize > 8


@pytest.mark.parametrize("dt", list(_dtypes()), ids=lambda d: d.str)
def test_result_dtype_follows_numpy_fft_promotion(dt):
    """The output dtype follows np.fft.fft2(x).real.dtype whatever the byte order.  The one deliberate exception is long
    double (float128 / complex256), where NumPy keeps long double and this library returns float64: the device computes in
    float32 and has no long double type."""
    x = np.zeros((2, 2), dt)
    want = np.fft.fft2(x).real.dtype
    got = D.result_dtype(x)
    assert got in (np.float32, np.float64)          # callers compare with `is`
    if _is_longdouble(dt):
        assert want == np.longdouble and got is np.float64
    else:
        assert np.dtype(got) == want, (dt, got, want)
    assert D.result_dtype(x.astype(dt.newbyteorder("S"))) is got
    if dt.kind == "c":                              # fft2d / ifft2d of complex input
        cwant = np.complex128 if _is_longdouble(dt) else np.fft.fft2(x).dtype.type
        assert F._complex_result_dtype(x) is cwant


def test_result_dtype_of_tensors():
    torch = pytest.importorskip("torch")
    for dt, want in ((torch.float32, np.float32), (torch.float16, np.float32), (torch.bfloat16, np.float32),
                     (torch.complex64, np.float32), (torch.float64, np.float64), (torch.complex128, np.float64),
                     (torch.uint8, np.float64), (torch.int16, np.float64), (torch.int64, np.float64), (torch.bool, np.float64)):
        assert D.result_dtype(torch.zeros(2, dtype=dt)) is want, dt


@pytest.mark.parametrize("dt", list(_dtypes()), ids=lambda d: d.str)
def test_staged_route_by_kind_and_size_in_either_byte_order(dt):
    """C-contiguous arrays of _UPLOAD_MIN_BYTES and more whose kind and item size has a b4d_to_f32 code are staged, in
    either byte order; native float32 keeps the plain copy; smaller, non-contiguous and broadcast arrays never stage."""
    n = -(-D._UPLOAD_MIN_BYTES // dt.itemsize)
    n += n % 2
    at = np.empty(n, dt)                             # never written: no host memory is touched
    want = TO_F32_CODES.get((dt.kind, dt.itemsize))
    if dt.kind == "f" and dt.itemsize == 4 and dt.isnative:
        want = None
    assert D.staged_code(at) == want, dt
    assert D.staged_code(at.reshape(2, -1)) == want, dt
    if want is not None:
        assert D._UPLOAD_CODES[dt.name] == want
    assert D.staged_code(np.empty(D._UPLOAD_MIN_BYTES // dt.itemsize - 1, dt)) is None
    assert D.staged_code(np.empty((2, n // 2), dt, order="F")) is None
    assert D.staged_code(at.reshape(2, -1)[::-1]) is None
    assert D.staged_code(at[::2]) is None
    assert D.staged_code(np.broadcast_to(np.zeros(n // 2, dt), (2, n // 2))) is None


# ---- the reference pins the contract: its outputs do not change dtype when the input's byte order does
def _ref_rows():
    from oracle import load_reference as L

    R = L.load()
    norm = importlib.import_module("barc4dip.preprocessing.normalize")
    stat = importlib.import_module("barc4dip.metrics.statistics")
    sl = (slice(15, 48), slice(15, 48))
    # template_matching and deconvolve_psf need OpenCV or scikit-image, which this tier does not have; the reference has no
    # distortion correction, displacement map or temporal statistics entry point
    return {
        "fft2d": lambda f, s, c: R.fft.fft2d(c(f[0])),
        "ifft2d_c8": lambda f, s, c: R.fft.ifft2d(c(s.astype(np.complex64))),
        "ifft2d_c16": lambda f, s, c: R.fft.ifft2d(c(s)),
        "psd2d": lambda f, s, c: R.fft.psd2d(c(f[0])),
        "autocorr2d": lambda f, s, c: R.corr.autocorr2d(c(f[0])),
        "xcorr2d": lambda f, s, c: R.corr.xcorr2d(c(f[0]), c(f[1])),
        "phase_correlation": lambda f, s, c: R.tracking.phase_correlation(c(f[0][sl]), c(f[1]), slices_yx=sl),
        "speckle_stats": lambda f, s, c: R.speckles.speckle_stats(c(np.tile(f[0], (2, 2))), verbose=False),  # 128 px minimum
        "sharpness_stats": lambda f, s, c: R.sharpness.sharpness_stats(c(f[0]), verbose=False),
        "distribution_moments": lambda f, s, c: stat.distribution_moments(c(f[0])),
        "radial_mean_binned": lambda f, s, c: R.radial.radial_mean_binned(c(f[0])),
        "flat_field_correction": lambda f, s, c: norm.flat_field_correction(c(f[:2]), flats=c(f[2]), darks=c(f[1] // 4)),
    }


def _dtypes_of(x, path=""):
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            yield from _dtypes_of(x[k], f"{path}/{k}")
    elif isinstance(x, (tuple, list)):
        for i, e in enumerate(x):
            yield from _dtypes_of(e, f"{path}[{i}]")
    else:
        yield path, np.asarray(x).dtype


REF_ROWS = ["fft2d", "ifft2d_c8", "ifft2d_c16", "psd2d", "autocorr2d", "xcorr2d", "phase_correlation",
            "speckle_stats", "sharpness_stats", "distribution_moments", "radial_mean_binned", "flat_field_correction"]


@pytest.mark.needs_reference
@pytest.mark.parametrize("img_dtype", ["uint16", "float32"])
@pytest.mark.parametrize("row", REF_ROWS)
def test_reference_output_dtypes_do_not_depend_on_byte_order(row, img_dtype):
    from barc4dip_amd import synth

    frames = np.stack([synth.speckle_frame(64, 5 + t) for t in range(3)]).astype(img_dtype)
    spec = np.fft.fftshift(np.fft.fft2(frames[0].astype(np.float64)))
    fn = _ref_rows()[row]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        native = list(_dtypes_of(fn(frames, spec, lambda a: a)))
        swapped = list(_dtypes_of(fn(frames, spec, lambda a: a.astype(a.dtype.newbyteorder(">")))))
    assert [k for k, _ in native] == [k for k, _ in swapped]
    for (k, a), (_, b) in zip(native, swapped):
        assert a.kind == b.kind and a.itemsize == b.itemsize, (row, k, a, b)
