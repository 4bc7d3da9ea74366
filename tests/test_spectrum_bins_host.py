"""CPU tier of tests/test_gpu_spectrum_bins.py: the check has teeth, and the route table says what the dispatch does.

The frame builder and the checker of the GPU module run here on NumPy's float32 transform in place of the device's output: it
passes (the reference alone is within the bar), and each of five mutations of it -- the errors the normwise tests on frames with
a large mean cannot see -- is rejected.  On a frame those tests use, the same mutations stay under their bar.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_spectrum_bins as B
from barc4dip_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one thin power-of-two frame, one odd, one mixed-radix, one fused, one Bluestein
SHAPES = [(2048, 64), (33, 45), (171, 170), (6, 1072), (5, 1031)]


@pytest.fixture(scope="module")
def lib():
    from barc4dip_amd import _ffi

    if not os.path.exists(_ffi.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "barc4dip_amd", "csrc"), "libb4d.so"], check=True)
    return _ffi.load_library()


_CPU = {}


def cpu_outputs(shape):
    """per frame kind: (frame, float64 reference, outputs of NumPy's float32 transform); computed once, never modified"""
    if shape not in _CPU:
        stack = B.build_stack(shape)
        _CPU[shape] = {k: (stack[t], B.reference(stack[t]), B.float32_transform(stack[t])) for t, k in enumerate(B.KINDS)}
    return _CPU[shape]


def typical_bin(mag):
    """the bin of median magnitude and its right-hand neighbour"""
    order = np.argsort(mag, axis=None)
    i = np.unravel_index(int(order[order.size // 2]), mag.shape)
    return (int(i[0]), int(i[1])), (int(i[0]), (int(i[1]) + 1) % mag.shape[1])


def scale_one_bin(a, ref):
    i, _ = typical_bin(np.abs(ref))
    a[i] *= 1.0 + 1e-3


def swap_neighbours(a, ref):
    i, j = typical_bin(np.abs(ref))
    a[i], a[j] = a[j].copy(), a[i].copy()


def roll_kx0_column(a, ref):
    c = a.shape[1] // 2
    a[:, c] = np.roll(a[:, c], 1)


def conjugate_nyquist_row(a, ref):
    a[0, :] = np.conj(a[0, :])     # the shifted spectrum starts at ky = -ny/2 (an odd side: at its outermost row)


def move_strongest_bin(a, ref):
    i = np.unravel_index(int(np.argmax(np.abs(ref))), ref.shape)
    j = (i[0], (i[1] + 1) % a.shape[1])
    a[j], a[i] = a[i], 0.0


# (mutation, frame kind, entries it is applied to)
MUTATIONS = [
    (scale_one_bin, "noise0", ("fft", "psd_raw", "psd")),
    (swap_neighbours, "noise0", ("fft", "psd_raw", "psd")),
    (roll_kx0_column, "noise0", ("fft", "psd_raw")),
    (roll_kx0_column, "rowconst", ("fft", "psd")),
    (conjugate_nyquist_row, "noise1", ("fft",)),
    (conjugate_nyquist_row, "impedge", ("fft",)),
    (move_strongest_bin, "marker", ("psd_raw", "psd")),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_alone_is_within_the_bar(shape):
    figures = {}
    for kind, (frame, ref, f32) in cpu_outputs(shape).items():
        B.check_frame(kind, frame, f32, ref=ref)                      # asserts TOL on every figure
        B.check_frame(kind, frame, f32, ref=ref, record=lambda e, v: figures.__setitem__(e, max(v, figures.get(e, 0.0))))
    print(shape, {e: f"{v:.2e}" for e, v in sorted(figures.items())})
    assert figures["fft"] < 1e-6 and figures["psd_raw"] < 1e-6      # a decade inside the bar: the bar measures the device, not NumPy


@pytest.mark.parametrize("mutate,kind,entries", MUTATIONS, ids=lambda v: getattr(v, "__name__", None))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_mutation_is_rejected(shape, mutate, kind, entries):
    frame, ref, f32 = cpu_outputs(shape)[kind]
    for entry in entries:
        bad = np.array(f32[entry])
        mutate(bad, ref[entry])
        assert not np.array_equal(bad, f32[entry]), "the mutation changed nothing"
        with pytest.raises(AssertionError):
            B.check_frame(kind, frame, {entry: bad}, ref=ref)


def test_the_old_check_accepts_the_first_two_mutations():
    """On a frame the normwise tests use (speckle with its mean, 2048 x 64: DC = 8e3 typical |F| and 6e7 typical PSD bins) a bin off
    by 1e-3 passes nerr < 1e-5 in the spectrum (1.2e-7) and in the PSD; two swapped neighbours pass in the PSD (1.5e-8).  In the
    spectrum a swap is an error of a whole typical bin and reaches 1.0e-4: caught there, but by a factor of ten only, and an error
    of 8 % of a bin is not.  On the noise frames of this suite the same swap is 0.3 of the bar's reference, 3e4 times the bar."""
    x = np.ascontiguousarray(synth.speckle_frame(2048, 4321)[:, :64]).astype(np.float32)
    ref, f32 = B.reference(x), B.float32_transform(x)
    for entry in ("fft", "psd_raw", "psd"):
        assert B.nerr(f32[entry], ref[entry]) < B.TOL
        assert float(np.max(np.abs(ref[entry])) / np.median(np.abs(ref[entry]))) > (5e3 if entry == "fft" else 5e7)
        for mutate in (scale_one_bin, swap_neighbours):
            if mutate is swap_neighbours and entry == "fft":
                continue
            bad = np.array(f32[entry])
            mutate(bad, ref[entry])
            assert not np.array_equal(bad, f32[entry])
            e = B.nerr(bad, ref[entry])
            print(f"old check, {mutate.__name__} on {entry}: nerr {e:.3e}")
            assert e < B.TOL


def test_noise_frames_have_no_dominant_bin():
    """what makes the normwise bar a per-bin bar: the largest bin of a noise frame is a few typical bins, the DC bin is nothing"""
    _, ref, _ = cpu_outputs((2048, 64))["noise0"]
    F, P = np.abs(ref["fft"]), ref["psd_raw"]
    assert F.max() / np.sqrt(np.mean(F ** 2)) < 5.0 and P.max() / np.median(P) < 40.0
    assert F[1024, 32] < 1e-5 * F.max()
    _, mref, _ = cpu_outputs((2048, 64))["marker"]
    M = np.abs(mref["fft"])
    assert int((M > 1e-3 * M.max()).sum()) == 11 and np.sort(M, axis=None)[-12] < 1e-8 * M.max()
    from oracle import signal_np as S

    frame, nref, _ = cpu_outputs((33, 45))["noise0"]
    np.testing.assert_array_equal(nref["psd"], S.psd2d(frame.astype(np.float64))[0])   # reference() scales the unscaled oracle PSD itself
    for kind in ("imp00", "imp11", "impedge"):
        frame, iref, _ = cpu_outputs((33, 45))[kind]
        assert frame.sum() == 1.0 and B.nerr(iref["fft"], B.impulse_spectrum((33, 45), kind)) < 1e-12


# ------------------------------------------------------------------------------------------------------------- the route table
def header_route_flags():
    txt = open(os.path.join(ROOT, "include", "b4d.h")).read()
    return {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+B4D_ROUTE_([A-Z0-9_]+)\s+0x([0-9a-fA-F]+)u", txt)}


def test_route_flags_match_the_header():
    assert header_route_flags() == {"POW2": B.POW2, "PARITY": B.PARITY, "WMR": B.WMR, "FUSED": B.FUSED, "DFTMAT": B.DFTMAT,
                                    "PMROWS": B.PMROWS, "BLUESTEIN_Y": B.BLUESTEIN_Y, "BLUESTEIN_X": B.BLUESTEIN_X}


def test_route_table_agrees_with_the_dispatch(lib):
    """no GPU call: the query is host arithmetic, from the helper the plan constructor and the entry points branch on"""
    for case in B.ROUTES:
        (ny, nx), flags = case[1], case[2]
        assert lib.b4d_size_supported(ny, nx) == 1
        assert lib.b4d_size_route(ny, nx) == flags, (B.case_id(case), hex(lib.b4d_size_route(ny, nx)))
    for (ny, nx), flags in B.C2C_ROUTES:
        assert lib.b4d_size_route(ny, nx) == flags
    union = 0
    for case in B.ROUTES:
        union |= case[2]
    every = 0
    for v in header_route_flags().values():
        every |= v
    assert union == every, f"flags no shape of the table reports: {every & ~union:#x}"
    engines = B.POW2 | B.WMR | B.FUSED | B.DFTMAT | B.PMROWS
    for ny, nx in [(64, 64), (2048, 2048), (4096, 64), (171, 170), (2160, 2560), (100, 2048), (512, 512), (513, 512), (1042, 2048),
                   (8192, 8192), (2, 2)]:
        r = lib.b4d_size_route(ny, nx)
        assert bin(r & engines).count("1") == 1, (ny, nx, hex(r))
        assert bool(r & B.PARITY) == (bool(r & B.POW2) and ny == 2048)
        assert not (r & (B.BLUESTEIN_Y | B.BLUESTEIN_X)) or (r & B.PMROWS)
    for ny, nx in [(4099, 2048), (9000, 64), (1, 64), (64, 0), (8192, 16384)]:
        assert lib.b4d_size_supported(ny, nx) == 0 and lib.b4d_size_route(ny, nx) == 0


def test_mixed_radix_lengths_all_appear_on_both_axes(lib):
    src = open(os.path.join(ROOT, "barc4dip_amd", "csrc", "b4d_wiener_mr.hip")).read()
    table = src[src.index("#define B4D_WMR_LENGTHS(X)"):src.index("bool wmr_supported")]
    lengths = tuple(int(v) for v in re.findall(r"X\((\d+),", table))
    assert lengths == B.WMR_LENGTHS, "the literal copy in the GPU test drifted from the length table"
    rows = {c[1][0] for c in B.ROUTES if c[2] == B.WMR}
    cols = {c[1][1] for c in B.ROUTES if c[2] == B.WMR}
    assert rows == set(lengths) and cols == set(lengths)
    for L in lengths:
        assert lib.b4d_size_route(L, 170) == B.WMR and lib.b4d_size_route(171, L) == B.WMR
    assert lib.b4d_size_route(227, 228) == B.DFTMAT        # one side without a compiled kernel: not this route
