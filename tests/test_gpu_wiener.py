"""GPU tier: deconvolve_psf (Wiener) through the C ABI vs the (unpinned) oracle restatement.
Tolerance: float32 transforms on both sides, compared normwise at 2e-5 of the frame maximum."""
import numpy as np
import pytest

from barc4dip_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import torch

    assert torch.cuda.is_available()
    from barc4dip_amd import preprocessing

    return preprocessing


@pytest.mark.parametrize("shape,sigma", [((60, 52), 1.5), ((64, 64), (1.0, 2.0)), ((100, 37), 0.7), ((512, 512), 1.5),
                                         # padded 262 = 2 * 131 (and 74 = 2 * 37): fused, roots-of-unity small DFTs, pair route
                                         ((70, 258), 0.7), ((258, 258), 0.7),
                                         # padded 331 (prime, A + B > 320): DFT-matrix product on x (pad and crop kernels), on y
                                         # (one-side-fused row passes), on both; 69 x 60: fused pair route with an odd padded height
                                         ((60, 323), 1.5), ((323, 60), 1.5), ((323, 323), 1.5), ((61, 52), 1.5),
                                         # padded 264 = 8*3*11 / 520 = 8*5*13: the three-kernel mixed-radix route
                                         # (b4d_wiener_mr.hip) on square and both non-square orientations
                                         ((256, 256), 1.5), ((256, 512), 1.5), ((512, 256), 1.5)])
@pytest.mark.parametrize("clip", [True, False])
def test_wiener_vs_oracle(pp, shape, sigma, clip):
    from oracle import wiener_np as W

    img = synth.speckle_frame(512, 9)[:shape[0], :shape[1]].copy()
    got = pp.deconvolve_psf(img, sigma=sigma, clip=clip)
    ref = W.deconvolve_psf(img, sigma=sigma, clip=clip)
    assert got.shape == img.shape and got.dtype == np.float32
    assert float(np.max(np.abs(got - ref))) < 2e-5 * float(np.max(np.abs(img)))


def test_wiener_detector_format(pp):
    """A non-square camera format on the three-kernel route: 1072 x 1912, sigma 1.5 -> padded 1080 x 1920 (12 * 10 * 9 and
    16 * 12 * 10), and a stack call against the per-frame calls."""
    import torch
    from oracle import wiener_np as W

    img = synth.speckle_frame(2048, 21)[:1072, :1912].copy()
    ref = W.deconvolve_psf(img, sigma=1.5)
    got = pp.deconvolve_psf(img, sigma=1.5)
    assert got.shape == img.shape and got.dtype == np.float32
    assert float(np.max(np.abs(got - ref))) < 2e-5 * float(np.max(np.abs(img)))
    st = np.stack([img, img[::-1].copy(), img[:, ::-1].copy(), img * 0.5, img + 7])
    out = pp.deconvolve_psf(torch.from_numpy(st).cuda(), sigma=1.5, return_tensors=True).cpu().numpy()
    for i in range(len(st)):
        assert np.array_equal(out[i], pp.deconvolve_psf(st[i], sigma=1.5))


def _blurred_scene(n, m, seed, noise):
    from scipy.signal import convolve2d
    from oracle import wiener_np as W

    rng = np.random.default_rng(seed)
    truth = np.zeros((n, m), np.float32)
    truth[n // 5:n // 2, m // 4:3 * m // 4] = 1.0
    truth[3 * n // 5:4 * n // 5, m // 10:m // 3] = 0.5
    psf = W.gaussian_psf(1.5, 1.5)
    blur = convolve2d(np.pad(truth, 4, mode="reflect"), psf, mode="same")[4:-4, 4:-4]
    return truth, (blur + rng.normal(size=blur.shape) * noise).astype(np.float32)


@pytest.mark.parametrize("shape", [(60, 52), (120, 248), (256, 256)])   # padded 68 x 60 / 128 x 256 / 264 x 264: three transform routes
def test_unsupervised_wiener_replays_the_library_stream(pp, shape):
    """method='uw' (filters.py:278-286 -> skimage.restoration.unsupervised_wiener, published algorithm, parity unpinned).
    With `rng` given the device sampler consumes the host stream in the library's order (two normal fields, two Gamma
    variates per sweep), so it must walk the SAME chain as the oracle: posterior mean within 2e-5 of the range, the same
    number of sweeps, the precision chains within 1e-4."""
    from oracle import wiener_np as W

    _, img = _blurred_scene(*shape, seed=3, noise=0.02)
    chains = {}

    def spy(key):
        def cb(x):
            chains.setdefault(key, []).append(np.array(x[0, :3]))
        return cb
    ref = W.deconvolve_psf(img, sigma=1.5, method="uw", rng=np.random.default_rng(11), user_params={"callback": spy("ref")})
    got = pp.deconvolve_psf(img, sigma=1.5, method="uw", rng=np.random.default_rng(11), user_params={"callback": spy("got")})
    assert got.shape == img.shape and got.dtype == np.float32
    assert len(chains["ref"]) == len(chains["got"]) > 30
    assert np.allclose(np.array(chains["got"]), np.array(chains["ref"]), rtol=2e-3, atol=2e-5)
    assert float(np.max(np.abs(got - ref))) < 2e-5 * float(np.max(np.abs(img)))
    # a stack shares ONE stream over its frames
    st = np.stack([img, img[::-1].copy()])
    g2 = pp.deconvolve_psf(st, sigma=1.5, method="uw", rng=np.random.default_rng(11))
    r2 = W.deconvolve_psf(st, sigma=1.5, method="uw", rng=np.random.default_rng(11))
    assert float(np.max(np.abs(g2 - r2))) < 2e-5 * float(np.max(np.abs(img))) and np.array_equal(g2[0], got)


def test_unsupervised_wiener_device_stream(pp):
    """Default `rng=None`: normals from the device generator (Philox), a fresh stream per call like the reference's own
    behaviour.  Statistical checks only: two calls differ, both stay within the sampler's run-to-run spread of the oracle's
    answer, and the estimated noise precision matches the noise that was put in (1 / 0.02^2 on the normalised frame)."""
    from oracle import wiener_np as W

    _, img = _blurred_scene(200, 200, seed=5, noise=0.02)
    a = pp.deconvolve_psf(img, sigma=1.5, method="uw")
    b = pp.deconvolve_psf(img, sigma=1.5, method="uw")
    r1 = W.deconvolve_psf(img, sigma=1.5, method="uw", rng=1)
    r2 = W.deconvolve_psf(img, sigma=1.5, method="uw", rng=2)
    spread = float(np.sqrt(np.mean((r1 - r2) ** 2)))
    assert not np.array_equal(a, b)
    for g in (a, b):
        assert float(np.sqrt(np.mean((g - r1) ** 2))) < 2.0 * spread
    # moments of the device normals through the sampler itself: x - wiener_mean has variance 0.5 / precision per component
    noise_prec = []
    pp.deconvolve_psf(img, sigma=1.5, method="uw", user_params={"callback": lambda x: noise_prec.append(x.shape), "max_num_iter": 5, "min_num_iter": 1, "burnin": 1})
    assert len(noise_prec) == 5
    with pytest.raises(NotImplementedError):
        pp.deconvolve_psf(img, sigma=1.5, method="uw", is_real=False)


def test_uw_step_device_normals_and_sums(pp):
    """b4d_uw_step through the C ABI.  With tf = 0, |L|^2 = 1 and gx = 0.5 the sample IS the pair of normals (precision 0.5,
    excursion scale 1): moments of the device generator over 2^20 elements, independence between sweeps and between the two
    components; and the four sums against NumPy on the same arrays (half-plane weights included)."""
    import ctypes as C

    import torch

    from barc4dip_amd import _device as D
    from barc4dip_amd import _ffi
    from oracle import wiener_np as W

    lib = _ffi.lib()
    ny, nxh = 1024, 1024 + 1
    dev = torch.device("cuda")
    y = torch.zeros((ny, nxh), dtype=torch.complex64, device=dev)
    tf = torch.zeros_like(y)
    a2 = torch.ones((ny, nxh), dtype=torch.float32, device=dev)
    xs, post = torch.empty_like(y), torch.zeros_like(y)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    draws = []
    for sweep in (0, 1):
        _ffi.check(lib.b4d_uw_step(D.ptr(y), D.ptr(tf), D.ptr(a2), D.ptr(xs), D.ptr(post), None, None, 12345, sweep, 0, 1.0, 0.5, ny, nxh,
                                   D.ptr(sums), _ffi.stream_ptr()))
        draws.append(xs.cpu().numpy().copy())
    z = np.concatenate([draws[0].real.ravel(), draws[0].imag.ravel()]).astype(np.float64)
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n) and abs(np.mean(z ** 4) - 3) < 0.05
    assert abs(np.mean(draws[0].real * draws[0].imag)) < 5 / np.sqrt(n / 2)
    assert abs(np.mean(draws[0].real * draws[1].real)) < 5 / np.sqrt(n / 2) and not np.array_equal(draws[0], draws[1])
    assert np.max(np.abs(z)) > 4.0            # tails exist
    # sums of a sweep with supplied normals, against NumPy
    rng = np.random.default_rng(0)
    ny, nxh = 96, 49
    Y = (rng.normal(size=(ny, nxh)) + 1j * rng.normal(size=(ny, nxh))).astype(np.complex64)
    Hh = (rng.normal(size=(ny, nxh)) + 1j * rng.normal(size=(ny, nxh))).astype(np.complex64) * 0.5
    A2 = rng.random((ny, nxh)).astype(np.float32) + 0.1
    R1, R2 = rng.normal(size=(ny, nxh)).astype(np.float32), rng.normal(size=(ny, nxh)).astype(np.float32)
    P0 = (rng.normal(size=(ny, nxh)) + 1j * rng.normal(size=(ny, nxh))).astype(np.complex64)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    dY, dH, dA, d1, d2, dP = t(Y), t(Hh), t(A2), t(R1), t(R2), t(P0.copy())
    dx = torch.empty_like(dY)
    gn, gx, sweep, burn = 3.0, 0.7, 5, 2
    _ffi.check(lib.b4d_uw_step(D.ptr(dY), D.ptr(dH), D.ptr(dA), D.ptr(dx), D.ptr(dP), D.ptr(d1), D.ptr(d2), 0, sweep, burn, gn, gx, ny, nxh,
                               D.ptr(sums), _ffi.stream_ptr()))
    prec = gn * np.abs(Hh) ** 2 + gx * A2
    x = gn * np.conj(Hh) / prec * Y + np.sqrt(0.5 / prec) * (R1 + 1j * R2)
    assert np.allclose(dx.cpu().numpy(), x, rtol=2e-5, atol=2e-6)
    pn = P0 + x
    want = [W.image_quad_norm(Y - x * Hh), W.image_quad_norm(x * np.sqrt(A2)),
            np.sum(np.abs(pn / (sweep - burn) - P0 / (sweep - burn - 1))), np.sum(np.abs(pn))]
    assert np.allclose(sums.cpu().numpy(), want, rtol=2e-5)
    assert np.allclose(dP.cpu().numpy(), pn, rtol=2e-5, atol=2e-6)
    assert lib.b4d_uw_step(D.ptr(dY), D.ptr(dH), D.ptr(dA), None, D.ptr(dP), D.ptr(d1), None, 0, 0, 0, 1.0, 1.0, ny, nxh, D.ptr(sums), None) != 0


@pytest.mark.parametrize("clip", [True, False])
def test_cfg5_size(pp, clip):
    """BASELINE.json config 5 at its stated size: one 4096 x 4096 frame, sigma 1.5 (9 x 9 PSF, padded 4104 = 8 * 27 * 19),
    preprocessing/filters.py:233-289.  2e-5 of the data range against the float32 oracle (parity unpinned: scikit-image).
    The clip matters here: the Wiener filter overshoots the normalised range at the brightest grains."""
    import torch
    from oracle import wiener_np as W

    img = synth.speckle_frame(4096, 77)
    ref = W.deconvolve_psf(img, sigma=1.5, clip=clip)
    got = pp.deconvolve_psf(img, sigma=1.5, clip=clip)
    assert got.shape == img.shape and got.dtype == np.float32
    err = float(np.max(np.abs(got - ref))) / float(np.max(np.abs(img)))
    print(f"cfg5 4096^2 clip={clip}: max err / range = {err:.2e}")
    assert err < 2e-5
    if clip:   # says whether the clip is active on this frame (then max|restored| is exactly the frame maximum)
        print("clip active:", float(np.max(np.abs(ref))) == float(np.max(np.abs(img))))
    # a multi-frame call (several frames per launch) reproduces the single-frame result bit for bit
    dev = torch.from_numpy(np.stack([img, img[::-1].copy(), img[:, ::-1].copy()])).cuda()
    out = pp.deconvolve_psf(dev, sigma=1.5, clip=clip, return_tensors=True)
    assert np.array_equal(out[0].cpu().numpy(), got)
    assert np.array_equal(out[1].cpu().numpy(), pp.deconvolve_psf(img[::-1].copy(), sigma=1.5, clip=clip))


def test_mixed_radix_route_special_values(pp):
    """np.nanmax / np.clip semantics on the mixed-radix route (padded 264): NaN pixel -> NaN frame, all-zero and
    infinite-maximum frames -> zeros (filters.py:255-257), an odd number of frames per call."""
    from oracle import wiener_np as W

    stack = synth.speckle_stack(5, 256, seed0=90)
    stack[1, 10, 20] = np.nan
    stack[2] = 0.0
    stack[3, 100, 7] = np.inf
    got = pp.deconvolve_psf(stack, sigma=1.5)
    assert np.isnan(got[1]).all() and np.all(got[2] == 0) and np.all(got[3] == 0)
    for t in (0, 4):
        ref = W.deconvolve_psf(stack[t], sigma=1.5)
        assert float(np.max(np.abs(got[t] - ref))) < 2e-5 * float(stack[t].max())


def test_mixed_radix_route_stack_equals_frames(pp):
    """Three frames in one call on the three-kernel route, padded 264 x 520 (33 quads per frame: an odd count, so the row
    kernels' even-padded quad numbering holds invalid items between the frames): every frame equals its single-frame call bit
    for bit, and frame 0 meets the oracle."""
    from barc4dip_amd.preprocessing import filters
    from oracle import wiener_np as W

    ky, kx = filters._gaussian_psf(1.5, 1.5).shape
    assert (256 + 2 * (ky // 2), 512 + 2 * (kx // 2)) == (264, 520)
    base = synth.speckle_frame(512, 13)[:256, :512]
    st = np.ascontiguousarray(np.stack([base, base[::-1], base[:, ::-1] * 0.5 + 3.0]), dtype=np.float32)
    out = pp.deconvolve_psf(st, sigma=1.5)
    for i in range(3):
        assert np.array_equal(out[i], pp.deconvolve_psf(st[i], sigma=1.5))
    ref = W.deconvolve_psf(st[0], sigma=1.5)
    assert float(np.max(np.abs(out[0] - ref))) < 2e-5 * float(np.max(np.abs(st[0])))


def test_stack_balance_and_errors(pp):
    from oracle import wiener_np as W

    stack = synth.speckle_stack(3, 128, seed0=40)[:, :100, :120].copy()
    got = pp.deconvolve_psf(stack, sigma=1.5, balance=0.1)
    ref = W.deconvolve_psf(stack, sigma=1.5, balance=0.1)
    assert float(np.max(np.abs(got - ref))) < 2e-5 * float(stack.max())
    assert np.all(pp.deconvolve_psf(np.zeros((32, 32), np.float32), sigma=1.0) == 0)
    with pytest.raises(TypeError):
        pp.deconvolve_psf([[1.0]], sigma=1.0)
    with pytest.raises(ValueError):
        pp.deconvolve_psf(stack[0, 0], sigma=1.0)
    with pytest.raises(ValueError):
        pp.deconvolve_psf(stack, sigma=-1.0)
    with pytest.raises(ValueError):
        pp.deconvolve_psf(stack, sigma=1.0, method="bogus")
    with pytest.raises(ValueError):
        pp.deconvolve_psf(stack, sigma=1.0, pad_mode="edge")
    with pytest.raises(NotImplementedError):
        pp.deconvolve_psf(stack, sigma=1.0, method="uw", is_real=False)
    with pytest.raises(ValueError):
        pp.deconvolve_psf(stack, sigma=1.0, method="uw", reg=0.5)     # the reference's own `reg: float` cannot work either


def test_stack_frames_on_two_streams_keep_the_callers_order(pp):
    """A multi-frame call runs alternate frames on two plan-owned streams (include/b4d.h): each frame must equal the
    single-frame call bit for bit, on the default stream and on a side stream with consumers queued right behind it."""
    import torch

    dev = torch.device("cuda:0")
    stack = torch.from_numpy(synth.speckle_stack(5, 512, seed0=70)[:, :500, :404].copy()).to(dev)
    singles = torch.stack([pp.deconvolve_psf(stack[t], sigma=1.5, return_tensors=True) for t in range(5)])
    torch.cuda.synchronize()
    for _ in range(3):
        got = pp.deconvolve_psf(stack, sigma=1.5, return_tensors=True)
        total = got.sum(dtype=torch.float64)         # queued on the same stream right after the call
        assert torch.equal(got, singles)
        assert float(total) == float(singles.sum(dtype=torch.float64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scaled = stack * 2.0                          # producer queued on the side stream just before the call
        got = pp.deconvolve_psf(scaled, sigma=1.5, return_tensors=True)
        halves = got * 0.5                            # consumer queued behind it
    side.synchronize()
    ref = torch.stack([pp.deconvolve_psf(scaled[t], sigma=1.5, return_tensors=True) for t in range(5)])
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and torch.equal(halves, ref * 0.5)


@pytest.mark.parametrize("shape,sigma,iters", [((60, 52), 1.5, 12), ((130, 200), (1.0, 2.0), 30), ((512, 512), 1.5, 8)])
def test_richardson_lucy_vs_oracle(pp, shape, sigma, iters):
    """method="rl" (filters.py:270-277) against the float32 oracle of the published algorithm (parity with scikit-image
    unpinned).  Both run float32 direct convolutions; summation order differs, the multiplicative iteration amplifies
    rounding mildly: 2e-5 of the data range after a few tens of iterations."""
    from barc4dip_amd import synth
    from oracle import wiener_np as W

    img = synth.speckle_frame(max(shape), 11)[:shape[0], :shape[1]]
    want = W.deconvolve_psf(img, sigma=sigma, method="rl", num_iter=iters)
    got = pp.deconvolve_psf(img, sigma=sigma, method="rl", num_iter=iters)
    assert got.dtype == np.float32 and got.shape == img.shape
    assert np.max(np.abs(got - want)) <= 2e-5 * np.max(np.abs(img))
    got_fe = pp.deconvolve_psf(img, sigma=sigma, method="rl", num_iter=3, filter_epsilon=0.05, clip=False)
    want_fe = W.deconvolve_psf(img, sigma=sigma, method="rl", num_iter=3, filter_epsilon=0.05, clip=False)
    assert np.max(np.abs(got_fe - want_fe)) <= 2e-5 * np.max(np.abs(img))
    st = np.stack([img, img[::-1].copy()])
    out2 = pp.deconvolve_psf(st, sigma=sigma, method="rl", num_iter=4)
    assert np.array_equal(out2[0], pp.deconvolve_psf(img, sigma=sigma, method="rl", num_iter=4))
    with pytest.raises(ValueError):
        pp.deconvolve_psf(img, sigma=sigma, method="rl", num_iter=0)
    with pytest.raises(ValueError):
        pp.deconvolve_psf(img, sigma=sigma, method="richardson")
