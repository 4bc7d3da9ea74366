/* b4d.h -- C ABI of the MI355X (gfx950) hot path of barc4dip.
 *
 * The reference (barc4dip, pure Python) has no FFI: its boundary is the Python API of
 * barc4dip.signal / barc4dip.metrics / barc4dip.preprocessing.  This header is what a
 * maintainer binds (ctypes) to route those functions to the GPU.
 * Each entry point cites the reference function it serves (paths under
 * /root/reference/src/barc4dip).
 *
 * Conventions
 *   - every function returns 0 on success, a negative B4D_E* code on failure; the message
 *     is available from b4d_last_error() (thread local).  No C++ exceptions cross the ABI.
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. tensor.data_ptr());
 *     images are row-major (ny, nx) float32, stacks (batch, ny, nx).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *     asynchronous on that stream; a plan may be used from one stream at a time.
 *   - FFT outputs are fftshift-ed (DC at [ny/2, nx/2]) exactly as signal/fft.py:7-10 and
 *     signal/corr.py:7-10 define.
 */
#ifndef B4D_H
#define B4D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B4D_OK 0
#define B4D_EINVAL (-1)   /* bad argument (null pointer, batch <= 0, ...) */
#define B4D_ESIZE (-2)    /* (ny, nx) not supported by the compiled kernels */
#define B4D_EHIP (-3)     /* a HIP runtime call failed */
#define B4D_ENOMEM (-4)
#define B4D_ELOOP (-5)    /* a loop bound of the labelling kernels was reached (reported in n_regions, see b4d_label_regions) */

/* flags for b4d_autocorr2 / b4d_psd_autocorr2 (signal/corr.py:169-180 keyword arguments) */
#define B4D_REMOVE_MEAN 1u      /* remove_mean=True  : zero the DC bin of the power spectrum */
#define B4D_NORM_PEAK 2u        /* normalize="peak"  : divide by the zero-lag value, peak == 1 */
#define B4D_STANDARDIZE 4u      /* standardize=True  : divide by the variance (only visible with normalize="none") */

typedef struct b4d_plan b4d_plan;

/* Library / device ------------------------------------------------------------------- */
const char* b4d_version(void);
const char* b4d_last_error(void);
/* Process-wide switches that never change results, only the route taken (tests run every route):
 *   "track_predict_bin"  0 / 1 / 2 (default 1): 1 = b4d_phase_correlation counts and gathers the EXPECTED median bin of every
 *                        correlation map in the pass that produces it and (power-of-two sizes) does not store the map: the rows
 *                        around the peak are recomputed for the sub-pixel step, pairs whose expectation fails get their full map
 *                        from a second, gated pass; 0 = no expectation: full maps, full select; 2 = a deliberately wrong
 *                        expectation (test hook: every pair takes the gated pass).
 *   "lanes"              0 / 1 (default 1): 1 = the multi-pass entry points (b4d_fft2d, the general-size passes, b4d_wiener_apply,
 *                        b4d_phase_correlation) cut a stack into cache-sized launch groups and deal them alternately to the
 *                        caller's stream and ONE library-owned stream per device, forked from and joined into the caller's stream
 *                        by events inside the call (stream order as seen by the caller is unchanged); 0 = everything on the
 *                        caller's stream alone (for callers that must not see a second stream).
 *   "ysplit"             0 / 1 (default 1): 1 = PSD / autocorrelation of 2048-row frames (power-of-two plans) move one radix-2
 *                        stage of the column transform into the row passes, so that the column pass works on 32-column tiles of
 *                        every second spectrum row and stores whole 128-byte PSD lines; 0 = 16-column tiles of all rows.  The
 *                        route depends on the frame shape alone (results of a stack equal those of its frames, bit for bit); the
 *                        two routes split the column transform differently and agree to float32 rounding, not bit for bit.
 *   "row16"              0 / 1 (default 1): 1 = on the "ysplit" route the row passes move 16 bytes per lane to and from device memory
 *                        (the inverse row pass all of its loads and stores, the forward row pass its stores) where the pointers
 *                        allow it: the workspace, and for the inverse pass the caller's `autocorr`, must be 16-byte aligned --
 *                        checked per call, the 4- and 8-byte kernels run otherwise; 0 = the 4- and 8-byte kernels always.  Only
 *                        which lane moves which element differs: results are bit-identical.
 *   "colsets"            0 / 1 (default 1): 1 = on the "ysplit" route with "row16" (16-byte-aligned workspace, nx <= 2048) the forward
 *                        row pass hands the column pass "column-set" tiles: every 16 bytes hold rows n and n + 512 of ONE column, so
 *                        the column pass has the first of its two register sets complete after half of its loads and transforms it
 *                        while the other half lands; 0 = the plain [row][column] tiles.  Only the placement of the data in the
 *                        workspace and the order of independent work differ: results are bit-identical.
 *   "exp"                0 .. 255 (default 0): development switch for A/B runs of kernel variants under test in ONE process
 *                        (tools/dev_*.py); a shipped library has no reader of it.
 * Values outside an option's range and unknown names return B4D_EINVAL; the options are atomics, read once per entry-point call. */
int b4d_set_option(const char* name, int value);
/* 1 if (ny, nx) has a plan: powers of two in [64, 4096] (radix FFT kernels); any sides <= 512 (DFT-matrix products);
 * sides <= 8192 that split as 2^k * A * B with A + B <= 128 (fused in-LDS mixed radix) or any other side <= 4096
 * (Bluestein over that transform), at most 2^26 pixels. */
int b4d_size_supported(int ny, int nx);
/* Which kernels a plan from b4d_plan_create runs for (ny, nx), as flag bits; 0 for a size without a plan.  No GPU call: the plan
 * constructor and the entry points branch on the same bits, so a test can assert the route of a shape where it cannot run it.
 * Exactly one of POW2, WMR, FUSED, DFTMAT and PMROWS is set for a supported size. */
#define B4D_ROUTE_POW2 0x01u        /* power-of-two pipeline: radix FFT kernels, half spectrum between row and column pass */
#define B4D_ROUTE_PARITY 0x02u      /* ny == 2048: PSD + autocorrelation can take the parity tiles (options ysplit, row16, colsets) */
#define B4D_ROUTE_WMR 0x04u         /* both sides have compiled three-radix kernels: the three-kernel mixed-radix route */
#define B4D_ROUTE_FUSED 0x08u       /* a side beyond 512, both sides split as 2^k * A * B: fused half-spectrum route */
#define B4D_ROUTE_DFTMAT 0x10u      /* both sides <= 512: DFT-matrix products */
#define B4D_ROUTE_PMROWS 0x20u      /* a side beyond 512 and a side without such a split: full complex row transforms per axis */
#define B4D_ROUTE_BLUESTEIN_Y 0x40u /* (with PMROWS) ny has no 2^k * A * B split: its transforms run through Bluestein */
#define B4D_ROUTE_BLUESTEIN_X 0x80u /* the same for nx */
unsigned b4d_size_route(int ny, int nx);

/* Plans ------------------------------------------------------------------------------
 * A plan owns the twiddle tables and a workspace of `chunk` half-spectra
 * (chunk * ny * nx/2 complex64; general-length plans: three full complex buffers).  Batches larger
 * than `chunk` are processed chunk by chunk.                                            */
int b4d_plan_create(int ny, int nx, int chunk, b4d_plan** out);
int b4d_plan_destroy(b4d_plan* plan);
size_t b4d_plan_workspace_bytes(const b4d_plan* plan);

/* signal/fft.py:198-237 fft2d -- F = fftshift(fft2(img)) for a batch of real frames.
 * out: (batch, ny, nx) complex64 interleaved (re, im).                                  */
int b4d_fft2d(b4d_plan* plan, const float* frames, int batch, float* out_c64, void* stream);

/* Complex frames (signal/fft.py:198-258 accept complex input): plans from b4d_plan_create_general run the
 * general-length engines (DFT matrices up to 512, fused mixed radix beyond) for every size, powers of two included.
 * inverse == 0: out = fftshift(fft2(in));  inverse != 0: out = ifft2(ifftshift(in)), i.e. ifft2d of a shifted spectrum.
 * in / out: DEVICE (batch, ny, nx) complex64 (interleaved float pairs).                                               */
int b4d_plan_create_general(int ny, int nx, int chunk, b4d_plan** out);
int b4d_fft2d_c2c(b4d_plan* plan, const float* in_c64, int batch, int inverse, float* out_c64, void* stream);

/* signal/fft.py:261-309 psd2d -- P = |fftshift(fft2(img))|^2 * scale, scale = dx*dy/(nx*ny)
 * when scale=True else 1.  psd: (batch, ny, nx) float32.                                */
int b4d_psd2d(b4d_plan* plan, const float* frames, int batch, float* psd, float scale, void* stream);

/* signal/corr.py:256-320 autocorr2d -- circular autocorrelation, shifted, float32.
 * With B4D_NORM_PEAK the zero-lag sample is exactly 1.0f.                               */
int b4d_autocorr2d(b4d_plan* plan, const float* frames, int batch, float* autocorr, unsigned flags,
                   void* stream);

/* The north-star pipeline: one forward transform serves psd2d and
 * autocorr2d.  Either output pointer may be NULL.                                       */
int b4d_psd_autocorr2d(b4d_plan* plan, const float* frames, int batch, float* psd, float psd_scale,
                       float* autocorr, unsigned flags, void* stream);

/* Same call, but every kernel launch is bracketed by HIP events on `stream`; the elapsed times
 * (ms) of {row R2C, column FFT/PSD/inverse, zero-lag peak, row C2R} are ADDED to kernel_ms[0..3].
 * Synchronises the stream before returning.  Measurement aid for bench.py's roofline block.    */
int b4d_psd_autocorr2d_timed(b4d_plan* plan, const float* frames, int batch, float* psd, float psd_scale,
                             float* autocorr, unsigned flags, void* stream, float* kernel_ms);

/* Workspace placement (power-of-two plans; a no-op returning B4D_OK on the others).  Where a multi-GB allocation lands in
 * device memory decides 5-10 % of the time of every kernel that streams through it -- a property of the allocation that
 * stays with it until it is freed (same code, same virtual layout, two hipMalloc's of one process).
 * The plan owns its half-spectrum workspace, so it can measure: up to `candidates` - 1 (at most 7) further workspaces are
 * allocated one after the other, the caller's own b4d_psd_autocorr2d call is timed with each (two passes after an untimed
 * one), the fastest stays with the plan and the others are freed.  An allocation failure only ends the search.  Synchronises
 * `stream`; on return psd / autocorr hold the result of a normal call.  best_ms / worst_ms (optional) receive the time per
 * pass on the kept and on the slowest candidate.  All candidates are alive until the choice is made: up to
 * (candidates - 1) x b4d_plan_workspace_bytes of extra device memory for the duration of the call.
 * A diagnostic since round 3: five consecutive processes on one box ran the untuned plan within 0.3 % of the tuned one
 * (profiles/r03_placement.txt), and bench.py no longer calls it (only `--tune-compare K` does, after its timed region).        */
int b4d_plan_tune(b4d_plan* plan, const float* frames, int batch, float* psd, float psd_scale, float* autocorr,
                  unsigned flags, int candidates, float* best_ms, float* worst_ms, void* stream);

/* signal/corr.py:169-253 xcorr2d -- fftshift(ifft2(fft2(a) * conj(fft2(b)))), real part,
 * float32, scaled 1/(nx*ny) like ifft2.  B4D_REMOVE_MEAN zeroes the DC bin of the cross
 * spectrum (= both means removed), B4D_NORM_PEAK divides by max|corr|.                   */
int b4d_xcorr2d(b4d_plan* plan, const float* a, const float* b, int batch, float* corr, unsigned flags,
                void* stream);

/* signal/tracking.py:191-297 phase_correlation (backend="internal") for `npairs` (image,
 * template) pairs.  images: (nimg, ny, nx) raw frames.  Templates are ROIs of the frames in
 * tpl_src (ntplsrc, ny, nx): template k = frame tpl_frame[k], rows [roi[4k], roi[4k+1]),
 * columns [roi[4k+2], roi[4k+3]).  Pair i correlates image pair_img[i] with template
 * pair_tpl[i].  Every distinct image and template is transformed ONCE.  z-scoring
 * (tracking.py:308-311), zero-embedding (geometry/roi.py:175-222), whitening, |ifft2|,
 * first-occurrence arg-max, peak, exact median for the SNR (tracking.py:314-321) and the 3x3
 * Taylor step (324-375, including its swapped corrections) all run on the device.
 * The index arrays (tpl_frame, tpl_roi, pair_img, pair_tpl) are HOST pointers; out
 * (npairs, 4) float64 rows {dy, dx, peak, snr} and peak_ij (npairs, 2) int32 (nullable) are
 * DEVICE pointers.                                                                        */
int b4d_phase_correlation(b4d_plan* plan, const float* images, int nimg, const float* tpl_src, int ntplsrc,
                          const int32_t* tpl_frame, const int32_t* tpl_roi, int ntpl, const int32_t* pair_img,
                          const int32_t* pair_tpl, int npairs, int subpixel, double eps, double* out,
                          int32_t* peak_ij, void* stream);

/* signal/tracking.py:81-188 template_matching: zero-mean normalised cross-correlation of z-scored templates with
 * full frames over the "valid" window positions (the arithmetic of cv2.matchTemplate(TM_CCOEFF_NORMED) /
 * skimage.feature.match_template(pad_input=False), which the reference imports), first-occurrence arg-max, peak,
 * snr = |peak| / (median |ncc| + eps), 3x3 Taylor step, centre-to-centre shift against each template's ROI.
 * Same operands as b4d_phase_correlation, plus img_h x img_w: the extent of the images inside the plan's (ny, nx)
 * power-of-two canvas (0 = the whole canvas; frames of other sizes are zero-padded by the caller, which is exact for
 * the "valid" correlation).  zscore_image != 0: the image is z-scored as a whole ("opencv" path,
 * tracking.py:157); 0: raw float32 image ("skimage" path, tracking.py:166).  out: DEVICE (npairs, 4) float64
 * {dy, dx, peak, snr}; peak_ij: DEVICE (npairs, 2) int32 arg-max in the (ny-h+1, nx-w+1) map, or null.            */
int b4d_template_match(b4d_plan* plan, const float* images, int nimg, const float* tpl_src, int ntplsrc,
                       const int32_t* tpl_frame, const int32_t* tpl_roi, int ntpl, const int32_t* pair_img,
                       const int32_t* pair_tpl, int npairs, int img_h, int img_w, int zscore_image, int subpixel, double eps,
                       double* out, int32_t* peak_ij, void* stream);

/* Dense NCC displacement map (barc4dip_amd.signal.displacement_map): for every pair z (reference frame pair_ref[z], image
 * frame pair_img[z]) and every window of the grid y0 = search_y + k * step_y (all k with y0 + win_y + search_y <= h; likewise
 * for x) the result of template_matching(ref[y0:y0+win_y, x0:x0+win_x], img[y0-search_y:y0+win_y+search_y, x0-search_x:...],
 * slices_yx=(slice(search_y, search_y+win_y), slice(search_x, search_x+win_x))): zero-mean NCC over the
 * (2 search_y + 1) x (2 search_x + 1) local shifts, first-occurrence arg-max, peak, snr = |peak| / (median |ncc| + eps),
 * 3x3 Taylor step for subpixel = 1 (swapped corrections included, as the reference), the same step with each correction on
 * its own axis for subpixel = 2 (Newton), none for 0.  zscore_image != 0: each search box is z-scored ("opencv", tracking.py:157);
 * 0: raw box ("skimage").  Direct space, one workgroup per window, one launch for all pairs, on `stream`.
 * ref (nref, h, w), img (nimg, h, w): DEVICE float32 frames.  pair_ref, pair_img (npairs,): HOST int32 indices.
 * out: DEVICE (npairs, gy, gx, 4) float64 {dy, dx, peak, snr}; peak_ij: DEVICE (npairs, gy, gx, 2) int32 arg-max in the map,
 * or null.  Limits: 1 <= win <= 128 and 1 <= search <= 32 per axis (B4D_ESIZE beyond), step >= 1, at least one window
 * (B4D_EINVAL otherwise), gy and npairs <= 65535.                                                                          */
int b4d_displacement_map(const float* ref, int nref, const float* img, int nimg, const int32_t* pair_ref,
                         const int32_t* pair_img, int npairs, int h, int w, int win_y, int win_x, int step_y, int step_x,
                         int search_y, int search_x, int zscore_image, int subpixel, double eps, double* out, int32_t* peak_ij,
                         void* stream);

/* Distortion correction (barc4dip_amd.preprocessing.distortion; the reference reserves it in preprocessing/distortion.py):
 * out[t, y, x] = scipy.ndimage.map_coordinates(frame t, [y + dy(t, y, x), x + dx(t, y, x)], order, mode, cval) in float32.
 * mode: 0 "nearest", 1 "reflect", 2 "mirror", 3 "constant" (cval where y + dy or x + dx lies outside [0, side - 1]).
 * order: 0, 1, or 3 (cubic B-spline).  All on `stream`, one launch per pass for the whole stack.
 * b4d_spline_prefilter: the order-3 coefficients of src (n, h, w) for `mode` into coef (n, h + 2 p, w + 2 p), p = 12 for
 *   "nearest" (scipy's edge padding), else 0: separable truncated FIR sqrt(3) (sqrt(3) - 2)^|k|, |k| <= 14 (2.4e-8 of scipy's
 *   recursive filter).  Limits: n <= 65535, h <= 262140, w + 2 p <= 16384 (B4D_ESIZE beyond).
 * b4d_warp_dense / b4d_warp_grid: src is the frames (n, h, w) for order 0 and 1, the coefficients of b4d_spline_prefilter with
 *   the SAME mode for order 3.  field_frames = 1: one field for every frame; = n: field plane t warps frame t.
 *   dense: dy, dx (field_frames, h, w) per-pixel displacements.
 *   grid: dy, dx (field_frames, gy, gx) at window centres y0 + i step_y, x0 + j step_x; the field at (y, x) is
 *   map_coordinates(grid, [(y - y0) / step_y, (x - x0) / step_x], order=1, mode="nearest"), evaluated in the kernel.
 *   Taps and weights come from the float32 displacement, not from a float32 absolute coordinate.  out (n, h, w).
 *   Limits: n <= 65535, h <= 262140 (B4D_ESIZE); gy, gx >= 1, finite non-zero steps (B4D_EINVAL).                          */
int b4d_spline_prefilter(const float* src, int n, int h, int w, int mode, float* coef, void* stream);
int b4d_warp_dense(const float* src, int n, int h, int w, int order, int mode, float cval, const float* dy, const float* dx,
                   int field_frames, float* out, void* stream);
int b4d_warp_grid(const float* src, int n, int h, int w, int order, int mode, float cval, const float* dy, const float* dx,
                  int field_frames, int gy, int gx, double y0, double step_y, double x0, double step_x, float* out,
                  void* stream);

/* Temporal per-pixel statistics (io/rw.py:129-132 for the mean).
 * accumulate: sum_x += sum_t x, sum_xx += sum_t x^2 over `nframes` frames of npix pixels
 * (float64 accumulators, caller zero-initialises; any npix / alignment).  finalize: mean, var (ddof 0),
 * contrast = sqrt(var)/mean as float32 maps from the (all-reduced) sums.                */
int b4d_temporal_accumulate(const float* frames, int nframes, size_t npix, double* sum_x, double* sum_xx,
                            void* stream);
int b4d_temporal_finalize(const double* sum_x, const double* sum_xx, double count, size_t npix, float* mean,
                          float* var, float* contrast, void* stream);
/* accumulate on pixels [pix0, pix0 + npix) of frames that are frame_stride pixels apart (row chunks of an image, so that
 * the all-reduce of finished rows overlaps the accumulation of the rest); sum_x / sum_xx point at the
 * accumulators of pixel pix0.  Any pixel count and alignment (odd frame sizes take a dword kernel). */
int b4d_temporal_accumulate_range(const float* frames, int nframes, size_t frame_stride, size_t pix0, size_t npix,
                                  double* sum_x, double* sum_xx, void* stream);
/* finalize with the frame count read from DEVICE memory: the count travels in the same all-reduced float64 buffer as the
 * sums, so the host never waits for it. */
int b4d_temporal_finalize_dev(const double* sum_x, const double* sum_xx, const double* count_dev, size_t npix, float* mean,
                              float* var, float* contrast, void* stream);

/* metrics/statistics.py:17-125 distribution_moments + speckles.py:640-645 visibility inputs:
 * per-frame finite-only power sums in float64.
 * out: (batch, 8) float64 {n_finite, sum, sum2(centered), sum3(centered), sum4(centered), n_zero, n_sat, min}... see DESIGN.md */
int b4d_moments(const float* frames, int batch, size_t npix, double eps, double saturation, double* out,
                void* stream);

/* metrics/sharpness.py:405-530 tenengrad + laplacian_variance: scipy.ndimage sobel/laplace
 * with mode="reflect", fused with their reductions.
 * out: (batch, 4) float64 {mean(gx^2), mean(gy^2), mean(lap), mean(lap^2)} over finite pixels. */
int b4d_sobel_laplace_stats(const float* frames, int batch, int ny, int nx, double* out, void* stream);

/* preprocessing/normalize.py:12-145 flat_field_correction, float32 arithmetic in the reference's order:
 *   b4d_stack_mean_f32   :86-93  mean of a (frames, npix) flat / dark stack along axis 0 (NumPy's float32 reduction
 *                                order: sequential adds in frame order, one division)
 *   b4d_flat_den         :107-113 den = F - D (D = 0 when dark is null); mask_bad != 0 writes NaN where den <= eps
 *                                (input of the median / mean selections, which skip NaN)
 *   b4d_flat_field       :115-132 out = ((I - D) / (F - D)) * scale, 0 where F - D <= eps; flat null: I - D
 *   b4d_repair_pixels    :134-140 replaces the listed pixels (idx: DEVICE int64 linear indices into one frame) by the
 *                                3x3 median (scipy "reflect") of the frame as it was on entry.  Synchronises the stream. */
int b4d_stack_mean_f32(const float* stack, int frames, size_t npix, float* out, void* stream);
int b4d_flat_den(const float* flat, const float* dark, size_t npix, float eps, int mask_bad, float* den, void* stream);
int b4d_flat_field(const float* frames, int batch, size_t npix, const float* flat, const float* dark, float eps, float scale,
                   int apply_scale, float* out, void* stream);
int b4d_repair_pixels(float* frames, int batch, int ny, int nx, const long long* idx, int nbad, void* stream);

/* images.astype(np.float32) on the device for raw detector words staged through pinned memory (barc4dip_amd/ingest.py):
 * dtype 0 u8, 1 u16, 2 i16, 3 i32, 4 u32, 5 f32, 6 f64.  src / dst: DEVICE, n elements. */
int b4d_to_f32(const void* src, int dtype, size_t n, float* dst, void* stream);

/* metrics/sharpness.py:752-861 eigenvalues (STA2): J = (x - mean(x)) / ||x||_2, eig_i = s_i(J)^2 / (M N - 1).
 * The reference takes every singular value from LAPACK and uses the first k (default 5); this returns the leading
 * nout (<= 8) of them, descending, from the Gram matrix of the smaller side (MFMA) and a 32-vector block subspace
 * iteration with float64 Cholesky-QR / Rayleigh-Ritz; frames with min(ny, nx) < 64 take every eigenvalue of the Gram
 * matrix from a parallel cyclic Jacobi in float64.
 * frames: DEVICE (batch, ny, nx) float32.  out: HOST (batch, nout) float64; NaN rows for frames holding non-finite
 * pixels or no energy.  Synchronises the stream.                                                                  */
int b4d_sta2_eigenvalues(const float* frames, int batch, int ny, int nx, double* out, int nout, void* stream);

/* utils/range.py:44-54 percentile_minmax_range / np.nanpercentile (linear interpolation): exact selection
 * of the two bracketing order statistics of the non-NaN pixels of every frame.  q: HOST array of nq (<= 16)
 * percentiles in [0, 100].  out: DEVICE (batch, nq, 4) float64 {x_lo, x_hi, fraction, n_valid}.
 * Rank and fraction come from NumPy's virtual index for method="linear", evaluated in NumPy's operation order with
 * individually rounded operations: vi = n*qf + (1 + qf*(1 - 1 - 1)) - 1 with qf = q/100 and n = n_valid;
 * x_lo = s[lo], lo = floor(vi) clamped to [0, n-1]; x_hi = s[min(lo + 1, n-1)]; fraction = vi - floor(vi).
 * The caller finishes like NumPy's _lerp in float64 with THIS fraction (x_lo + (x_hi - x_lo) * fraction, or
 * x_hi - (x_hi - x_lo) * (1 - fraction) for fraction >= 0.5); a fraction recomputed from another rank formula can
 * belong to a different pair.  A frame without a non-NaN pixel gives {NaN, NaN, 0, 0}.  Synchronises the stream.  */
int b4d_percentiles(const float* frames, int batch, size_t npix, const double* q, int nq, double* out, void* stream);

/* maths/radial.py:101-169 radial_mean_interpolated: nr x ntheta polar samples, bilinear interpolation on the
 * pixel-centre grid, zero outside, mean over theta.  out: DEVICE (batch, nr) float64.                      */
int b4d_radial_profile(const float* maps, int batch, int ny, int nx, int nr, int ntheta, double r_max, double* out,
                       void* stream);

/* metrics/speckles.py:669-817 bandwidth + metrics/sharpness.py:536-629 spectral_entropy from a shifted PSD
 * map (DC bin treated as zero).  out: DEVICE (batch, 8) float64 {S_disc, sum FR^2 P, sum FX^2 P, sum FY^2 P,
 * sum P^2 (all four over the inscribed frequency disc), S_all, sum P ln P (all bins), f95 (square maps; NaN when
 * ny != nx)}.                                                                                                  */
int b4d_psd_stats(const float* psd, int batch, int ny, int nx, double* out, void* stream);

/* preprocessing/filters.py:17-289 deconvolve_psf, method="wiener" (BASELINE.json config 5).
 * create: frame shape (h, w), PSF (ky, kx odd; HOST pointer, row-major float32, filters.py:217-230), Wiener-Hunt
 *   regularisation `balance` (skimage.restoration.wiener, Laplacian regulariser).  The padded size (h + 2*(ky/2),
 *   w + 2*(kx/2)) may be any integer whose odd part is <= 4200 (4096 + 8 = 4104 = 8 * 513 for sigma 1.5).
 * apply: per frame reflect-pad, divide by max|.|, filter in the Fourier domain of the padded size, clip to [-1, 1]
 *   (if clip), rescale, crop -> out (batch, h, w) float32.  Ordering is that of `stream`: a call with batch > 1 runs
 *   alternate frames on two plan-owned streams that wait for the work already queued on `stream` and that `stream`
 *   waits for before anything queued after the call (no host synchronisation).                                  */
typedef struct b4d_wiener b4d_wiener;
int b4d_wiener_create(int h, int w, const float* psf, int ky, int kx, float balance, b4d_wiener** out);
int b4d_wiener_apply(b4d_wiener* plan, const float* frames, int batch, float* out, int clip, void* stream);
int b4d_wiener_destroy(b4d_wiener* plan);

/* preprocessing/filters.py:270-277 method="rl": Richardson-Lucy deconvolution as published for
 * skimage.restoration.richardson_lucy (parity unpinned) with the reference's reflect padding by half the kernel,
 * normalisation by max|frame| and crop (filters.py:252-261, 287-289).  frames/out: DEVICE (batch, h, w) float32;
 * psf: HOST (ky, kx) float32, odd sides <= 33; filter_epsilon <= 0: none.  Synchronises the stream.            */
int b4d_richardson_lucy(const float* frames, int batch, int h, int w, const float* psf, int ky, int kx, int num_iter,
                        float filter_epsilon, int clip, float* out, void* stream);

/* preprocessing/filters.py:278-286 method="uw": ONE Gibbs sweep of skimage.restoration.unsupervised_wiener (published
 * algorithm, parity unpinned and stochastic: the reference passes no rng) over the unitary half-plane spectrum.  All pointers
 * DEVICE.  y, tf, x_sample (optional), postmean: (ny, nxh) complex64 (rfft2 layout, nxh = nx/2 + 1); areg2: (ny, nxh) float32
 * = |Laplacian transfer function|^2; r1 / r2: (ny, nxh) float32 standard normals, or both null: generated on the device
 * (Philox-4x32-10, key `seed`, counter = element and sweep).  Does
 *   x = gn conj(tf) / (gn |tf|^2 + gx areg2) * y + sqrt(0.5 / (..)) (r1 + i r2);  postmean += x for sweep > burnin
 * and leaves in sums4 (4 doubles): ||y - x tf||^2, ||x L||^2 (half-plane weights as the library's image_quad_norm),
 * sum |postmean/(sweep-burnin) - previous/(sweep-burnin-1)| and sum |postmean| (0 before they are defined).  The Gamma
 * draws of the two precisions and the loop belong to the caller.  Asynchronous on `stream`.                       */
int b4d_uw_step(const void* y, const void* tf, const float* areg2, void* x_sample, void* postmean, const float* r1,
                const float* r2, unsigned long long seed, int sweep, int burnin, float gn, float gx, int ny, int nxh,
                double* sums4, void* stream);

/* Wavefront reconstruction (barc4dip_amd/signal/wavefront.py; no counterpart in the reference, which stops at the shift map).
 * b4d_integrate_gradient: least-squares integration of the slope fields gy = d phi / dy, gx = d phi / dx given on the nodes of a
 *   regular (ny, nx) grid with spacings hy, hx > 0, in Southwell geometry: the slope on the edge between two neighbouring nodes
 *   is the mean of the two node slopes, and phi is the zero-mean minimiser of
 *     sum ((phi[i+1][j] - phi[i][j]) / hy - gbar_y[i][j])^2 + sum ((phi[i][j+1] - phi[i][j]) / hx - gbar_x[i][j])^2.
 *   Solved exactly through the orthonormal DCT-II, which diagonalises the 5-point Neumann Laplacian of the normal equations:
 *   one elementwise launch for the right-hand side and four float32 matrix products on the matrix cores for the whole batch.
 *   gy, gx, out: DEVICE (n, ny, nx) float32, out distinct from gy and gx; workspace: DEVICE, b4d_integrate_workspace_bytes(n, ny, nx)
 *   bytes (0 for an unsupported shape).  Sides 1 .. 2048 (B4D_ESIZE beyond), n <= 65535.  Non-finite input propagates.
 *   Asynchronous on `stream`; the DCT basis of a side is built on first use (float64 on the host, a blocking upload) and cached.
 * b4d_poly2_fit: least-squares fit of c0 + c1 u + c2 v + c3 u^2 + c4 u v + c5 v^2 to every map w (n, ny, nx), with
 *   u = (j - (nx-1)/2) / max((nx-1)/2, 1) along x and v likewise along y (both in [-1, 1]); float64 moments on the device, the
 *   inverse Gram matrix of the grid from the host.  A term that a side of 1 or 2 nodes cannot tell from the earlier ones gets 0.
 *   coeff: DEVICE (n, 6) float64.  residual (DEVICE (n, ny, nx) float32, may be w itself) and rms (DEVICE (n) float64) are
 *   optional, both or neither: residual = scale * (w - the terms whose bit is set in remove_mask, bit k for c_k), rms = its
 *   population standard deviation.  Asynchronous on `stream`. */
size_t b4d_integrate_workspace_bytes(int n, int ny, int nx);
int b4d_integrate_gradient(const float* gy, const float* gx, int n, int ny, int nx, double hy, double hx, void* workspace,
                           float* out, void* stream);
int b4d_poly2_fit(const float* w, int n, int ny, int nx, unsigned remove_mask, double scale, double* coeff, float* residual,
                  double* rms, void* stream);

/* Weighted and masked wavefront reconstruction.
 * b4d_integrate_gradient_weighted: as b4d_integrate_gradient with a weight w >= 0 per node.  A node whose weight is not finite
 *   and positive, or whose gy or gx is not finite, has weight 0 and its slopes are never read into a result.  Edge weights are
 *   the harmonic mean 2ab / (a + b) of the two node weights (0 if either is 0); phi minimises
 *     sum wy ((phi[i+1][j] - phi[i][j]) / hy - gbar_y[i][j])^2 + sum wx ((phi[i][j+1] - phi[i][j]) / hx - gbar_x[i][j])^2.
 *   Solved by conjugate gradients from phi = 0, preconditioned with the unweighted DCT solve, which fixes the gauge: the
 *   minimiser of smallest unweighted Laplacian energy with zero mean over the grid (disconnected pieces are levelled against
 *   each other, not measured; weight-0 nodes are filled harmonically).  float32 vectors; dot products, alpha and beta in float64
 *   on the device, reduced in a fixed order, so a map gives the same bits alone and inside any batch.  A map stops when its
 *   recurrence residual |r| <= rtol |b|, when b = 0, or when p.Ap is not finite and positive; the call stops after max_iter
 *   iterations or when every map has stopped (the host reads one int per map every 4 iterations: the call waits for `stream`).
 *   w: DEVICE float32, (n, ny, nx) with w_stride = ny * nx or one (ny, nx) map shared by the batch with w_stride = 0.
 *   nan_invalid != 0 writes NaN at the weight-0 nodes of out, else they keep the harmonic fill.  iterations: DEVICE (n) int32;
 *   residual: DEVICE (n) float64, the final |r| / |b| (0 for b = 0).  workspace: DEVICE,
 *   b4d_integrate_weighted_workspace_bytes(n, ny, nx) bytes (0 for an unsupported shape), 256-byte aligned; after the call its
 *   first n * ny * nx floats hold the effective node weights.  Limits and errors as b4d_integrate_gradient.
 * b4d_poly2_fit_weighted: b4d_poly2_fit with node weights (layout as above; not finite and positive counts as 0, and the map is
 *   not read there): the weighted moments of the map in float64 on the device, where one lane solves the 6 x 6 system with the
 *   factorisation and drop rule of the unweighted fit (a map with a single valid row gets no v terms).  u, v are the full-grid
 *   coordinates.  rms = sqrt(sum w r^2 / sum w - (sum w r / sum w)^2), NaN without a valid node; nan_invalid != 0 writes NaN at
 *   the weight-0 nodes of residual. */
size_t b4d_integrate_weighted_workspace_bytes(int n, int ny, int nx);
int b4d_integrate_gradient_weighted(const float* gy, const float* gx, const float* w, long long w_stride, int n, int ny, int nx,
                                    double hy, double hx, double rtol, int max_iter, int nan_invalid, void* workspace, float* out,
                                    int* iterations, double* residual, void* stream);
int b4d_poly2_fit_weighted(const float* w_map, const float* weights, long long weight_stride, int n, int ny, int nx,
                           unsigned remove_mask, double scale, int nan_invalid, double* coeff, float* residual, double* rms,
                           void* stream);

/* Modal fits of wavefront maps (barc4dip_amd/signal/modal.py).
 * Geometry, basis-agnostic: node (i, j) has v = (i - cy) * sy along y and u = (j - cx) * sx along x.
 *   basis 0, Zernike: modes 1 .. n_modes in Noll's order and normalisation (rms 1 over the unit disc, even j the cosine, theta from
 *     +x towards +y) in rho = hypot(u, v); the caller passes sy = dy / radius, sx = dx / radius.  Nodes with rho^2 > 1 + 1e-9 have
 *     weight 0.
 *   basis 1, Legendre: sqrt(2a+1) sqrt(2b+1) P_a(u) P_b(v), ordered by total degree a + b and within a degree by growing b; the
 *     caller passes sy = 1 / max(cy, 1), sx = 1 / max(cx, 1).
 *   The modes are evaluated in float64 by recurrence (no trigonometry, no division by rho); 1 <= n_modes <= 66 (B4D_ESIZE beyond).
 * b4d_modal_fit: weighted least-squares coefficients of every map.  maps: DEVICE (n, ny, nx) float32.  weights: DEVICE float32,
 *   (n, ny, nx) with weight_stride = ny * nx, one shared (ny, nx) map with weight_stride = 0, or null for all ones.  A node whose
 *   weight is not finite and positive, or whose map value is not finite, has weight 0 and its map value enters no sum.  The
 *   normal equations [A phi]^T W [A phi] are accumulated in float64 on the matrix cores, per chunk of nodes, and the chunks are
 *   added in a fixed order that depends on (ny, nx, n_modes) alone: a map gives the same bits alone and inside any batch.  They
 *   are factored by Cholesky without pivoting in mode order; a mode whose remainder after the kept ones is not above 1e-12 of
 *   its own diagonal entry, or whose diagonal entry is not > 0, is dropped and gets coefficient 0.  coeff: DEVICE (n, n_modes)
 *   float64; kept: DEVICE (n, n_modes) bytes, 1 for a kept mode.  workspace: DEVICE, b4d_modal_workspace_bytes(n, ny, nx, n_modes)
 *   bytes (0 for an unsupported shape), 8-byte aligned.
 * b4d_modal_residual: out = scale * (map - sum of c_j mode_j over the modes with remove[j] != 0; remove: DEVICE n_modes bytes
 *   shared by the batch, null removes all), evaluated in float64 and stored as float32 (out may be maps itself).
 *   rms: DEVICE (n) float64, sqrt(sum w r^2 / sum w - (sum w r / sum w)^2) of the stored values over the nodes of positive weight,
 *   NaN without one.  nan_invalid != 0 writes NaN at the weight-0 nodes, else the subtraction is evaluated there too, outside the
 *   disc included (a map value that is not finite stays so).  valid: DEVICE (n, ny, nx) bytes or null, 1 at the nodes of positive
 *   weight.  workspace as for b4d_modal_fit; the rms partials of the workgroups live in it, in a part the fit does not use.
 * b4d_modal_eval: out (DEVICE (n, ny, nx) float32) = sum of c_j mode_j, coeff DEVICE (n, n_modes) float64; nothing is masked.
 * Sides 1 .. 2048 (B4D_ESIZE beyond), n <= 65535.  Asynchronous on `stream`; the table of recurrence coefficients is built on
 * first use (float64 on the host, a blocking upload) and cached per device and basis. */
size_t b4d_modal_workspace_bytes(int n, int ny, int nx, int n_modes);
int b4d_modal_fit(const float* maps, const float* weights, long long weight_stride, int n, int ny, int nx, int basis, int n_modes,
                  double cy, double cx, double sy, double sx, void* workspace, double* coeff, unsigned char* kept, void* stream);
int b4d_modal_residual(const float* maps, const float* weights, long long weight_stride, int n, int ny, int nx, int basis,
                       int n_modes, double cy, double cx, double sy, double sx, const double* coeff, const unsigned char* remove,
                       double scale, int nan_invalid, void* workspace, float* out, double* rms, unsigned char* valid, void* stream);
int b4d_modal_eval(const double* coeff, int n, int ny, int nx, int basis, int n_modes, double cy, double cx, double sy, double sx,
                   float* out, void* stream);

/* Focal spot and caustic of a measured wavefront (barc4dip_amd/signal/focus.py): the Fresnel integral of
 * one pupil per (map, plane) pair as a zero-padded 2-D DFT on the canvas (Py, Px) of a plan from b4d_plan_create_general.
 * Node (i, j) of map t has v = (i - (ny-1)/2) hy along y and u = (j - (nx-1)/2) hx along x (metres) and the phase, in float64,
 *   phi = (2 pi / wavelength) (err + c0 + c1 u + c2 v + c3 u^2 + c4 u v + c5 v^2) + (pi / (wavelength z)) (u^2 + v^2),
 * c = coeff[t], z = z[k] the signed distance of plane k from the measurement plane.  The pupil A exp(i phi) -- A = amp, or 1
 * without one -- sits at [0:ny, 0:nx] of the zero canvas; a node whose err is not finite, or whose amp is not finite and > 0,
 * is outside the aperture (pupil 0, no part in any sum).  The plane's intensity is I = |fftshift(fft2(canvas))|^2 / (sum A)^2,
 * sum A over the valid nodes of the map in float64: the unit is the peak of the aberration-free, in-focus pupil of the same
 * amplitude, so the peak of I is the Strehl ratio, and sum I = Py Px sum A^2 / (sum A)^2.
 *   err: DEVICE (n, ny, nx) float32, metres.  amp: DEVICE float32 or NULL; (n, ny, nx) with amp_stride = ny * nx, or one map
 *   shared by all with amp_stride = 0.  coeff: DEVICE (n, 6) float64.  z: HOST (nz) float64, each finite and non-zero (read
 *   before the call returns).  ny <= Py, nx <= Px; Py, Px <= 4096.
 *   intensity: NULL, or DEVICE (n, nz, cy, cx) float32: the window of cy x cx bins centred on the DC bin, rows
 *   Py/2 - cy/2 .. Py/2 - cy/2 + cy - 1 of the shifted plane and likewise along x; cy <= Py, cx <= Px.
 *   stats: DEVICE (n, nz, 10) float64 over the WHOLE canvas, p and q the integer bin offsets from the DC bin along y and x:
 *     [0] sum I   [1] peak of I   [2] first index of the peak in row-major order of the shifted plane (row * Px + column)
 *     [3] sum I p   [4] sum I q   [5] sum I p^2   [6] sum I q^2   [7] sum I p q   [8] sum A   [9] sum A^2
 *   marg_x: NULL or DEVICE (n, nz, Px) float64, the sum of I over the rows; marg_y: NULL or DEVICE (n, nz, Py), over the columns;
 *   both in shifted order.  A map without a valid node gets NaN in [0] .. [7], in its marginals and in its intensity, no error.
 *   workspace: DEVICE, b4d_focal_spot_workspace_bytes(plan, n, nz) bytes (0 for a plan or counts that cannot run), 256-byte
 *   aligned.  The pairs pass through the plan's buffers `chunk` at a time; every sum is taken in an order fixed by (Py, Px), so
 *   the results are the same bits from run to run and for any chunk.  Asynchronous on `stream`.
 * B4D_EINVAL: a plan that is not general, a map larger than the canvas, a crop larger than the canvas, nz < 1, a z that is 0 or
 * not finite, a wavelength or spacing that is not finite and positive. */
size_t b4d_focal_spot_workspace_bytes(const b4d_plan* plan, int n, int nz);
int b4d_focal_spot(b4d_plan* general_plan, const float* err, const float* amp, long long amp_stride, int n, int ny, int nx,
                   const double* coeff, double hy, double hx, double wavelength, const double* z, int nz, int cy, int cx,
                   float* intensity, double* stats, double* marg_x, double* marg_y, void* workspace, void* stream);

/* Fringe analysis of grating interferograms (barc4dip_amd/signal/fringes.py).
 * Window grid: origins y0 = Y sty for every Y with y0 + wy <= H (gy of them), likewise x0 = X stx (gx); no search margin.
 * Taper: the half-sample Hann h_w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / w), j = 0 .. w-1.
 * b4d_fringe_demodulate: for every frame and carrier f_k = (fy, fx) = carriers[2k], carriers[2k+1] (HOST float64, cycles per
 *   pixel, read before the call returns) the harmonic map
 *     S_k[Y][X] = sum_j sum_i h_wy[j] h_wx[i] I[y0+j][x0+i] exp(-2 pi i (fy (y0+j) + fx (x0+i))) / (sum h_wy . sum h_wx)
 *   with ABSOLUTE pixel coordinates in the phase, whose argument is reduced modulo 1 in float64 before it is rounded to float32.
 *   frames: DEVICE (n, H, W) float32.  out: DEVICE (n, n_carriers + 1, gy, gx) complex64; plane 0 is S_0, the same sum with
 *   f = 0 (imaginary part 0), plane k + 1 is S_k.  1 <= n_carriers <= 4; windows 2 .. 256 px per axis (B4D_ESIZE beyond), steps
 *   >= 1, n <= 65535.  float32 sums in an order fixed by the geometry: a frame gives the same bits alone and inside any batch.
 *   workspace: DEVICE, b4d_fringe_demodulate_workspace_bytes(n_carriers, H, W, wy, wx) bytes (0 for unsupported arguments),
 *   256-byte aligned: the taper and phasor tables, written by the call.
 * b4d_fringe_compare: elementwise on harmonic maps.  sample: DEVICE (n, n_carriers + 1, gy, gx) complex64.  reference: the same
 *   with reference_stride = (n_carriers + 1) gy gx (one per sample), one set shared by all with reference_stride = 0, or NULL
 *   (absolute mode).  Per node and carrier k:
 *     phase[k] = arg(S_k conj R_k) in (-pi, pi] (arg S_k in absolute mode)      visibility[k] = 2 |S_k| / S_0
 *     transmission = S_0 / R_0      dark_field[k] = (|S_k| / S_0) / (|R_k| / R_0)      peak = min_k visibility[k]
 *   phase, visibility, dark_field: DEVICE (n, n_carriers, gy, gx) float32; transmission: DEVICE (n, gy, gx) float32; peak: DEVICE
 *   (n, gy, gx) float64.  transmission and dark_field are required with a reference and not written without one.
 * b4d_phase_unwrap: least-squares unwrapping with a congruence step, per map.  The wrapped differences W(a) = a - 2 pi round(a / 2 pi)
 *   of neighbouring nodes along y and x are the edge slopes of the 5-point Neumann Poisson problem of b4d_integrate_gradient
 *   (unit spacings, no Southwell means); its zero-mean solution p, shifted to equal the input at node (ny / 2, nx / 2), selects
 *   the level: out = phase + 2 pi round((p - phase) / 2 pi).  The data are never smoothed, and a node whose level is 0 keeps its
 *   bits.  Whole-grid and unweighted: a node that is not finite spoils its map (b4d_phase_unwrap_weighted below takes weights
 *   and masks).  phase, out: DEVICE (n, ny, nx) float32, distinct;
 *   workspace: DEVICE, b4d_phase_unwrap_workspace_bytes(n, ny, nx) bytes (0 for an unsupported shape).  Sides 1 .. 2048
 *   (B4D_ESIZE beyond), n <= 65535.
 * b4d_fringe_shift: (dy, dx) = -Minv (phase1, phase2) / 2 pi per node, in float64.  minv: HOST 4 float64, row-major inverse of
 *   M = [[f1y, f1x], [f2y, f2x]].  phase1, phase2: DEVICE float32, map m at offset m * stride (stride >= gy gx); dy, dx: DEVICE
 *   (n, gy, gx) float64.
 * All four are asynchronous on `stream` and have no host fallback. */
size_t b4d_fringe_demodulate_workspace_bytes(int n_carriers, int H, int W, int wy, int wx);
int b4d_fringe_demodulate(const float* frames, int n, int H, int W, const double* carriers, int n_carriers, int wy, int wx, int sty,
                          int stx, void* workspace, void* out, void* stream);
int b4d_fringe_compare(const void* sample, const void* reference, long long reference_stride, int n, int n_carriers, int gy, int gx,
                       float* phase, float* visibility, float* transmission, float* dark_field, double* peak, void* stream);
size_t b4d_phase_unwrap_workspace_bytes(int n, int ny, int nx);
int b4d_phase_unwrap(const float* phase, int n, int ny, int nx, void* workspace, float* out, void* stream);
int b4d_fringe_shift(const float* phase1, const float* phase2, long long stride, int n, int gy, int gx, const double* minv, double* dy,
                     double* dx, void* stream);

/* Weighted and masked phase unwrapping.
 * b4d_phase_unwrap_weighted: b4d_phase_unwrap with a weight w >= 0 per node (layout, w_stride, limits, rtol, max_iter, iterations
 *   and residual as b4d_integrate_gradient_weighted, and the same conjugate-gradient solver).  A node whose weight is not finite
 *   and positive, or whose phase is not finite, has weight 0 and its phase is never read into a result.  Edge weights are the
 *   harmonic means of the node weights, edge slopes the wrapped differences (unit spacings), and p minimises
 *     sum wy (p[i+1][j] - p[i][j] - W(phase[i+1][j] - phase[i][j]))^2 + sum wx (p[i][j+1] - p[i][j] - W(phase[i][j+1] - phase[i][j]))^2
 *   in the gauge of section 14.  Seed node: the valid node of largest weight, ties to the smallest (i - ny/2)^2 + (j - nx/2)^2, then
 *   to the smallest row-major index (with equal weights: node (ny / 2, nx / 2)).  p is shifted to equal the input at the seed and
 *   out = phase + 2 pi round((p - phase) / 2 pi) at the valid nodes; a valid node whose level is 0 keeps its bits.  Weight-0 nodes
 *   get NaN (nan_invalid != 0) or the shifted p.  Pieces of the valid region that no edge connects are levelled against each
 *   other as smoothly as possible: their relative level is NOT measured.  A map without a valid node is NaN, 0 iterations.
 *   phase, out: DEVICE (n, ny, nx) float32, distinct.  workspace: DEVICE, b4d_phase_unwrap_weighted_workspace_bytes(n, ny, nx)
 *   bytes (0 for an unsupported shape), 256-byte aligned; after the call its first n * ny * nx floats hold the effective node
 *   weights.  The call waits for `stream` every 4 iterations, as the weighted integration does.
 * b4d_fringe_weights: node weights of the phase maps from the harmonic maps of b4d_fringe_demodulate (sample, reference and
 *   reference_stride as b4d_fringe_compare; reference may be NULL).  A node is valid if S_0 >= min_level * (largest finite S_0 of
 *   its frame), likewise R_0 within the reference frame, and if every visibility 2 |S_k| / S_0 and 2 |R_k| / R_0, over all
 *   carriers, is >= min_visibility; a threshold of 0 switches its test off (0 <= min_level <= 1, min_visibility >= 0).  The tests
 *   are made in float64.  w_out: DEVICE (n, n_carriers, gy, gx) float32, 0 at nodes that are not valid, else for carrier k
 *     mode 0: 1      mode 1: 1 / (S_0 / |S_k|^2 + R_0 / |R_k|^2), without a reference |S_k|^2 / S_0
 *   (the inverse shot-noise variance of the phase up to a constant), 0 where that is not finite and positive.  The frame maxima
 *   are reduced in two stages on the device.  workspace: DEVICE, b4d_fringe_weights_workspace_bytes(n, gy, gx) bytes.
 * b4d_fringe_shift_levels: b4d_fringe_shift from the wrapped maps and their unwrapped copies (all DEVICE float32, map m at offset
 *   m * stride): the phase is formed again in float64 as wrapped + 2 pi round((unwrapped - wrapped) / 2 pi), so the half spacing
 *   that the float32 unwrapped phase carries at tens of radians does not reach the shift; NaN where an unwrapped map is NaN.
 * All are asynchronous on `stream` apart from the waits named above and have no host fallback. */
size_t b4d_phase_unwrap_weighted_workspace_bytes(int n, int ny, int nx);
int b4d_phase_unwrap_weighted(const float* phase, const float* w, long long w_stride, int n, int ny, int nx, double rtol, int max_iter,
                              int nan_invalid, void* workspace, float* out, int* iterations, double* residual, void* stream);
size_t b4d_fringe_weights_workspace_bytes(int n, int gy, int gx);
int b4d_fringe_weights(const void* sample, const void* reference, long long reference_stride, int n, int n_carriers, int gy, int gx,
                       double min_level, double min_visibility, int mode, float* w_out, void* workspace, void* stream);
int b4d_fringe_shift_levels(const float* wrapped1, const float* wrapped2, const float* unwrapped1, const float* unwrapped2,
                            long long stride, int n, int gy, int gx, const double* minv, double* dy, double* dx, void* stream);

/* Transmission and dark-field maps of speckle tracking (barc4dip_amd.signal.speckle_contrast): the weighted
 * moments of every window of a reference frame and of the image window that its tracked displacement points at.
 * Grid and pairing are those of b4d_displacement_map with margin in the place of search: origins y0 = margin_y + k * step_y for
 * every k with y0 + win_y + margin_y <= h, likewise for x; pair z compares reference frame pair_ref[z] with image frame
 * pair_img[z] (HOST int32, read before the call returns); ref (nref, h, w), img (nimg, h, w): DEVICE float32.
 * dy, dx: DEVICE float64 displacements in pixels.  LAYOUT: field_stride is the offset (in doubles) from the field of one pair to
 * that of the next and must be n * gy * gx with an integer n >= 1 (B4D_EINVAL otherwise); n is the stride between neighbouring
 * nodes: node (Y, X) of pair z is read at dy[z * field_stride + (Y * gx + X) * n], the same for dx.  Two planar (npairs, gy, gx)
 * maps have field_stride = gy * gx; the (npairs, gy, gx, 4) output `o` of b4d_displacement_map is passed without a copy as
 * dy = o, dx = o + 1, field_stride = 4 * gy * gx.
 * Per window: r[j][i] = ref[y0+j][x0+i]; s[j][i] = the image at (y0 + j + dy, x0 + i + dx), the convention of
 * b4d_warp_grid: the image window displaced by the tracked shift matches the reference window.  order 0 takes the pixel at
 * floor(d + 0.5) per axis; order 1 is bilinear with the taps floor(d), floor(d) + 1 and the weights 1 - f, f for
 * f = d - floor(d), formed and combined in float64; a tap whose weight is exactly 0 is not read.  taper 0 is flat, 1 the
 * half-sample Hann h_w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / w) per axis.  With the weights h[j][i] = h_wy[j] h_wx[i] normalised
 * to sum 1 the weighted means Rm, Sm, variances VR, VS and covariance C are formed in float64 from power sums shifted by the
 * window's first pixel.  out: DEVICE (npairs, gy, gx, 6) float64
 *   0 transmission = Sm / Rm                         3 correlation = C / sqrt(VS VR)
 *   1 dark_field = (sqrt(VS) / Sm) / (sqrt(VR) / Rm)   4 visibility_ref = sqrt(VR) / Rm
 *   2 dark_field_fit = C / (VR transmission)         5 visibility = sqrt(VS) / Sm
 * dark_field is the visibility ratio (noise raises it), dark_field_fit the least-squares slope of s on r over the transmission.
 * A quantity whose denominator is not above 0 is NaN, and so is the square root of a variance that is not above 0: a window
 * without contrast (a single pixel, a constant patch) has a transmission and nothing else.  A window whose displacement is not
 * finite, or whose taps of non-zero weight would leave [0, h - 1] x [0, w - 1], gets six NaNs and no address is formed for it;
 * |d| <= margin always stays inside.  One launch, grid (gx, gy, npairs), one workgroup per window, on `stream`; the summation
 * order depends on the window shape alone, so a frame gives the same bits alone and inside any batch.
 * Limits: 1 <= win <= 128 and 0 <= margin <= 32 per axis (B4D_ESIZE beyond), step >= 1, order and taper 0 or 1, at least one
 * window (B4D_EINVAL otherwise), gy and npairs <= 65535.  All argument errors are returned before any launch.              */
int b4d_speckle_contrast(const float* ref, int nref, const float* img, int nimg, const int32_t* pair_ref,
                         const int32_t* pair_img, int npairs, int h, int w, int win_y, int win_x, int step_y, int step_x,
                         int margin_y, int margin_x, const double* dy, const double* dx, long long field_stride, int order,
                         int taper, double* out, void* stream);

/* Two-time correlation of a speckle stack (barc4dip_amd.metrics.two_time_correlation).
 * Input is a stack x[t, p] of T >= 2 frames, p over the npix = H W pixels, and an optional label map: label 0 takes no part,
 * labels 1 .. R name regions (q-rings, mirror zones, detector modules); values outside 0 .. R count as 0.  Region r is the set
 * P_r of pixels that carry label r and are FINITE IN ALL T FRAMES, N_r = |P_r|.  Per region, in exact arithmetic:
 *   m_i    = (1/N) sum_p x_ip                          var_i = cov_ii
 *   cov_ij = (1/N) sum_p (x_ip - m_i)(x_jp - m_j)      contrast_i = sqrt(var_i) / m_i
 *   norm B4D_TWO_TIME_PEARSON:    C_ij = cov_ij / sqrt(var_i var_j)
 *   norm B4D_TWO_TIME_INTENSITY:  C_ij = 1 + cov_ij / (m_i m_j)     (= <I_i I_j> / (<I_i><I_j>), the XPCS two-time function)
 *   norm B4D_TWO_TIME_COVARIANCE: C_ij = cov_ij
 *   g2[tau]     = mean of C_ij over the computed entries with j - i = tau (n_tau = T - tau of them), tau = 0 .. L
 *   g2_err[tau] = population standard deviation of those entries / sqrt(n_tau)
 * A quotient whose denominator is not above 0 is NaN, and so is the square root of a variance that is not above 0: a constant
 * frame is a NaN row and column under PEARSON but finite under COVARIANCE, a frame of mean 0 is NaN under INTENSITY.  N_r = 0
 * gives NaN everywhere for that region and n_pixels = 0; it is not an error.  The matrix is exactly symmetric (both triangles
 * are written from one value); under PEARSON the diagonal is exactly 1.0 wherever var_i > 0.  max_lag = L (0 <= L <= T - 1):
 * entries with |i - j| > L are NaN, frame-block pairs (blocks of 128 frames) wholly outside the band are not computed, entries
 * inside the band are bit-identical to the full run.
 * Arithmetic: the data is centred before the product, Xc = x - c[r][i] with c the float32-rounded mean of the region's pixels
 * that are finite in frame i; the float32 matrix cores (v_mfma_f32_32x32x2_f32) take the products over chunks of 2048 pixels of
 * the region's raster-ordered pixel list (float32 chains of 256 products, eight of them added per chunk), and everything across
 * chunks, the sums s_i of the stored values and the correction
 * cov_ij = Gc_ij / N - (s_i / N)(s_j / N), m_i = c_i + s_i / N is float64.  Every sum runs in an order fixed by (T, npix,
 * max_lag) and the region's own pixel list: the same bits from run to run, and for a region alone or among others.
 * stack: DEVICE (T, npix) float32; labels: DEVICE npix int32 or NULL (then n_regions must be 1 and every pixel is region 1);
 * two_time: DEVICE (R, T, T) float64; mean, var: DEVICE (R, T) float64; n_pixels: DEVICE (R) int64; workspace: DEVICE,
 * b4d_two_time_workspace_bytes(T, npix, n_regions, max_lag) bytes (0 for an unsupported shape): the packed centred copy
 * T (npix / 2048 + R) 2048 floats, one 128 x 128 float tile per (chunk, frame-block pair), and the per-span partial sums.
 * b4d_two_time_lags reads a matrix stack in that layout.  Asynchronous on `stream`, no host synchronisation.
 * Limits: 2 <= T <= 2048, R <= 64, npix < 2^31 (B4D_ESIZE beyond); all argument errors are returned before any launch.   */
#define B4D_TWO_TIME_PEARSON 0
#define B4D_TWO_TIME_INTENSITY 1
#define B4D_TWO_TIME_COVARIANCE 2
size_t b4d_two_time_workspace_bytes(int T, long long npix, int n_regions, int max_lag);
int b4d_two_time(const float* stack, int T, long long npix, const int* labels, int n_regions, int norm, int max_lag, void* workspace,
                 double* two_time, double* mean, double* var, long long* n_pixels, void* stream);
/* The same call with HIP events on `stream` around its stages; waits for the last one.  stage_ms: HOST float[4], the milliseconds
 * of the scan (labels, sums, offsets), the pack (counts, prefix, packed copy, its sums), the product and the reduction with the
 * normalisation (tools/bench_two_time.py). */
int b4d_two_time_timed(const float* stack, int T, long long npix, const int* labels, int n_regions, int norm, int max_lag,
                       void* workspace, double* two_time, double* mean, double* var, long long* n_pixels, void* stream, float* stage_ms);
int b4d_two_time_lags(const double* two_time, int n_regions, int T, int max_lag, double* g2, double* g2_err, void* stream);

/* Multi-tau correlation of a long or streamed speckle stack (barc4dip_amd.metrics.multi_tau_correlation).
 * Input is a stack x[t, p] of T >= 2 frames that arrives in pushes, and an optional label map with the rules of b4d_two_time:
 * label 0 takes no part, labels 1 .. R name regions, values outside 0 .. R count as 0.  Region r is the set of pixels that carry
 * label r and are FINITE IN ALL T FRAMES, N their number.  m = lags per level, one of 8, 16, 32.
 *   Levels.  I_0[k] = x[k], T_0 = T;  I_l[k] = (I_{l-1}[2k] + I_{l-1}[2k+1]) / 2 in float32, T_l = floor(T / 2^l): a last
 *            unpaired frame of a level never forms a frame of the next.
 *   Lags.    Level 0 has j = 0 .. m - 1, level l >= 1 has j = m/2 .. m - 1; the delay is tau = j 2^l frames.  Level l >= 1
 *            exists while T_l >= m/2 + 1, and max_level caps the last level used.  A lag is reported when n = T_l - j >= 1, in
 *            the order of level, then j.  T = 37, m = 16: 25 lags, delays 0 .. 15, 16, 18 .. 30, 32 (the last with n = 1).
 *            T = 100 000, m = 16: 116 lags, the last delay 90 112 frames.
 *   Sums over the region's pixels and k = 0 .. n - 1:
 *            P = sum I_l[k] I_l[k+j]    Q = sum (I_l[k] I_l[k+j])^2    A = sum I_l[k]    B = sum I_l[k+j]
 *   g2     = (P / Nn) / ((A / Nn)(B / Nn))                                 (the symmetric normalisation)
 *   g2_err = sqrt(max(Q / Nn - (P / Nn)^2, 0) / (Nn)) / ((A / Nn)(B / Nn)) (the standard error of the mean product IF the products
 *            were independent: a lower bound on the real error)
 *   mean[r] = the mean of the region over all T level-0 frames.
 * A quotient whose denominator is not above 0 is NaN in both g2 and g2_err; an empty region is NaN with n_pixels = 0.
 * Arithmetic: a lane owns a pixel and sums its products in float32 over runs of 8 frames; everything across runs, lanes, waves
 * and pushes is float64.  There are no atomics: every wave adds into a slot of its own, and the slots of a region are summed in
 * wave order.  A and B are formed as S - (the level's last j frames) and S - (its first j frames) from float64 frame sums.
 * Every sum runs in an order fixed by T, npix, the label map, m and the sequence of push lengths: the same bits from run to run,
 * and for a region alone or among others.
 * Calls, all stateless, DEVICE pointers throughout, asynchronous on `stream`, no host synchronisation:
 *   scan    ORs "non-finite in some frame of frames (n, npix)" into bad[p] (npix bytes, zeroed by the caller); once per chunk.
 *   init    builds the region-ordered pixel list (raster order within a region, regions start on a wave boundary) from labels
 *           (npix int32 or NULL: then n_regions must be 1) and bad (or NULL), and zeroes the state.
 *   push    consumes frames (n, npix) float32 after t0 earlier frames, 1 <= n <= max_push, any parity.  The cascade state follows
 *           from t0: level l has received floor(t0 / 2^l) frames and holds an unpaired frame when that is odd.  Per level and
 *           used pixel the workspace carries the last m - 1 frames (the newest of them is the unpaired frame) and, per wave,
 *           the float64 sums.
 *   finish  T = frames pushed; n_levels as b4d_multi_tau_lags returns it for (T, m, max_level).  g2, g2_err: (R, n_lags) float64,
 *           mean: (R) float64, n_pixels: (R) int64.
 *   lags    HOST helper and the one definition of the lag table: fills lags, levels, n_pairs (n_lags entries each, or NULL) and
 *           *n_levels (or NULL), returns n_lags, or a negative error code.  max_level < 0: no cap.
 * workspace: b4d_multi_tau_workspace_bytes(npix, n_regions, m, n_levels, max_push) bytes (0 for an unsupported shape): per level
 * m frames of npix + 64 R floats, two scratch buffers of max_push / 2 and max_push / 4 such frames, and the per-wave sums.
 * Limits: m in {8, 16, 32}, R <= 64, npix < 2^31, T < 2^31, at most 24 levels (B4D_ESIZE beyond).                          */
size_t b4d_multi_tau_workspace_bytes(long long npix, int n_regions, int m, int n_levels, int max_push);
int b4d_multi_tau_lags(long long T, int m, int max_level, long long* lags, int* levels, long long* n_pairs, int* n_levels);
int b4d_multi_tau_scan(const float* frames, int n, long long npix, unsigned char* bad, void* stream);
int b4d_multi_tau_init(const int* labels, const unsigned char* bad, long long npix, int n_regions, int m, int n_levels, int max_push,
                       void* workspace, void* stream);
int b4d_multi_tau_push(const float* frames, long long t0, int n, long long npix, int n_regions, int m, int n_levels, int max_push,
                       void* workspace, void* stream);
int b4d_multi_tau_finish(long long T, long long npix, int n_regions, int m, int n_levels, int max_push, void* workspace, double* g2,
                         double* g2_err, double* mean, long long* n_pixels, void* stream);

/* Spatial rank filters (scipy.ndimage.median_filter / rank_filter / percentile_filter on every frame of (batch, ny, nx) float32),
 * the range-only variant behind utils/range.py:14-86, fused outlier repair, and the uint16 scaling of utils/dtype.py:15-53.
 * A rank filter is a selection: on finite input the output equals SciPy's bit for bit.  NaN sorts above +Inf and -0 below +0
 * (np.sort's order; SciPy leaves NaN unspecified).  DEVICE pointers throughout, asynchronous on `stream`, no synchronisation.
 * b4d_rank_filter: out[t, y, x] = the rank-th smallest (0-based) of the size_y x size_x window placed as SciPy places it (offsets
 *   -(size / 2) .. size - 1 - size / 2 per axis), 1 <= size <= 15, 0 <= rank < size_y * size_x.
 *   mode: the codes of b4d_warp_* -- 0 "nearest", 1 "reflect", 2 "mirror", 3 "constant" (cval) -- and 4 "wrap", with SciPy's
 *   meanings, for any overhang (a window larger than the frame reflects or wraps repeatedly).
 *   flags bit 0: take the general route (32 counting passes per output) also where the register route applies (the median of
 *   3 x 3, 5 x 5, 7 x 7); both are exact, so the outputs are identical.
 *   out: (batch, ny, nx) or NULL.  minmax: (batch, 2) float32 {nanmin, nanmax} of every filtered frame, NaN for a frame whose
 *   filtered values are all NaN, or NULL; with out == NULL nothing but minmax is written (4 B per pixel of traffic).  The
 *   reduction is integer min / max on ordered keys: deterministic.
 * b4d_despeckle: out = median of the size x size window (size 3, 5 or 7) where the centre pixel x is an outlier, else x.  With
 *   med the window median and d = x - med, in float32 and in this operation order:
 *     scale_kind 0 "absolute": |d| > threshold
 *     scale_kind 1 "mad"     : |d| > threshold * max(1.4826f * mad, min_scale), mad = median of |w_i - med| over the same window
 *     scale_kind 2 "poisson" : d * d > (threshold * threshold) * max(med, min_scale), the square formed in float32 on the host
 *   (max as np.maximum: NaN stays NaN).  polarity 0 both, 1 hot (and d > 0), 2 dead (and d < 0); a non-finite centre pixel is
 *   always an outlier.  mask: (batch, ny, nx) bytes, 1 = replaced, or NULL.  counts: (batch) int64 replaced pixels per frame
 *   (integer adds), or NULL.  threshold >= 0, min_scale >= 0.
 * b4d_scale_to_u16: out[i] = (uint16) clip((in[i] - vmin) * inv, 0, 65535), truncated: the subtraction in float32; the product
 *   in float64 rounded once to float32 when mul_f64 (NumPy's float32 array times a float64 scalar), else in float32 by
 *   (float) inv.  NaN -> 0.
 * B4D_EINVAL: sizes, rank, mode or kinds out of range, batch < 1, overlapping buffers (in == out), no output at all.        */
int b4d_rank_filter(const float* in, int batch, int ny, int nx, int size_y, int size_x, int rank, int mode, float cval, int flags,
                    float* out, float* minmax, void* stream);
int b4d_despeckle(const float* in, int batch, int ny, int nx, int size, int scale_kind, float threshold, float min_scale, int polarity,
                  int mode, float cval, float* out, unsigned char* mask, long long* counts, void* stream);
int b4d_scale_to_u16(const float* in, size_t n, float vmin, double inv, int mul_f64, unsigned short* out, void* stream);

/* Phase-stepping analysis of grating scans (barc4dip_amd.signal.stepping).  A scan is (T, npix) float32, a
 * stack of scans (n, T, npix).  Per pixel, with step phases phi_t and K = harmonics in {1, 2}, M = 2K + 1:
 *   I_t = a0 + sum_k (c_k cos k phi_t + s_k sin k phi_t),   a_k = hypot(c_k, s_k),   phi_k = atan2(-s_k, c_k).
 * basis: HOST (T, M) float64, row t = (1, cos phi_t, sin phi_t, cos 2 phi_t, sin 2 phi_t); gram: HOST (M, M) = basis^T basis;
 * gram_inv: HOST (M, M), its inverse, or NULL if it has none (every pixel then takes the per-pixel solve).  A sample is dropped
 * for its pixel if it is not finite or >= saturation (+inf: no level).  A pixel without a dropped sample gets gram_inv b with
 * b = sum_t B_t I_t; one with dropped samples is solved by Cholesky of gram - sum_dropped B_t B_t^T.  It is valid if at least M
 * samples are kept and every pivot exceeds 1e-10 times the largest diagonal entry; otherwise its coefficients and residual are
 * NaN.  All sums are float64, in the order of t.
 * b4d_stepping_fit: coeff DEVICE (n, M, npix) float32 in the order (a0, c_1, s_1, c_2, s_2); residual DEVICE (n, npix) float32,
 *   sqrt(max(sum I^2 - b^T x, 0) / n_kept); n_samples DEVICE (n, npix) bytes, the kept samples.  3 <= T <= 64 (B4D_ESIZE),
 *   T >= M.  16-byte accesses where npix is a multiple of 4 and stack, coeff, residual are 16-byte aligned (n_samples 4-byte),
 *   dword accesses otherwise; the results are the same bits.
 * b4d_stepping_compare: elementwise on coefficient maps.  With reference (DEVICE (M, npix) and reference_stride 0, or
 *   (n, M, npix) and reference_stride M * npix): phase = wrap_(-pi, pi](phi_k,s - phi_k,r) formed in float64, visibility and
 *   visibility_ref = a_k / a0 of sample and reference, dark_field their quotient (all (n, K, npix) float32), transmission =
 *   a0_s / a0_r (n, npix), valid (n, K, npix) bytes = both pixels valid, both a0 > 0 and a_k,r > 0; amplitude (sample) optional.
 *   Without reference (NULL): phase = phi_k, visibility and amplitude of the sample; valid (optional) = the pixel is valid;
 *   transmission, visibility_ref, dark_field must be NULL.
 * b4d_stepping_calibrate_step: one iteration of the step self-calibration (K = 1, 5 <= T <= 32) on one scan: one pass over the
 *   stack fits (a0, c, s) with basis / gram_inv (HOST, formed from the current steps delta, HOST (T)), sums over the pixels
 *   without a dropped sample the products a0 I_t, c I_t, s I_t and the 3 x 3 matrix of (a0, c, s), and one workgroup solves
 *   I_t(p) ~ g_t a0(p) + u_t c(p) + v_t s(p) and sets delta_t <- atan2(v_t, u_t) - atan2(v_0, u_0), unwrapped towards the
 *   previous delta_t.  out: DEVICE 1 + 3 T float64: max |change|, the new delta (T), the dose factors g (T), the modulations
 *   hypot(u, v) (T); NaN throughout if no pixel takes part.  Works in the library's per-stream scratch buffer.
 * No float atomics, every cross-lane and cross-workgroup sum in a fixed order: the same bits from run to run.  Asynchronous on
 * `stream`, no host synchronisation; all argument errors are returned before any launch.                                    */
int b4d_stepping_fit(const float* stack, int n, int T, long long npix, int harmonics, const double* basis, const double* gram,
                     const double* gram_inv, double saturation, float* coeff, float* residual, unsigned char* n_samples, void* stream);
int b4d_stepping_compare(const float* sample, const float* reference, long long reference_stride, int n, int harmonics, long long npix,
                         float* phase, float* visibility, float* amplitude, float* transmission, float* visibility_ref,
                         float* dark_field, unsigned char* valid, void* stream);
int b4d_stepping_calibrate_step(const float* stack, int T, long long npix, const double* basis, const double* gram_inv,
                                const double* delta, double saturation, double* out, void* stream);

/* Speckle scanning (speckle-vector tracking, "UMPA") at detector resolution (barc4dip_amd.signal.speckle_scan; DESIGN.md
 * section 24).  ref (n, h, w) and samples (m, n, h, w): DEVICE float32, the same n diffuser positions without and with the
 * sample, m scans against one reference; weights: DEVICE (n,) float64, g[n] >= 0 and not all 0 (the caller checks; a scan
 * without a position of weight above 0 comes back NaN).  A position of weight 0 is never read.
 * Taper per axis h_w[j] = 1 (taper 0) or 0.5 - 0.5 cos(2 pi (j + 0.5) / w) (taper 1); pooled weights
 * W[n][j][i] = g[n] h_wy[j] h_wx[i] / (sum g sum h_wy sum h_wx).  For pixel p and the shift u = (uy, ux), |uy| <= search_y,
 * |ux| <= search_x, the reference window is centred on p and the sample window on p + u (the convention of
 * b4d_displacement_map); Rm, VR are the mean and variance of R[n][p + .] under W, Sm(u), VS(u) those of S[n][p + u + .] and
 * C(u) the covariance of the two, all pooled over n and the window.  rho(u) = C(u) / sqrt(VR VS(u)); a candidate is undefined
 * when VR <= 1e-12 Rm^2 or VS(u) <= 1e-12 Sm(u)^2.  The peak u* is the defined candidate of largest rho, the first in row-major
 * order (uy, then ux ascending) among equals.  With subpixel = 1 each axis adds d = 0.5 (a - c) / (a - 2 b + c) clipped to
 * +-0.5 from a, b, c = rho(u* - e), rho(u*), rho(u* + e); d = 0 when a - 2 b + c >= 0, when a neighbour is undefined or when
 * u* lies on the border of the search range on that axis (which also sets the edge flag, with subpixel = 0 too).
 * out: DEVICE (m, 6, h, w) float64, planar:
 *   0 dy, 1 dx = u* + d     2 correlation = rho(u*)     3 transmission = Sm(u*) / Rm
 *   4 dark_field = C(u*) / (VR transmission)            5 flags: 1.0 valid, + 2.0 edge
 * A pixel is NaN in planes 0 .. 4 with flags 0 when its margin (win / 2 + search per axis) leaves the frame, when a reference
 * value of its window or a sample value of its window grown by the search is not finite in a position of weight above 0, or
 * when no candidate is defined; such a value counts as 0 for every other pixel, which keeps the bits it has with 0 in its place.
 * All sums are float64, of values shifted by one pixel of the workgroup's tile; each product R_n[q] S_n[q + u] is formed once
 * and shared by the windows that cover q through a separable filter.  Two launches on `stream`, no atomics, every sum in a fixed
 * order: a scan gives the same bits alone and inside any batch.  Works in the library's per-stream scratch buffer
 * (16 (1 + m) h w bytes).
 * Limits: odd win <= 31, 0 <= search <= 16 per axis, n <= 4096 (B4D_ESIZE beyond); an even window, a frame smaller than
 * win + 2 search, m > 65534 or h w >= 2^31: B4D_EINVAL.  All argument errors are returned before any launch.               */
int b4d_speckle_scan(const float* ref, const float* samples, int m, int n, int h, int w, int win_y, int win_x, int search_y,
                     int search_x, const double* weights, int taper, int subpixel, double* out, void* stream);

/* Per-pixel order statistics along the frame axis of a stack (barc4dip_amd.metrics.order, barc4dip_amd.preprocessing.combine;
 * DESIGN.md section 25).  stack: DEVICE (T, npix) float32, frames frame_stride >= npix elements apart; the caller offsets the base
 * pointers to address a pixel range (the convention of b4d_temporal_accumulate_range).  Per pixel the samples are sorted in
 * np.sort's order (NaN above +Inf, -0 below +0).
 * b4d_temporal_quantiles: q HOST, n_q fractions in [0, 1], 1 <= n_q <= 8; out DEVICE (n_q, npix) float32; n_valid DEVICE (npix)
 *   uint16, the non-NaN samples per pixel, or NULL.  nan_policy 0 "propagate": all T samples take part and a pixel with any NaN
 *   is NaN in every output (np.percentile, np.median); 1 "omit": the n non-NaN samples take part, n = 0 gives NaN
 *   (np.nanpercentile, np.nanmedian).  With s[0 .. n) the sorted samples taking part and h = q (n - 1) in float64, method
 *     0 linear: i = floor(h), g = h - i      1 lower: i = floor(h), g = 0      2 higher: i = ceil(h), g = 0
 *     3 nearest: i = rint(h), half to even, g = 0      4 midpoint: i = floor(h), g = 0.5 if h > i, else 0.
 *   g == 0: the result is s[i] itself; otherwise (float) (a + (b - a) g), a = (double) s[i], b = (double) s[i + 1], the
 *   difference, product and sum each rounded once in float64.  The median is q = 0.5 with the midpoint method.
 * b4d_temporal_robust_mean: a sample that is not finite takes no part (it sorts as NaN and is always rejected); n is the count of
 *   finite samples, med the midpoint median of them (NaN for n = 0), d_t = x_t - med in float32, mad the midpoint median of
 *   |d_t|.  A sample is rejected, in float32 and in b4d_despeckle's operation order, when
 *     scale_kind 0 "absolute": |d| > threshold
 *     scale_kind 1 "mad"     : |d| > threshold * max(1.4826f * mad, min_scale)
 *     scale_kind 2 "poisson" : d * d > (threshold * threshold) * max(med, min_scale), the square formed in float32 on the host
 *   (max as np.maximum), restricted by polarity 0 both, 1 hot (and d > 0), 2 dead (and d < 0).  If more than half of a pixel's
 *   samples are equal, mad is 0: with min_scale = 0 every differing sample is then rejected.
 *   mean (npix) float32 = (float) (sum of the kept x_t / n_kept) in float64, NaN for n_kept = 0; the kept samples are added in
 *   eight partial sums, partial s over t = s, s + 8, .. in ascending t, joined as ((P0 + P1) + (P2 + P3)) + ((P4 + P5) + (P6 + P7)).
 *   Optional (NULL to skip): median (npix) float32; scale (npix) float32, the right-hand side of the test that was applied;
 *   n_kept (npix) uint16; rejected (T, npix) bytes and cleaned (T, npix) float32 (a rejected sample replaced by med), both with
 *   rows out_stride >= npix elements apart.
 * Limits: 1 <= T <= 1024 (B4D_ESIZE above).  B4D_EINVAL: frame_stride or out_stride < npix, a q outside [0, 1] or not finite,
 *   n_q, method, nan_policy, scale_kind, polarity or flags out of range, a negative (or NaN) threshold or min_scale, an output
 *   that overlaps the stack.  All argument errors are returned before any launch.
 * T <= 64 sorts the samples in registers (one read of the stack; wide accesses where npix, the strides and every base allow,
 *   dword accesses otherwise); longer stacks, and any T with flags bit 0, select by counting on a tile in LDS.  Both routes and
 *   all access widths give the same bits.  No atomics; asynchronous on `stream`, no host synchronisation.                     */
int b4d_temporal_quantiles(const float* stack, int T, long long frame_stride, long long npix, const double* q, int n_q, int method,
                           int nan_policy, int flags, float* out, unsigned short* n_valid, void* stream);
int b4d_temporal_robust_mean(const float* stack, int T, long long frame_stride, long long npix, int scale_kind, float threshold,
                             float min_scale, int polarity, int flags, float* mean, float* median, float* scale, unsigned short* n_kept,
                             unsigned char* rejected, float* cleaned, long long out_stride, void* stream);

/* Linear separable filters and local statistics on every frame of (batch, ny, nx) float32 (barc4dip_amd.preprocessing.smooth,
 * barc4dip_amd.metrics.contrast).  Frames and outputs are DEVICE pointers, the taps HOST float64 arrays
 * that are read before the call returns (they travel in the kernel arguments); asynchronous on `stream`, no synchronisation.
 * mode and cval: the codes and meanings of b4d_rank_filter (0 nearest, 1 reflect, 2 mirror, 3 constant, 4 wrap), for any overhang.
 * b4d_separable_filter: a correlation with SciPy's placement (scipy.ndimage.correlate1d, origin 0) along x, then along y:
 *     r[y, x] = sum_k wx[k] in[y, x - n_x / 2 + k]        g[y, x] = sum_k wy[k] r[y - n_y / 2 + k, x]
 *   (integer division: an even window is one sample longer on the left).  The border rule of the second pass sees r, as SciPy's
 *   sequence of 1-D filters does: under "constant" a row of r outside the frame is cval.  Each tap is rounded once to float32; a
 *   sum starts with its first product and adds the others by float32 FMA in ascending k, on both routes, which therefore give
 *   the same bits.  An axis with n = 1 and w = {1} is skipped.  Non-finite input propagates as IEEE arithmetic does: a NaN
 *   poisons exactly the outputs whose windows contain it, taps that are zero included.
 *   epilogue, applied in the last pass to g and the input pixel x: 0 out = g; 1 out = x - g; 2 out = x / max(g, eps) (max as
 *   np.maximum: a NaN g stays).  1 <= n <= 511 per axis.
 *   flags bit 0: take the two-pass route (row kernel -> the library's per-stream scratch buffer, at most 128 MiB of it -> column
 *   kernel) also where the fused route (one launch, both passes in LDS) applies: half-widths up to 4, i.e. n <= 9 per axis.
 *   flags bit 1: take the fused route up to n <= 49 per axis (what its kernel can hold; for timing the boundary).
 *   16-byte accesses to memory where nx % 4 == 0 and the base is 16-byte aligned, dword accesses otherwise; the same bits.
 * b4d_local_stats: windowed mean, population variance and contrast of the size_y x size_x window (1 .. 63 per axis, SciPy's
 *   placement) of the frame padded in two dimensions by the border rule.  taps_y = taps_x = NULL: box window, S1 = sum x,
 *   S2 = sum x * x, W = size_y size_x.  Otherwise both are given (size_y and size_x float64 taps): S1 = sum wy wx x,
 *   S2 = sum wy wx x * x, W = sum wy wx, summed by the same code.  x * x is formed in float64 (exact) and every sum is float64,
 *   along x, then along y, in ascending tap order.  mean = S1 / W, variance = max(S2 / W - mean * mean, 0) (a NaN stays),
 *   contrast = sqrt(variance) / mean where mean > 0, NaN elsewhere; each (batch, ny, nx) float32 or NULL.  On integer-valued
 *   frames the box sums are exact.  One launch, one read of the stack.
 * No atomics: a frame gives the same bits alone and inside any batch.  All argument errors are returned before any launch:
 * B4D_EINVAL for tap counts, sizes, mode or epilogue out of range, batch < 1, a null frame or tap pointer, an output that overlaps
 * the input (in == out), no output at all; B4D_ESIZE where ny * nx >= 2^31.                                                  */
int b4d_separable_filter(const float* in, int batch, int ny, int nx, const double* taps_y, int n_y, const double* taps_x, int n_x,
                         int mode, float cval, int epilogue, float eps, int flags, float* out, void* stream);
int b4d_local_stats(const float* in, int batch, int ny, int nx, int size_y, int size_x, const double* taps_y, const double* taps_x,
                    int mode, float cval, float* mean, float* variance, float* contrast, void* stream);

/* How close every frame of img (batch, ny, nx) float32 is to a reference frame (barc4dip_amd.metrics.perceptual; DESIGN.md
 * section 28).  All pointers are DEVICE pointers except the taps (HOST float64, read before the call returns: they travel in the
 * kernel arguments); asynchronous on `stream`, no synchronisation.  ref_stride is the element stride between reference frames:
 * 0 = one reference frame serves the whole batch, ny * nx = the frames are paired (any stride >= ny * nx is taken).
 * b4d_ssim: structural similarity (Wang et al. 2004) as scikit-image's structural_similarity forms it.  Window sizes (SciPy's
 *   placement), taps, the two-dimensional padding by mode / cval and W are those of b4d_local_stats: NULL taps = box window (weights
 *   1, W = size_y size_x), otherwise both float64 tap arrays.  Per output pixel five float64 sums over the window, along x, then
 *   along y, in ascending tap order (box: s += v; taps: s = fma(w, v, s)): S_r, S_x, S_rr, S_xx, S_rx, the products r r, x x, r x
 *   formed in float64, where they are exact.  Then, every operation a float64 operation of its own, in this order:
 *       iw   = 1 / W  (the one division by W)            mu_r = S_r * iw          mu_x = S_x * iw
 *       v_r  = cov_norm * (S_rr * iw - mu_r * mu_r)      v_x = cov_norm * (S_xx * iw - mu_x * mu_x)
 *       v_rx = cov_norm * (S_rx * iw - mu_r * mu_x)      (variances are not clamped)
 *       cs   = (2 * v_rx + c2) / (v_r + v_x + c2)
 *       ssim = ((2 * (mu_r * mu_x) + c1) / (mu_r * mu_r + mu_x * mu_x + c1)) * cs
 *   Identical frames give exactly 1; exchanging ref and img gives the same bits.  ssim_map, cs_map: (batch, ny, nx) float32 or
 *   NULL.  means: (batch, 2) float64 or NULL, per frame the mean of the FLOAT64 ssim and cs over rows [crop_y, ny - crop_y) and
 *   columns [crop_x, nx - crop_x): a workgroup (a 32 x 32 tile, 512 lanes; lane l holds column l % 32 and rows 2 (l / 32) and
 *   2 (l / 32) + 1, added in that order) sums its pixels of the region by block_sum (down the wave, then the eight waves in order) into its slot of the
 *   library's per-stream scratch buffer; a second launch gives lane l of 256 the tiles l, l + 256, .. of a frame in ascending
 *   row-major order, adds the 256 lane sums by a halving tree (sh[l] += sh[l + o], o = 128 .. 1) and divides by the pixel count.
 *   With only `means`, nothing of frame size is written.  NaN propagates: it poisons the maps over its footprint and the means of
 *   its frame.
 *   Window limit: 1 .. 63 per axis (B4D_EINVAL beyond) as far as one workgroup's LDS holds both staged tiles and five planes of
 *   row sums: with rows = 31 + size_y,  8 * ceil4(rows * ceil4(31 + size_x)) + 1280 * rows + 128 <= 163840 bytes (B4D_ESIZE
 *   beyond).  Every window up to 52 x 52 passes (33 x 33: 114 816 bytes), as do 63 x 25 and 48 x 63 (size_y x size_x); the default 11 x 11 takes
 *   68 672 bytes, two workgroups a CU.
 *   B4D_EINVAL: c1 <= 0, c2 <= 0, cov_norm <= 0 (or NaN), a negative crop, a crop that leaves no pixel while means is given, one
 *   tap array without the other, all three outputs NULL, an output that overlaps an input, 0 < ref_stride < ny * nx.
 * b4d_pair_errors: out (batch, 8) float64, per frame  sum (x - r)^2,  sum |x - r|,  max |x - r|,  sum r^2,  sum r,  min r,
 *   max r,  sum x  (r the reference pixel, x the image pixel; differences and squares in float64).  The pixels of a frame are taken
 *   in groups of four; workgroup s of split = min(1024, ceil(groups / 2048)) takes ceil(groups / split) consecutive groups, lane l
 *   of it the groups l, l + 256, .. in ascending order; block_sum adds the lanes, the workgroup's row goes to the scratch buffer,
 *   and a second launch merges the rows (lane l the rows l, l + 256, ..; then the halving tree above).  The split depends on
 *   ny * nx alone and the walk not on the access width.  The extrema are exact.  They are merged by "take the newcomer if it is
 *   smaller (larger) or a NaN"; a NaN that is held loses no comparison, so a NaN in r makes the sums of r, min r and max r NaN and
 *   a NaN in r or x makes the sums and the maximum of the differences NaN (and sum x, if it is in x).
 * b4d_pool2: out (batch, ny / 2, nx / 2), out[y, x] = ((in[2y, 2x] + in[2y, 2x + 1]) + (in[2y + 1, 2x] + in[2y + 1, 2x + 1]))
 *   * 0.25f in float32, in that order; a trailing odd row or column is dropped.  ny < 2 or nx < 2: B4D_EINVAL.
 * No atomics: a frame gives the same bits alone and inside any batch.  All argument errors are returned before any launch:
 * B4D_EINVAL also for batch < 1, an empty shape, a null frame pointer, a mode out of range, in / out that overlap;
 * B4D_ESIZE where ny * nx >= 2^31.                                                                                            */
int b4d_ssim(const float* ref, long long ref_stride, const float* img, int batch, int ny, int nx, int size_y, int size_x,
             const double* taps_y, const double* taps_x, int mode, float cval, double c1, double c2, double cov_norm, int crop_y,
             int crop_x, float* ssim_map, float* cs_map, double* means, void* stream);
int b4d_pair_errors(const float* ref, long long ref_stride, const float* img, int batch, int ny, int nx, double* out, void* stream);
int b4d_pool2(const float* in, int batch, int ny, int nx, float* out, void* stream);

/* Histogram equalisation of every frame of in (batch, ny, nx) float32 (barc4dip_amd.preprocessing.enhancement, metrics.histogram;
 * DESIGN.md section 29): contrast-limited adaptive equalisation by OpenCV's CPU rule (cv::CLAHE), cv::equalizeHist's rule at any
 * depth, and the tile histograms behind both.  DEVICE pointers throughout, asynchronous on `stream`, no synchronisation, no
 * allocation: the caller passes the workspaces.  Every float32 operation below is rounded on its own (the unit is compiled without
 * contraction), every count is an integer: results are specified to the bit and a frame gives the same bits alone and in a batch.
 *   levels L: 2 .. 65536.  tiles_x / tiles_y: tiles along x / along y (OpenCV's order), >= 1, tiles_x * tiles_y <= 4096.
 *   qparams: (batch, 4) float32 per frame {lo, s, inv, unused}, 16-byte aligned.  s = float32(L / (float64(hi) - float64(lo))),
 *   inv = float32((float64(hi) - float64(lo)) / (L - 1)); whole-number frames (uint8 / uint16 levels) take {0, 1, 1}.
 *   s == 0 marks a frame that b4d_lut_apply copies unchanged.
 * Quantiser: bin = clamp(floor((x - lo) * s), 0, L - 1).  The clamp is applied to the float before the conversion, so +-Inf and
 *   products beyond the int range take the end bins and a NaN product (0 * Inf) bin 0; on every other value this is the
 *   clamp(int(floor(.))) of the rule.  A NaN pixel has no bin.
 * Tiles: an axis of n pixels and t tiles is extended by pad = (t - n % t) % t pixels behind its end, extended pixel e >= n
 *   being pixel 2 (n - 1) - e (reflection without repeating the edge); pad <= n - 1 is required.  Tile side = (n + pad) / t; tile
 *   area <= 2^24.  Extended pixels are counted; no padded copy is written.  Tiles of extended pixels only are legal.
 * b4d_tile_histogram: counts (batch, tiles_y, tiles_x, L) uint32 = pixels of every tile per bin, n_valid (batch, tiles_y, tiles_x)
 *   uint32 = non-NaN pixels of every tile.  One workgroup per tile up to L = 32768 (integer LDS atomics on min(16, 8192 / L)
 *   copies of the histogram, added up on the way out); above, one workgroup per 32768-bin slice of a tile, which reads the tile
 *   again.  Plain stores to memory.  16-byte loads from the first 16-byte boundary of every tile row on; its ragged ends and the
 *   reflected columns one by one.
 * b4d_equalize_lut: lut (batch, tiles, L) uint16 from counts and n_valid (tiles = tiles_y * tiles_x), one workgroup per tile.
 *   A tile with n = n_valid == 0 gets lut[i] = i.
 *   mode 0 (CLAHE): clip = 0 for clip_limit == 0, else c = clip_limit * n / L in float64 and clip = n where c >= n (nothing
 *   exceeds it), else max(int(c), 1).  With clip > 0: excess = sum max(h[i] - clip, 0), h[i] = min(h[i], clip) + excess / L, and
 *   with residual = excess % L > 0, step = max(L / residual, 1), one more in the bins i with i % step == 0 and
 *   i / step < residual.  scale = float32(L - 1) / float32(n), lut[i] = clamp(rint(float32(sum_{j <= i} h[j]) * scale), 0, L - 1),
 *   rint to even.
 *   mode 1 (equalize_hist; tiles == 1): i0 = first non-empty bin; h[i0] == n (or n == 0) sets unchanged[frame] = 1 (else 0) and
 *   the identity table; otherwise scale = float32(L - 1) / float32(n - h[i0]), lut[i <= i0] = 0 and
 *   lut[i > i0] = clamp(rint(float32(sum_{i0 < j <= i} h[j]) * scale), 0, L - 1).  unchanged: (batch) int32, NULL in mode 0.
 * b4d_lut_apply: out (batch, ny, nx) float32.  With th, tw the tile sides and inv_h = 1.0f / th: tyf = y * inv_h - 0.5f,
 *   t1 = floor(tyf), ya = tyf - t1, ya1 = 1.0f - ya, tile rows max(t1, 0) and min(t1 + 1, tiles_y - 1); columns likewise.  With v
 *   the four table entries at the pixel's bin, res = (v11 * xa1 + v12 * xa) * ya1 + (v21 * xa1 + v22 * xa) * ya, left to right.
 *   flags bit 0 clear: out = clamp(rint(res), 0, L - 1); set: out = res * inv + lo.  flags bit 1 (one tile only): res = lut[bin]
 *   without the interpolation, and frames with unchanged[frame] != 0 (unchanged may be NULL) are copied.  A NaN pixel and every
 *   pixel of a frame with s == 0 is copied.  The row terms are formed once per row, the column terms once per lane for 16 rows;
 *   16-byte accesses where nx % 4 == 0 and in / out are 16-byte aligned, the same bits otherwise.
 * All argument errors are returned before any launch: B4D_EINVAL for a null pointer, batch < 1, an empty axis, tiles < 1, a
 * padding longer than its axis less one, a mode or flags out of range, clip_limit < 0 or NaN, in / out that overlap, qparams off
 * 16 bytes; B4D_ESIZE for levels outside 2 .. 65536, more than 4096 tiles, a tile of more than 2^24 pixels, ny * nx >= 2^31,
 * batch > 65535.                                                                                                               */
int b4d_tile_histogram(const float* in, int batch, int ny, int nx, int tiles_x, int tiles_y, int levels, const float* qparams,
                       unsigned* counts, unsigned* n_valid, void* stream);
int b4d_equalize_lut(const unsigned* counts, const unsigned* n_valid, int batch, int tiles, int levels, double clip_limit, int mode,
                     unsigned short* lut, int* unchanged, void* stream);
int b4d_lut_apply(const float* in, int batch, int ny, int nx, int tiles_x, int tiles_y, int levels, const float* qparams,
                  const unsigned short* lut, const int* unchanged, int flags, float* out, void* stream);

/* Hartmann sensor: spot centroids over a lattice of rectangular cells (barc4dip_amd.signal.hartmann).
 * frames (batch, ny, nx): DEVICE float32.  y_edges (gy + 1), x_edges (gx + 1): HOST int32, ascending; cell (i, j) is the rows
 * [y_edges[i], y_edges[i + 1]) by the columns [x_edges[j], x_edges[j + 1]), every side 2 .. 128, all cells inside the frame.  Pixels
 * outside every cell are never read for a result.  out: DEVICE (batch, gy, gx, 14) float64, per cell
 *   {cy, cx, flux, peak, peak_y, peak_x, background, noise, var_y, var_x, cov_yx, n_pixels, n_saturated, n_nan}.
 * All arithmetic is float64 on the float32 pixels; NaN pixels take no part anywhere.  Positions are in frame coordinates.
 *   peak: the largest value, at (peak_y, peak_x): first occurrence in row-major order within the cell (NaN x 3 in an all-NaN cell).
 *   n_nan: NaN pixels.  n_saturated: pixels with v >= saturation (+inf disables it).
 *   ring: the non-NaN pixels of the cell's one-pixel outer ring, m their mean; noise = sqrt(sum (v - m)^2 / n) over them, 0 where
 *   n < 2; computed in every mode.
 *   background b: background_mode 0: 0; 1: background_value; 2: the cell's minimum; 3: m.
 *   t = b + threshold * (peak - b), 0 <= threshold < 1; weight w = v - t where that is > 0, else 0 (continuous in t).
 *   n_pixels: pixels with w > 0.  flux F = sum w.  With (yc, xc) the cell's geometric centre ((first + last) / 2 per axis):
 *   cy = yc + sum w (y - yc) / F, cx likewise; var_y = sum w (y - cy)^2 / F, var_x likewise, cov_yx = sum w (y - cy)(x - cx) / F.
 *   A cell with F == 0 (constant, empty or all NaN) gets NaN in cy, cx and the three moments, 0 in flux and n_pixels.
 *   method 1 (iteratively weighted centre of gravity): from that (cy, cx), `iterations` times
 *   c <- centre + sum w g (p - centre) / sum w g with g = exp(-((y - cy)^2 + (x - cx)^2) / (2 sigma^2)) over the whole cell; cy, cx are
 *   the last iterate, the other twelve quantities those of method 0.
 * One workgroup stages a span of one cell row (its rows by a run of up to 16 neighbouring cells, at most 64 KiB) in LDS, so a
 * frame is read once per call whatever `iterations` is: 16-byte loads from the first 16-byte boundary of a span row on where
 * nx % 4 == 0 and frames is 16-byte aligned, the ragged ends and every other stack pixel by pixel.  One wave per cell: lane l adds
 * the pixels l, l + 64, .. (row-major), then a fixed butterfly over the lanes: the same bits run to run, alone or in any batch.
 * On `stream`; the edge tables are copied into the stream's scratch buffer.  B4D_EINVAL: null pointer, empty batch / frame /
 * lattice, edges that do not ascend or leave the frame, a mode, threshold, method, sigma, iterations or saturation (NaN) out of
 * range; B4D_ESIZE: a cell side outside 2 .. 128, gy > 65535, ny * nx >= 2^31.                                                  */
int b4d_spot_centroids(const float* frames, int batch, int ny, int nx, const int32_t* y_edges, int gy, const int32_t* x_edges, int gx,
                       int background_mode, double background_value, double threshold, int method, double sigma, int iterations,
                       double saturation, double* out, void* stream);

/* Regions: connected-component labelling, per-region measurements, relabelling (barc4dip_amd.geometry.labels,
 * barc4dip_amd.metrics.regions).  Device pointers, the caller's stream, nothing synchronises.
 * b4d_label_regions: exactly one of frames (batch, ny, nx) DEVICE float32 with thresholds (batch) DEVICE float32, and mask
 *   (batch, ny, nx) DEVICE bytes, is non-NULL.  Foreground: frames[p] > thresholds[frame], strict (a NaN is background, +inf is
 *   foreground), or mask[p] != 0.  connectivity 1: pixels that share an edge are connected; 2: an edge or a corner.
 *   labels (batch, ny, nx) DEVICE int32: 0 on the background, 1 .. N on the foreground; two foreground pixels have the same label
 *   if and only if they are connected; the labels of a frame are numbered in the raster order of each component's first pixel
 *   (scipy.ndimage.label with generate_binary_structure(2, connectivity)).  n_regions (batch) DEVICE int32: N per frame.
 *   Integers throughout: the same result for a frame alone and in any batch, run after run.
 *   Passes (separate launches, no workgroup waits for another): union-find over 32 x 64 tiles in LDS (links point to a smaller
 *   raster index, the root of a set is its smallest; integer atomicMin), a pass over the tile seams (tile-corner diagonals
 *   included), a flatten pass, an exclusive scan of the root flags in blocks of 2048 pixels, the roots' numbers, every pixel's
 *   number from its root.  labels is the only frame-sized array; the stream's scratch buffer takes batch * ceil(ny nx / 2048)
 *   words.  Every find and every retry ends by construction (links strictly decrease) and carries an explicit bound, the number
 *   of cells; a bound that is reached sets an error word, and every frame of the call then gets n_regions = B4D_ELOOP (labels
 *   unspecified): the call has returned B4D_OK by then, so the code reaches the caller with n_regions, which it reads to size
 *   the table below.
 *   B4D_EINVAL: both or neither input, a null pointer, batch < 1, an empty axis, connectivity not 1 or 2; B4D_ESIZE: ny * nx
 *   >= 2^31 - 2048, ny > 2097120.
 * b4d_region_properties: labels (batch, ny, nx) DEVICE int32 from any source (regions need not be connected); offsets (batch + 1)
 *   HOST int32, offsets[0] = 0, ascending: frame t has the labels 1 .. offsets[t + 1] - offsets[t] and its rows start at
 *   offsets[t]; pixels with another value belong to no region.  frames (batch, ny, nx) DEVICE float32 or NULL (geometry only).
 *   out (offsets[batch], 20) DEVICE float64, per region
 *     {area, y0, y1, x0, x1, cy, cx, sum, min, max, max_y, max_x, flux, wcy, wcx, var_y, var_x, cov_yx, n_nan, n_saturated}:
 *     area: pixels.  [y0, y1) x [x0, x1): the bounding box.  cy, cx: the mean pixel position (integer sums, one division).
 *     NaN pixels take no part in any value column and are counted in n_nan.  n_saturated: pixels with v >= saturation (+inf:
 *     none).  sum = sum v; min, max; (max_y, max_x): the first occurrence of max in raster order.  w = max(v - background, 0);
 *     flux = sum w; wcy = y0 + sum w (y - y0) / flux, wcx likewise; var_y = sum w (y - wcy)^2 / flux, var_x likewise, cov_yx =
 *     sum w (y - wcy)(x - wcx) / flux, summed about the box corner; NaN in these five where flux is not > 0.
 *     A region without a non-NaN pixel has NaN min / max, (-1, -1) as their position, sum 0.  A label without a pixel has area 0,
 *     the box (0, 0, 0, 0), NaN centroids.  With frames == NULL sum, min, max, flux and the five are NaN, the position (-1, -1).
 *   All arithmetic is float64 on the float32 pixels.  Every integer-valued column is exact; every column has the same bits run
 *   to run, for a frame alone and in any batch: boxes by integer atomicMin / atomicMax (from the pixels on a region's outline),
 *   then lane l of one wave (box area <= 4096) or of one 512-lane workgroup (above) adds the box pixels l, l + lanes, .. in
 *   row-major order, a fixed butterfly joins the lanes of a wave, and the waves are added in order.  No float atomics.
 *   Reads about 8 bytes per BOX pixel per pass (two passes where flux > 0): cheap for blobs, many reads of the frame for nested
 *   frame-sized regions.  Scratch: 5 words per region.
 *   B4D_EINVAL: null labels / offsets / out, batch < 1, an empty axis, offsets that do not start at 0 or descend, a background
 *   that is not finite, a NaN saturation; B4D_ESIZE: ny * nx >= 2^31.
 * b4d_relabel: out[p] = map[offsets[t] + labels[p] - 1] where 1 <= labels[p] <= offsets[t + 1] - offsets[t], else 0.  map
 *   (offsets[batch]) DEVICE int32: old label -> new label, 0 drops the region.  out may be labels itself.                        */
int b4d_label_regions(const float* frames, const float* thresholds, const unsigned char* mask, int batch, int ny, int nx,
                      int connectivity, int32_t* labels, int32_t* n_regions, void* stream);
int b4d_region_properties(const float* frames, const int32_t* labels, int batch, int ny, int nx, const int32_t* offsets,
                          double background, double saturation, double* out, void* stream);
int b4d_relabel(const int32_t* labels, int batch, int ny, int nx, const int32_t* offsets, const int32_t* map, int32_t* out,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* B4D_H */
