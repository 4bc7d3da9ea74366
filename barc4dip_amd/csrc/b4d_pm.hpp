// b4d_pm.hpp -- interface of the general-length 1-D engine (b4d_pm.hip): rows of length n = P * M, P <= 16 a power of two,
// used by the general plans of b4d_general.hip (pm_rows*) and by the Wiener plan of b4d_wiener.hip (dft_rows).
#pragma once
#include "b4d_fft2d.hpp"

namespace b4d {

// What the fused row transform (k_pm_fused) reads ...
enum class PmIn {
    Complex,       // complex rows
    Real,          // real rows
    Reflect,       // rows of the reflect-padded, max-normalised frame taken straight from the (h, w) frame io.frame
                   // (np.pad(..., "reflect") / max|frame|, filters.py:252-261: no padded copy in memory)
    ReflectPair,   // as Reflect for the row PAIR (2 s, 2 s + 1) packed as real + i imaginary part of one transform
    HermPair,      // the Hermitian pair: half rows 2 s, 2 s + 1 (io.half values each) extended to Ga + i Gb (inverse pass)
    RealPair,      // two plain real rows of a (frames, io.rows, N) float stack packed as real + i imaginary part
};
// ... and writes.  Pair modes index sequences as s = frame * ceil(io.rows / 2) + pair: pairs never straddle two frames.
enum class PmOut {
    Complex,     // complex rows
    Crop,        // clip(Re, -1, 1) * max|frame| cropped back to (h, w) in io.crop (filters.py:266, 287-289)
    HalfPair,    // the pair's half spectra Fa, Fb (k = 0 .. io.half - 1) unpacked to half rows 2 s, 2 s + 1
    CropPair,    // as Crop for the pair: real part -> row 2 s, imaginary part -> row 2 s + 1
    ShiftPair,   // the pair's two real rows written fftshift-ed into a (frames, io.rows, N) float stack (io.crop), scaled or
                 // divided by the frame's zero-lag value io.amax[frame] (autocorrelation peak normalisation)
};
struct FusedIO {
    const float* frame;   // Reflect*: the (h, w) frame read
    float* crop;          // Crop* / ShiftPair: the real array written
    const float* amax;    // max|frame| (device scalar)
    int h, w, py, px, clip;
    int half, rows;       // pair modes: half-row length N/2 + 1 and the number of (padded) rows
    int filt_bcast;       // the pointwise multiplier is ONE row shared by every sequence (Bluestein's chirp spectrum)
    int norm_peak;        // ShiftPair: divide by io.amax[frame] when it is > 0 and force the zero lag to exactly 1
};

// One transform length: n = P * M, and M = A * B when the fused in-LDS transform applies (A = B = 0: DFT-matrix product)
struct PmAxis {
    int n = 0, P = 1, M = 0, A = 0, B = 0;
    const float2* tw = nullptr;   // n-point twiddles exp(-2 pi i k / n)
    const float2* dm = nullptr;   // M x M DFT matrix (only read when A == 0)
};
PmAxis pm_axis(int n, const float2* tw = nullptr, const float2* dm = nullptr);   // the split; the tables stay the caller's

// S contiguous sequences of length ax.n: out = DFT(in) (forward) or conj(DFT(conj(in))) * scale (inverse); optional pointwise
// multiplier `filt` on the forward output.  Without a fused split only PmIn::Complex / Real -> PmOut::Complex exist and tmp,
// tmp2 (S * n complex values each) are needed: in != tmp != tmp2 != out (the first and last steps are permutations).
int dft_rows(const PmAxis& ax, const void* in, PmIn im, float2* tmp, float2* tmp2, float2* out, PmOut om, int S, bool inverse,
             const float2* filt, float scale, hipStream_t st, const FusedIO* fio = nullptr);
int transpose_batch(const float2* in, float2* out, int rows, int cols, int batch, hipStream_t st);

bool pm_fusable(int n);
bool pm_supported(int n);   // fused split, or Bluestein over a power-of-two fused transform (n <= 4096)
// S contiguous sequences of length n: out = DFT(in), or conj(DFT(conj(in))) * scale when inverse; tw: n-point twiddles
int pm_rows(const void* in, bool real_in, float2* out, int S, int n, const float2* tw, bool inverse, float scale, hipStream_t st);
// Real rows in pairs (SURVEY's R2C / C2R passes for general lengths; n must have a fused split):
//   forward: (frames, rows, n) float -> (frames, rows, n/2 + 1) half spectra
//   inverse: half rows -> (frames, rows, n) float, fftshift-ed in both axes, scaled by `scale` or, with `peak`
//            (device, one unscaled zero-lag value per frame), divided by it with the zero lag forced to 1
int pm_rows_pair_fwd(const float* in, float2* half_out, int frames, int rows, int n, const float2* tw, hipStream_t st);
int pm_rows_pair_inv(const float2* half_in, float* real_out, int frames, int rows, int n, const float2* tw, float scale, const float* peak,
                     hipStream_t st);

// index i of np.pad(x, p, mode="reflect") taken back into [0, n)  (-p <= i < n + p, p < n)
__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
// the frame's max|.| is usable as a scale (an all-zero or non-finite frame comes back as zeros)
__device__ __forceinline__ bool scale_ok(float sc) { return isfinite(sc) && sc != 0.f; }
// restored value: optional clip to [-1, 1] (np.clip: NaN stays NaN), then back to the frame's units
__device__ __forceinline__ float clip_rescale(float v, int clip, bool ok, float sc) {
    if (clip) v = (v > 1.f ? 1.f : (v < -1.f ? -1.f : v));
    return ok ? v * sc : 0.f;
}

}  // namespace b4d
