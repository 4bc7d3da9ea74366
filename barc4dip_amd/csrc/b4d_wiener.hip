// b4d_wiener.hip -- Gaussian-PSF Wiener deconvolution of barc4dip.preprocessing.deconvolve_psf
// (preprocessing/filters.py:17-289, method="wiener"; BASELINE.json config 5) and Richardson-Lucy on gfx950.
//
// The reference pads every frame by psf//2 with "reflect", normalises by max|.|, applies the Wiener-Hunt
// filter of skimage.restoration.wiener in the Fourier domain of the PADDED size, clips to [-1, 1], rescales
// and crops.  The padded sizes are awkward by construction (1024 + 2*4 = 1032 = 8 * 3 * 43).  Sizes with a compiled
// three-radix kernel on both sides (4104 = 8 * 27 * 19 among them) run the three kernels of b4d_wiener_mr.hip; every other
// size runs here, on the general-length row transforms of b4d_pm.hip (dft_rows: fused in LDS, or a DFT-matrix product):
//
// 2-D: row pass, transpose, row pass (the spectrum stays transposed: the filter is stored transposed as well),
// multiply, and the same two passes back with conjugated inputs/outputs.
// Parity: UNPINNED (scikit-image is not installable here); oracle/wiener_np.py restates the published algorithm.
#include "b4d_pm.hpp"
#include "b4d_wiener_mr.hpp"

namespace b4d {

// amax[0] = max of the `nparts` partial maxima (one wave)
__global__ void __launch_bounds__(64) k_absmax_final(float* __restrict__ amax, int nparts) {
    float m = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 64) m = fmaxf(m, amax[i]);
    m = wave_max(m);
    if (threadIdx.x == 0) amax[0] = m;
}

// np.pad(frame, ((py,py),(px,px)), mode="reflect") / scale  (filters.py:252-261); scale = max|frame| read from `amax`
__global__ void __launch_bounds__(256) k_pad_reflect(const float* __restrict__ frame, int h, int w, int py, int px,
                                                     const float* __restrict__ amax, float* __restrict__ out) {
    const float sc = amax[0];   // reduced by k_absmax_final
    const int H = h + 2 * py, W = w + 2 * px;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)H * W) return;
    const int y = reflect_idx((int)(e / W) - py, h), x = reflect_idx((int)(e % W) - px, w);
    out[e] = scale_ok(sc) ? frame[(size_t)y * w + x] / sc : 0.f;
}

// restored = clip(Re(z), -1, 1) * scale, cropped back to (h, w)  (filters.py:266, 287-289); z: the padded inverse transform
// (float2) or the padded Richardson-Lucy estimate (float)
__device__ __forceinline__ float real_of(float v) { return v; }
__device__ __forceinline__ float real_of(float2 v) { return v.x; }
template <typename T>
__global__ void __launch_bounds__(256) k_crop_out(const T* __restrict__ z, int h, int w, int py, int px,
                                                  const float* __restrict__ amax, int clip, float* __restrict__ out) {
    const float sc = amax[0];
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)h * w) return;
    const int y = (int)(e / w), x = (int)(e % w), W = w + 2 * px;
    out[e] = clip_rescale(real_of(z[(size_t)(y + py) * W + x + px]), clip, scale_ok(sc), sc);
}

// max|x| partials, NaN-ignoring (np.nanmax(np.abs(padded)))
__global__ void __launch_bounds__(1024) k_nanabsmax(const float* __restrict__ x, size_t n, float* __restrict__ part) {
    __shared__ float sh[16];
    float m = 0.f;
    auto take = [&](float v) {
        const float a = fabsf(v);
        if (a == a) m = fmaxf(m, a);
    };
    // 16-byte loads, four per lane in flight (a frame is one stream: the scalar grid-stride loop was latency-bound)
    const size_t n4 = ((reinterpret_cast<size_t>(x) & 15) == 0) ? n / 4 : 0, stride = (size_t)gridDim.x * blockDim.x;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
        take(a.x); take(a.y); take(a.z); take(a.w);
        take(b.x); take(b.y); take(b.z); take(b.w);
        take(c.x); take(c.y); take(c.z); take(c.w);
        take(d.x); take(d.y); take(d.z); take(d.w);
    }
    for (; i < n4; i += stride) {
        const float4 a = x4[i];
        take(a.x); take(a.y); take(a.z); take(a.w);
    }
    for (size_t j = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) take(x[j]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = fmaxf(m, sh[i]);
        part[blockIdx.x] = m;
    }
}

// W^T = conj(H) / (|H|^2 + balance |L|^2) from the (transposed) transfer functions of the PSF and the Laplacian
__global__ void __launch_bounds__(256) k_wiener_filter(const float2* __restrict__ Hf, const float2* __restrict__ Lf, size_t n,
                                                       float balance, float2* __restrict__ Wf) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float2 h = Hf[e], l = Lf[e];
    const float den = (h.x * h.x + h.y * h.y) + balance * (l.x * l.x + l.y * l.y);
    Wf[e] = make_float2(h.x / den, -h.y / den);
}

// ---- Richardson-Lucy (skimage.restoration.richardson_lucy as published; filters.py:270-277)
// One step of the iteration on a (H, W) float32 image with a (ky, kx) kernel, "same" convolution, zero boundary:
//   MODE 0: dst = image / (conv(src, psf) + 1e-12)          (0 where conv < feps when feps > 0)
//   MODE 1: dst = dst * conv(src, flip(psf))
// 64 x 32 output tile per workgroup, source tile + halo and the kernel staged in LDS.  grid (ceil(W/64), ceil(H/32))
constexpr int RL_TX = 64, RL_TY = 32, RL_MAXK = 33;
template <int MODE>
__global__ void __launch_bounds__(256) k_rl_step(const float* __restrict__ src, const float* __restrict__ image, float* __restrict__ dst,
                                                 const float* __restrict__ psf, int H, int W, int ky, int kx, float feps) {
    extern __shared__ float rl_sm[];
    const int hy = ky / 2, hx = kx / 2, tw = RL_TX + 2 * hx, th = RL_TY + 2 * hy;
    float* tile = rl_sm;              // th x tw
    float* kk = rl_sm + th * tw;      // ky x kx, already oriented for a correlation-style inner loop
    const int x0 = blockIdx.x * RL_TX, y0 = blockIdx.y * RL_TY;
    for (int i = threadIdx.x; i < th * tw; i += 256) {
        const int y = y0 - hy + i / tw, x = x0 - hx + i % tw;
        tile[i] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(size_t)y * W + x] : 0.f;
    }
    // conv(f, k)[y, x] = sum_{i, j} f[y + hy - i, x + hx - j] k[i, j] = sum_{p, q} tile[ty + p, tx + q] k[ky-1-p, kx-1-q];
    // MODE 1 convolves with the flipped kernel: the two flips cancel
    for (int i = threadIdx.x; i < ky * kx; i += 256) kk[i] = MODE == 0 ? psf[ky * kx - 1 - i] : psf[i];
    __syncthreads();
    const int tx = threadIdx.x % RL_TX, tyb = threadIdx.x / RL_TX;   // 4 rows of 64 lanes; each lane 8 output rows
#pragma unroll 1
    for (int r = 0; r < RL_TY / 4; ++r) {
        const int ty = tyb + 4 * r, y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        float acc = 0.f;
        for (int p = 0; p < ky; ++p) {
            const float* row = tile + (ty + p) * tw + tx;
            const float* krow = kk + p * kx;
            for (int q = 0; q < kx; ++q) acc = fmaf(row[q], krow[q], acc);
        }
        const size_t o = (size_t)y * W + x;
        if (MODE == 0) {
            const float conv = acc + 1e-12f;
            dst[o] = (feps > 0.f && conv < feps) ? 0.f : image[o] / conv;
        } else {
            dst[o] = dst[o] * acc;
        }
    }
}

__global__ void __launch_bounds__(256) k_fill(float* __restrict__ x, size_t n, float v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}

}  // namespace b4d

using namespace b4d;

#ifndef B4D_WIENER_LANES
#define B4D_WIENER_LANES 2
#endif
struct b4d_wiener {
    std::recursive_mutex mu;     // host-side re-entrancy (several host threads, one plan)
    int h, w, py, px, H, W;      // frame, half kernel, padded sizes
    PmAxis ax, ay;               // rows (length W) and columns (length H), with their tables (owned)
    float2* filt = nullptr;      // transposed Wiener filter (W, H)
    // one set of work buffers per lane (lane 0: created with the plan) + internal streams (lazily created by the first
    // multi-frame call): consecutive frames run on alternate streams, so one frame's row transforms fill the chip while another's
    // last partial round of workgroups (2052 rows on 512 resident workgroups: 4 full rounds + 4 stragglers) and its HBM bursts drain
    struct Lane {
        float2* a = nullptr;         // (H*W) work buffers
        float2* b = nullptr;
        float2* c = nullptr;
        float* padded = nullptr;     // (H, W) real
        float* amax = nullptr;       // 256 partial maxima
        hipStream_t st = nullptr;
        hipEvent_t done = nullptr;
    };
    Lane lane[B4D_WIENER_LANES];
    hipEvent_t fork = nullptr;
    // mixed-radix route (b4d_wiener_mr.hip): both padded sides have a compiled three-radix kernel
    bool mr = false;
    WmrGeom geom{};
    float2* mr_filt = nullptr;   // (Wh, Hp) transposed half filter (general PSF)
    float2* mr_sepx = nullptr;   // separable, point-symmetric PSF (the Gaussian of deconvolve_psf): {hx, lx}[Wh] and {hy, ly}[H] instead,
    float2* mr_sepy = nullptr;   // the filter is rebuilt per element in the column pass (b4d_wiener_mr.hip: WmrSep)
    float mr_balance = 0.f;
    float2* mr_T = nullptr;      // (mr_cap, Wh, Hp) transposed half spectra of the frames of one launch
    float* mr_amax = nullptr;    // (mr_cap * (hp + 1)): max|frame| per frame, then the pair maxima
    int mr_cap = 0, mr_slots = 0;   // frames per slot, slots (one per lane of wiener_mr_apply)
    static constexpr int MR_LANES = 2;
    hipStream_t mr_aux[MR_LANES] = {};      // lane 1: the library's shared lane_stream(0) (lane 0 is the caller's stream)
    hipEvent_t mr_fork = nullptr, mr_join[MR_LANES] = {};
};

// frames per launch of the mixed-radix route on ONE lane: the persistent row kernels hand 513 quads per 4k frame to 256 workgroups
// (2.004 rounds), so a launch needs several frames to amortise its last, nearly empty round (measured on MI355X,
// 4096^2: 1 frame per launch 5.6 k frames/s, 4: 6.8 k, 8: 7.15 k, 16: 7.2 k); 68 MB of workspace per frame.  On two lanes
// (wiener_mr_apply) the other lane's kernels fill that round and ONE frame per group (64 MiB of workspace) is best: it stays in the
// memory-side cache between the passes (same box, 64 x 4096^2: one lane x 8 frames 7.65-7.78 k frames/s; two lanes x 8: 7.9-8.1 k,
// x 4: 8.1 k, x 2: 7.8-8.0 k, x 1: 8.1-8.4 k; three lanes x 1: 7.4-7.6 k, four: 6.9 k)
#ifndef B4D_WIENER_FPL
#define B4D_WIENER_FPL 8
#endif
static int wiener_fpl(bool lanes, size_t t_bytes) {   // t_bytes: transposed half spectrum of one frame
    static const int v = [] {
        const char* e = getenv("B4D_WIENER_FPL");   // tuning aid (tools/dev_cfg5.py); results do not depend on it
        const int n = e ? atoi(e) : 0;
        return n >= 1 && n <= 64 ? n : 0;
    }();
    return v ? v : lanes ? (int)std::min<size_t>(64, std::max<size_t>(1, ((size_t)64 << 20) / t_bytes)) : B4D_WIENER_FPL;
}

// forward 2-D DFT of a real (H, W) array -> TRANSPOSED spectrum (W, H), left in lane 0's a (b, c are scratch).
// dft_rows needs in != tmp != tmp2 != out (its first and last steps are permutations).
static int fft2_real_T(b4d_wiener* pl, const float* x, hipStream_t st) {
    const b4d_wiener::Lane& L = pl->lane[0];
    int rc = dft_rows(pl->ax, x, PmIn::Real, L.a, L.b, L.c, PmOut::Complex, pl->H, false, nullptr, 1.f, st);
    if (rc) return rc;
    if ((rc = transpose_batch(L.c, L.a, pl->H, pl->W, 1, st))) return rc;
    return dft_rows(pl->ay, L.a, PmIn::Complex, L.b, L.c, L.a, PmOut::Complex, pl->W, false, nullptr, 1.f, st);
}

// the tables of one padded side
static int wiener_tables(PmAxis* ax) {
    float2* tw = nullptr;
    float2* dm = nullptr;
    int rc = make_twiddles(ax->n, &tw);
    ax->tw = tw;
    if (rc == B4D_OK && !ax->A) rc = make_dft_matrix(ax->M, &dm);
    ax->dm = dm;
    return rc;
}

extern "C" {

int b4d_wiener_destroy(b4d_wiener* p) {
    if (!p) return B4D_OK;
    for (void* q : {(void*)p->ax.tw, (void*)p->ay.tw, (void*)p->ax.dm, (void*)p->ay.dm, (void*)p->filt, (void*)p->mr_filt, (void*)p->mr_T,
                    (void*)p->mr_amax, (void*)p->mr_sepx, (void*)p->mr_sepy})
        if (q) (void)hipFree(q);
    for (int l = 0; l < B4D_WIENER_LANES; ++l) {
        b4d_wiener::Lane& L = p->lane[l];
        for (void* q : {(void*)L.a, (void*)L.b, (void*)L.c, (void*)L.padded, (void*)L.amax})
            if (q) (void)hipFree(q);
        if (L.st) (void)hipStreamSynchronize(L.st);   // shared lane_stream(l): not destroyed with the plan
        if (L.done) (void)hipEventDestroy(L.done);
    }
    if (p->fork) (void)hipEventDestroy(p->fork);
    for (int l = 1; l < b4d_wiener::MR_LANES; ++l) {
        if (p->mr_aux[l]) (void)hipStreamSynchronize(p->mr_aux[l]);
        if (p->mr_join[l]) (void)hipEventDestroy(p->mr_join[l]);
    }
    if (p->mr_fork) (void)hipEventDestroy(p->mr_fork);
    delete p;
    return B4D_OK;
}

int b4d_wiener_create(int h, int w, const float* psf_host, int ky, int kx, float balance, b4d_wiener** out) {
    if (!out || !psf_host) return fail(B4D_EINVAL, "null argument");
    *out = nullptr;
    if (h < 2 || w < 2 || ky < 1 || kx < 1 || !(ky & 1) || !(kx & 1)) return fail(B4D_EINVAL, "bad frame or kernel shape");
    if (ky / 2 >= h || kx / 2 >= w) return fail(B4D_EINVAL, "kernel larger than the frame");
    b4d_wiener* p = new b4d_wiener();
    p->h = h;
    p->w = w;
    p->py = ky / 2;
    p->px = kx / 2;
    p->H = h + 2 * p->py;
    p->W = w + 2 * p->px;
    p->ax = pm_axis(p->W);
    p->ay = pm_axis(p->H);
    if (p->ax.M > 4200 || p->ay.M > 4200) {
        const std::string msg = "padded size " + std::to_string(p->H) + "x" + std::to_string(p->W) + " has an odd factor > 4200";
        b4d_wiener_destroy(p);
        return fail(B4D_ESIZE, msg);
    }
    int rc = wiener_tables(&p->ax);
    if (rc == B4D_OK) rc = wiener_tables(&p->ay);
    b4d_wiener::Lane& L0 = p->lane[0];
    const size_t n = (size_t)p->H * p->W;
    hipError_t e = hipSuccess;
    if (rc == B4D_OK) {
        e = hipMalloc((void**)&p->filt, sizeof(float2) * n);
        if (e == hipSuccess) e = hipMalloc((void**)&L0.a, sizeof(float2) * n);
        if (e == hipSuccess) e = hipMalloc((void**)&L0.b, sizeof(float2) * n);
        if (e == hipSuccess) e = hipMalloc((void**)&L0.c, sizeof(float2) * n);
        if (e == hipSuccess) e = hipMalloc((void**)&L0.padded, sizeof(float) * n);
        if (e == hipSuccess) e = hipMalloc((void**)&L0.amax, sizeof(float) * 256);
        if (e != hipSuccess) rc = fail(B4D_ENOMEM, std::string("wiener workspace: ") + hipGetErrorString(e));
    }
    if (rc != B4D_OK) {
        b4d_wiener_destroy(p);
        return rc;
    }
    // transfer functions (published skimage.restoration.uft.ir2tf): kernel in the top-left corner of a zero (H, W)
    // array, every axis rolled by -floor(size/2), 2-D DFT.  Built on the host, transformed on the device.
    auto impulse = [&](const float* k, int kh, int kw, std::vector<float>& img) {
        img.assign(n, 0.f);
        for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j) {
                const int y = ((i - kh / 2) % p->H + p->H) % p->H, x = ((j - kw / 2) % p->W + p->W) % p->W;
                img[(size_t)y * p->W + x] = k[i * kw + j];
            }
    };
    std::vector<float> img;
    float2* Hf = nullptr;
    e = hipMalloc((void**)&Hf, sizeof(float2) * n);
    if (e != hipSuccess) {
        b4d_wiener_destroy(p);
        return fail(B4D_ENOMEM, "wiener setup allocation");
    }
    hipStream_t st = nullptr;
    impulse(psf_host, ky, kx, img);
    rc = (hipMemcpy(L0.padded, img.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess) ? B4D_OK : fail(B4D_EHIP, "memcpy");
    if (rc == B4D_OK) rc = fft2_real_T(p, L0.padded, st);
    if (rc == B4D_OK && hipMemcpyAsync(Hf, L0.a, sizeof(float2) * n, hipMemcpyDeviceToDevice, st) != hipSuccess)
        rc = fail(B4D_EHIP, "memcpy");
    const float lap[9] = {0.f, -1.f, 0.f, -1.f, 4.f, -1.f, 0.f, -1.f, 0.f};
    if (rc == B4D_OK) {
        impulse(lap, 3, 3, img);
        rc = (hipMemcpy(L0.padded, img.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess) ? B4D_OK : fail(B4D_EHIP, "memcpy");
    }
    if (rc == B4D_OK) rc = fft2_real_T(p, L0.padded, st);  // Laplacian transfer function in lane 0's a
    if (rc == B4D_OK) {
        hipLaunchKernelGGL(k_wiener_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Hf, L0.a, n, balance, p->filt);
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(B4D_EHIP, "wiener filter setup failed");
    }
    (void)hipFree(Hf);
    if (rc == B4D_OK && wmr_supported(p->H) && wmr_supported(p->W)) {
        // mixed-radix route: keep the Wh = W/2 + 1 independent filter columns at the workspace pitch, drop the work
        // buffers of the general route (only the set-up transforms above needed them)
        WmrGeom& g = p->geom;
        g.h = h, g.w = w, g.py = p->py, g.px = p->px, g.H = p->H, g.W = p->W;
        g.Wh = p->W / 2 + 1;
        g.Hp = wmr_pitch(p->H);
        g.hp = (p->H + 1) / 2;
        g.clip = 0;
        g.inv = 1.0f / ((float)p->H * (float)p->W);
        // Separable (rank one) and point-symmetric kernel?  psf = u v^T / s with u = row sums, v = column sums, s = total; then the
        // transfer function is the real product hx[k] hy[ky] of two cosine sums and the column pass needs no filter table at all.
        std::vector<double> u(ky, 0.0), v(kx, 0.0);
        double tot = 0.0, amaxk = 0.0;
        for (int i = 0; i < ky; ++i)
            for (int j = 0; j < kx; ++j) {
                const double q = psf_host[i * kx + j];
                u[i] += q;
                v[j] += q;
                tot += q;
                amaxk = std::max(amaxk, std::fabs(q));
            }
        bool sep = tot != 0.0 && std::getenv("B4D_WIENER_TABLE") == nullptr;
        for (int i = 0; i < ky && sep; ++i) {
            if (std::fabs(u[i] - u[ky - 1 - i]) > 1e-7 * std::fabs(tot)) sep = false;
            for (int j = 0; j < kx && sep; ++j)
                if (std::fabs(psf_host[i * kx + j] * tot - u[i] * v[j]) > 2e-6 * amaxk * std::fabs(tot)) sep = false;
        }
        for (int j = 0; j < kx && sep; ++j)
            if (std::fabs(v[j] - v[kx - 1 - j]) > 1e-7 * std::fabs(tot)) sep = false;
        if (sep) {
            std::vector<float2> sx(g.Wh), sy(p->H);
            for (int n = 0; n < p->H; ++n) {
                double hy = 0.0;
                for (int i = 0; i < ky; ++i) hy += u[i] * std::cos(2.0 * M_PI * (double)n * (double)(i - ky / 2) / (double)p->H);
                sy[n] = make_float2((float)hy, (float)(2.0 - 2.0 * std::cos(2.0 * M_PI * (double)n / (double)p->H)));
            }
            for (int k = 0; k < g.Wh; ++k) {
                double hx = 0.0;
                for (int j = 0; j < kx; ++j) hx += v[j] / tot * std::cos(2.0 * M_PI * (double)k * (double)(j - kx / 2) / (double)p->W);
                sx[k] = make_float2((float)hx, (float)(2.0 - 2.0 * std::cos(2.0 * M_PI * (double)k / (double)p->W)));
            }
            e = hipMalloc((void**)&p->mr_sepx, sizeof(float2) * sx.size());
            if (e == hipSuccess) e = hipMalloc((void**)&p->mr_sepy, sizeof(float2) * sy.size());
            if (e == hipSuccess) e = hipMemcpy(p->mr_sepx, sx.data(), sizeof(float2) * sx.size(), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(p->mr_sepy, sy.data(), sizeof(float2) * sy.size(), hipMemcpyHostToDevice);
            p->mr_balance = balance;
        } else {
            e = hipMalloc((void**)&p->mr_filt, sizeof(float2) * (size_t)g.Wh * g.Hp);
            if (e == hipSuccess) e = hipMemset(p->mr_filt, 0, sizeof(float2) * (size_t)g.Wh * g.Hp);
            if (e == hipSuccess)
                e = hipMemcpy2D(p->mr_filt, sizeof(float2) * g.Hp, p->filt, sizeof(float2) * p->H, sizeof(float2) * p->H, g.Wh,
                                hipMemcpyDeviceToDevice);
        }
        if (e != hipSuccess) rc = fail(B4D_ENOMEM, std::string("wiener filter (mixed-radix route): ") + hipGetErrorString(e));
        if (rc == B4D_OK) {
            for (float2** q : {&p->filt, &L0.a, &L0.b, &L0.c}) {
                (void)hipFree(*q);
                *q = nullptr;
            }
            (void)hipFree(L0.padded);
            L0.padded = nullptr;
            p->mr = true;
        }
    }
    if (rc != B4D_OK) {
        b4d_wiener_destroy(p);
        return rc;
    }
    *out = p;
    return B4D_OK;
}

// frames [0, batch) through the three kernels of b4d_wiener_mr.hip, B4D_WIENER_FPL frames per launch; the launch groups are
// dealt alternately to `st` and a second stream, each with its own slot of the workspace (two lanes: the passes of one group run
// under those of the other)
static int wiener_mr_apply(b4d_wiener* p, const float* frames, int batch, float* out, int clip, hipStream_t st) {
    WmrGeom g = p->geom;
    g.clip = clip;
    static const int lanes_env = [] {
        const char* e = getenv("B4D_WIENER_LANES2");   // tuning aid (tools/dev_cfg5.py); results do not depend on it
        const int n = e ? atoi(e) : 2;
        return n >= 1 && n <= b4d_wiener::MR_LANES ? n : 2;
    }();
    const int nl = g_opt_lanes.load() ? std::min(lanes_env, batch) : 1;
    int fpl = std::min(batch, wiener_fpl(nl > 1, sizeof(float2) * (size_t)g.Wh * g.Hp));
    if (nl > 1) fpl = std::min(fpl, (batch + nl - 1) / nl);
    if (fpl > p->mr_cap || nl > p->mr_slots) {   // work queued earlier on other streams may still use the old buffers: drain before freeing
        const int cap = std::max(fpl, p->mr_cap), slots = std::max(nl, p->mr_slots);
        B4D_HIP(hipDeviceSynchronize());
        for (void* q : {(void*)p->mr_T, (void*)p->mr_amax})
            if (q) (void)hipFree(q);
        p->mr_T = nullptr;
        p->mr_amax = nullptr;
        p->mr_cap = p->mr_slots = 0;
        hipError_t e = hipMalloc((void**)&p->mr_T, sizeof(float2) * (size_t)slots * cap * g.Wh * g.Hp);
        if (e == hipSuccess) e = hipMalloc((void**)&p->mr_amax, sizeof(float) * (size_t)slots * cap * (g.hp + 1));
        if (e != hipSuccess) return fail(B4D_ENOMEM, std::string("wiener workspace: ") + hipGetErrorString(e));
        p->mr_cap = cap;
        p->mr_slots = slots;
    }
    if (nl > 1) {
        if (!p->mr_fork) B4D_HIP(hipEventCreateWithFlags(&p->mr_fork, hipEventDisableTiming));
        B4D_HIP(hipEventRecord(p->mr_fork, st));
        for (int l = 1; l < nl; ++l) {
            if (!p->mr_aux[l]) {
                const int rs = lane_stream(l - 1, &p->mr_aux[l]);
                if (rs) return rs;
            }
            if (!p->mr_join[l]) B4D_HIP(hipEventCreateWithFlags(&p->mr_join[l], hipEventDisableTiming));
            B4D_HIP(hipStreamWaitEvent(p->mr_aux[l], p->mr_fork, 0));
        }
    }
    const size_t fp = (size_t)g.h * g.w;
    int rc = B4D_OK, grp = 0;
    for (int b0 = 0; b0 < batch && rc == B4D_OK; b0 += fpl, ++grp) {
        const int nf = std::min(fpl, batch - b0), lane = grp % nl;
        hipStream_t ls = lane ? p->mr_aux[lane] : st;
        float2* T = p->mr_T + (size_t)lane * p->mr_cap * g.Wh * g.Hp;
        float* amax = p->mr_amax + (size_t)lane * p->mr_cap * (g.hp + 1);
        float* pmax = amax + p->mr_cap;
        rc = wmr_rows_fwd(frames + b0 * fp, T, p->ax.tw, pmax, g, nf, ls);
        if (rc == B4D_OK) rc = wmr_cols(T, p->mr_filt, p->ay.tw, pmax, amax, g, nf, ls, p->mr_sepx, p->mr_sepy, p->mr_balance);
        if (rc == B4D_OK) rc = wmr_rows_inv(T, out + b0 * fp, p->ax.tw, amax, g, nf, ls);
    }
    for (int l = 1; l < nl; ++l) {
        B4D_HIP(hipEventRecord(p->mr_join[l], p->mr_aux[l]));
        B4D_HIP(hipStreamWaitEvent(st, p->mr_join[l], 0));
    }
    return rc;
}

// one frame through pad/normalise -> rows -> columns x filter -> inverse, on stream st with the work buffers of `lane`
static int wiener_frame(b4d_wiener* p, int lane, const float* f, float* o, int clip, hipStream_t st) {
    const b4d_wiener::Lane& L = p->lane[lane];
    const PmAxis &ax = p->ax, &ay = p->ay;
    const size_t fp = (size_t)p->h * p->w, n = (size_t)p->H * p->W;
    const float inv = 1.0f / (float)n;
    hipLaunchKernelGGL(k_nanabsmax, dim3(256), dim3(1024), 0, st, f, fp, L.amax);
    hipLaunchKernelGGL(k_absmax_final, dim3(1), dim3(64), 0, st, L.amax, 256);
    B4D_HIP(hipGetLastError());
    const FusedIO io{f, o, L.amax, p->h, p->w, p->py, p->px, clip, p->W / 2 + 1, p->H};
    int rc;
    if (ax.A && ay.A) {
        // real input: rows ride in pairs (a + i b) through one complex transform, only the W/2 + 1 independent
        // columns go through the column passes (the filter of a real PSF is Hermitian), the inverse row pass
        // rebuilds each pair from its two half rows
        const int Wh = p->W / 2 + 1, Hp = (p->H + 1) / 2;
        if ((rc = dft_rows(ax, nullptr, PmIn::ReflectPair, L.a, L.b, L.c, PmOut::HalfPair, Hp, false, nullptr, 1.f, st, &io))) return rc;
        if ((rc = transpose_batch(L.c, L.a, p->H, Wh, 1, st))) return rc;
        if ((rc = dft_rows(ay, L.a, PmIn::Complex, L.b, L.c, L.a, PmOut::Complex, Wh, false, p->filt, 1.f, st))) return rc;
        if ((rc = dft_rows(ay, L.a, PmIn::Complex, L.b, L.c, L.a, PmOut::Complex, Wh, true, nullptr, 1.f, st))) return rc;
        if ((rc = transpose_batch(L.a, L.b, Wh, p->H, 1, st))) return rc;
        return dft_rows(ax, L.b, PmIn::HermPair, L.c, L.a, L.c, PmOut::CropPair, Hp, true, nullptr, inv, st, &io);
    }
    // forward: rows (frame -> c), transpose (c -> a), columns + filter (a -> a), all in the transposed domain after that
    if (ax.A) {  // reflect padding and normalisation folded into the row pass's loads
        rc = dft_rows(ax, nullptr, PmIn::Reflect, L.a, L.b, L.c, PmOut::Complex, p->H, false, nullptr, 1.f, st, &io);
    } else {
        hipLaunchKernelGGL(k_pad_reflect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f, p->h, p->w, p->py, p->px, L.amax, L.padded);
        B4D_HIP(hipGetLastError());
        rc = dft_rows(ax, L.padded, PmIn::Real, L.a, L.b, L.c, PmOut::Complex, p->H, false, nullptr, 1.f, st);
    }
    if (rc) return rc;
    if ((rc = transpose_batch(L.c, L.a, p->H, p->W, 1, st))) return rc;
    if ((rc = dft_rows(ay, L.a, PmIn::Complex, L.b, L.c, L.a, PmOut::Complex, p->W, false, p->filt, 1.f, st))) return rc;
    // inverse: columns (a -> a), transpose (a -> b), rows (b -> b) with the 1/(H W) factor
    if ((rc = dft_rows(ay, L.a, PmIn::Complex, L.b, L.c, L.a, PmOut::Complex, p->W, true, nullptr, 1.f, st))) return rc;
    if ((rc = transpose_batch(L.a, L.b, p->W, p->H, 1, st))) return rc;
    if (ax.A)   // clip, rescale and crop folded into the last pass's stores
        return dft_rows(ax, L.b, PmIn::Complex, L.c, L.a, L.b, PmOut::Crop, p->H, true, nullptr, inv, st, &io);
    if ((rc = dft_rows(ax, L.b, PmIn::Complex, L.c, L.a, L.b, PmOut::Complex, p->H, true, nullptr, inv, st))) return rc;
    hipLaunchKernelGGL(k_crop_out<float2>, dim3((unsigned)((fp + 255) / 256)), dim3(256), 0, st, L.b, p->h, p->w, p->py, p->px, L.amax, clip, o);
    B4D_HIP(hipGetLastError());
    return B4D_OK;
}

// every lane: work buffers (lane 0 has them since the plan was created), a non-blocking stream and its join event
static int wiener_lanes(b4d_wiener* p) {
    if (p->fork) return B4D_OK;
    const size_t n = (size_t)p->H * p->W;
    for (int l = 0; l < B4D_WIENER_LANES; ++l) {
        b4d_wiener::Lane& L = p->lane[l];
        // each step only if still missing: a call that failed half-way (out of memory) can be repeated
        if (!L.a) B4D_HIP(hipMalloc((void**)&L.a, sizeof(float2) * n));
        if (!L.b) B4D_HIP(hipMalloc((void**)&L.b, sizeof(float2) * n));
        if (!L.c) B4D_HIP(hipMalloc((void**)&L.c, sizeof(float2) * n));
        if (!L.padded) B4D_HIP(hipMalloc((void**)&L.padded, sizeof(float) * n));
        if (!L.amax) B4D_HIP(hipMalloc((void**)&L.amax, sizeof(float) * 256));
        if (!L.st) {
            const int rs = lane_stream(l, &L.st);
            if (rs) return rs;
        }
        if (!L.done) B4D_HIP(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    }
    B4D_HIP(hipEventCreateWithFlags(&p->fork, hipEventDisableTiming));
    return B4D_OK;
}

int b4d_wiener_apply(b4d_wiener* p, const float* frames, int batch, float* out, int clip, void* stream) {
    if (!p) return fail(B4D_EINVAL, "null argument");
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    if (!p || !frames || !out) return fail(B4D_EINVAL, "null argument");
    if (batch < 1) return fail(B4D_EINVAL, "batch must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    const size_t fp = (size_t)p->h * p->w;
    if (p->mr) return wiener_mr_apply(p, frames, batch, out, clip, st);
    if (batch == 1) return wiener_frame(p, 0, frames, out, clip, st);
    if (!g_opt_lanes.load()) {   // option "lanes" 0: the caller's stream only
        int r1 = B4D_OK;
        for (int b = 0; b < batch && r1 == B4D_OK; ++b) r1 = wiener_frame(p, 0, frames + b * fp, out + b * fp, clip, st);
        return r1;
    }
    int rc = wiener_lanes(p);
    if (rc) return rc;
    // fork: the lanes start after everything already queued on the caller's stream; join: the caller's stream waits for all
    const int nl = std::min(batch, B4D_WIENER_LANES);
    B4D_HIP(hipEventRecord(p->fork, st));
    for (int l = 0; l < nl; ++l) B4D_HIP(hipStreamWaitEvent(p->lane[l].st, p->fork, 0));
    for (int b = 0; b < batch && rc == B4D_OK; ++b) rc = wiener_frame(p, b % nl, frames + b * fp, out + b * fp, clip, p->lane[b % nl].st);
    for (int l = 0; l < nl; ++l) {
        B4D_HIP(hipEventRecord(p->lane[l].done, p->lane[l].st));
        B4D_HIP(hipStreamWaitEvent(st, p->lane[l].done, 0));
    }
    return rc;
}

int b4d_richardson_lucy(const float* frames, int batch, int h, int w, const float* psf_host, int ky, int kx, int num_iter,
                        float filter_epsilon, int clip, float* out, void* stream) {
    B4D_SCRATCH_LOCK();
    if (!frames || !out || !psf_host) return fail(B4D_EINVAL, "null argument");
    if (batch < 1 || h < 2 || w < 2 || num_iter < 1) return fail(B4D_EINVAL, "batch, num_iter >= 1 and h, w >= 2 required");
    if (ky < 1 || kx < 1 || !(ky & 1) || !(kx & 1) || ky > RL_MAXK || kx > RL_MAXK) return fail(B4D_EINVAL, "kernel sides must be odd and <= 33");
    if (ky / 2 >= h || kx / 2 >= w) return fail(B4D_EINVAL, "kernel larger than the frame");
    hipStream_t st = (hipStream_t)stream;
    const int py = ky / 2, px = kx / 2, H = h + 2 * py, W = w + 2 * px;
    const size_t n = (size_t)H * W, fp = (size_t)h * w;
    void* ws = nullptr;
    int rc = get_scratch(sizeof(float) * (3 * n + 256 + (size_t)ky * kx) + 1024, &ws, (hipStream_t)stream);
    if (rc) return rc;
    float* work = static_cast<float*>(ws);
    float* est = work + n;
    float* rel = est + n;
    float* amax = rel + n;
    float* psf = amax + 256;
    B4D_HIP(hipMemcpyAsync(psf, psf_host, sizeof(float) * ky * kx, hipMemcpyHostToDevice, st));
    B4D_HIP(hipStreamSynchronize(st));   // psf_host is caller-owned
    // dynamic LDS of k_rl_step: the haloed tile and the kernel; at most 4 (96 * 64 + 33 * 33) = 28 932 bytes (ky = kx = RL_MAXK)
    const size_t lds = sizeof(float) * ((size_t)(RL_TX + 2 * px) * (RL_TY + 2 * py) + (size_t)ky * kx);
    const dim3 grid((W + RL_TX - 1) / RL_TX, (H + RL_TY - 1) / RL_TY);
    for (int b = 0; b < batch; ++b) {
        const float* f = frames + b * fp;
        hipLaunchKernelGGL(k_nanabsmax, dim3(256), dim3(1024), 0, st, f, fp, amax);
        hipLaunchKernelGGL(k_absmax_final, dim3(1), dim3(64), 0, st, amax, 256);
        hipLaunchKernelGGL(k_pad_reflect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f, h, w, py, px, amax, work);
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, est, n, 0.5f);
        for (int it = 0; it < num_iter; ++it) {
            if ((rc = launch(k_rl_step<0>, grid, dim3(256), lds, st, est, work, rel, psf, H, W, ky, kx, filter_epsilon))) return rc;
            if ((rc = launch(k_rl_step<1>, grid, dim3(256), lds, st, rel, work, est, psf, H, W, ky, kx, 0.f))) return rc;
        }
        hipLaunchKernelGGL(k_crop_out<float>, dim3((unsigned)((fp + 255) / 256)), dim3(256), 0, st, est, h, w, py, px, amax, clip, out + b * fp);
        B4D_HIP(hipGetLastError());
    }
    B4D_HIP(hipStreamSynchronize(st));   // the shared scratch must outlive the kernels
    return B4D_OK;
}

}  // extern "C"
