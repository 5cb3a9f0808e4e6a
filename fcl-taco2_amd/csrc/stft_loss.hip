// stft_loss.hip — multi-resolution STFT loss: spectral convergence and log-magnitude distance of a generated waveform x against a target y, with the
// gradient with respect to x (include/fcl_hip.h "Multi-resolution STFT loss").  gfx950 only.  One resolution (n_fft, hop, window) per call,
// on the LDS-resident real FFT of gl_fft.h; the analysis is fx_logmel_kernel's (features.hip), the inverse transform gl_synth_kernel's and the
// gather gl_ola_kernel's (griffinlim.hip).
//   stl_sums_kernel<N>         a workgroup of 256 threads holds GlGeo<N>::FPW frames of x AND of y (two sets of FFT planes, 33.8 KB of LDS): reflected
//                              gather, times the window, forward FFT, split; p = re^2 + im^2, m = sqrt(max(p, 1e-7)).  Thread j of a frame slot owns
//                              the bins j, j + TPS, j + 2 TPS, j + 3 TPS (thread 0: and bin N / 2) and sums its (m_y - m_x)^2, m_y^2 and
//                              |log m_y - log m_x|; a tree in LDS over the slot's TPS threads gives frame_sums [frames, 3].  Nothing of size
//                              frames x bins reaches HBM.
//   stl_utt_sums_kernel        one workgroup of 64 threads per utterance: lane l adds the frames of its contiguous chunk in ascending order in float64,
//                              lane 0 adds the 64 chunk totals in ascending order -> utt_sums [n_utt, 3] double.  The chunks depend on the
//                              utterance's own frame count only.
//   stl_grad_frames_kernel<N>  recomputes both transforms in LDS (nothing is kept from the forward pass but the sums behind coef), forms
//                              dm = coef0 (m_y - m_x) - coef1 sign(log m_y - log m_x) / m_x, G = (dm / m_x) X where p_x > 1e-7 and 0 elsewhere, the
//                              half spectrum Yh (G / 2 between the real end bins), the inverse real FFT as gl_synth_kernel does, times 2 w:
//                              fr [frames, N] = w N irfft(Yh).
//   stl_grad_gather_kernel     one thread per sample j of x: sums fr over the frames that cover the padded position j + N / 2, then those that cover
//                              its left mirror N / 2 - j (1 <= j <= N / 2), then its right mirror N / 2 + 2 (L - 1) - j (L - 1 - N / 2 <= j <= L - 2),
//                              each in ascending frame order: gl_ola_kernel's scheme plus the adjoint of the reflection.
// No atomics and no order that depends on the batch: a batch is bit for bit its per-utterance runs.  Utterance u owns the samples smp_off[u] ..
// smp_off[u + 1] of x and of y and the frames utt_off[u] .. utt_off[u + 1]; T = L / hop + 1.
// The mel-spectrogram loss (msl_*) follows the STFT loss's kernels below and is described there.
#include <algorithm>
#include <cmath>

#include "fcl_common.h"
#include "gl_fft.h"

namespace fcl {

constexpr float STL_CLAMP = 1e-7f;

// the FPW frames of one signal into buffer 0 of re / im: fx_logmel_kernel's gather (clamped frame_utt, reflected index clamped into the utterance)
template <int N>
__device__ __forceinline__ void stl_load(const float* __restrict__ x, const int* __restrict__ smp_off, const int* __restrict__ frame_utt,
                                         const int* __restrict__ utt_off, const float* __restrict__ window, int hop, int frames, int n_utt, long long f0,
                                         float* re, float* im, int tid) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, FPW = G::FPW;
    for (int i = tid; i < FPW * M; i += 256) {
        const int slot = i / M, n = i % M;
        const long long f = f0 + slot;
        float v[2] = {0.f, 0.f};
        if (f < frames) {
            const int u = min(max(frame_utt[f], 0), n_utt - 1), t = (int)f - utt_off[u], s0 = smp_off[u], L = smp_off[u + 1] - s0;
            if (L > 0) {
                const float2 w = *reinterpret_cast<const float2*>(window + 2 * n);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    int q = t * hop + 2 * n + e - N / 2;
                    q = q < 0 ? -q : q;
                    q = q >= L ? (L - 1) - (q - (L - 1)) : q;
                    q = min(max(q, 0), L - 1);  // (no effect for L >= N / 2 + 1, the supported range: keeps every other call inside x)
                    v[e] = x[(long long)s0 + q] * (e ? w.y : w.x);
                }
            }
        }
        re[slot * SLOT + gl_pad(n)] = v[0];
        im[slot * SLOT + gl_pad(n)] = v[1];
    }
}

// X[k] = (Z[k] + conj Z[M - k]) / 2 + W_N^k (Z[k] - conj Z[M - k]) / (2 i), k = 0 .. M, Z[M] = Z[0]; zr / zi: one frame slot of the FFT's result
template <int N>
__device__ __forceinline__ float2 stl_bin(const float* zr, const float* zi, const float2* __restrict__ tw, int k) {
    constexpr int M = N / 2;
    const int a = gl_pad(k & (M - 1)), b = gl_pad((M - k) & (M - 1));
    const float2 zk = make_float2(zr[a], zi[a]), zm = make_float2(zr[b], -zi[b]);
    const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
    const float2 d = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
    const float2 o = gl_cmul(tw[k], d);
    float2 c = make_float2(e.x + o.x, e.y + o.y);
    if (k == 0 || k == M) c.y = 0.f;
    return c;
}

__device__ __forceinline__ float stl_power(float2 c) { return fmaf(c.x, c.x, c.y * c.y); }

template <int N>
__global__ __launch_bounds__(256) void stl_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ smp_off,
                                                       const int* __restrict__ frame_utt, const int* __restrict__ utt_off, const float* __restrict__ window,
                                                       const float2* __restrict__ tw, int hop, int frames, int n_utt, float* __restrict__ frame_sums) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, PLANE = G::PLANE, FPW = G::FPW, TPS = 256 / FPW;  // TPS threads per frame slot: M == 4 TPS
    __shared__ float xre[2 * PLANE], xim[2 * PLANE], yre[2 * PLANE], yim[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
    stl_load<N>(x, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, xre, xim, tid);
    stl_load<N>(y, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, yre, yim, tid);
    __syncthreads();
    const int cur = gl_fft<N, false>(xre, xim, tw, tid);
    gl_fft<N, false>(yre, yim, tw, tid);  // the same pass count: the same buffer
    const int slot = tid / TPS, j = tid % TPS;
    const float *xr = xre + cur * PLANE + slot * SLOT, *xi = xim + cur * PLANE + slot * SLOT;
    const float *yr = yre + cur * PLANE + slot * SLOT, *yi = yim + cur * PLANE + slot * SLOT;
    float *pa = xre + (cur ^ 1) * PLANE, *pb = xim + (cur ^ 1) * PLANE, *pc = yre + (cur ^ 1) * PLANE;  // the buffers the FFTs left behind: [256] each
    float sa = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int k = r < 4 ? j + r * TPS : M;
        if (r == 4 && j != 0) break;
        const float mx = sqrtf(fmaxf(stl_power(stl_bin<N>(xr, xi, tw, k)), STL_CLAMP));
        const float my = sqrtf(fmaxf(stl_power(stl_bin<N>(yr, yi, tw, k)), STL_CLAMP));
        const float d = my - mx;
        sa = fmaf(d, d, sa);
        sb = fmaf(my, my, sb);
        sc += fabsf(logf(my) - logf(mx));
    }
    pa[tid] = sa;
    pb[tid] = sb;
    pc[tid] = sc;
    __syncthreads();
#pragma unroll
    for (int h = TPS / 2; h >= 1; h >>= 1) {
        if (j < h) {
            pa[tid] += pa[tid + h];
            pb[tid] += pb[tid + h];
            pc[tid] += pc[tid + h];
        }
        __syncthreads();
    }
    if (j == 0 && f0 + slot < frames) {
        float* o = frame_sums + (size_t)(f0 + slot) * 3;
        o[0] = pa[tid];
        o[1] = pb[tid];
        o[2] = pc[tid];
    }
}

__global__ __launch_bounds__(64) void stl_utt_sums_kernel(const float* __restrict__ frame_sums, const int* __restrict__ utt_off, int frames,
                                                          double* __restrict__ utt_sums) {
    __shared__ double part[64 * 3];
    const int u = blockIdx.x, l = threadIdx.x;
    const int lo = min(max(utt_off[u], 0), frames), hi = min(max(utt_off[u + 1], lo), frames);
    const int T = hi - lo, chunk = (T + 63) / 64;
    const int a = min(lo + l * chunk, hi), b = min(a + chunk, hi);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int f = a; f < b; ++f) {
        s0 += (double)frame_sums[(size_t)f * 3];
        s1 += (double)frame_sums[(size_t)f * 3 + 1];
        s2 += (double)frame_sums[(size_t)f * 3 + 2];
    }
    part[l * 3] = s0;
    part[l * 3 + 1] = s1;
    part[l * 3 + 2] = s2;
    __syncthreads();
    if (l < 3) {
        double s = 0.0;
        for (int i = 0; i < 64; ++i) s += part[i * 3 + l];
        utt_sums[(size_t)u * 3 + l] = s;
    }
}

template <int N>
__global__ __launch_bounds__(256) void stl_grad_frames_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ smp_off,
                                                              const int* __restrict__ frame_utt, const int* __restrict__ utt_off,
                                                              const float* __restrict__ window, const float2* __restrict__ tw,
                                                              const float* __restrict__ coef, int hop, int frames, int n_utt, float* __restrict__ fr) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, PLANE = G::PLANE, BINS = G::BINS, FPW = G::FPW;
    __shared__ float xre[2 * PLANE], xim[2 * PLANE], yre[2 * PLANE], yim[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
    stl_load<N>(x, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, xre, xim, tid);
    stl_load<N>(y, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, yre, yim, tid);
    __syncthreads();
    const int cur = gl_fft<N, false>(xre, xim, tw, tid);
    gl_fft<N, false>(yre, yim, tw, tid);
    float *hr = xre + (cur ^ 1) * PLANE, *hi = xim + (cur ^ 1) * PLANE;  // Yh [FPW][BINS] (FPW BINS <= PLANE) in the buffer x's FFT left behind
    for (int i = tid; i < FPW * BINS; i += 256) {
        const int slot = i / BINS, k = i - slot * BINS;
        const long long f = f0 + slot;
        float2 g = make_float2(0.f, 0.f);
        if (f < frames) {
            const int u = min(max(frame_utt[f], 0), n_utt - 1);
            const float2 cx = stl_bin<N>(xre + cur * PLANE + slot * SLOT, xim + cur * PLANE + slot * SLOT, tw, k);
            const float px = stl_power(cx), py = stl_power(stl_bin<N>(yre + cur * PLANE + slot * SLOT, yim + cur * PLANE + slot * SLOT, tw, k));
            if (px > STL_CLAMP) {  // the clamp passes no gradient
                const float mx = sqrtf(px), my = sqrtf(fmaxf(py, STL_CLAMP));
                const float dl = logf(my) - logf(mx);
                const float sg = dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f);
                const float dm = coef[2 * u] * (my - mx) - coef[2 * u + 1] * sg / mx;
                const float s = (k == 0 || k == M ? 1.f : 0.5f) * dm / mx;
                g = make_float2(s * cx.x, s * cx.y);
            }
        }
        hr[i] = g.x;
        hi[i] = g.y;
    }
    __syncthreads();
    // Z[k] = E[k] + i O[k], E = (Yh[k] + conj Yh[M - k]) / 2, O = (Yh[k] - conj Yh[M - k]) / 2 * conj(W_N^k), into buffer 0 of y's planes (y's spectrum is used up)
    for (int i = tid; i < FPW * M; i += 256) {
        const int slot = i / M, k = i % M;
        const float2 xk = make_float2(hr[slot * BINS + k], hi[slot * BINS + k]), xm = make_float2(hr[slot * BINS + M - k], hi[slot * BINS + M - k]);
        const float2 e = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
        const float2 w = tw[k];
        const float2 o = gl_cmul(d, make_float2(w.x, -w.y));
        yre[slot * SLOT + gl_pad(k)] = e.x - o.y;
        yim[slot * SLOT + gl_pad(k)] = e.y + o.x;
    }
    __syncthreads();
    const int ci = gl_fft<N, true>(yre, yim, tw, tid);
    // w N irfft(Yh): the unscaled inverse of M points is M irfft at the even (re) and odd (im) samples
    for (int i = tid; i < FPW * M; i += 256) {
        const int slot = i / M, n = i % M;
        const long long f = f0 + slot;
        if (f >= frames) continue;
        const float2 w = *reinterpret_cast<const float2*>(window + 2 * n);
        const float a = 2.f * yre[ci * PLANE + slot * SLOT + gl_pad(n)], b = 2.f * yim[ci * PLANE + slot * SLOT + gl_pad(n)];
        *reinterpret_cast<float2*>(fr + (size_t)f * N + 2 * n) = make_float2(a * w.x, b * w.y);
    }
}

// the frames t of an utterance (T of them from frame lo) that cover the padded position p, in ascending order
__device__ __forceinline__ float stl_gather_pos(const float* __restrict__ fr, int p, int lo, int T, int n_fft, int hop, float acc) {
    const int t_lo = p >= n_fft ? (p - n_fft) / hop + 1 : 0, t_hi = min(p / hop, T - 1);
    for (int t = t_lo; t <= t_hi; ++t) acc += fr[(size_t)(lo + t) * n_fft + (p - t * hop)];
    return acc;
}

__global__ __launch_bounds__(256) void stl_grad_gather_kernel(const float* __restrict__ fr, const int* __restrict__ smp_off, const int* __restrict__ utt_off,
                                                              int n_fft, int hop, int samples, int frames, int n_utt, int accumulate,
                                                              float* __restrict__ gx) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= samples) return;
    int a = 0, b = n_utt - 1;  // the utterance whose samples hold g: the last u with smp_off[u] <= g
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (smp_off[m] <= g) a = m; else b = m - 1;
    }
    const int u = a, s0 = smp_off[u], L = smp_off[u + 1] - s0, j = (int)g - s0;
    const int lo = min(max(utt_off[u], 0), frames), T = min(max(utt_off[u + 1] - lo, 0), frames - lo), h = n_fft / 2;
    float acc = 0.f;
    if (j >= 0 && j < L) {  // (always, on maps the package builds)
        acc = stl_gather_pos(fr, j + h, lo, T, n_fft, hop, acc);
        if (j >= 1 && j <= h) acc = stl_gather_pos(fr, h - j, lo, T, n_fft, hop, acc);
        if (j >= L - 1 - h && j <= L - 2) acc = stl_gather_pos(fr, h + (L - 1) + (L - 1 - j), lo, T, n_fft, hop, acc);
    }
    gx[g] = accumulate ? gx[g] + acc : acc;
}

static int stl_check(const fcl_stl_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n_fft == 512 || a->n_fft == 1024 || a->n_fft == 2048, FCL_ERR_SHAPE, "%s: n_fft must be 512, 1024 or 2048 (got %d)", who, a->n_fft);
    FCL_REQUIRE(a->hop >= 1 && a->hop <= a->n_fft / 2, FCL_ERR_SHAPE, "%s: 1 <= hop <= n_fft / 2 expected (got hop %d, n_fft %d)", who, a->hop, a->n_fft);
    FCL_REQUIRE(a->frames >= 1 && a->n_utt >= 1 && a->n_utt <= a->frames, FCL_ERR_SHAPE, "%s: frames >= n_utt >= 1 expected (got %lld, %d)", who,
                (long long)a->frames, a->n_utt);
    FCL_REQUIRE(a->frames * (int64_t)a->n_fft < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: frames x n_fft must stay below 2^31 (got %lld frames)", who,
                (long long)a->frames);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->x && a->y && a->smp_off && a->frame_utt && a->utt_off, FCL_ERR_INVALID, "%s: null x / y / smp_off / frame_utt / utt_off", who);
    FCL_REQUIRE(a->window && a->twiddle, FCL_ERR_INVALID, "%s: null window / twiddle", who);
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->window) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->twiddle) & 7u) == 0, FCL_ERR_ALIGN,
                "%s: window and twiddle must be 8-byte aligned", who);
    return FCL_OK;
}

// ---- mel-spectrogram loss (include/fcl_hip.h "Mel-spectrogram loss"): the L1 distance of the log10 mels of x and y on the same two-signal
// transform; stl_load, stl_bin, stl_power and stl_grad_gather_kernel above are used as they are.
//   msl_sums_kernel<N>         after both FFTs: m = sqrt(max(p, 1e-10)) of x and of y per bin into the re planes the FFTs left behind; one thread per
//                              (frame slot, channel) sums its band fb_w[fb_off[c] .. fb_off[c + 1]) from bin fb_lo[c] in ascending k for both signals,
//                              M = max(sum, 1e-10), and writes |log10 M_x - log10 M_y|; thread j of a slot adds the channels j, j + TPS, .. in ascending
//                              order, a tree over the slot's TPS threads gives frame_sums [frames].
//   msl_utt_sums_kernel        stl_utt_sums_kernel's chunking on one column -> utt_sums [n_utt] double.
//   msl_grad_frames_kernel<N>  recomputes transforms, magnitudes and mels; dl [FPW][n_mels] = coef sign(l_x - l_y) / M_x (0 at the floor) in the im plane
//                              y's FFT left behind; one thread per (slot, bin) sums dm = sum bt_w dl[bt_ch] over bt_off[k] .. bt_off[k + 1] (the
//                              bin-major transpose of the filterbank, channels ascending), G = (dm / m_x) X where p_x > 1e-10, Yh over the two planes
//                              x's FFT left behind; merge, inverse FFT and fr as stl_grad_frames_kernel.
constexpr float MSL_FLOOR = 1e-10f;
constexpr int MSL_MEL_MAX = 256;  // features.hip's FX_MEL_MAX: FPW n_mels <= 1024 fits one LDS plane

// S [FPW][BINS] = sqrt(max(p, 1e-10)) of the spectrum in zr / zi (one FFT's result)
template <int N>
__device__ __forceinline__ void msl_magnitudes(const float* zr, const float* zi, const float2* __restrict__ tw, float* S, int tid) {
    using G = GlGeo<N>;
    constexpr int SLOT = G::SLOT, BINS = G::BINS, FPW = G::FPW;
    for (int i = tid; i < FPW * BINS; i += 256) {
        const int slot = i / BINS, k = i - slot * BINS;
        S[i] = sqrtf(fmaxf(stl_power(stl_bin<N>(zr + slot * SLOT, zi + slot * SLOT, tw, k)), MSL_FLOOR));
    }
}

// channel c's band, clamped as fx_logmel_kernel clamps: the weights fb_w[o0 .. o0 + len) over the bins from lo
__device__ __forceinline__ void msl_band(const int* __restrict__ fb_lo, const int* __restrict__ fb_off, int c, int nnz, int bins, int& o0, int& lo, int& len) {
    o0 = min(max(fb_off[c], 0), nnz);
    const int o1 = min(max(fb_off[c + 1], o0), nnz);
    lo = min(max(fb_lo[c], 0), bins);
    len = min(o1 - o0, bins - lo);
}

__device__ __forceinline__ float msl_mel(const float* sf, const float* __restrict__ w, int len) {
    float acc = 0.f;
    for (int j = 0; j < len; ++j) acc = fmaf(sf[j], w[j], acc);
    return acc;
}

template <int N>
__global__ __launch_bounds__(256) void msl_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ smp_off,
                                                       const int* __restrict__ frame_utt, const int* __restrict__ utt_off, const float* __restrict__ window,
                                                       const float2* __restrict__ tw, const int* __restrict__ fb_lo, const int* __restrict__ fb_off,
                                                       const float* __restrict__ fb_w, int hop, int frames, int n_utt, int n_mels, int nnz,
                                                       float* __restrict__ frame_sums) {
    using G = GlGeo<N>;
    constexpr int PLANE = G::PLANE, BINS = G::BINS, FPW = G::FPW, TPS = 256 / FPW;
    __shared__ float xre[2 * PLANE], xim[2 * PLANE], yre[2 * PLANE], yim[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
    stl_load<N>(x, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, xre, xim, tid);
    stl_load<N>(y, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, yre, yim, tid);
    __syncthreads();
    const int cur = gl_fft<N, false>(xre, xim, tw, tid);
    gl_fft<N, false>(yre, yim, tw, tid);
    float *sx = xre + (cur ^ 1) * PLANE, *sy = yre + (cur ^ 1) * PLANE;    // S_x, S_y [FPW][BINS]
    float *dl = xim + (cur ^ 1) * PLANE, *part = yim + (cur ^ 1) * PLANE;  // |l_x - l_y| [FPW][n_mels], part [256]
    msl_magnitudes<N>(xre + cur * PLANE, xim + cur * PLANE, tw, sx, tid);
    msl_magnitudes<N>(yre + cur * PLANE, yim + cur * PLANE, tw, sy, tid);
    __syncthreads();
    for (int i = tid; i < FPW * n_mels; i += 256) {
        const int slot = i / n_mels, c = i - slot * n_mels;
        int o0, lo, len;
        msl_band(fb_lo, fb_off, c, nnz, BINS, o0, lo, len);
        const float ax = msl_mel(sx + slot * BINS + lo, fb_w + o0, len), ay = msl_mel(sy + slot * BINS + lo, fb_w + o0, len);
        dl[i] = fabsf(log10f(fmaxf(ax, MSL_FLOOR)) - log10f(fmaxf(ay, MSL_FLOOR)));
    }
    __syncthreads();
    const int slot = tid / TPS, j = tid % TPS;
    float acc = 0.f;
    for (int c = j; c < n_mels; c += TPS) acc += dl[slot * n_mels + c];
    part[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int h = TPS / 2; h >= 1; h >>= 1) {
        if (j < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (j == 0 && f0 + slot < frames) frame_sums[f0 + slot] = part[tid];
}

__global__ __launch_bounds__(64) void msl_utt_sums_kernel(const float* __restrict__ frame_sums, const int* __restrict__ utt_off, int frames,
                                                          double* __restrict__ utt_sums) {
    __shared__ double part[64];
    const int u = blockIdx.x, l = threadIdx.x;
    const int lo = min(max(utt_off[u], 0), frames), hi = min(max(utt_off[u + 1], lo), frames);
    const int T = hi - lo, chunk = (T + 63) / 64;
    const int a = min(lo + l * chunk, hi), b = min(a + chunk, hi);
    double s = 0.0;
    for (int f = a; f < b; ++f) s += (double)frame_sums[f];
    part[l] = s;
    __syncthreads();
    if (l == 0) {
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += part[i];
        utt_sums[u] = t;
    }
}

template <int N>
__global__ __launch_bounds__(256) void msl_grad_frames_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ smp_off,
                                                              const int* __restrict__ frame_utt, const int* __restrict__ utt_off,
                                                              const float* __restrict__ window, const float2* __restrict__ tw,
                                                              const int* __restrict__ fb_lo, const int* __restrict__ fb_off, const float* __restrict__ fb_w,
                                                              const int* __restrict__ bt_off, const int* __restrict__ bt_ch, const float* __restrict__ bt_w,
                                                              const float* __restrict__ coef, int hop, int frames, int n_utt, int n_mels, int nnz,
                                                              float* __restrict__ fr) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, PLANE = G::PLANE, BINS = G::BINS, FPW = G::FPW;
    __shared__ float xre[2 * PLANE], xim[2 * PLANE], yre[2 * PLANE], yim[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
    stl_load<N>(x, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, xre, xim, tid);
    stl_load<N>(y, smp_off, frame_utt, utt_off, window, hop, frames, n_utt, f0, yre, yim, tid);
    __syncthreads();
    const int cur = gl_fft<N, false>(xre, xim, tw, tid);
    gl_fft<N, false>(yre, yim, tw, tid);
    float *hr = xre + (cur ^ 1) * PLANE, *hi = xim + (cur ^ 1) * PLANE;  // phase one: S_x in hr; phase three: Yh [FPW][BINS] in hr / hi
    float *sy = yre + (cur ^ 1) * PLANE, *dl = yim + (cur ^ 1) * PLANE;  // S_y [FPW][BINS], dl [FPW][n_mels]
    msl_magnitudes<N>(xre + cur * PLANE, xim + cur * PLANE, tw, hr, tid);
    msl_magnitudes<N>(yre + cur * PLANE, yim + cur * PLANE, tw, sy, tid);
    __syncthreads();
    for (int i = tid; i < FPW * n_mels; i += 256) {
        const int slot = i / n_mels, c = i - slot * n_mels;
        const long long f = f0 + slot;
        float d = 0.f;
        if (f < frames) {
            int o0, lo, len;
            msl_band(fb_lo, fb_off, c, nnz, BINS, o0, lo, len);
            const float ax = msl_mel(hr + slot * BINS + lo, fb_w + o0, len), ay = msl_mel(sy + slot * BINS + lo, fb_w + o0, len);
            if (ax > MSL_FLOOR) {  // the floor passes no gradient
                const float dd = log10f(ax) - log10f(fmaxf(ay, MSL_FLOOR));
                const float sg = dd > 0.f ? 1.f : (dd < 0.f ? -1.f : 0.f);
                d = coef[min(max(frame_utt[f], 0), n_utt - 1)] * sg / ax;
            }
        }
        dl[i] = d;
    }
    __syncthreads();  // S_x is used up: Yh goes over it
    for (int i = tid; i < FPW * BINS; i += 256) {
        const int slot = i / BINS, k = i - slot * BINS;
        float2 g = make_float2(0.f, 0.f);
        if (f0 + slot < frames) {
            const float2 cx = stl_bin<N>(xre + cur * PLANE + slot * SLOT, xim + cur * PLANE + slot * SLOT, tw, k);
            const float px = stl_power(cx);
            if (px > MSL_FLOOR) {  // nor does the magnitude's floor
                const int e0 = min(max(bt_off[k], 0), nnz), e1 = min(max(bt_off[k + 1], e0), nnz);
                float dm = 0.f;
                for (int e = e0; e < e1; ++e) dm = fmaf(bt_w[e], dl[slot * n_mels + min(max(bt_ch[e], 0), n_mels - 1)], dm);
                const float s = (k == 0 || k == M ? 1.f : 0.5f) * dm / sqrtf(px);
                g = make_float2(s * cx.x, s * cx.y);
            }
        }
        hr[i] = g.x;
        hi[i] = g.y;
    }
    __syncthreads();
    // the merge, the inverse transform and fr: stl_grad_frames_kernel's, into buffer 0 of y's planes (y's spectrum, S_y and dl are used up)
    for (int i = tid; i < FPW * M; i += 256) {
        const int slot = i / M, k = i % M;
        const float2 xk = make_float2(hr[slot * BINS + k], hi[slot * BINS + k]), xm = make_float2(hr[slot * BINS + M - k], hi[slot * BINS + M - k]);
        const float2 e = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
        const float2 w = tw[k];
        const float2 o = gl_cmul(d, make_float2(w.x, -w.y));
        yre[slot * SLOT + gl_pad(k)] = e.x - o.y;
        yim[slot * SLOT + gl_pad(k)] = e.y + o.x;
    }
    __syncthreads();
    const int ci = gl_fft<N, true>(yre, yim, tw, tid);
    for (int i = tid; i < FPW * M; i += 256) {
        const int slot = i / M, n = i % M;
        const long long f = f0 + slot;
        if (f >= frames) continue;
        const float2 w = *reinterpret_cast<const float2*>(window + 2 * n);
        const float a = 2.f * yre[ci * PLANE + slot * SLOT + gl_pad(n)], b = 2.f * yim[ci * PLANE + slot * SLOT + gl_pad(n)];
        *reinterpret_cast<float2*>(fr + (size_t)f * N + 2 * n) = make_float2(a * w.x, b * w.y);
    }
}

static int msl_check(const fcl_msl_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n_fft == 512 || a->n_fft == 1024 || a->n_fft == 2048, FCL_ERR_SHAPE, "%s: n_fft must be 512, 1024 or 2048 (got %d)", who, a->n_fft);
    FCL_REQUIRE(a->hop >= 1 && a->hop <= a->n_fft / 2, FCL_ERR_SHAPE, "%s: 1 <= hop <= n_fft / 2 expected (got hop %d, n_fft %d)", who, a->hop, a->n_fft);
    FCL_REQUIRE(a->n_mels >= 1 && a->n_mels <= MSL_MEL_MAX, FCL_ERR_SHAPE, "%s: 1 <= n_mels <= %d expected (got %d)", who, MSL_MEL_MAX, a->n_mels);
    FCL_REQUIRE(a->nnz >= 1, FCL_ERR_SHAPE, "%s: nnz (the length of fb_w and of bt_w) must be positive (got %d)", who, a->nnz);
    FCL_REQUIRE(a->frames >= 1 && a->n_utt >= 1 && a->n_utt <= a->frames, FCL_ERR_SHAPE, "%s: frames >= n_utt >= 1 expected (got %lld, %d)", who,
                (long long)a->frames, a->n_utt);
    FCL_REQUIRE(a->frames * (int64_t)a->n_fft < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: frames x n_fft must stay below 2^31 (got %lld frames)", who,
                (long long)a->frames);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->x && a->y && a->smp_off && a->frame_utt && a->utt_off, FCL_ERR_INVALID, "%s: null x / y / smp_off / frame_utt / utt_off", who);
    FCL_REQUIRE(a->window && a->twiddle, FCL_ERR_INVALID, "%s: null window / twiddle", who);
    FCL_REQUIRE(a->fb_lo && a->fb_off && a->fb_w, FCL_ERR_INVALID, "%s: null fb_lo / fb_off / fb_w", who);
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->window) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->twiddle) & 7u) == 0, FCL_ERR_ALIGN,
                "%s: window and twiddle must be 8-byte aligned", who);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_stl_sums_fwd(const fcl_stl_t* a, fcl_stream_t stream) {
    const int rc = stl_check(a, "stl_sums_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->frame_sums && a->utt_sums, FCL_ERR_INVALID, "stl_sums_fwd: null frame_sums / utt_sums");
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->utt_sums) & 7u) == 0, FCL_ERR_ALIGN, "stl_sums_fwd: utt_sums (double) must be 8-byte aligned");
    const double flops = 2.0 * 2.5 * a->n_fft * std::log2((double)a->n_fft) * (double)a->frames;
#define STL_SUMS(NN)                                                                                                                                          \
    {                                                                                                                                                         \
        ProfScope ps("stl_sums_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                             \
        hipLaunchKernelGGL(stl_sums_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, a->x, \
                           a->y, a->smp_off, a->frame_utt, a->utt_off, a->window, reinterpret_cast<const float2*>(a->twiddle), a->hop, (int)a->frames,       \
                           a->n_utt, a->frame_sums);                                                                                                          \
    }
    if (a->n_fft == 512) {
        STL_SUMS(512);
    } else if (a->n_fft == 1024) {
        STL_SUMS(1024);
    } else {
        STL_SUMS(2048);
    }
#undef STL_SUMS
    {
        ProfScope ps("stl_utt_sums_kernel", 0.0, (double)a->frames, (hipStream_t)stream);
        hipLaunchKernelGGL(stl_utt_sums_kernel, dim3((unsigned)a->n_utt), dim3(64), 0, (hipStream_t)stream, a->frame_sums, a->utt_off, (int)a->frames, a->utt_sums);
    }
    return check_hip(hipGetLastError(), "stl_sums_fwd");
}

int fcl_stl_grad_bwd(const fcl_stl_t* a, fcl_stream_t stream) {
    const int rc = stl_check(a, "stl_grad_bwd");
    if (rc) return rc;
    FCL_REQUIRE(a->coef && a->fr && a->gx, FCL_ERR_INVALID, "stl_grad_bwd: null coef / fr / gx");
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->fr) & 7u) == 0, FCL_ERR_ALIGN, "stl_grad_bwd: fr must be 8-byte aligned");
    const double flops = 3.0 * 2.5 * a->n_fft * std::log2((double)a->n_fft) * (double)a->frames;
#define STL_GRAD(NN)                                                                                                                                          \
    {                                                                                                                                                         \
        ProfScope ps("stl_grad_frames_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                      \
        hipLaunchKernelGGL(stl_grad_frames_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, \
                           a->x, a->y, a->smp_off, a->frame_utt, a->utt_off, a->window, reinterpret_cast<const float2*>(a->twiddle), a->coef, a->hop,        \
                           (int)a->frames, a->n_utt, a->fr);                                                                                                  \
    }
    if (a->n_fft == 512) {
        STL_GRAD(512);
    } else if (a->n_fft == 1024) {
        STL_GRAD(1024);
    } else {
        STL_GRAD(2048);
    }
#undef STL_GRAD
    {
        ProfScope ps("stl_grad_gather_kernel", 0.0, (double)a->samples, (hipStream_t)stream);
        hipLaunchKernelGGL(stl_grad_gather_kernel, dim3((unsigned)((a->samples + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->fr, a->smp_off, a->utt_off,
                           a->n_fft, a->hop, (int)a->samples, (int)a->frames, a->n_utt, a->accumulate, a->gx);
    }
    return check_hip(hipGetLastError(), "stl_grad_bwd");
}

int fcl_msl_sums_fwd(const fcl_msl_t* a, fcl_stream_t stream) {
    const int rc = msl_check(a, "msl_sums_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->frame_sums && a->utt_sums, FCL_ERR_INVALID, "msl_sums_fwd: null frame_sums / utt_sums");
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->utt_sums) & 7u) == 0, FCL_ERR_ALIGN, "msl_sums_fwd: utt_sums (double) must be 8-byte aligned");
    const double flops = (2.0 * 2.5 * a->n_fft * std::log2((double)a->n_fft) + 4.0 * a->nnz) * (double)a->frames;
#define MSL_SUMS(NN)                                                                                                                                          \
    {                                                                                                                                                         \
        ProfScope ps("msl_sums_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                             \
        hipLaunchKernelGGL(msl_sums_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, a->x, \
                           a->y, a->smp_off, a->frame_utt, a->utt_off, a->window, reinterpret_cast<const float2*>(a->twiddle), a->fb_lo, a->fb_off, a->fb_w, \
                           a->hop, (int)a->frames, a->n_utt, a->n_mels, a->nnz, a->frame_sums);                                                               \
    }
    if (a->n_fft == 512) {
        MSL_SUMS(512);
    } else if (a->n_fft == 1024) {
        MSL_SUMS(1024);
    } else {
        MSL_SUMS(2048);
    }
#undef MSL_SUMS
    {
        ProfScope ps("msl_utt_sums_kernel", 0.0, (double)a->frames, (hipStream_t)stream);
        hipLaunchKernelGGL(msl_utt_sums_kernel, dim3((unsigned)a->n_utt), dim3(64), 0, (hipStream_t)stream, a->frame_sums, a->utt_off, (int)a->frames, a->utt_sums);
    }
    return check_hip(hipGetLastError(), "msl_sums_fwd");
}

int fcl_msl_grad_bwd(const fcl_msl_t* a, fcl_stream_t stream) {
    const int rc = msl_check(a, "msl_grad_bwd");
    if (rc) return rc;
    FCL_REQUIRE(a->bt_off && a->bt_ch && a->bt_w, FCL_ERR_INVALID, "msl_grad_bwd: null bt_off / bt_ch / bt_w");
    FCL_REQUIRE(a->coef && a->fr && a->gx, FCL_ERR_INVALID, "msl_grad_bwd: null coef / fr / gx");
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->fr) & 7u) == 0, FCL_ERR_ALIGN, "msl_grad_bwd: fr must be 8-byte aligned");
    const double flops = (3.0 * 2.5 * a->n_fft * std::log2((double)a->n_fft) + 6.0 * a->nnz) * (double)a->frames;
#define MSL_GRAD(NN)                                                                                                                                          \
    {                                                                                                                                                         \
        ProfScope ps("msl_grad_frames_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                      \
        hipLaunchKernelGGL(msl_grad_frames_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, \
                           a->x, a->y, a->smp_off, a->frame_utt, a->utt_off, a->window, reinterpret_cast<const float2*>(a->twiddle), a->fb_lo, a->fb_off,    \
                           a->fb_w, a->bt_off, a->bt_ch, a->bt_w, a->coef, a->hop, (int)a->frames, a->n_utt, a->n_mels, a->nnz, a->fr);                      \
    }
    if (a->n_fft == 512) {
        MSL_GRAD(512);
    } else if (a->n_fft == 1024) {
        MSL_GRAD(1024);
    } else {
        MSL_GRAD(2048);
    }
#undef MSL_GRAD
    {
        ProfScope ps("stl_grad_gather_kernel", 0.0, (double)a->samples, (hipStream_t)stream);
        hipLaunchKernelGGL(stl_grad_gather_kernel, dim3((unsigned)((a->samples + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->fr, a->smp_off, a->utt_off,
                           a->n_fft, a->hop, (int)a->samples, (int)a->frames, a->n_utt, a->accumulate, a->gx);
    }
    return check_hip(hipGetLastError(), "msl_grad_bwd");
}

}  // extern "C"
