// griffinlim.hip — Griffin-Lim vocoder (mel -> waveform without a trained generator; include/fcl_hip.h "Griffin-Lim vocoder").  gfx950 only.
// The library links no FFT: the real FFT of n_fft = 512 / 1024 / 2048 points lives here, LDS-resident, as a complex FFT of M = n_fft / 2 points on
// z[n] = x[2n] + i x[2n + 1] plus the split stage.
//   gl_fft<N, INV>         Stockham autosort, radix 4 (one radix-2 pass at the end for M = 512), ping-pong between two LDS buffers, one barrier per
//                          pass.  A workgroup of 256 threads holds 1024 complex points = 4 / 2 / 1 frames at n_fft = 512 / 1024 / 2048, so every
//                          thread owns exactly one radix-4 butterfly per pass.  Reads of a pass are contiguous over the threads; its writes have
//                          stride 4 s (s = 1, 4, 16, ..): re and im are separate planes and word i sits at i + (i >> 5), which makes the stride-4
//                          pass conflict free on the 32 banks of ds_write_b32 and leaves the stride-16 pass at most 2-way.
//                          Twiddles W_N^k = exp(-2 pi i k / N), k < N, come from a table computed in double on the host (W_M^k = W_N^2k).
//   gl_mel2lin_kernel      de-normalise, exp10f, [frames, n_mels] x [n_mels, F] in fp32 FMA (ascending mel channel), floor 1e-10
//   gl_phase_init_kernel   P = exp(2 pi i u), u = counter hash of (utt_seed[utterance], frame within the utterance, bin)
//   gl_synth_kernel<N>     X = S P -> inverse real FFT -> times the window -> fr [frames, N]
//   gl_ola_kernel          overlap-add as a GATHER: one thread per output sample sums its <= ceil(N / hop) frames in ascending frame order, divides by
//                          the window-sum-square it accumulates beside it (left undivided where that is <= FLT_MIN) and drops N / 2 samples at both
//                          ends.  No atomics: a batch is bit for bit its per-utterance runs.
//   gl_analysis_kernel<N>  gathers the frame with the utterance's own reflection, times the window, forward FFT, split; the phase update
//                          A = C - alpha C_prev, P = A / (|A| + 1e-16), C_prev = C runs in the epilogue, so C is never re-read.
// Utterance bounds come from frame_utt [frames] / utt_off [n_utt + 1] like the other vocoder kernels; utterance u (T frames from frame utt_off[u])
// owns hop (T - 1) samples from sample hop (utt_off[u] - u) of y.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "fcl_common.h"
#include "gl_fft.h"

namespace fcl {

// ---- mel -> linear magnitudes -----------------------------------------------------------------------------------------------------------------
constexpr int GL_MEL_ROWS = 8, GL_MEL_MAX = 256;

__global__ __launch_bounds__(256) void gl_mel2lin_kernel(const float* __restrict__ mel, const float* __restrict__ stats, const float* __restrict__ pinv_t,
                                                         float* __restrict__ S, int frames, int n_mels, int bins) {
    __shared__ float sm[GL_MEL_ROWS * GL_MEL_MAX];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * GL_MEL_ROWS;
    for (int i = tid; i < GL_MEL_ROWS * n_mels; i += 256) {
        const int r = i / n_mels, c = i - r * n_mels;
        float v = 0.f;
        if (f0 + r < frames) {
            float lm = mel[(f0 + r) * n_mels + c];
            if (stats) lm = fmaf(lm, stats[n_mels + c] + 1e-8f, stats[c]);
            v = exp10f(lm);
        }
        sm[i] = v;
    }
    __syncthreads();
    for (int k = tid; k < bins; k += 256) {
        float acc[GL_MEL_ROWS];
#pragma unroll
        for (int r = 0; r < GL_MEL_ROWS; ++r) acc[r] = 0.f;
        for (int c = 0; c < n_mels; ++c) {
            const float w = pinv_t[(size_t)c * bins + k];
#pragma unroll
            for (int r = 0; r < GL_MEL_ROWS; ++r) acc[r] = fmaf(sm[r * n_mels + c], w, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < GL_MEL_ROWS; ++r)
            if (f0 + r < frames) S[(f0 + r) * bins + k] = fmaxf(1e-10f, acc[r]);
    }
}

// ---- initial phase --------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline float gl_uniform(unsigned int seed, unsigned int t_local, unsigned int k) {
    const unsigned int a = hash_u32(seed ^ hash_u32(t_local + 0x9E3779B9u));
    const unsigned int h = hash_u32(a ^ (k * 0x85EBCA6Bu));
    return (float)(h >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
}

__global__ __launch_bounds__(256) void gl_phase_init_kernel(const unsigned int* __restrict__ utt_seed, const int* __restrict__ frame_utt,
                                                            const int* __restrict__ utt_off, long long total, int bins, float2* __restrict__ P,
                                                            float* __restrict__ u_out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int f = (int)(g / bins), k = (int)(g - (long long)f * bins);
    const int u = frame_utt[f];
    const float uv = gl_uniform(utt_seed[u], (unsigned int)(f - utt_off[u]), (unsigned int)k);
    float sn, cs;
    sincospif(2.f * uv, &sn, &cs);
    P[g] = make_float2(cs, sn);
    if (u_out) u_out[g] = uv;
}

// ---- synthesis: S P -> inverse real FFT -> window ----------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void gl_synth_kernel(const float* __restrict__ S, const float2* __restrict__ P, const float* __restrict__ window,
                                                       const float2* __restrict__ tw, float* __restrict__ fr, int frames) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, PLANE = G::PLANE, BINS = G::BINS;
    __shared__ float re[2 * PLANE], im[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * G::FPW;
    // Z[k] = E[k] + i O[k], E = (X[k] + conj X[M - k]) / 2, O = (X[k] - conj X[M - k]) / 2 * conj(W_N^k); the imaginary parts of X[0] and X[M] are ignored
    for (int i = tid; i < G::FPW * M; i += 256) {
        const int slot = i / M, k = i % M;
        const long long f = f0 + slot;
        float2 z = make_float2(0.f, 0.f);
        if (f < frames) {
            const size_t row = (size_t)f * BINS;
            const float sk = S[row + k], sm = S[row + M - k];
            const float2 pk = P[row + k], pm = P[row + M - k];
            float2 xk = make_float2(sk * pk.x, sk * pk.y), xm = make_float2(sm * pm.x, sm * pm.y);
            if (k == 0) xk.y = xm.y = 0.f;
            const float2 e = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
            const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
            const float2 w = tw[k];
            const float2 o = gl_cmul(d, make_float2(w.x, -w.y));
            z = make_float2(e.x - o.y, e.y + o.x);
        }
        re[slot * SLOT + gl_pad(k)] = z.x;
        im[slot * SLOT + gl_pad(k)] = z.y;
    }
    __syncthreads();
    const int cur = gl_fft<N, true>(re, im, tw, tid);
    const float scale = 1.f / M;  // a power of two
    for (int i = tid; i < G::FPW * M; i += 256) {
        const int slot = i / M, n = i % M;
        const long long f = f0 + slot;
        if (f >= frames) continue;
        const float2 w = *reinterpret_cast<const float2*>(window + 2 * n);
        const float a = re[cur * PLANE + slot * SLOT + gl_pad(n)] * scale, b = im[cur * PLANE + slot * SLOT + gl_pad(n)] * scale;
        *reinterpret_cast<float2*>(fr + (size_t)f * N + 2 * n) = make_float2(a * w.x, b * w.y);
    }
}

// ---- overlap-add as a gather ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gl_ola_kernel(const float* __restrict__ fr, const float* __restrict__ window, const int* __restrict__ frame_utt,
                                                     const int* __restrict__ utt_off, int n_fft, int hop, long long total, float* __restrict__ y) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;  // sample g of a layout with hop samples per FRAME; the last hop of an utterance are unused
    if (g >= total) return;
    const int f = (int)(g / hop), u = frame_utt[f], lo = utt_off[u], T = utt_off[u + 1] - lo;
    const int j = (int)(g - (long long)lo * hop);
    if (j >= hop * (T - 1)) return;
    const int p = j + n_fft / 2;  // position in the utterance's untrimmed buffer
    const int t_lo = p >= n_fft ? (p - n_fft) / hop + 1 : 0, t_hi = min(p / hop, T - 1);
    float acc = 0.f, wss = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int n = p - t * hop;
        const float w = window[n];
        acc += fr[(size_t)(lo + t) * n_fft + n];
        wss = fmaf(w, w, wss);
    }
    if (wss > FLT_MIN) acc /= wss;
    y[(long long)(lo - u) * hop + j] = acc;
}

// ---- analysis: reflected gather -> window -> forward real FFT -> phase update ---------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void gl_analysis_kernel(const float* __restrict__ y, const float* __restrict__ window, const float2* __restrict__ tw,
                                                          const int* __restrict__ frame_utt, const int* __restrict__ utt_off, int hop, int frames, float alpha,
                                                          float2* __restrict__ P, float2* __restrict__ c_prev, float2* __restrict__ c_out) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, PLANE = G::PLANE, BINS = G::BINS;
    __shared__ float re[2 * PLANE], im[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * G::FPW;
    for (int i = tid; i < G::FPW * M; i += 256) {
        const int slot = i / M, n = i % M;
        const long long f = f0 + slot;
        float v[2] = {0.f, 0.f};
        if (f < frames) {
            const int u = frame_utt[f], lo = utt_off[u], T = utt_off[u + 1] - lo, t = (int)f - lo, L = hop * (T - 1);
            const float* yu = y + (long long)(lo - u) * hop;
            if (L > 0) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    int q = t * hop + 2 * n + e - N / 2;
                    q = q < 0 ? -q : q;
                    q = q >= L ? 2 * (L - 1) - q : q;
                    q = min(max(q, 0), L - 1);  // (no effect for T >= N / (2 hop) + 2, the supported range: keeps every other call inside y)
                    v[e] = yu[q] * window[2 * n + e];
                }
            }
        }
        re[slot * SLOT + gl_pad(n)] = v[0];
        im[slot * SLOT + gl_pad(n)] = v[1];
    }
    __syncthreads();
    const int cur = gl_fft<N, false>(re, im, tw, tid);
    const float *zr = re + cur * PLANE, *zi = im + cur * PLANE;
    // X[k] = (Z[k] + conj Z[M - k]) / 2 + W_N^k (Z[k] - conj Z[M - k]) / (2 i), k = 0 .. M, Z[M] = Z[0]
    for (int i = tid; i < G::FPW * BINS; i += 256) {
        const int slot = i / BINS, k = i - slot * BINS;
        const long long f = f0 + slot;
        if (f >= frames) continue;
        const int a = slot * SLOT + gl_pad(k & (M - 1)), b = slot * SLOT + gl_pad((M - k) & (M - 1));
        const float2 zk = make_float2(zr[a], zi[a]), zm = make_float2(zr[b], -zi[b]);
        const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
        const float2 d = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));  // (Z[k] - conj Z[M - k]) / (2 i)
        const float2 o = gl_cmul(tw[k], d);
        float2 c = make_float2(e.x + o.x, e.y + o.y);
        if (k == 0 || k == M) c.y = 0.f;
        const size_t at = (size_t)f * BINS + k;
        float2 av = c;
        if (c_prev) {
            const float2 cp = c_prev[at];
            av = make_float2(c.x - alpha * cp.x, c.y - alpha * cp.y);
            c_prev[at] = c;
        }
        if (c_out) c_out[at] = c;
        const float inv = 1.f / (sqrtf(av.x * av.x + av.y * av.y) + 1e-16f);
        P[at] = make_float2(av.x * inv, av.y * inv);
    }
}

// ---- entries ----------------------------------------------------------------------------------------------------------------------------------------
static int gl_check(const fcl_gl_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n_fft == 512 || a->n_fft == 1024 || a->n_fft == 2048, FCL_ERR_SHAPE, "%s: n_fft must be 512, 1024 or 2048 (got %d)", who, a->n_fft);
    FCL_REQUIRE(a->hop >= 1 && a->hop <= a->n_fft / 2, FCL_ERR_SHAPE, "%s: 1 <= hop <= n_fft / 2 expected (got hop %d, n_fft %d)", who, a->hop, a->n_fft);
    FCL_REQUIRE(a->frames >= 1 && a->n_utt >= 1 && a->n_utt <= a->frames, FCL_ERR_SHAPE, "%s: frames >= n_utt >= 1 expected (got %lld, %d)", who,
                (long long)a->frames, a->n_utt);
    FCL_REQUIRE(a->frames * (int64_t)std::max(a->n_fft, a->hop) < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: frames x n_fft must stay below 2^31 (got %lld frames)", who,
                (long long)a->frames);
    FCL_REQUIRE(a->frame_utt && a->utt_off, FCL_ERR_INVALID, "%s: null frame_utt / utt_off", who);
    return FCL_OK;
}

#define GL_DISPATCH(n_fft, CALL)   \
    do {                           \
        if ((n_fft) == 512) {      \
            CALL(512);             \
        } else if ((n_fft) == 1024) { \
            CALL(1024);            \
        } else {                   \
            CALL(2048);            \
        }                          \
    } while (0)

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_gl_mel2lin_fwd(const float* mel, const float* mel_stats, const float* pinv_t, float* s, int64_t frames, int n_mels, int bins, fcl_stream_t stream) {
    FCL_REQUIRE(mel && pinv_t && s, FCL_ERR_INVALID, "gl_mel2lin_fwd: null argument");
    FCL_REQUIRE(frames >= 1 && n_mels >= 1 && n_mels <= GL_MEL_MAX && bins >= 2 && frames * (int64_t)std::max(bins, n_mels) < 0x7fffffffLL, FCL_ERR_SHAPE,
                "gl_mel2lin_fwd: 1 <= n_mels <= %d, bins >= 2 and frames x bins below 2^31 expected (got %d, %d, %lld)", GL_MEL_MAX, n_mels, bins, (long long)frames);
    ProfScope ps("gl_mel2lin_kernel", 2.0 * frames * n_mels * bins, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(gl_mel2lin_kernel, dim3((unsigned)((frames + GL_MEL_ROWS - 1) / GL_MEL_ROWS)), dim3(256), 0, (hipStream_t)stream, mel, mel_stats, pinv_t, s,
                       (int)frames, n_mels, bins);
    return check_hip(hipGetLastError(), "gl_mel2lin_fwd");
}

int fcl_gl_phase_init(const fcl_gl_t* a, fcl_stream_t stream) {
    const int rc = gl_check(a, "gl_phase_init");
    if (rc) return rc;
    FCL_REQUIRE(a->utt_seed && a->p, FCL_ERR_INVALID, "gl_phase_init: null utt_seed / p");
    const long long total = a->frames * (long long)(a->n_fft / 2 + 1);
    ProfScope ps("gl_phase_init_kernel", 0.0, (double)a->frames, (hipStream_t)stream);
    hipLaunchKernelGGL(gl_phase_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->utt_seed, a->frame_utt, a->utt_off, total,
                       a->n_fft / 2 + 1, reinterpret_cast<float2*>(a->p), a->u_out);
    return check_hip(hipGetLastError(), "gl_phase_init");
}

int fcl_gl_synth_fwd(const fcl_gl_t* a, fcl_stream_t stream) {
    const int rc = gl_check(a, "gl_synth_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->s && a->p && a->window && a->twiddle && a->fr, FCL_ERR_INVALID, "gl_synth_fwd: null s / p / window / twiddle / fr");
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->p) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->twiddle) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(a->fr) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->window) & 7u) == 0,
                FCL_ERR_ALIGN, "gl_synth_fwd: p, twiddle, window and fr must be 8-byte aligned");
    const double flops = 2.5 * a->n_fft * std::log2((double)a->n_fft) * (double)a->frames;
#define GL_SYNTH(NN)                                                                                                                                       \
    {                                                                                                                                                      \
        ProfScope ps("gl_synth_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                          \
        hipLaunchKernelGGL(gl_synth_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, a->s, \
                           reinterpret_cast<const float2*>(a->p), a->window, reinterpret_cast<const float2*>(a->twiddle), a->fr, (int)a->frames);        \
    }
    GL_DISPATCH(a->n_fft, GL_SYNTH);
#undef GL_SYNTH
    return check_hip(hipGetLastError(), "gl_synth_fwd");
}

int fcl_gl_ola_fwd(const fcl_gl_t* a, fcl_stream_t stream) {
    const int rc = gl_check(a, "gl_ola_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->fr && a->window && a->y, FCL_ERR_INVALID, "gl_ola_fwd: null fr / window / y");
    const long long total = a->frames * (long long)a->hop;
    ProfScope ps("gl_ola_kernel", 0.0, (double)a->frames, (hipStream_t)stream);
    hipLaunchKernelGGL(gl_ola_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->fr, a->window, a->frame_utt, a->utt_off, a->n_fft,
                       a->hop, total, a->y);
    return check_hip(hipGetLastError(), "gl_ola_fwd");
}

int fcl_gl_analysis_fwd(const fcl_gl_t* a, fcl_stream_t stream) {
    const int rc = gl_check(a, "gl_analysis_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->y && a->window && a->twiddle && a->p, FCL_ERR_INVALID, "gl_analysis_fwd: null y / window / twiddle / p");
    FCL_REQUIRE(a->momentum >= 0.f && a->momentum <= 1.f, FCL_ERR_INVALID, "gl_analysis_fwd: momentum must lie in [0, 1] (got %g)", (double)a->momentum);
    FCL_REQUIRE(a->momentum == 0.f || a->c_prev, FCL_ERR_INVALID, "gl_analysis_fwd: momentum %g needs c_prev", (double)a->momentum);
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->p) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->twiddle) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(a->c_prev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->c_out) & 7u) == 0,
                FCL_ERR_ALIGN, "gl_analysis_fwd: p, twiddle, c_prev and c_out must be 8-byte aligned");
    const float alpha = a->momentum / (1.f + a->momentum);
    float2* cp = a->momentum == 0.f ? nullptr : reinterpret_cast<float2*>(a->c_prev);  // the classic form keeps no C_prev
    const double flops = 2.5 * a->n_fft * std::log2((double)a->n_fft) * (double)a->frames;
#define GL_ANA(NN)                                                                                                                                            \
    {                                                                                                                                                         \
        ProfScope ps("gl_analysis_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                          \
        hipLaunchKernelGGL(gl_analysis_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, a->y, \
                           a->window, reinterpret_cast<const float2*>(a->twiddle), a->frame_utt, a->utt_off, a->hop, (int)a->frames, alpha,                  \
                           reinterpret_cast<float2*>(a->p), cp, reinterpret_cast<float2*>(a->c_out));                                                        \
    }
    GL_DISPATCH(a->n_fft, GL_ANA);
#undef GL_ANA
    return check_hip(hipGetLastError(), "gl_analysis_fwd");
}

}  // extern "C"
