// features.hip — log-mel and energy feature extraction (waveform -> the training inputs; include/fcl_hip.h "Feature extraction").  gfx950 only.
// The forward half of csrc/griffinlim.hip's analysis on the same LDS-resident real FFT (gl_fft.h), fused up to the log-mel rows:
//   fx_logmel_kernel<N>     a workgroup of 256 threads holds GlGeo<N>::FPW frames (4 / 2 / 1 at n_fft 512 / 1024 / 2048): reflected gather of the
//                           utterance's samples, times the window, forward FFT, split; |X[k]| goes to the LDS buffer the FFT no longer needs (and to
//                           mag_out when asked for), the frame's energy sqrt(sum_k S[k]^2) is a tree in LDS over a fixed partition of the bins, and one
//                           thread per (frame slot, mel channel) sums its triangle's contiguous run of bins in ascending k, then log10 with the floor
//                           1e-10 and the optional mean / std normalisation.  The magnitudes never reach HBM unless the caller passes mag_out.
//                           No atomics and no order that depends on the batch: a batch is bit for bit its per-utterance runs.
//   fx_segment_mean_kernel  one thread per phoneme: the mean of its frames' values in ascending frame order (optionally only of the frames whose mask
//                           is non-zero: the log-F0 rule); the frame range comes from the exclusive sum of the durations inside the utterance.
// Utterance u owns the samples smp_off[u] .. smp_off[u + 1] of x and the frames utt_off[u] .. utt_off[u + 1]; T = L / hop + 1.
#include <algorithm>
#include <cmath>

#include "fcl_common.h"
#include "gl_fft.h"

namespace fcl {

constexpr int FX_MEL_MAX = 256;

template <int N>
__global__ __launch_bounds__(256) void fx_logmel_kernel(const float* __restrict__ x, const int* __restrict__ smp_off, const int* __restrict__ frame_utt,
                                                        const int* __restrict__ utt_off, const float* __restrict__ window, const float2* __restrict__ tw,
                                                        const int* __restrict__ fb_lo, const int* __restrict__ fb_off, const float* __restrict__ fb_w,
                                                        const float* __restrict__ stats, int hop, int frames, int n_utt, int n_mels, int nnz,
                                                        float* __restrict__ mel, float* __restrict__ energy, float* __restrict__ mag_out) {
    using G = GlGeo<N>;
    constexpr int M = G::M, SLOT = G::SLOT, PLANE = G::PLANE, BINS = G::BINS, FPW = G::FPW, TPS = 256 / FPW;  // TPS threads per frame slot: M == 4 TPS
    __shared__ float re[2 * PLANE], im[2 * PLANE];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
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
                    q = q >= L ? 2 * (L - 1) - q : q;
                    q = min(max(q, 0), L - 1);  // (no effect for L >= N / 2 + 1, the supported range: keeps every other call inside x)
                    v[e] = x[(long long)s0 + q] * (e ? w.y : w.x);
                }
            }
        }
        re[slot * SLOT + gl_pad(n)] = v[0];
        im[slot * SLOT + gl_pad(n)] = v[1];
    }
    __syncthreads();
    const int cur = gl_fft<N, false>(re, im, tw, tid);
    const float *zr = re + cur * PLANE, *zi = im + cur * PLANE;
    float *S = re + (cur ^ 1) * PLANE, *part = im + (cur ^ 1) * PLANE;  // the buffer the FFT left behind: S [FPW][BINS] (FPW BINS <= PLANE), part [256]
    // X[k] = (Z[k] + conj Z[M - k]) / 2 + W_N^k (Z[k] - conj Z[M - k]) / (2 i), k = 0 .. M, Z[M] = Z[0]
    for (int i = tid; i < FPW * BINS; i += 256) {
        const int slot = i / BINS, k = i - slot * BINS;
        const long long f = f0 + slot;
        const int a = slot * SLOT + gl_pad(k & (M - 1)), b = slot * SLOT + gl_pad((M - k) & (M - 1));
        const float2 zk = make_float2(zr[a], zi[a]), zm = make_float2(zr[b], -zi[b]);
        const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
        const float2 d = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));  // (Z[k] - conj Z[M - k]) / (2 i)
        const float2 o = gl_cmul(tw[k], d);
        float2 c = make_float2(e.x + o.x, e.y + o.y);
        if (k == 0 || k == M) c.y = 0.f;
        const float s = sqrtf(fmaf(c.x, c.x, c.y * c.y));
        S[i] = s;
        if (mag_out && f < frames) mag_out[(size_t)f * BINS + k] = s;
    }
    __syncthreads();
    {  // energy: thread j of a slot sums the squares of bins j, j + TPS, j + 2 TPS, j + 3 TPS (thread 0: and bin M), then a tree over the slot's TPS threads
        const int slot = tid / TPS, j = tid % TPS;
        const float* sf = S + slot * BINS;
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = fmaf(sf[j + r * TPS], sf[j + r * TPS], acc);
        if (j == 0) acc = fmaf(sf[M], sf[M], acc);
        part[tid] = acc;
        __syncthreads();
#pragma unroll
        for (int h = TPS / 2; h >= 1; h >>= 1) {
            if (j < h) part[tid] += part[tid + h];
            __syncthreads();
        }
        if (j == 0 && f0 + slot < frames) energy[f0 + slot] = sqrtf(part[tid]);
    }
    // mel: one thread per (frame slot, channel); the channel's triangle is the run fb_w[fb_off[c] .. fb_off[c + 1]) over the bins from fb_lo[c]
    for (int i = tid; i < FPW * n_mels; i += 256) {
        const int slot = i / n_mels, c = i - slot * n_mels;
        const long long f = f0 + slot;
        if (f >= frames) continue;
        const int o0 = min(max(fb_off[c], 0), nnz), o1 = min(max(fb_off[c + 1], o0), nnz), lo = min(max(fb_lo[c], 0), BINS);
        const int len = min(o1 - o0, BINS - lo);  // (no effect on the package's tables: keeps any other table inside S and fb_w)
        const float* sf = S + slot * BINS + lo;
        float acc = 0.f;
        for (int j = 0; j < len; ++j) acc = fmaf(sf[j], fb_w[o0 + j], acc);
        float v = log10f(fmaxf(1e-10f, acc));
        if (stats) v = (v - stats[c]) / (stats[n_mels + c] + 1e-8f);
        mel[(size_t)f * n_mels + c] = v;
    }
}

__global__ __launch_bounds__(256) void fx_segment_mean_kernel(const float* __restrict__ v, const float* __restrict__ mask, const int* __restrict__ dur,
                                                              const int* __restrict__ ph_utt, const int* __restrict__ ph_off, const int* __restrict__ utt_off,
                                                              int n_ph, int n_utt, int nonzero_only, float* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_ph) return;
    const int u = min(max(ph_utt[p], 0), n_utt - 1), lo = utt_off[u], hi = utt_off[u + 1];
    long long a = lo;
    for (int j = ph_off[u]; j < p; ++j) a += max(dur[j], 0);  // exclusive sum of the durations inside the utterance
    const long long b = min(a + max(dur[p], 0), (long long)hi);  // (a package-made batch has sum(dur) == T: the clamp keeps any other inside v)
    float acc = 0.f;
    int cnt = 0;
    for (long long i = min(a, (long long)hi); i < b; ++i) {
        if (nonzero_only && mask[i] == 0.f) continue;
        acc += v[i];
        ++cnt;
    }
    out[p] = cnt ? acc / (float)cnt : 0.f;
}

static int fx_check(const fcl_fx_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n_fft == 512 || a->n_fft == 1024 || a->n_fft == 2048, FCL_ERR_SHAPE, "%s: n_fft must be 512, 1024 or 2048 (got %d)", who, a->n_fft);
    FCL_REQUIRE(a->hop >= 1 && a->hop <= a->n_fft / 2, FCL_ERR_SHAPE, "%s: 1 <= hop <= n_fft / 2 expected (got hop %d, n_fft %d)", who, a->hop, a->n_fft);
    FCL_REQUIRE(a->n_mels >= 1 && a->n_mels <= FX_MEL_MAX, FCL_ERR_SHAPE, "%s: 1 <= n_mels <= %d expected (got %d)", who, FX_MEL_MAX, a->n_mels);
    FCL_REQUIRE(a->nnz >= 1, FCL_ERR_SHAPE, "%s: nnz (the length of fb_w) must be positive (got %d)", who, a->nnz);
    FCL_REQUIRE(a->frames >= 1 && a->n_utt >= 1 && a->n_utt <= a->frames, FCL_ERR_SHAPE, "%s: frames >= n_utt >= 1 expected (got %lld, %d)", who,
                (long long)a->frames, a->n_utt);
    FCL_REQUIRE(a->frames * (int64_t)std::max(a->n_fft / 2 + 1, a->n_mels) < 0x7fffffffLL, FCL_ERR_SHAPE,
                "%s: frames x max(n_fft / 2 + 1, n_mels) must stay below 2^31 (got %lld frames)", who, (long long)a->frames);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->x && a->smp_off && a->frame_utt && a->utt_off, FCL_ERR_INVALID, "%s: null x / smp_off / frame_utt / utt_off", who);
    FCL_REQUIRE(a->window && a->twiddle && a->fb_lo && a->fb_off && a->fb_w, FCL_ERR_INVALID, "%s: null window / twiddle / fb_lo / fb_off / fb_w", who);
    FCL_REQUIRE(a->mel && a->energy, FCL_ERR_INVALID, "%s: null mel / energy", who);
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(a->window) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->twiddle) & 7u) == 0, FCL_ERR_ALIGN,
                "%s: window and twiddle must be 8-byte aligned", who);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_fx_logmel_fwd(const fcl_fx_t* a, fcl_stream_t stream) {
    const int rc = fx_check(a, "fx_logmel_fwd");
    if (rc) return rc;
    const double flops = (2.5 * a->n_fft * std::log2((double)a->n_fft) + 2.0 * a->nnz) * (double)a->frames;
#define FX_LOGMEL(NN)                                                                                                                                        \
    {                                                                                                                                                        \
        ProfScope ps("fx_logmel_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                           \
        hipLaunchKernelGGL(fx_logmel_kernel<NN>, dim3((unsigned)((a->frames + GlGeo<NN>::FPW - 1) / GlGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, a->x, \
                           a->smp_off, a->frame_utt, a->utt_off, a->window, reinterpret_cast<const float2*>(a->twiddle), a->fb_lo, a->fb_off, a->fb_w,     \
                           a->mel_stats, a->hop, (int)a->frames, a->n_utt, a->n_mels, a->nnz, a->mel, a->energy, a->mag_out);                               \
    }
    if (a->n_fft == 512) {
        FX_LOGMEL(512);
    } else if (a->n_fft == 1024) {
        FX_LOGMEL(1024);
    } else {
        FX_LOGMEL(2048);
    }
#undef FX_LOGMEL
    return check_hip(hipGetLastError(), "fx_logmel_fwd");
}

int fcl_fx_segment_mean_fwd(const float* v, const float* mask, const int32_t* dur, const int32_t* ph_utt, const int32_t* ph_off, const int32_t* utt_off,
                            float* out, int64_t n_ph, int n_utt, int64_t frames, int nonzero_only, fcl_stream_t stream) {
    FCL_REQUIRE(v && dur && ph_utt && ph_off && utt_off && out, FCL_ERR_INVALID, "fx_segment_mean_fwd: null v / dur / ph_utt / ph_off / utt_off / out");
    FCL_REQUIRE(!nonzero_only || mask, FCL_ERR_INVALID, "fx_segment_mean_fwd: nonzero_only needs mask");
    FCL_REQUIRE(n_utt >= 1 && n_ph >= n_utt && frames >= n_utt && n_ph < 0x7fffffffLL && frames < 0x7fffffffLL, FCL_ERR_SHAPE,
                "fx_segment_mean_fwd: n_ph >= n_utt >= 1, frames >= n_utt and both below 2^31 expected (got n_ph %lld, n_utt %d, frames %lld)", (long long)n_ph,
                n_utt, (long long)frames);
    ProfScope ps("fx_segment_mean_kernel", 0.0, (double)n_ph, (hipStream_t)stream);
    hipLaunchKernelGGL(fx_segment_mean_kernel, dim3((unsigned)((n_ph + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, mask, dur, ph_utt, ph_off, utt_off,
                       (int)n_ph, n_utt, nonzero_only, out);
    return check_hip(hipGetLastError(), "fx_segment_mean_fwd");
}

}  // extern "C"
