// pitch.hip — YIN F0 tracking on the mel features' frame grid (waveform -> frame-level F0 in Hz; include/fcl_hip.h "F0 tracking").  gfx950 only.
//   px_yin_kernel<N>     a workgroup of 256 threads holds 1024 / N frames (2 / 1 at N 512 / 1024): reflected gather of the utterance's samples (no
//                        window) into LDS, the difference function d(tau) = sum_{j < N / 2} (x[j] - x[j + tau])^2 for tau <= tau_max + 1 summed directly
//                        -- a thread owns 8 neighbouring lags and one segment of the j range, its 16-sample window slides through registers, the
//                        segments' partial sums are added in ascending segment order -- then the cumulative-mean normalisation (blocks of 8 lags in
//                        ascending tau, the block totals in ascending block order), the first dip below the threshold, the parabola and F0.  The
//                        direct sum is chosen over a correlation by FFT because its rounding error is relative to d(tau) itself, not to the frame's
//                        energy: d' keeps its relative accuracy inside the dips, where the pick compares neighbouring values.
//                        d' reaches HBM only when the caller passes cmnd_out.  No atomics and no order that depends on the batch.
//   px_short_run_kernel  one thread per frame: a voiced run shorter than min_voiced frames inside its utterance becomes 0 (out of place).
// Utterance u owns the samples smp_off[u] .. smp_off[u + 1] of x and the frames utt_off[u] .. utt_off[u + 1]; T = L / hop + 1 (as csrc/features.hip).
#include <algorithm>
#include <cmath>

#include "fcl_common.h"

namespace fcl {

// LDS geometry of px_yin_kernel<N>: FPW frame slots of TPF threads each.  A slot's samples x[0 .. N + 16) (zero behind N: the last lag group reads up to
// 7 lags past tau_max + 1) are stored with one pad word per 8, so that lanes whose lag groups are 8 samples apart read 9 words apart: no bank conflict
// among the 32 lanes of a ds_read_b32 group.  part [8][TPF] per slot: lag r of item i at r TPF + i, afterwards d' [8 groups] in the same words.
template <int N>
struct PxGeo {
    static constexpr int W = N / 2, FPW = 1024 / N, TPF = 256 / FPW, NCH = W / 8, XLEN = N + 16, XS = XLEN + XLEN / 8, GMAX = W / 8 + 1;
};

__device__ __forceinline__ int px_pad(int i) { return i + (i >> 3); }

template <int N>
__global__ __launch_bounds__(256) void px_yin_kernel(const float* __restrict__ x, const int* __restrict__ smp_off, const int* __restrict__ frame_utt,
                                                     const int* __restrict__ utt_off, int hop, int frames, int n_utt, int tau_min, int tau_max, float threshold,
                                                     float fs, float* __restrict__ f0, float* __restrict__ cmnd_out, int* __restrict__ tau_out) {
    using G = PxGeo<N>;
    constexpr int FPW = G::FPW, TPF = G::TPF, NCH = G::NCH, XLEN = G::XLEN, XS = G::XS, GMAX = G::GMAX;
    __shared__ float xs[FPW * XS], part[FPW * 8 * TPF], tot[FPW * GMAX];
    __shared__ int cand[FPW * GMAX];
    const int tid = threadIdx.x;
    const long long fbase = (long long)blockIdx.x * FPW;
    const int n_lag = tau_max + 2;                      // lags 0 .. tau_max + 1
    const int groups = min((n_lag + 7) / 8, GMAX);     // (the entry has checked tau_max <= W - 1: the min has no effect)
    const int n_seg = max(1, min(NCH, TPF / groups));  // groups n_seg <= TPF items per slot
    for (int i = tid; i < FPW * XLEN; i += 256) {
        const int slot = i / XLEN, n = i - slot * XLEN;
        const long long f = fbase + slot;
        float v = 0.f;
        if (f < frames && n < N) {
            const int u = min(max(frame_utt[f], 0), n_utt - 1), t = (int)f - utt_off[u], s0 = smp_off[u], L = smp_off[u + 1] - s0;
            if (L > 0) {
                int q = t * hop + n - N / 2;
                q = q < 0 ? -q : q;
                q = q >= L ? 2 * (L - 1) - q : q;
                q = min(max(q, 0), L - 1);  // (no effect for L >= N / 2 + 1, the supported range: keeps every other call inside x)
                v = x[(long long)s0 + q];
            }
        }
        xs[slot * XS + px_pad(n)] = v;
    }
    __syncthreads();
    const int slot = tid / TPF, it = tid - slot * TPF;
    const float* xf = xs + slot * XS;
    float* pf = part + slot * 8 * TPF;
    if (it < groups * n_seg) {  // item (g, s): the lags 8 g .. 8 g + 7 over the j chunks c0 .. c1 (8 samples each)
        const int s = it / groups, g = it - s * groups;
        const int c0 = s * NCH / n_seg, c1 = (s + 1) * NCH / n_seg;
        float acc[8], win[16];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) win[8 + i] = xf[9 * (c0 + g) + i];
        for (int c = c0; c < c1; ++c) {
            float xj[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                xj[i] = xf[9 * c + i];
                win[i] = win[8 + i];
                win[8 + i] = xf[9 * (c + g + 1) + i];  // c + g + 1 <= NCH + GMAX - 1: inside the zero-filled XLEN
            }
#pragma unroll
            for (int a = 0; a < 8; ++a) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float df = xj[a] - win[a + r];
                    acc[r] = fmaf(df, df, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) pf[r * TPF + it] = acc[r];
    }
    __syncthreads();
    float d[8], cum[8];
    if (it < groups) {  // thread g: d of its 8 lags (segments in ascending order) and their running sum in ascending tau
        float run = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float v = 0.f;
            for (int s = 0; s < n_seg; ++s) v += pf[r * TPF + s * groups + it];
            d[r] = v;
            run += v;  // (d(0) == 0 exactly: the sum starts at tau = 1 all the same)
            cum[r] = run;
        }
        tot[slot * GMAX + it] = run;
    }
    __syncthreads();
    if (it == 0) {  // the block totals in ascending order -> each block's offset
        float run = 0.f;
        for (int g = 0; g < groups; ++g) {
            const float v = tot[slot * GMAX + g];
            tot[slot * GMAX + g] = run;
            run += v;
        }
    }
    __syncthreads();
    const long long f = fbase + slot;
    if (it < groups) {
        const float off = tot[slot * GMAX + it];
        int first = 0x7fffffff;
#pragma unroll
        for (int r = 7; r >= 0; --r) {
            const int tau = 8 * it + r;
            const float sum = off + cum[r];
            const float v = (tau == 0 || sum == 0.f) ? 1.f : d[r] * (float)tau / sum;
            pf[tau] = v;  // every read of part is behind the barriers above
            if (tau >= tau_min && tau <= tau_max && v < threshold) first = tau;
            if (cmnd_out && f < frames && tau < n_lag) cmnd_out[(size_t)f * n_lag + tau] = v;
        }
        cand[slot * GMAX + it] = first;
    }
    __syncthreads();
    if (it == 0 && f < frames) {
        int tau = 0x7fffffff;
        for (int g = 0; g < groups; ++g) tau = min(tau, cand[slot * GMAX + g]);
        float hz = 0.f;
        if (tau != 0x7fffffff) {
            while (tau < tau_max && pf[tau + 1] < pf[tau]) ++tau;
            const float a = pf[tau - 1], b = pf[tau], c = pf[tau + 1];  // tau_min >= 2 and tau_max + 1 < 8 groups
            const float den = (a - 2.f * b) + c;
            float dl = den > 0.f ? 0.5f * (a - c) / den : 0.f;
            dl = fminf(fmaxf(dl, -0.5f), 0.5f);
            hz = fs / ((float)tau + dl);
        } else {
            tau = 0;
        }
        f0[f] = hz;
        if (tau_out) tau_out[f] = tau;
    }
}

__global__ __launch_bounds__(256) void px_short_run_kernel(const float* __restrict__ in, const int* __restrict__ frame_utt, const int* __restrict__ utt_off,
                                                           int frames, int n_utt, int min_voiced, float* __restrict__ out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    const float v = in[f];
    float keep = v;
    if (v != 0.f && min_voiced > 1) {
        const int u = min(max(frame_utt[f], 0), n_utt - 1);
        const long long lo = min(max(utt_off[u], 0), frames), hi = min(max(utt_off[u + 1], 0), frames);
        int run = 1;
        for (long long i = f - 1; i >= lo && run < min_voiced && in[i] != 0.f; --i) ++run;
        for (long long i = f + 1; i < hi && run < min_voiced && in[i] != 0.f; ++i) ++run;
        if (run < min_voiced) keep = 0.f;
    }
    out[f] = keep;
}

static int px_check(const fcl_px_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n == 512 || a->n == 1024, FCL_ERR_SHAPE, "%s: the frame length n must be 512 or 1024 (got %d)", who, a->n);
    FCL_REQUIRE(a->hop >= 1, FCL_ERR_SHAPE, "%s: hop >= 1 expected (got %d)", who, a->hop);
    FCL_REQUIRE(a->tau_min >= 2 && a->tau_min < a->tau_max && a->tau_max <= a->n / 2 - 1, FCL_ERR_SHAPE,
                "%s: 2 <= tau_min < tau_max <= n / 2 - 1 expected (got tau_min %d, tau_max %d, n %d)", who, a->tau_min, a->tau_max, a->n);
    FCL_REQUIRE(a->threshold > 0.f && a->threshold <= 1.f && a->fs > 0.f, FCL_ERR_SHAPE, "%s: 0 < threshold <= 1 and fs > 0 expected (got %g, %g)", who,
                (double)a->threshold, (double)a->fs);
    FCL_REQUIRE(a->frames >= 1 && a->n_utt >= 1 && a->n_utt <= a->frames, FCL_ERR_SHAPE, "%s: frames >= n_utt >= 1 expected (got %lld, %d)", who,
                (long long)a->frames, a->n_utt);
    FCL_REQUIRE(a->frames * (int64_t)(a->tau_max + 2) < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: frames x (tau_max + 2) must stay below 2^31 (got %lld frames)", who,
                (long long)a->frames);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->x && a->smp_off && a->frame_utt && a->utt_off, FCL_ERR_INVALID, "%s: null x / smp_off / frame_utt / utt_off", who);
    FCL_REQUIRE(a->f0, FCL_ERR_INVALID, "%s: null f0", who);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_px_yin_fwd(const fcl_px_t* a, fcl_stream_t stream) {
    const int rc = px_check(a, "px_yin_fwd");
    if (rc) return rc;
    const double flops = 3.0 * (a->n / 2) * (double)(a->tau_max + 2) * (double)a->frames;
#define PX_YIN(NN)                                                                                                                                         \
    {                                                                                                                                                      \
        ProfScope ps("px_yin_kernel<" #NN ">", flops, (double)a->frames, (hipStream_t)stream);                                                            \
        hipLaunchKernelGGL(px_yin_kernel<NN>, dim3((unsigned)((a->frames + PxGeo<NN>::FPW - 1) / PxGeo<NN>::FPW)), dim3(256), 0, (hipStream_t)stream, a->x, \
                           a->smp_off, a->frame_utt, a->utt_off, a->hop, (int)a->frames, a->n_utt, a->tau_min, a->tau_max, a->threshold, a->fs, a->f0,   \
                           a->cmnd_out, a->tau_out);                                                                                                      \
    }
    if (a->n == 512) {
        PX_YIN(512);
    } else {
        PX_YIN(1024);
    }
#undef PX_YIN
    return check_hip(hipGetLastError(), "px_yin_fwd");
}

int fcl_px_short_run_fwd(const float* f0_in, const int32_t* frame_utt, const int32_t* utt_off, float* f0_out, int64_t frames, int n_utt, int min_voiced,
                         fcl_stream_t stream) {
    FCL_REQUIRE(f0_in && frame_utt && utt_off && f0_out, FCL_ERR_INVALID, "px_short_run_fwd: null f0_in / frame_utt / utt_off / f0_out");
    FCL_REQUIRE(f0_in != f0_out, FCL_ERR_INVALID, "px_short_run_fwd: f0_out must not be f0_in (a thread reads its neighbours' input)");
    FCL_REQUIRE(n_utt >= 1 && frames >= n_utt && frames < 0x7fffffffLL, FCL_ERR_SHAPE,
                "px_short_run_fwd: frames >= n_utt >= 1 and frames below 2^31 expected (got frames %lld, n_utt %d)", (long long)frames, n_utt);
    FCL_REQUIRE(min_voiced >= 1, FCL_ERR_SHAPE, "px_short_run_fwd: min_voiced >= 1 expected (got %d)", min_voiced);
    ProfScope ps("px_short_run_kernel", 0.0, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(px_short_run_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f0_in, frame_utt, utt_off, (int)frames,
                       n_utt, min_voiced, f0_out);
    return check_hip(hipGetLastError(), "px_short_run_fwd");
}

}  // extern "C"
