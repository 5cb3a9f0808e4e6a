// pwg.hip — Parallel WaveGAN generator (BASELINE configs[4]: the stage the reference shells out to,
// inference_student.sh:20-23).  gfx950 only.  Rows are SAMPLES (time-major, utterances concatenated, zero padding at utterance edges through
// the GEMM's segment bounds); channels are the contiguous dimension, so every convolution of the residual stack is a K-term of the pre-split
// operand GEMM (gemm_planes.hip):
//     z[M, 128]  = x[t-d] W_0^T + x[t] W_1^T + x[t+d] W_2^T + c_up[t] W_aux^T + b          (4 terms: K = 3 x 64 + 80)
//     g[M, 64]   = tanh(z[:, :64]) * sigmoid(z[:, 64:])                                     (pwg_gate_kernel, writes planes)
//     o[M, 128]  = g [W_out ; W_skip]^T + [b_out ; b_skip]                                  (1 term: K = 64)
//     x          = (o[:, :64] + x) * sqrt(0.5) ;  skips += o[:, 64:]                        (pwg_resid_kernel, writes fp32 + planes)
// The upsampling network (nearest-neighbour stretch + 1 x (2s+1) smoothing, four times) and the 1 -> 64 / 64 -> 1 end convolutions are
// HBM-bound row kernels.  Published architecture: kan-bayashi/ParallelWaveGAN, ParallelWaveGANGenerator (v1, LJSpeech); see oracle/pwg_oracle.py.
#include <algorithm>

#include "fcl_common.h"

namespace fcl {


// ---- one stage of UpsampleNetwork: Stretch2d(scale, nearest) + Conv2d(1, 1, (1, 2*scale+1), padding (0, scale), no bias), per channel.
// in: [frames * rate_in rows, C]; out: [frames * rate_in * scale rows, C] (fp32 and / or planes with ldp lines per row, zero past C).
// A row's utterance comes from its frame: frame_utt[frame], bounds utt_off[u] .. utt_off[u+1] (in frames): the zero padding of the smoothing
// convolution applies at UTTERANCE edges, as when each utterance is upsampled on its own.
__global__ __launch_bounds__(256) void pwg_upsample_stage_kernel(const float* __restrict__ in, const int* __restrict__ frame_utt,
                                                                 const int* __restrict__ utt_off, long long rows_out, int rate_in, int scale,
                                                                 const float* __restrict__ w, float* __restrict__ out, u16* __restrict__ out_p, int ldp,
                                                                 int C, int chunk_major) {
    // item = (output row, 4 channels).  The 2*scale+1 taps of a row fall on at most three rows of the stage input (nearest-neighbour stretch), so
    // they collapse to three coefficients per row (sums of the taps that land on each input row and lie inside the utterance: the zero padding
    // of the smoothing convolution); then 3 float4 loads and 12 FMAs per item.  C % 4 == 0.
    const int cq = out_p ? ldp * 8 : C >> 2;  // channel quads per row (planes: the zero padding up to the last 32-column line is written too)
    const long long total = rows_out * cq;
    const int rate_out = rate_in * scale;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cq;
        const int c = (int)(i - r * cq) * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            const int u = frame_utt[r / rate_out];
            const long long lo = (long long)utt_off[u] * rate_out, hi = (long long)utt_off[u + 1] * rate_out;
            const long long i0 = r / scale;  // input row of the centre tap
            float k[3] = {0.f, 0.f, 0.f};    // coefficients of input rows i0 - 1, i0, i0 + 1
            for (int j = -scale; j <= scale; ++j) {
                const long long q = r + j;
                if (q < lo || q >= hi) continue;
                k[(int)(q / scale - i0) + 1] += w[j + scale];
            }
            const long long rows_in = rows_out / scale;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const long long ri = i0 + d - 1;
                if (k[d] != 0.f && ri >= 0 && ri < rows_in) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(in + ri * C + c);
                    acc += k[d] * v;
                }
            }
            if (out) *reinterpret_cast<f32x4*>(out + r * C + c) = acc;
        }
        if (out_p) {
            uint2 h, l;
            split4(acc, h, l);
            u16* line = chunk_major ? out_p + ((size_t)(c >> 5) * rows_out + r) * 64 + (c & 31) : out_p + ((size_t)r * ldp + (c >> 5)) * 64 + (c & 31);
            *reinterpret_cast<uint2*>(line) = h;
            *reinterpret_cast<uint2*>(line + 32) = l;
        }
    }
}

// first_conv: x[m, ch] = w[ch] * z[m] + b[ch]  (Conv1d1x1(1 -> R))
__global__ __launch_bounds__(256) void pwg_first_conv_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ b,
                                                             float* __restrict__ x, u16* __restrict__ xp, long long M, int R, int chunk_major) {
    const int rq = R >> 2;  // item = (sample, 4 channels): one 8-byte store per plane
    const long long total = M * rq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / rq;
        const int ch = (int)(i - m * rq) * 4;
        const float zm = z[m];
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + ch) * zm + *reinterpret_cast<const f32x4*>(b + ch);
        if (x) *reinterpret_cast<f32x4*>(x + m * R + ch) = v;
        uint2 h, l;
        split4(v, h, l);
        u16* line = chunk_major ? xp + ((size_t)(ch >> 5) * M + m) * 64 + (ch & 31) : xp + ((size_t)m * (R >> 5) + (ch >> 5)) * 64 + (ch & 31);
        *reinterpret_cast<uint2*>(line) = h;
        *reinterpret_cast<uint2*>(line + 32) = l;
    }
}

// g = tanh(z[:, :H]) * sigmoid(z[:, H:])  -> planes [M, H]
__global__ __launch_bounds__(256) void pwg_gate_kernel(const float* __restrict__ z, u16* __restrict__ gp, long long M, int H) {
    const long long total = M * H;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / H;
        const int ch = (int)(i - m * H);
        const float a = z[m * 2 * H + ch], b = z[m * 2 * H + H + ch];
        const float v = tanhf(a) * (1.0f / (1.0f + __expf(-b)));
        store_p32(gp + (size_t)m * (H >> 5) * 64, H >> 5, 0, ch, v);
    }
}

// x = (o[:, :R] + x) * sqrt(0.5) (fp32 + planes) ; skips += o[:, R:]
__global__ __launch_bounds__(256) void pwg_resid_kernel(const float* __restrict__ o, float* __restrict__ x, u16* __restrict__ xp, float* __restrict__ skips,
                                                        long long M, int R, int first) {
    const long long total = M * R;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / R;
        const int ch = (int)(i - m * R);
        const float v = (o[m * 2 * R + ch] + x[i]) * 0.70710678118654752440f;
        x[i] = v;
        store_p32(xp + (size_t)m * (R >> 5) * 64, R >> 5, 0, ch, v);
        const float s = o[m * 2 * R + R + ch];
        skips[i] = first ? s : skips[i] + s;
    }
}

// y = relu(skips * scale) -> planes [M, S]
__global__ __launch_bounds__(256) void pwg_relu_scale_kernel(const float* __restrict__ skips, float scale, u16* __restrict__ yp, long long M, int S) {
    const long long total = M * S;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / S;
        const int ch = (int)(i - m * S);
        store_p32(yp + (size_t)m * (S >> 5) * 64, S >> 5, 0, ch, fmaxf(skips[i] * scale, 0.f));
    }
}

// wav[m] = sum_ch relu(h[m, ch]) * w[ch] + b   (last ReLU + Conv1d1x1(S -> 1)); one wave per 4 rows of S = 64 channels
__global__ __launch_bounds__(256) void pwg_out_kernel(const float* __restrict__ h, const float* __restrict__ w, float b, float* __restrict__ wav, long long M,
                                                      int S) {
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long m = wave; m < M; m += nwaves) {
        float acc = 0.f;
        for (int ch = lane; ch < S; ch += 64) acc += fmaxf(h[m * S + ch], 0.f) * w[ch];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) wav[m] = acc + b;
    }
}

// coefficient lines of the frame-rate auxiliary term (include/fcl_hip.h: fcl_pwg_aux_coeff): one 128-byte line per sample
__global__ __launch_bounds__(256) void pwg_aux_coeff_kernel(const float* __restrict__ kc, long long M, int hop, long long frames, u16* __restrict__ kp) {
    for (long long m = blockIdx.x * (long long)blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const long long f = m / hop;
        const int r = (int)(f & 31);
        const long long w0 = (r >= 2 && r <= 29) ? (f >> 5) * 32 : ((f + 16) >> 5) * 32 - 16;
        const f32x4 k03 = *reinterpret_cast<const f32x4*>(kc + m * 8);
        const float k4 = kc[m * 8 + 4];
        const float kv[5] = {k03[0], k03[1], k03[2], k03[3], k4};
        unsigned hw[16], lw[16];  // 32 columns, two bf16 per word
#pragma unroll
        for (int i = 0; i < 16; ++i) hw[i] = lw[i] = 0u;
        const int p0 = (int)(f - 2 - w0);  // column of frame f - 2 (0 .. 27)
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const long long g = f - 2 + d;
            if (g < 0 || g >= frames) continue;
            float v = 0.f;
            const int c = (int)(g % 5);
#pragma unroll
            for (int e = 0; e < 5; ++e) v = c == e ? kv[e] : v;
            const __bf16 h = (__bf16)v;
            const unsigned hb = __builtin_bit_cast(unsigned short, h), lb = __builtin_bit_cast(unsigned short, (__bf16)(v - (float)h));
            const int col = p0 + d;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i == (col >> 1)) {
                    hw[i] |= hb << ((col & 1) * 16);
                    lw[i] |= lb << ((col & 1) * 16);
                }
        }
        uint4* line = reinterpret_cast<uint4*>(kp + (size_t)m * 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            line[i] = make_uint4(hw[4 * i], hw[4 * i + 1], hw[4 * i + 2], hw[4 * i + 3]);
            line[4 + i] = make_uint4(lw[4 * i], lw[4 * i + 1], lw[4 * i + 2], lw[4 * i + 3]);
        }
    }
}

// z ~ N(0, 1): Box-Muller on two hashed 24-bit uniforms per element (counter-based: element i of a given seed is reproducible on any grid)
__device__ __forceinline__ float pwg_noise_at(long long i, unsigned int seed) {
    const unsigned int lo = (unsigned int)i, hi = (unsigned int)(i >> 32);
    const unsigned int h1 = hash_u32(lo ^ hash_u32(seed ^ (hi * 0x9E3779B9u))), h2 = hash_u32(h1 ^ 0x85EBCA6Bu ^ lo);
    const float u1 = ((h1 >> 8) + 1) * (1.0f / 16777216.0f), u2 = (h2 >> 8) * (1.0f / 16777216.0f);  // u1 in (0, 1]
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530717958647692f * u2);
}

__global__ __launch_bounds__(256) void pwg_noise_kernel(float* __restrict__ z, long long n, unsigned int seed) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) z[i] = pwg_noise_at(i, seed);
}

// ---- capacity forms (fcl_hip.h "capacity form of the vocoder"): every buffer and grid is sized by a CAPACITY; what is live comes from the device.
// live record int32 [4] = {frames, samples, padded frame rows, utterances with frames}, written by pwg_maps_kernel.
constexpr int PWG_MAPS_MAX_UTT = 1024;

// largest u in [0, n) with a[u] <= v (a non-decreasing, a[0] <= v): with equal neighbours (utterances without frames) the LAST one, i.e. the
// utterance that owns v
__device__ __forceinline__ int pwg_owner(const int* a, int n, int v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The vocoder's index maps from the synthesis pass's frame starts, to capacity, in one launch.  Every workgroup rebuilds the two small prefix tables
// (frame starts, padded-row starts: B + 1 words each) in LDS and then fills its share of the maps.  Frames [live, frames_cap) form one pseudo-utterance
// (index B) whose padded rows are [live_pad, pad_cap) and whose samples are [live * hop, frames_cap * hop): dead rows only ever see dead rows.
__global__ __launch_bounds__(256) void pwg_maps_kernel(const int* __restrict__ utt_frame0, unsigned int* status, int B, int frames_cap, int ctx, int hop,
                                                       int* __restrict__ pad_idx, int* __restrict__ lo, int* __restrict__ hi, int* __restrict__ keep,
                                                       int* __restrict__ frame_utt, int* __restrict__ utt_off, int* __restrict__ seg_lo,
                                                       int* __restrict__ seg_hi, int* __restrict__ live) {
    __shared__ int off[PWG_MAPS_MAX_UTT + 1], pb[PWG_MAPS_MAX_UTT + 1];
    __shared__ int s_ok;
    const int tid = threadIdx.x;
    for (int i = tid; i <= B; i += blockDim.x) off[i] = utt_frame0[i];
    __syncthreads();
    if (tid == 0) {
        // *status is read here by every workgroup while workgroup 0 may OR FCL_STATUS_VOCODER_CAP into it at the end of the kernel; nothing orders
        // the two, and nothing has to.  Workgroup 0 writes only when ITS `ok` is false, and `ok` is a function of the word as it was at launch and of
        // utt_frame0 (read-only here): a reader that sees the old word evaluates exactly what workgroup 0 evaluated -> false; a reader that sees the
        // new word sees a non-zero word -> false as well.  When `ok` is true nobody writes.  So all workgroups agree on `ok`, whatever they observe.
        bool ok = *status == 0u && off[0] == 0 && off[B] <= frames_cap;
        for (int u = 0; u < B; ++u) ok = ok && off[u + 1] >= off[u];
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    if (!ok)
        for (int i = tid; i <= B; i += blockDim.x) off[i] = 0;  // nothing is live: the whole capacity is the dead pseudo-utterance
    __syncthreads();
    if (tid == 0) {
        int p = 0;
        for (int u = 0; u < B; ++u) {
            pb[u] = p;
            if (off[u + 1] > off[u]) p += off[u + 1] - off[u] + 2 * ctx;
        }
        pb[B] = p;
    }
    __syncthreads();
    const int nlive = off[B], live_pad = pb[B];
    const int pad_cap = frames_cap + 2 * ctx * (B + 1);
    const long long m_live = (long long)nlive * hop, m_cap = (long long)frames_cap * hop;
    const long long g0 = blockIdx.x * (long long)blockDim.x + tid, gs = (long long)gridDim.x * blockDim.x;
    for (long long f = g0; f < frames_cap; f += gs) {
        int u = B, k = live_pad + ctx + ((int)f - nlive);
        if (f < nlive) {
            u = pwg_owner(off, B, (int)f);
            k = pb[u] + ctx + ((int)f - off[u]);
        }
        frame_utt[f] = u;
        keep[f] = k;
    }
    for (long long j = g0; j < pad_cap; j += gs) {
        int src = 0, l = live_pad, h = pad_cap;
        if (j < live_pad) {
            const int u = pwg_owner(pb, B, (int)j), n = off[u + 1] - off[u];
            src = off[u] + min(max((int)j - pb[u] - ctx, 0), n - 1);
            l = pb[u];
            h = pb[u] + n + 2 * ctx;
        }
        pad_idx[j] = src;
        lo[j] = l;
        hi[j] = h;
    }
    for (long long q = g0; q * 4 < m_cap; q += gs) {  // four samples of one frame (hop % 4 == 0) per item
        const long long m = q * 4;
        int l = (int)m_live, h = (int)m_cap;
        if (m < m_live) {
            const int u = pwg_owner(off, B, (int)(m / hop));
            l = off[u] * hop;
            h = off[u + 1] * hop;
        }
        *reinterpret_cast<int4*>(seg_lo + m) = make_int4(l, l, l, l);
        *reinterpret_cast<int4*>(seg_hi + m) = make_int4(h, h, h, h);
    }
    if (blockIdx.x == 0) {
        for (int i = tid; i <= B; i += blockDim.x) utt_off[i] = off[i];
        if (tid == 0) {
            utt_off[B + 1] = frames_cap;
            int nz = 0;
            for (int u = 0; u < B; ++u) nz += off[u + 1] > off[u];
            live[0] = nlive;
            live[1] = (int)m_live;
            live[2] = live_pad;
            live[3] = nz;
            if (!ok) atomicOr(status, (unsigned int)FCL_STATUS_VOCODER_CAP);
        }
    }
}

// replicate-padded feature rows of the live utterances; zeros for the dead rows (whatever the synthesis buffer holds past its total never enters)
__global__ __launch_bounds__(256) void pwg_gather_pad_kernel(const float* __restrict__ mel, int mel_rows, const int* __restrict__ pad_idx,
                                                             const int* __restrict__ live, int pad_cap, int C, float* __restrict__ out) {
    const int cq = C >> 2, live_pad = uniform_word(live, 2);
    const long long total = (long long)pad_cap * cq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i / cq), c = (int)(i - (long long)j * cq) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j < live_pad) {
            const int src = pad_idx[j];
            if ((unsigned)src < (unsigned)mel_rows) v = *reinterpret_cast<const f32x4*>(mel + (size_t)src * C + c);
        }
        *reinterpret_cast<f32x4*>(out + (size_t)j * C + c) = v;
    }
}

__global__ __launch_bounds__(256) void pwg_noise_cap_kernel(float* __restrict__ z, long long n_cap, unsigned int seed, const unsigned int* __restrict__ seed_dev,
                                                            const int* __restrict__ live) {
    const long long n = min((long long)uniform_word(live, 1), n_cap);
    if (seed_dev) seed += *seed_dev;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) z[i] = pwg_noise_at(i, seed);
}

// first_conv into chunk-major planes whose chunk stride is the capacity's
__global__ __launch_bounds__(256) void pwg_first_conv_cap_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ b,
                                                                 u16* __restrict__ xp, long long m_cap, int R, const int* __restrict__ live) {
    const int rq = R >> 2;
    const long long total = min((long long)uniform_word(live, 1), m_cap) * rq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / rq;
        const int ch = (int)(i - m * rq) * 4;
        const float zm = z[m];
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + ch) * zm + *reinterpret_cast<const f32x4*>(b + ch);
        uint2 h, l;
        split4(v, h, l);
        u16* line = xp + ((size_t)(ch >> 5) * m_cap + m) * 64 + (ch & 31);
        *reinterpret_cast<uint2*>(line) = h;
        *reinterpret_cast<uint2*>(line + 32) = l;
    }
}

// float waveform -> int16: clip(rint(double(x) * 32767), -32768, 32767), ties to even (a float times 32767 is exact in double, so this is the numpy
// rule of vocoder_decode.write_wav bit for bit); a non-finite sample becomes 0 and raises FCL_STATUS_PCM_NONFINITE.  Four samples per item.
__global__ __launch_bounds__(256) void pwg_pcm16_kernel(const float* __restrict__ wav, short* __restrict__ pcm, long long n_cap, const int* __restrict__ live,
                                                        unsigned int* status) {
    const long long n = live ? min((long long)uniform_word(live, 1), n_cap) : n_cap;
    bool bad = false;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q * 4 < n; q += (long long)gridDim.x * blockDim.x) {
        const long long i = q * 4;
        short o[4] = {0, 0, 0, 0};
        if (i + 4 <= n) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(wav + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = v[e];
                if (!(fabsf(x) <= 3.4028234663852886e38f)) { bad = true; continue; }
                o[e] = (short)fmin(fmax(rint((double)x * 32767.0), -32768.0), 32767.0);
            }
            uint2 w;
            w.x = (unsigned)(unsigned short)o[0] | ((unsigned)(unsigned short)o[1] << 16);
            w.y = (unsigned)(unsigned short)o[2] | ((unsigned)(unsigned short)o[3] << 16);
            *reinterpret_cast<uint2*>(pcm + i) = w;
        } else {
            for (long long k = i; k < n; ++k) {
                const float x = wav[k];
                short r = 0;
                if (!(fabsf(x) <= 3.4028234663852886e38f)) bad = true;
                else r = (short)fmin(fmax(rint((double)x * 32767.0), -32768.0), 32767.0);
                pcm[k] = r;
            }
        }
    }
    if (bad) atomicOr(status, (unsigned int)FCL_STATUS_PCM_NONFINITE);
}

static unsigned grid_1d(long long n, int per_block) {
    long long b = (n + per_block - 1) / per_block;
    return (unsigned)std::min<long long>(std::max<long long>(b, 1), 1 << 20);
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_pwg_upsample_stage(const float* in, const int32_t* frame_utt, const int32_t* utt_off, int64_t frames, int rate_in, int scale, const float* w,
                           float* out, uint16_t* out_p, int c, int chunk_major, fcl_stream_t stream) {
    FCL_REQUIRE(in && frame_utt && utt_off && w && (out || out_p) && frames > 0 && rate_in >= 1 && scale >= 1 && c > 0 && (c & 3) == 0, FCL_ERR_INVALID,
                "pwg_upsample_stage: bad arguments (channels must be a multiple of 4)");
    FCL_REQUIRE((reinterpret_cast<uintptr_t>(out_p) & 127u) == 0, FCL_ERR_ALIGN, "pwg_upsample_stage: planes must be 128-byte aligned");
    FCL_REQUIRE(aligned16(in) && aligned16(out), FCL_ERR_ALIGN, "pwg_upsample_stage: in / out must be 16-byte aligned");
    const long long rows_out = (long long)frames * rate_in * scale;
    const int ldp = (c + 31) / 32;
    hipLaunchKernelGGL(pwg_upsample_stage_kernel, dim3(grid_1d(rows_out * (out_p ? ldp * 8 : c / 4), 256)), dim3(256), 0, (hipStream_t)stream, in, frame_utt, utt_off,
                       rows_out, rate_in, scale, w, out, out_p, ldp, c, chunk_major);
    return check_hip(hipGetLastError(), "pwg_upsample_stage");
}

int fcl_pwg_aux_coeff(const float* kc, int64_t m, int hop, int64_t frames, uint16_t* kp, fcl_stream_t stream) {
    FCL_REQUIRE(kc && kp && m > 0 && hop > 0 && frames > 0 && m <= frames * (int64_t)hop, FCL_ERR_INVALID, "pwg_aux_coeff: bad arguments");
    FCL_REQUIRE(aligned16(kc) && (reinterpret_cast<uintptr_t>(kp) & 127u) == 0, FCL_ERR_ALIGN, "pwg_aux_coeff: kc must be 16-byte, kp 128-byte aligned");
    hipLaunchKernelGGL(pwg_aux_coeff_kernel, dim3(grid_1d(m, 256)), dim3(256), 0, (hipStream_t)stream, kc, (long long)m, hop, (long long)frames, kp);
    return check_hip(hipGetLastError(), "pwg_aux_coeff");
}

int fcl_pwg_noise(float* z, int64_t n, uint32_t seed, fcl_stream_t stream) {
    FCL_REQUIRE(z && n > 0, FCL_ERR_INVALID, "pwg_noise: bad arguments");
    hipLaunchKernelGGL(pwg_noise_kernel, dim3(grid_1d(n, 1024)), dim3(256), 0, (hipStream_t)stream, z, (long long)n, seed);
    return check_hip(hipGetLastError(), "pwg_noise");
}

int fcl_pwg_first_conv(const float* z, const float* w, const float* b, float* x, uint16_t* xp, int64_t m, int r, int chunk_major, fcl_stream_t stream) {
    FCL_REQUIRE(z && w && b && xp && m > 0 && r > 0 && (r & 31) == 0, FCL_ERR_INVALID, "pwg_first_conv: bad arguments (R must be a multiple of 32)");
    FCL_REQUIRE(aligned16(w) && aligned16(b) && aligned16(x) && (reinterpret_cast<uintptr_t>(xp) & 127u) == 0, FCL_ERR_ALIGN,
                "pwg_first_conv: w / b / x must be 16-byte aligned, the planes 128-byte aligned");
    hipLaunchKernelGGL(pwg_first_conv_kernel, dim3(grid_1d(m * (r / 4), 256)), dim3(256), 0, (hipStream_t)stream, z, w, b, x, xp, (long long)m, r, chunk_major);
    return check_hip(hipGetLastError(), "pwg_first_conv");
}

int fcl_pwg_maps_build(const int32_t* utt_frame0, uint32_t* status, int batch, int64_t frames_cap, int ctx, int hop, int32_t* pad_idx, int32_t* lo, int32_t* hi,
                       int32_t* keep, int32_t* frame_utt, int32_t* utt_off, int32_t* seg_lo, int32_t* seg_hi, int32_t* live, fcl_stream_t stream) {
    FCL_REQUIRE(utt_frame0 && status && pad_idx && lo && hi && keep && frame_utt && utt_off && seg_lo && seg_hi && live, FCL_ERR_INVALID,
                "pwg_maps_build: null argument");
    FCL_REQUIRE(batch >= 1 && batch <= PWG_MAPS_MAX_UTT && frames_cap >= 1 && ctx >= 0 && ctx <= 64, FCL_ERR_INVALID,
                "pwg_maps_build: 1 <= batch <= %d, frames_cap >= 1 and 0 <= aux_context_window <= 64 expected", PWG_MAPS_MAX_UTT);
    FCL_REQUIRE(hop >= 128 && hop % 128 == 0, FCL_ERR_SHAPE, "pwg_maps_build: the capacity form needs a hop that is a multiple of 128 (got %d)", hop);
    FCL_REQUIRE(frames_cap * (int64_t)hop < 0x7fffffffLL && frames_cap + 2LL * ctx * (batch + 1) < 0x7fffffffLL, FCL_ERR_SHAPE,
                "pwg_maps_build: frames_cap * hop must stay below 2^31 samples");
    FCL_REQUIRE(aligned16(seg_lo) && aligned16(seg_hi), FCL_ERR_ALIGN, "pwg_maps_build: seg_lo / seg_hi must be 16-byte aligned");
    ProfScope ps("pwg_maps_kernel", 0.0, (double)frames_cap, (hipStream_t)stream);
    const unsigned grid = std::min(grid_1d(frames_cap * (int64_t)hop / 4, 1024), 2048u);
    hipLaunchKernelGGL(pwg_maps_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, utt_frame0, status, batch, (int)frames_cap, ctx, hop, pad_idx, lo, hi, keep,
                       frame_utt, utt_off, seg_lo, seg_hi, live);
    return check_hip(hipGetLastError(), "pwg_maps_build");
}

int fcl_pwg_gather_pad(const float* mel, int64_t mel_rows, const int32_t* pad_idx, const int32_t* live, int64_t pad_cap, int c, float* out, fcl_stream_t stream) {
    FCL_REQUIRE(mel && pad_idx && live && out && mel_rows >= 1 && mel_rows <= 0x7fffffffLL && pad_cap >= 1 && pad_cap <= 0x7fffffffLL && c > 0 && (c & 3) == 0,
                FCL_ERR_INVALID, "pwg_gather_pad: bad arguments (channels must be a multiple of 4)");
    FCL_REQUIRE(aligned16(mel) && aligned16(out), FCL_ERR_ALIGN, "pwg_gather_pad: mel / out must be 16-byte aligned");
    ProfScope ps("pwg_gather_pad_kernel", 0.0, (double)pad_cap, (hipStream_t)stream);
    hipLaunchKernelGGL(pwg_gather_pad_kernel, dim3(grid_1d(pad_cap * (c / 4), 256)), dim3(256), 0, (hipStream_t)stream, mel, (int)mel_rows, pad_idx, live,
                       (int)pad_cap, c, out);
    return check_hip(hipGetLastError(), "pwg_gather_pad");
}

int fcl_pwg_noise_cap(float* z, int64_t n_cap, uint32_t seed, const uint32_t* seed_dev, const int32_t* live, fcl_stream_t stream) {
    FCL_REQUIRE(z && live && n_cap > 0, FCL_ERR_INVALID, "pwg_noise_cap: bad arguments");
    ProfScope ps("pwg_noise_cap_kernel", 0.0, (double)n_cap, (hipStream_t)stream);
    hipLaunchKernelGGL(pwg_noise_cap_kernel, dim3(grid_1d(n_cap, 1024)), dim3(256), 0, (hipStream_t)stream, z, (long long)n_cap, seed, seed_dev, live);
    return check_hip(hipGetLastError(), "pwg_noise_cap");
}

int fcl_pwg_first_conv_cap(const float* z, const float* w, const float* b, uint16_t* xp, int64_t m_cap, int r, const int32_t* live, fcl_stream_t stream) {
    FCL_REQUIRE(z && w && b && xp && live && m_cap > 0 && r > 0 && (r & 31) == 0, FCL_ERR_INVALID, "pwg_first_conv_cap: bad arguments (R must be a multiple of 32)");
    FCL_REQUIRE(aligned16(w) && aligned16(b) && (reinterpret_cast<uintptr_t>(xp) & 127u) == 0, FCL_ERR_ALIGN,
                "pwg_first_conv_cap: w / b must be 16-byte aligned, the planes 128-byte aligned");
    ProfScope ps("pwg_first_conv_cap_kernel", 0.0, (double)m_cap, (hipStream_t)stream);
    hipLaunchKernelGGL(pwg_first_conv_cap_kernel, dim3(grid_1d(m_cap * (r / 4), 256)), dim3(256), 0, (hipStream_t)stream, z, w, b, xp, (long long)m_cap, r, live);
    return check_hip(hipGetLastError(), "pwg_first_conv_cap");
}

int fcl_pwg_layer_cap_fwd(const fcl_pwg_layer_t* a, const int32_t* live, fcl_stream_t stream) {
    FCL_REQUIRE(a && live && a->m > 0 && a->xp_out && a->xp && (a->kp || (a->cp && a->w_aux_p)) && a->w_conv_p && a->b_conv && a->w_os_p && a->b_os && a->skips &&
                    a->seg_lo && a->seg_hi,
                FCL_ERR_INVALID, "pwg_layer_cap_fwd: null argument (the capacity form is the one-launch block: xp_out is required)");
    FCL_REQUIRE(a->r == 64 && a->ksize == 3 && a->aux > 0 && a->aux <= 96 && a->dilation >= 1 && a->xp_out != a->xp, FCL_ERR_SHAPE,
                "pwg_layer_cap_fwd: the capacity form is built for r = 64, ksize = 3, aux <= 96 and needs xp_out != xp");
    FCL_REQUIRE(a->m <= 0x7fffffffLL && a->m % 128 == 0, FCL_ERR_SHAPE, "pwg_layer_cap_fwd: the capacity must be a multiple of 128 samples below 2^31");
    FCL_REQUIRE(((reinterpret_cast<uintptr_t>(a->xp) | reinterpret_cast<uintptr_t>(a->xp_out) | reinterpret_cast<uintptr_t>(a->cp)) & 127u) == 0, FCL_ERR_ALIGN,
                "pwg_layer_cap_fwd: xp / xp_out / cp must be 128-byte aligned");
    if (a->kp) {
        FCL_REQUIRE(a->pt_a && a->pt_b && a->ld_pt > 0, FCL_ERR_INVALID, "pwg_layer_cap_fwd: the frame-rate auxiliary term needs pt_a / pt_b / ld_pt");
        FCL_REQUIRE(a->hop > 0 && a->hop % 128 == 0, FCL_ERR_SHAPE, "pwg_layer_cap_fwd: hop must be a multiple of 128");
        FCL_REQUIRE(((reinterpret_cast<uintptr_t>(a->kp) | reinterpret_cast<uintptr_t>(a->pt_a) | reinterpret_cast<uintptr_t>(a->pt_b)) & 127u) == 0, FCL_ERR_ALIGN,
                    "pwg_layer_cap_fwd: kp / pt_a / pt_b must be 128-byte aligned");
        FCL_REQUIRE((a->m + a->hop - 1) / a->hop + 16 <= (int64_t)a->ld_pt * 32, FCL_ERR_SHAPE, "pwg_layer_cap_fwd: ld_pt does not cover the capacity's frames");
    }
    return launch_pwg_layer_fused(*a, (hipStream_t)stream, live);
}

int fcl_pwg_last_cap_fwd(const float* skips, float scale, const uint16_t* w1p, const float* b1, const float* w2, float b2, float* wav, int64_t m_cap, int s_ch,
                         const int32_t* live, fcl_stream_t stream) {
    FCL_REQUIRE(skips && w1p && b1 && w2 && wav && live && m_cap > 0 && m_cap <= 0x7fffffffLL, FCL_ERR_INVALID, "pwg_last_cap_fwd: bad arguments");
    FCL_REQUIRE(s_ch == 64, FCL_ERR_SHAPE, "pwg_last_cap_fwd: the capacity form is built for 64 skip channels (got %d)", s_ch);
    FCL_REQUIRE(aligned16(skips) && (reinterpret_cast<uintptr_t>(w1p) & 15u) == 0, FCL_ERR_ALIGN, "pwg_last_cap_fwd: skips / w1p must be 16-byte aligned");
    return launch_pwg_last_fused(skips, scale, w1p, b1, w2, b2, wav, m_cap, (hipStream_t)stream, live);
}

int fcl_pcm16_fwd(const float* wav, int16_t* pcm, int64_t n_cap, const int32_t* live, uint32_t* status, fcl_stream_t stream) {
    FCL_REQUIRE(wav && pcm && status && n_cap > 0, FCL_ERR_INVALID, "pcm16_fwd: bad arguments");
    FCL_REQUIRE(aligned16(wav) && (reinterpret_cast<uintptr_t>(pcm) & 7u) == 0, FCL_ERR_ALIGN, "pcm16_fwd: wav must be 16-byte, pcm 8-byte aligned");
    ProfScope ps("pwg_pcm16_kernel", 0.0, (double)n_cap, (hipStream_t)stream);
    hipLaunchKernelGGL(pwg_pcm16_kernel, dim3(grid_1d((n_cap + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, wav, pcm, (long long)n_cap, live, status);
    return check_hip(hipGetLastError(), "pcm16_fwd");
}

int fcl_pwg_layer_fwd(const fcl_pwg_layer_t* a, fcl_stream_t stream) {
    FCL_REQUIRE(a && a->m > 0 && (a->x || a->xp_out) && a->xp && (a->kp || (a->cp && a->w_aux_p)) && a->w_conv_p && a->b_conv && a->w_os_p && a->b_os && a->skips &&
                    a->seg_lo && a->seg_hi,
                FCL_ERR_INVALID, "pwg_layer_fwd: null argument");
    if (a->kp) {
        FCL_REQUIRE(a->xp_out && a->pt_a && a->pt_b && a->ld_pt > 0 && a->hop > 0 && a->hop % 128 == 0, FCL_ERR_INVALID,
                    "pwg_layer_fwd: the frame-rate auxiliary term needs the one-launch form (xp_out), pt_a / pt_b / ld_pt and a hop that is a multiple of 128");
        FCL_REQUIRE(((reinterpret_cast<uintptr_t>(a->kp) | reinterpret_cast<uintptr_t>(a->pt_a) | reinterpret_cast<uintptr_t>(a->pt_b)) & 127u) == 0, FCL_ERR_ALIGN,
                    "pwg_layer_fwd: kp / pt_a / pt_b must be 128-byte aligned");
        FCL_REQUIRE((a->m + a->hop - 1) / a->hop + 16 <= (int64_t)a->ld_pt * 32, FCL_ERR_SHAPE, "pwg_layer_fwd: ld_pt does not cover the frames");
    }
    FCL_REQUIRE(a->r > 0 && (a->r & 31) == 0 && a->aux > 0 && a->dilation >= 1 && a->ksize >= 1 && (a->ksize & 1) && a->ksize + 1 <= FCL_MAX_TERMS, FCL_ERR_SHAPE,
                "pwg_layer_fwd: residual channels must be a multiple of 32, kernel size odd and < %d", FCL_MAX_TERMS);
    FCL_REQUIRE(a->m <= 0x7fffffffLL, FCL_ERR_SHAPE, "pwg_layer_fwd: more than 2^31 samples in one call");
    if (a->xp_out) {
        FCL_REQUIRE(a->r == 64 && a->ksize == 3 && a->aux <= 96 && a->xp_out != a->xp, FCL_ERR_SHAPE,
                    "pwg_layer_fwd: the one-launch block is built for r = 64, ksize = 3, aux <= 96 and needs xp_out != xp");
        return launch_pwg_layer_fused(*a, (hipStream_t)stream);
    }
    FCL_REQUIRE(a->z && a->gp && a->o && a->x, FCL_ERR_WORKSPACE, "pwg_layer_fwd: the unfused path needs x and the z / g / o workspaces");
    hipStream_t s = (hipStream_t)stream;
    const int R = a->r, G = 2 * R, M = (int)a->m;
    const int ldx = R / 32, ldc = (a->aux + 31) / 32;
    GemmArgs g = {};
    for (int j = 0; j < a->ksize; ++j) {
        g.term[j].K = R;
        g.term[j].shift = (j - (a->ksize - 1) / 2) * a->dilation;
        g.term[j].Ap = a->xp; g.term[j].lda_p = ldx;
        g.term[j].Wp = a->w_conv_p + (size_t)j * G * ldx * 64; g.term[j].ldw_p = ldx;
    }
    g.term[a->ksize].K = a->aux;
    g.term[a->ksize].Ap = a->cp; g.term[a->ksize].lda_p = ldc;
    g.term[a->ksize].Wp = a->w_aux_p; g.term[a->ksize].ldw_p = ldc;
    g.nterms = a->ksize + 1;
    g.M = M; g.N = G;
    g.seg_lo = a->seg_lo; g.seg_hi = a->seg_hi;
    g.bias = a->b_conv;
    g.Y = a->z; g.ldy = G;
    int rc = launch_gemm(g, s);
    if (rc) return rc;
    hipLaunchKernelGGL(pwg_gate_kernel, dim3(grid_1d((long long)M * R, 1024)), dim3(256), 0, s, a->z, a->gp, (long long)M, R);
    GemmArgs h = {};
    h.term[0].K = R;
    h.term[0].Ap = a->gp; h.term[0].lda_p = ldx;
    h.term[0].Wp = a->w_os_p; h.term[0].ldw_p = ldx;
    h.nterms = 1;
    h.M = M; h.N = G;
    h.bias = a->b_os;
    h.Y = a->o; h.ldy = G;
    rc = launch_gemm(h, s);
    if (rc) return rc;
    hipLaunchKernelGGL(pwg_resid_kernel, dim3(grid_1d((long long)M * R, 1024)), dim3(256), 0, s, a->o, a->x, a->xp, a->skips, (long long)M, R, a->first_layer);
    return check_hip(hipGetLastError(), "pwg_layer_fwd");
}

int fcl_pwg_last_fwd(const float* skips, float scale, const uint16_t* w1p, const float* b1, const float* w2, float b2, uint16_t* yp, float* h, float* wav,
                     int64_t m, int s_ch, fcl_stream_t stream) {
    FCL_REQUIRE(skips && w1p && b1 && w2 && wav && m > 0 && m <= 0x7fffffffLL && s_ch > 0 && (s_ch & 31) == 0, FCL_ERR_INVALID,
                "pwg_last_fwd: bad arguments (skip channels must be a multiple of 32)");
    hipStream_t s = (hipStream_t)stream;
    if (s_ch == 64 && aligned16(skips) && (reinterpret_cast<uintptr_t>(w1p) & 15u) == 0)  // one launch, skips read once; no workspaces
        return launch_pwg_last_fused(skips, scale, w1p, b1, w2, b2, wav, m, s);
    FCL_REQUIRE(yp && h, FCL_ERR_WORKSPACE, "pwg_last_fwd: this channel count needs the yp / h workspaces");
    hipLaunchKernelGGL(pwg_relu_scale_kernel, dim3(grid_1d(m * s_ch, 1024)), dim3(256), 0, s, skips, scale, yp, (long long)m, s_ch);
    GemmArgs g = {};
    g.term[0].K = s_ch;
    g.term[0].Ap = yp; g.term[0].lda_p = s_ch / 32;
    g.term[0].Wp = w1p; g.term[0].ldw_p = s_ch / 32;
    g.nterms = 1;
    g.M = (int)m; g.N = s_ch;
    g.bias = b1;
    g.Y = h; g.ldy = s_ch;
    int rc = launch_gemm(g, s);
    if (rc) return rc;
    hipLaunchKernelGGL(pwg_out_kernel, dim3(grid_1d(m, 16)), dim3(256), 0, s, h, w2, b2, wav, (long long)m, s_ch);
    return check_hip(hipGetLastError(), "pwg_last_fwd");
}

}  // extern "C"
