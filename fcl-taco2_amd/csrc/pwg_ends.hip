// pwg_ends.hip -- the two ends of the Parallel WaveGAN generator in its training form, forward and backward (include/fcl_hip.h "Parallel WaveGAN generator,
// the ends"; fcl_taco2_amd/pwg_generator.py; restated in float64 numpy in tests/pwge_ref.py).  Input side: the upsampling network (conv_in and
// one stretch-and-filter stage per scale) into the [samples, A] rows the residual stack reads, and first_conv into its [samples, R] rows.  Output side: the
// sqrt(1 / layers) scale, ReLU, the R -> R layer, ReLU and the R -> 1 layer.  The stack between them is pwg_train.hip.
//
// Layout is pwg_rows.h's: float32, channel-last, packed rows, the utterances back to back, row t's utterance [seg_lo[t], seg_hi[t]) in samples.  A stage
// that runs at 1 / q of the sample rate takes its bounds from the same tables (seg_lo[t q] / q: every utterance starts at a multiple of the hop).  The
// R -> R layer and its gradients are pwr_contract / pwr_dw_kernel; everything else is a few FMAs per element and plain code.  No atomics: every sum over
// samples leaves per-chunk partials that pwe_reduce_kernel adds in ascending chunk order.
#include <algorithm>

#include "pwg_rows.h"

namespace fcl {

constexpr int PWE_CHUNK = PWR_DW_CHUNK;  // rows per partial of the sums over samples
constexpr int PWE_FCHUNK = 256;          // frames per partial of conv_in's weight gradient
constexpr int PWE_MAX_SCALES = 6, PWE_MAX_SCALE = 16, PWE_MAX_TAPS = 2 * PWE_MAX_SCALE + 1, PWE_MAX_CTX = 8;
constexpr int PWE_LANES = 16, PWE_TROWS = 16;  // a workgroup of the plain kernels: 16 rows x 16 channel lanes (a lane takes channels lane, lane + 16, ..)
constexpr int PWE_MAX_CL = 8;                  // channels per lane: 128 / 16

// the utterance of frame f: frame_off [n_utt + 1] ascending, frame_off[0] = 0
__device__ __forceinline__ int pwe_utt(const int32_t* __restrict__ frame_off, int n_utt, int f) {
    int b = 0;
    while (b + 1 < n_utt && frame_off[b + 1] <= f) ++b;
    return b;
}

// ---- conv_in: u0[f, :] = sum_j c_b[f + j, :] Win_j.  Utterance b's rows of c start at frame_off[b] + 2 ctx b, so the 2 ctx + 1 rows of a frame are one run
// of K = (2 ctx + 1) A floats against w [K, A].
__global__ __launch_bounds__(256) void pwe_convin_kernel(const float* __restrict__ c, const float* __restrict__ w, const int32_t* __restrict__ frame_off,
                                                         int n_utt, int frames, int A, int ctx, float* __restrict__ u0) {
    const int lane = threadIdx.x & (PWE_LANES - 1), f = blockIdx.x * PWE_TROWS + (threadIdx.x >> 4);
    if (f >= frames) return;
    const int b = pwe_utt(frame_off, n_utt, f), K = (2 * ctx + 1) * A;
    const float* src = c + (size_t)(f + 2 * ctx * b) * A;
    for (int a = lane; a < A; a += PWE_LANES) {
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < K; ++k) acc = fmaf(src[k], w[(size_t)k * A + a], acc);
        u0[(size_t)f * A + a] = acc;
    }
}

// ---- one stage: out[t, a] = sum_{j = 0 .. 2 s} h[j] in[(t + j - s) div s, a] over the taps inside the utterance.  q = samples per output row.
__global__ __launch_bounds__(256) void pwe_stage_kernel(const float* __restrict__ in, const float* __restrict__ h, const int32_t* __restrict__ seg_lo,
                                                        const int32_t* __restrict__ seg_hi, int q, int s, int A, int rows_out, float* __restrict__ out) {
    const int lane = threadIdx.x & (PWE_LANES - 1);
    const long long t = (long long)blockIdx.x * PWE_TROWS + (threadIdx.x >> 4);
    if (t >= rows_out) return;
    const long long lo = max(0, seg_lo[t * q]) / q, hi = min((long long)rows_out, (long long)seg_hi[t * q] / q);
    float acc[PWE_MAX_CL];
#pragma unroll
    for (int i = 0; i < PWE_MAX_CL; ++i) acc[i] = 0.f;
    for (int j = 0; j <= 2 * s; ++j) {
        const long long p = t + j - s;
        if (p < lo || p >= hi) continue;
        const float hj = h[j];
        const float* src = in + (size_t)(p / s) * A + lane;
#pragma unroll
        for (int i = 0; i < PWE_MAX_CL; ++i)
            if (i * PWE_LANES + lane < A) acc[i] = fmaf(hj, src[i * PWE_LANES], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < PWE_MAX_CL; ++i)
        if (i * PWE_LANES + lane < A) out[(size_t)t * A + i * PWE_LANES + lane] = acc[i];
}

// ---- one stage backward, gather form: din[m, a] = sum over the output rows t and taps j with (t + j - s) div s == m of h[j] g[t, a]; t runs over
// [s m - s, s m + 2 s) inside the utterance, j over [s m + s - t, s m + 2 s - 1 - t] inside [0, 2 s].  q = samples per OUTPUT row.
__global__ __launch_bounds__(256) void pwe_stage_bwd_kernel(const float* __restrict__ g, const float* __restrict__ h, const int32_t* __restrict__ seg_lo,
                                                            const int32_t* __restrict__ seg_hi, int q, int s, int A, int rows_in, float* __restrict__ din) {
    const int lane = threadIdx.x & (PWE_LANES - 1);
    const long long m = (long long)blockIdx.x * PWE_TROWS + (threadIdx.x >> 4);
    if (m >= rows_in) return;
    const long long rows_out = (long long)rows_in * s, at = m * s * q;  // (a sample of input row m)
    const long long lo = max(0, seg_lo[at]) / q, hi = min(rows_out, (long long)seg_hi[at] / q);
    float acc[PWE_MAX_CL];
#pragma unroll
    for (int i = 0; i < PWE_MAX_CL; ++i) acc[i] = 0.f;
    for (long long t = max(lo, m * s - s); t < min(hi, m * s + 2 * s); ++t) {
        float gv[PWE_MAX_CL];
#pragma unroll
        for (int i = 0; i < PWE_MAX_CL; ++i) gv[i] = i * PWE_LANES + lane < A ? g[(size_t)t * A + i * PWE_LANES + lane] : 0.f;
        const int j_lo = (int)max(0LL, m * s + s - t), j_hi = (int)min((long long)2 * s, m * s + 2 * s - 1 - t);
        for (int j = j_lo; j <= j_hi; ++j) {
            const float hj = h[j];
#pragma unroll
            for (int i = 0; i < PWE_MAX_CL; ++i) acc[i] = fmaf(hj, gv[i], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < PWE_MAX_CL; ++i)
        if (i * PWE_LANES + lane < A) din[(size_t)m * A + i * PWE_LANES + lane] = acc[i];
}

// ---- a stage's filter gradient: partial[chunk][j] = sum over the chunk's output rows t and all channels a of in[(t + j - s) div s, a] g[t, a].  The 2 s + 1
// taps of an output row read three input rows at the most (m0 = t div s - 1 and the two after it: tap j reads row m0 + (t mod s + j) div s), so an
// element costs four loads whatever s is.  1024 threads: 64 rows x 16 channel lanes at a time (one wave per SIMD would wait out every load on its own).  A
// thread sums its elements (rows 64 apart, channels 16 apart, ascending), six exchanges add a wave's lanes, then thread j adds the 16 waves in order.
__global__ __launch_bounds__(1024) void pwe_dh_kernel(const float* __restrict__ in, const float* __restrict__ g, const int32_t* __restrict__ seg_lo,
                                                      const int32_t* __restrict__ seg_hi, int q, int s, int A, int rows_out, float* __restrict__ partial) {
    __shared__ float red[16][PWE_MAX_TAPS];
    const int lane = threadIdx.x & (PWE_LANES - 1), taps = 2 * s + 1;
    const long long t_begin = (long long)blockIdx.x * PWE_CHUNK, t_end = min((long long)rows_out, t_begin + PWE_CHUNK);
    const long long rows_in = rows_out / s;
    float acc[PWE_MAX_TAPS];
#pragma unroll
    for (int j = 0; j < PWE_MAX_TAPS; ++j) acc[j] = 0.f;
    for (long long t = t_begin + (threadIdx.x >> 4); t < t_end; t += 64) {
        const long long lo = max(0, seg_lo[t * q]) / q, hi = min((long long)rows_out, (long long)seg_hi[t * q] / q);
        const long long p0 = t - s, m0 = t / s - 1;  // floor(p0 / s)
        const int r0 = (int)(t - (m0 + 1) * s);      // p0 - m0 s = t mod s
        const float* row0 = in + (size_t)min(max(m0, 0LL), rows_in - 1) * A;
        const float* row1 = in + (size_t)min(max(m0 + 1, 0LL), rows_in - 1) * A;
        const float* row2 = in + (size_t)min(max(m0 + 2, 0LL), rows_in - 1) * A;
        for (int a = lane; a < A; a += PWE_LANES) {
            const float gv = g[(size_t)t * A + a], v0 = row0[a], v1 = row1[a], v2 = row2[a];
#pragma unroll
            for (int j = 0; j < PWE_MAX_TAPS; ++j) {
                if (j < taps) {
                    const long long p = p0 + j;
                    const int rj = r0 + j;
                    const float v = rj < s ? v0 : (rj < 2 * s ? v1 : v2);
                    acc[j] = fmaf(pwr_keep(v, p >= lo && p < hi), gv, acc[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PWE_MAX_TAPS; ++j) {
        if (j < taps) {
            float v = acc[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < taps) {
        float sum = 0.f;
        for (int k = 0; k < 16; ++k) sum += red[k][threadIdx.x];
        partial[(size_t)blockIdx.x * taps + threadIdx.x] = sum;
    }
}

// ---- conv_in's weight gradient: partial[chunk][k][a] = sum over the chunk's frames f (ascending) of c_run(f)[k] du0[f, a], k over the (2 ctx + 1) A run
__global__ __launch_bounds__(256) void pwe_dwin_kernel(const float* __restrict__ c, const float* __restrict__ du0, const int32_t* __restrict__ frame_off,
                                                       int n_utt, int frames, int A, int ctx, float* __restrict__ partial) {
    const int K = (2 * ctx + 1) * A, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * A) return;
    const int k = e / A, a = e - k * A;
    const int f_begin = blockIdx.y * PWE_FCHUNK, f_end = min(frames, f_begin + PWE_FCHUNK);
    int b = pwe_utt(frame_off, n_utt, f_begin);
    float acc = 0.f;
    for (int f = f_begin; f < f_end; ++f) {
        while (b + 1 < n_utt && frame_off[b + 1] <= f) ++b;
        acc = fmaf(c[(size_t)(f + 2 * ctx * b) * A + k], du0[(size_t)f * A + a], acc);
    }
    partial[(size_t)blockIdx.y * K * A + e] = acc;
}

// ---- conv_in backward to the conditioning: dc_b[i, ai] = sum_j sum_ao du0_b[i - j, ao] Win_j[ai, ao] over the frames 0 <= i - j < F_b
__global__ __launch_bounds__(256) void pwe_dc_kernel(const float* __restrict__ du0, const float* __restrict__ w, const int32_t* __restrict__ frame_off,
                                                     int n_utt, int c_rows, int A, int ctx, float* __restrict__ dc) {
    const int lane = threadIdx.x & (PWE_LANES - 1), row = blockIdx.x * PWE_TROWS + (threadIdx.x >> 4);
    if (row >= c_rows) return;
    int b = 0;
    while (b + 1 < n_utt && frame_off[b + 1] + 2 * ctx * (b + 1) <= row) ++b;
    const int i = row - (frame_off[b] + 2 * ctx * b), F = frame_off[b + 1] - frame_off[b];
    for (int a = lane; a < A; a += PWE_LANES) {
        float acc = 0.f;
        for (int j = 0; j <= 2 * ctx; ++j) {
            const int fl = i - j;
            if (fl < 0 || fl >= F) continue;
            const float* d = du0 + (size_t)(frame_off[b] + fl) * A;
            const float* wr = w + ((size_t)j * A + a) * A;
            for (int ao = 0; ao < A; ++ao) acc = fmaf(d[ao], wr[ao], acc);
        }
        dc[(size_t)row * A + a] = acc;
    }
}

// ---- first_conv: x0[t, r] = z[t] w0[r] + b0[r]
__global__ __launch_bounds__(256) void pwe_first_kernel(const float* __restrict__ z, const float* __restrict__ w0, const float* __restrict__ b0, int R,
                                                        long long n, float* __restrict__ x0) {
    const int lane = threadIdx.x & (PWE_LANES - 1);
    const long long t = (long long)blockIdx.x * PWE_TROWS + (threadIdx.x >> 4);
    if (t >= n) return;
    const float zv = z[t];
    for (int r = lane; r < R; r += PWE_LANES) x0[t * R + r] = fmaf(zv, w0[r], b0[r]);
}

// ---- first_conv backward to the noise: dz[t] = sum_r dx0[t, r] w0[r]
__global__ __launch_bounds__(256) void pwe_first_dz_kernel(const float* __restrict__ dx0, const float* __restrict__ w0, int R, long long n,
                                                           float* __restrict__ dz) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) acc = fmaf(dx0[t * R + r], w0[r], acc);
    dz[t] = acc;
}

// ---- the sums of a scalar-times-row layer: partial[chunk] = (sum_t s[t] X[t, :] | sum_t X[t, :] | sum_t s[t]), 2 R + 1 floats.  first_conv: s = z, X = dx0
// (dw0 | db0 | -); the last layer: s = dwav, X = y1 (dw3 | - | db3).  A thread sums rows 16 apart (ascending), then thread e adds the 16 row groups in order.
__global__ __launch_bounds__(256) void pwe_outer_kernel(const float* __restrict__ sc, const float* __restrict__ X, int R, long long n,
                                                        float* __restrict__ partial) {
    __shared__ float red[PWE_TROWS][2 * 64 + 1];
    const int lane = threadIdx.x & (PWE_LANES - 1), grp = threadIdx.x >> 4;
    const long long t_begin = (long long)blockIdx.x * PWE_CHUNK, t_end = min(n, t_begin + PWE_CHUNK);
    float sx[4] = {0.f, 0.f, 0.f, 0.f}, x1[4] = {0.f, 0.f, 0.f, 0.f}, s1 = 0.f;
    for (long long t = t_begin + grp; t < t_end; t += PWE_TROWS) {
        const float sv = sc[t];
        s1 += sv;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i * PWE_LANES + lane < R) {
                const float xv = X[t * R + i * PWE_LANES + lane];
                sx[i] = fmaf(sv, xv, sx[i]);
                x1[i] += xv;
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i * PWE_LANES + lane < R) {
            red[grp][i * PWE_LANES + lane] = sx[i];
            red[grp][R + i * PWE_LANES + lane] = x1[i];
        }
    if (lane == 0) red[grp][2 * R] = s1;
    __syncthreads();
    if ((int)threadIdx.x < 2 * R + 1) {
        float sum = 0.f;
        for (int k = 0; k < PWE_TROWS; ++k) sum += red[k][threadIdx.x];
        partial[(size_t)blockIdx.x * (2 * R + 1) + threadIdx.x] = sum;
    }
}

// out[e] = sum over the chunks k (ascending) of partial[k stride + off + e], e < count
__global__ __launch_bounds__(256) void pwe_reduce_kernel(const float* __restrict__ partial, int chunks, int stride, int off, int count, float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * stride + off + e];
    out[e] = s;
}

// ---- output side forward: y1 = relu(relu(sigma S) W1 + b1) (KEPT), wav[t] = y1[t, :] . w3 + b3.  The wave holds a row's R columns in 16 lanes x NT tiles:
// a lane adds its tiles' products in ascending tile order, then four exchanges add the 16 lanes (every lane of the group ends with the same sum).
template <int NT>
__global__ __launch_bounds__(256) void pwe_out_kernel(PwrA A, const float* __restrict__ w, const float* __restrict__ b1, const float* __restrict__ w3,
                                                      const float* __restrict__ b3, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                      float* __restrict__ y1, float* __restrict__ wav, long long n) {
    constexpr int R = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_RELU, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const float bias3 = b3[0];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const long long row = t0 + mt * 16 + 4 * q + reg;
            float dot = 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + r;
                const float y = fmaxf(acc[mt][nt][reg] + b1[col], 0.f);
                if (row < n) y1[row * R + col] = y;
                dot = fmaf(y, w3[col], dot);
            }
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) dot += __shfl_xor(dot, d, 64);
            if (row < n && r == 0) wav[row] = dot + bias3;
        }
}

// ---- output side backward, the seed: dy1[t, c] = dwav[t] w3[c] where y1 > 0
__global__ __launch_bounds__(256) void pwe_dy1_kernel(const float* __restrict__ dwav, const float* __restrict__ w3, const float* __restrict__ y1, int R,
                                                      long long n, float* __restrict__ dy1) {
    const int lane = threadIdx.x & (PWE_LANES - 1);
    const long long t = (long long)blockIdx.x * PWE_TROWS + (threadIdx.x >> 4);
    if (t >= n) return;
    const float g = dwav[t];
    for (int c = lane; c < R; c += PWE_LANES) dy1[t * R + c] = y1[t * R + c] > 0.f ? g * w3[c] : 0.f;
}

// ---- dS = sigma (dy1 W1^T) where sigma S > 0 (the forward's own test of v)
template <int NT>
__global__ __launch_bounds__(256) void pwe_ds_kernel(PwrA A, const float* __restrict__ w, const float* __restrict__ S, float sigma,
                                                     const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* __restrict__ ds,
                                                     long long n) {
    constexpr int R = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long row = t0 + mt * 16 + 4 * q + reg;
                if (row >= n) continue;
                const int col = nt * 16 + r;
                ds[row * R + col] = S[row * R + col] * sigma > 0.f ? sigma * acc[mt][nt][reg] : 0.f;
            }
}

static unsigned pwe_blocks(long long rows, int per) { return (unsigned)((rows + per - 1) / per); }
static long long pwe_hop(const fcl_pwe_t* a) {
    long long hop = 1;
    for (int i = 0; i < a->n_scales; ++i) hop *= a->scales[i];
    return hop;
}
static size_t pwe_round4(size_t floats) { return (floats + 3) & ~(size_t)3; }
// the workspace: the partials of the largest sum, then two [samples / s_last, A] buffers for the gradients of the stage inputs
static size_t pwe_partial_floats(const fcl_pwe_t* a) {
    const size_t chunks = (size_t)pwr_chunks(a->samples), R = a->residual, A = a->aux;
    const size_t fchunks = ((size_t)a->frames + PWE_FCHUNK - 1) / PWE_FCHUNK;
    return pwe_round4(std::max({chunks * (2 * R + 1), chunks * (size_t)PWE_MAX_TAPS, chunks * (R + 1) * R, fchunks * (size_t)(2 * a->ctx + 1) * A * A}));
}
static size_t pwe_du_floats(const fcl_pwe_t* a) { return pwe_round4((size_t)(a->samples / a->scales[a->n_scales - 1]) * a->aux); }

// what every entry checks: the struct, the widths, the context, the scales, the row counts, the tables
static int pwe_check(const fcl_pwe_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->residual >= 16 && a->residual <= 64 && a->residual % 16 == 0, FCL_ERR_SHAPE,
                "%s: residual (= skip) channels must be a multiple of 16 from 16 to 64 (got %d)", who, a->residual);
    FCL_REQUIRE(a->aux >= 16 && a->aux <= 128 && a->aux % 16 == 0, FCL_ERR_SHAPE, "%s: aux channels must be a multiple of 16 from 16 to 128 (got %d)", who,
                a->aux);
    FCL_REQUIRE(a->ctx >= 0 && a->ctx <= PWE_MAX_CTX, FCL_ERR_SHAPE, "%s: aux_context_window must be 0 to %d (got %d)", who, PWE_MAX_CTX, a->ctx);
    FCL_REQUIRE(a->n_scales >= 1 && a->n_scales <= PWE_MAX_SCALES, FCL_ERR_SHAPE, "%s: 1 to %d upsample scales expected (got %d)", who, PWE_MAX_SCALES,
                a->n_scales);
    for (int i = 0; i < a->n_scales; ++i)
        FCL_REQUIRE(a->scales[i] >= 2 && a->scales[i] <= PWE_MAX_SCALE, FCL_ERR_SHAPE, "%s: upsample scale %d must be 2 to %d (got %d)", who, i, PWE_MAX_SCALE,
                    a->scales[i]);
    FCL_REQUIRE(a->n_utt >= 1 && a->frames >= a->n_utt, FCL_ERR_SHAPE, "%s: at least one utterance of at least one frame each expected (got %d frames, %d utterances)",
                who, a->frames, a->n_utt);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL && a->samples == (long long)a->frames * pwe_hop(a), FCL_ERR_SHAPE,
                "%s: samples = frames x hop below 2^31 expected (got %lld samples, %d frames, hop %lld)", who, (long long)a->samples, a->frames, pwe_hop(a));
    FCL_REQUIRE(a->seg_lo && a->seg_hi && a->frame_off, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi / frame_off", who);
    return FCL_OK;
}

static int pwe_check_workspace(const fcl_pwe_t* a, const char* who) {
    FCL_REQUIRE(a->workspace, FCL_ERR_INVALID, "%s: null workspace", who);
    FCL_REQUIRE(aligned16(a->workspace), FCL_ERR_ALIGN, "%s: the workspace must be 16-byte aligned", who);
    FCL_REQUIRE(a->workspace_bytes >= fcl_pwe_workspace_bytes(a), FCL_ERR_WORKSPACE, "%s: the workspace holds %zu bytes, fcl_pwe_workspace_bytes asks for %zu", who,
                a->workspace_bytes, fcl_pwe_workspace_bytes(a));
    return FCL_OK;
}

static void pwe_reduce(hipStream_t s, const float* partial, int chunks, int stride, int off, int count, float* out) {
    ProfScope ps("pwe_reduce_kernel", 0.0, (double)chunks, s);
    hipLaunchKernelGGL(pwe_reduce_kernel, dim3(pwe_blocks(count, 256)), dim3(256), 0, s, partial, chunks, stride, off, count, out);
}

#define PWE_R_TILES(CALL)       \
    switch (R / 16) {           \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
    }

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_pwe_workspace_bytes(const fcl_pwe_t* a) {
    if (!a || a->samples < 1 || a->frames < 1 || a->residual < 1 || a->aux < 1 || a->ctx < 0 || a->n_scales < 1 || a->n_scales > PWE_MAX_SCALES) return 0;
    for (int i = 0; i < a->n_scales; ++i)
        if (a->scales[i] < 1) return 0;
    return (pwe_partial_floats(a) + 2 * pwe_du_floats(a)) * sizeof(float);
}

int fcl_pwe_in_fwd(const fcl_pwe_t* a, fcl_stream_t stream) {
    const int rc = pwe_check(a, "pwe_in_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->c && a->z && a->w_in && a->w0 && a->b0 && a->cu && a->x0, FCL_ERR_INVALID, "pwe_in_fwd: null c / z / w_in / w0 / b0 / cu / x0");
    for (int i = 0; i < a->n_scales; ++i) FCL_REQUIRE(a->h[i] && a->u[i], FCL_ERR_INVALID, "pwe_in_fwd: null h[%d] / u[%d]", i, i);
    hipStream_t s = (hipStream_t)stream;
    const int A = a->aux, R = a->residual;
    const long long n = a->samples;
    {
        ProfScope ps("pwe_convin_kernel", 2.0 * (2 * a->ctx + 1) * A * A * (double)a->frames, (double)a->frames, s);
        hipLaunchKernelGGL(pwe_convin_kernel, dim3(pwe_blocks(a->frames, PWE_TROWS)), dim3(256), 0, s, a->c, a->w_in, a->frame_off, a->n_utt, a->frames, A,
                           a->ctx, a->u[0]);
    }
    long long rows = a->frames, q = pwe_hop(a);
    for (int i = 0; i < a->n_scales; ++i) {
        const int sc = a->scales[i];
        rows *= sc;
        q /= sc;
        float* out = i + 1 < a->n_scales ? a->u[i + 1] : a->cu;
        ProfScope ps("pwe_stage_kernel", 2.0 * (2 * sc + 1) * A * (double)rows, (double)rows, s);
        hipLaunchKernelGGL(pwe_stage_kernel, dim3(pwe_blocks(rows, PWE_TROWS)), dim3(256), 0, s, a->u[i], a->h[i], a->seg_lo, a->seg_hi, (int)q, sc, A, (int)rows,
                           out);
    }
    {
        ProfScope ps("pwe_first_kernel", 2.0 * R * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwe_first_kernel, dim3(pwe_blocks(n, PWE_TROWS)), dim3(256), 0, s, a->z, a->w0, a->b0, R, n, a->x0);
    }
    return check_hip(hipGetLastError(), "pwe_in_fwd");
}

int fcl_pwe_in_bwd(const fcl_pwe_t* a, fcl_stream_t stream) {
    const int rc = pwe_check(a, "pwe_in_bwd");
    if (rc) return rc;
    FCL_REQUIRE(a->dcu && a->dx0, FCL_ERR_INVALID, "pwe_in_bwd: null dcu / dx0");
    const bool need_w = a->dw_in != nullptr;
    for (int i = 0; i < a->n_scales; ++i)
        FCL_REQUIRE((a->dh[i] != nullptr) == need_w, FCL_ERR_INVALID, "pwe_in_bwd: dw_in, dw0, db0 and every dh[i] are given together or not at all");
    FCL_REQUIRE((a->dw0 != nullptr) == need_w && (a->db0 != nullptr) == need_w, FCL_ERR_INVALID,
                "pwe_in_bwd: dw_in, dw0, db0 and every dh[i] are given together or not at all");
    const bool chain = need_w || a->dc;
    if (need_w) {
        FCL_REQUIRE(a->c && a->z, FCL_ERR_INVALID, "pwe_in_bwd: the weight gradients need c and z");
        for (int i = 0; i < a->n_scales; ++i) FCL_REQUIRE(a->u[i], FCL_ERR_INVALID, "pwe_in_bwd: the weight gradients need u[%d]", i);
    }
    if (chain)
        for (int i = 0; i < a->n_scales; ++i) FCL_REQUIRE(a->h[i], FCL_ERR_INVALID, "pwe_in_bwd: null h[%d]", i);
    FCL_REQUIRE(!a->dc || a->w_in, FCL_ERR_INVALID, "pwe_in_bwd: dc needs w_in");
    FCL_REQUIRE(!a->dz || a->w0, FCL_ERR_INVALID, "pwe_in_bwd: dz needs w0");
    if (chain) {
        const int rw = pwe_check_workspace(a, "pwe_in_bwd");
        if (rw) return rw;
    }
    hipStream_t s = (hipStream_t)stream;
    const int A = a->aux, R = a->residual, K = (2 * a->ctx + 1) * A;
    const long long n = a->samples;
    const int chunks = (int)pwr_chunks(n);
    float* partial = a->workspace;
    if (need_w) {
        {
            ProfScope ps("pwe_outer_kernel", 4.0 * R * (double)n, (double)n, s);
            hipLaunchKernelGGL(pwe_outer_kernel, dim3(chunks), dim3(256), 0, s, a->z, a->dx0, R, n, partial);
        }
        pwe_reduce(s, partial, chunks, 2 * R + 1, 0, R, a->dw0);
        pwe_reduce(s, partial, chunks, 2 * R + 1, R, R, a->db0);
    }
    if (a->dz) {
        ProfScope ps("pwe_first_dz_kernel", 2.0 * R * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwe_first_dz_kernel, dim3(pwe_blocks(n, 256)), dim3(256), 0, s, a->dx0, a->w0, R, n, a->dz);
    }
    if (chain) {
        float* du[2] = {a->workspace + pwe_partial_floats(a), a->workspace + pwe_partial_floats(a) + pwe_du_floats(a)};
        const float* g = a->dcu;
        long long rows = n, q = 1;  // rows of the stage's output, samples per output row
        for (int i = a->n_scales - 1; i >= 0; --i) {
            const int sc = a->scales[i];
            if (need_w) {
                const int ch = (int)pwr_chunks(rows);
                {
                    ProfScope ps("pwe_dh_kernel", 2.0 * (2 * sc + 1) * A * (double)rows, (double)rows, s);
                    hipLaunchKernelGGL(pwe_dh_kernel, dim3(ch), dim3(1024), 0, s, a->u[i], g, a->seg_lo, a->seg_hi, (int)q, sc, A, (int)rows, partial);
                }
                pwe_reduce(s, partial, ch, 2 * sc + 1, 0, 2 * sc + 1, a->dh[i]);
            }
            float* out = du[(a->n_scales - 1 - i) & 1];
            {
                ProfScope ps("pwe_stage_bwd_kernel", 2.0 * (2 * sc + 1) * A * (double)rows, (double)rows, s);
                hipLaunchKernelGGL(pwe_stage_bwd_kernel, dim3(pwe_blocks(rows / sc, PWE_TROWS)), dim3(256), 0, s, g, a->h[i], a->seg_lo, a->seg_hi, (int)q, sc, A,
                                   (int)(rows / sc), out);
            }
            g = out;
            rows /= sc;
            q *= sc;
        }
        if (need_w) {
            const int fch = (a->frames + PWE_FCHUNK - 1) / PWE_FCHUNK;
            {
                ProfScope ps("pwe_dwin_kernel", 2.0 * K * A * (double)a->frames, (double)a->frames, s);
                hipLaunchKernelGGL(pwe_dwin_kernel, dim3(pwe_blocks((long long)K * A, 256), fch), dim3(256), 0, s, a->c, g, a->frame_off, a->n_utt, a->frames, A,
                                   a->ctx, partial);
            }
            pwe_reduce(s, partial, fch, K * A, 0, K * A, a->dw_in);
        }
        if (a->dc) {
            const int c_rows = a->frames + 2 * a->ctx * a->n_utt;
            ProfScope ps("pwe_dc_kernel", 2.0 * K * A * (double)c_rows, (double)c_rows, s);
            hipLaunchKernelGGL(pwe_dc_kernel, dim3(pwe_blocks(c_rows, PWE_TROWS)), dim3(256), 0, s, g, a->w_in, a->frame_off, a->n_utt, c_rows, A, a->ctx, a->dc);
        }
    }
    return check_hip(hipGetLastError(), "pwe_in_bwd");
}

int fcl_pwe_out_fwd(const fcl_pwe_t* a, fcl_stream_t stream) {
    const int rc = pwe_check(a, "pwe_out_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->sigma > 0.f && a->sigma <= 1.f, FCL_ERR_SHAPE, "pwe_out_fwd: sigma = sqrt(1 / layers) in (0, 1] expected (got %g)", (double)a->sigma);
    FCL_REQUIRE(a->skips && a->w1 && a->b1 && a->w3 && a->b3 && a->y1 && a->wav, FCL_ERR_INVALID, "pwe_out_fwd: null skips / w1 / b1 / w3 / b3 / y1 / wav");
    FCL_REQUIRE(aligned16(a->skips) && aligned16(a->w1) && aligned16(a->y1), FCL_ERR_ALIGN, "pwe_out_fwd: skips, w1 and y1 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual;
    const PwrA in = {a->skips, R, R, 1, 1, a->sigma, nullptr, 0, 0};
    const dim3 grid(pwe_blocks(n, PWR_ROWS));
    ProfScope ps("pwe_out_kernel", 2.0 * (R + 1) * R * (double)n, (double)n, s);
#define PWE_CALL(NN) hipLaunchKernelGGL(pwe_out_kernel<NN>, grid, dim3(256), 0, s, in, a->w1, a->b1, a->w3, a->b3, a->seg_lo, a->seg_hi, a->y1, a->wav, n)
    PWE_R_TILES(PWE_CALL)
#undef PWE_CALL
    return check_hip(hipGetLastError(), "pwe_out_fwd");
}

int fcl_pwe_out_bwd(const fcl_pwe_t* a, fcl_stream_t stream) {
    const int rc = pwe_check(a, "pwe_out_bwd");
    if (rc) return rc;
    FCL_REQUIRE(a->sigma > 0.f && a->sigma <= 1.f, FCL_ERR_SHAPE, "pwe_out_bwd: sigma = sqrt(1 / layers) in (0, 1] expected (got %g)", (double)a->sigma);
    FCL_REQUIRE(a->skips && a->y1 && a->dwav && a->w1t && a->w3 && a->dy1 && a->ds, FCL_ERR_INVALID, "pwe_out_bwd: null skips / y1 / dwav / w1t / w3 / dy1 / ds");
    const bool need_w = a->dw1 != nullptr;
    FCL_REQUIRE((a->db1 != nullptr) == need_w && (a->dw3 != nullptr) == need_w && (a->db3 != nullptr) == need_w, FCL_ERR_INVALID,
                "pwe_out_bwd: dw1, db1, dw3 and db3 are given together or not at all");
    FCL_REQUIRE(aligned16(a->skips) && aligned16(a->y1) && aligned16(a->w1t) && aligned16(a->dy1) && aligned16(a->ds), FCL_ERR_ALIGN,
                "pwe_out_bwd: skips, y1, w1t, dy1 and ds must be 16-byte aligned");
    if (need_w) {
        const int rw = pwe_check_workspace(a, "pwe_out_bwd");
        if (rw) return rw;
    }
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual;
    {
        ProfScope ps("pwe_dy1_kernel", (double)R * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwe_dy1_kernel, dim3(pwe_blocks(n, PWE_TROWS)), dim3(256), 0, s, a->dwav, a->w3, a->y1, R, n, a->dy1);
    }
    {
        const PwrA in = {a->dy1, R, R, 1, 1, 1.f, nullptr, 0, 0};
        const dim3 grid(pwe_blocks(n, PWR_ROWS));
        ProfScope ps("pwe_ds_kernel", 2.0 * R * R * (double)n, (double)n, s);
#define PWE_CALL(NN) hipLaunchKernelGGL(pwe_ds_kernel<NN>, grid, dim3(256), 0, s, in, a->w1t, a->skips, a->sigma, a->seg_lo, a->seg_hi, a->ds, n)
        PWE_R_TILES(PWE_CALL)
#undef PWE_CALL
    }
    if (need_w) {
        const int chunks = (int)pwr_chunks(n);
        {
            // dW1^T [R (v) + 1][R (y1)] per chunk: the A operand is v = relu(sigma S) formed on load, B = dy1
            const PwrA in = {a->skips, R, R, 1, 1, a->sigma, nullptr, 0, 0};
            const dim3 grid((unsigned)chunks, (unsigned)((R / 16 + 1 + 3) / 4));
            ProfScope ps("pwe_dw_kernel<last>", 2.0 * R * R * (double)n, (double)n, s);
#define PWE_CALL(NN) \
    hipLaunchKernelGGL((pwr_dw_kernel<PWR_RELU, NN, 0>), grid, dim3(256), 0, s, in, a->dy1, a->dy1, R, 1.f, 0, a->seg_lo, a->seg_hi, a->workspace, n)
            PWE_R_TILES(PWE_CALL)
#undef PWE_CALL
        }
        pwe_reduce(s, a->workspace, chunks, (R + 1) * R, 0, R * R, a->dw1);
        pwe_reduce(s, a->workspace, chunks, (R + 1) * R, R * R, R, a->db1);
        {
            ProfScope ps("pwe_outer_kernel", 4.0 * R * (double)n, (double)n, s);
            hipLaunchKernelGGL(pwe_outer_kernel, dim3(chunks), dim3(256), 0, s, a->dwav, a->y1, R, n, a->workspace);
        }
        pwe_reduce(s, a->workspace, chunks, 2 * R + 1, 0, R, a->dw3);
        pwe_reduce(s, a->workspace, chunks, 2 * R + 1, 2 * R, 1, a->db3);
    }
    return check_hip(hipGetLastError(), "pwe_out_bwd");
}

}  // extern "C"
