// hifigan_end.hip -- the HiFi-GAN generator's output end in its training form: LeakyReLU at the end's own slope, output_conv (C -> 1 .. 4 channels) and
// tanh forward, and backward to the input, weight and bias gradients (include/fcl_hip.h "HiFi-GAN generator, output end";
// fcl_taco2_amd/hifigan_generator.py; restated in float64 numpy in tests/hfge_ref.py).  The stages before it are hifigan_train.hip.
//
// Layout is pwg_rows.h's: float32, channel-last, packed [rows, C], the utterances back to back, row t's utterance is [seg_lo[t], seg_hi[t]) and a tap
// outside it contributes zero.  The contraction has at most four output columns, so it is VALU work: a lane holds four consecutive channels of a row
// (one 16-byte load) and the weights lie [k][cout][C], so the same four channels of a weight row are one 16-byte load too -- forward and backward read
// the same matrix, the backward with the taps' shifts negated.  Unconditional loads from clamped rows masked with pwr_keep, 64-bit row arithmetic, no
// atomics: the weight gradient leaves per-chunk partials of PWR_DW_CHUNK rows that pwr_dw_reduce_kernel adds in ascending chunk order.
// dpre = dwav (1 - wav^2) is formed where dwav is loaded and never stored.
#include "pwg_rows.h"

namespace fcl {

constexpr int HFE_ROWS = 64;     // rows per workgroup of the forward: four lanes per row
constexpr int HFE_MAX_COUT = 4;  // output channels

__device__ __forceinline__ float hfe_lrelu(float v, float slope) { return v * (v > 0.f ? 1.f : slope); }
__device__ __forceinline__ float hfe_dpre(float dwav, float wav) { return dwav * (1.f - wav * wav); }

// ---- forward: wav[t, o] = tanh(b[o] + sum_j sum_ch l(x)[t + j - h, ch] w[j][o][ch]).  Lane `part` of a row's four takes the channels 16 i + 4 part .. + 3
// of every tap in ascending (tap, i) order, then two exchanges add the four lanes.
template <int CO>
__global__ __launch_bounds__(256) void hfe_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int C, int k,
                                                      float slope, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                      float* __restrict__ wav, long long n) {
    const int part = threadIdx.x & 3;
    const long long t = (long long)blockIdx.x * HFE_ROWS + (threadIdx.x >> 2);
    if (t >= n) return;  // (a row's four lanes leave together)
    long long lo, hi;
    pwr_bounds(seg_lo, seg_hi, t, n, lo, hi);
    const int h = (k - 1) >> 1, nq = C >> 4;
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.f;
    for (int j = 0; j < k; ++j) {
        const long long arow = t + j - h;
        const bool ok = arow >= lo && arow < hi;
        const float* src = x + min(max(arow, 0LL), n - 1) * C + 4 * part;
        const float* wj = w + (size_t)j * CO * C + 4 * part;
        for (int i = 0; i < nq; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + 16 * i);
            float a[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = pwr_keep(hfe_lrelu(v[s], slope), ok);
#pragma unroll
            for (int o = 0; o < CO; ++o) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wj + (size_t)o * C + 16 * i);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[o] = fmaf(a[s], wv[s], acc[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
        acc[o] += __shfl_xor(acc[o], 1, 64);
        acc[o] += __shfl_xor(acc[o], 2, 64);
    }
    if (part == 0) {
#pragma unroll
        for (int o = 0; o < CO; ++o) wav[t * CO + o] = tanhf(acc[o] + bias[o]);
    }
}

// ---- input gradient: dx[t, ch] = m(x[t, ch]) sum_j sum_o dpre[t - (j - h), o] w[j][o][ch].  A lane owns four channels of one row.
template <int CO>
__global__ __launch_bounds__(256) void hfe_dx_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ wav,
                                                     const float* __restrict__ dwav, int C, int k, float slope, const int32_t* __restrict__ seg_lo,
                                                     const int32_t* __restrict__ seg_hi, float* __restrict__ dx, long long n) {
    const int nq4 = C >> 2;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long t = e / nq4;
    if (t >= n) return;
    const int q4 = (int)(e - t * nq4);
    long long lo, hi;
    pwr_bounds(seg_lo, seg_hi, t, n, lo, hi);
    const int h = (k - 1) >> 1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
        const long long grow = t - (j - h), gc = min(max(grow, 0LL), n - 1);
        const bool ok = grow >= lo && grow < hi;
#pragma unroll
        for (int o = 0; o < CO; ++o) {
            const float d = pwr_keep(hfe_dpre(dwav[gc * CO + o], wav[gc * CO + o]), ok);
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + ((size_t)j * CO + o) * C + 4 * q4);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = fmaf(d, wv[s], acc[s]);
        }
    }
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + t * C + 4 * q4);
    f32x4 out;
#pragma unroll
    for (int s = 0; s < 4; ++s) out[s] = acc[s] * (xv[s] > 0.f ? 1.f : slope);
    *reinterpret_cast<f32x4*>(dx + t * C + 4 * q4) = out;
}

// ---- weight and bias gradient: partial[chunk][j][o][ch] = sum over the chunk's rows t of dpre[t, o] l(x)[t + j - h, ch], then partial[chunk][k cout C + o] =
// sum_t dpre[t, o].  blockIdx.x is the chunk, blockIdx.y the tap.  The 256 threads are C / 4 channel quads x 1 024 / C row groups; a thread sums its rows
// (row groups apart, ascending), then thread e adds the row groups in ascending order through LDS.
template <int CO>
__global__ __launch_bounds__(256) void hfe_dw_kernel(const float* __restrict__ x, const float* __restrict__ wav, const float* __restrict__ dwav, int C, int k,
                                                     float slope, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                     float* __restrict__ partial, long long n) {
    __shared__ float red[1024 * CO];  // [row group][o][C]
    __shared__ float redb[64 * CO];   // [row group][o]
    const int nq4 = C >> 2, groups = 256 / nq4;
    const int q4 = threadIdx.x % nq4, rg = threadIdx.x / nq4;
    const int j = blockIdx.y, sh = j - ((k - 1) >> 1);
    const long long t_begin = (long long)blockIdx.x * PWR_DW_CHUNK, t_end = min(n, t_begin + PWR_DW_CHUNK);
    float acc[CO][4], bs[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) {
        bs[o] = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[o][s] = 0.f;
    }
    // (C / 4 need not divide 256: the threads past the last whole row group idle)
    for (long long t = rg < groups ? t_begin + rg : t_end; t < t_end; t += groups) {
        long long lo, hi;
        pwr_bounds(seg_lo, seg_hi, t, n, lo, hi);
        const long long arow = t + sh;
        const bool ok = arow >= lo && arow < hi;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + min(max(arow, 0LL), n - 1) * C + 4 * q4);
        float a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = pwr_keep(hfe_lrelu(v[s], slope), ok);
#pragma unroll
        for (int o = 0; o < CO; ++o) {
            const float d = hfe_dpre(dwav[t * CO + o], wav[t * CO + o]);
            bs[o] += d;
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[o][s] = fmaf(d, a[s], acc[o][s]);
        }
    }
    if (rg < groups) {
#pragma unroll
        for (int o = 0; o < CO; ++o) {
#pragma unroll
            for (int s = 0; s < 4; ++s) red[(rg * CO + o) * C + 4 * q4 + s] = acc[o][s];
            if (q4 == 0) redb[rg * CO + o] = bs[o];
        }
    }
    __syncthreads();
    const size_t nw = (size_t)k * CO * C;
    float* out = partial + (size_t)blockIdx.x * (nw + CO);
    for (int e = threadIdx.x; e < CO * C; e += 256) {
        float sum = 0.f;
        for (int g = 0; g < groups; ++g) sum += red[g * CO * C + e];
        out[(size_t)j * CO * C + e] = sum;
    }
    if (j == 0 && (int)threadIdx.x < CO) {
        float sum = 0.f;
        for (int g = 0; g < groups; ++g) sum += redb[g * CO + threadIdx.x];
        out[nw + threadIdx.x] = sum;
    }
}

static int hfe_check(const fcl_hfe_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->slope >= 0.f && a->slope < 1.f, FCL_ERR_INVALID, "%s: slope must be in [0, 1) (got %g)", who, (double)a->slope);
    FCL_REQUIRE(a->cin >= 16 && a->cin <= 256 && a->cin % 16 == 0, FCL_ERR_SHAPE, "%s: cin must be a multiple of 16 from 16 to 256 (got %d)", who, a->cin);
    FCL_REQUIRE(a->cout >= 1 && a->cout <= HFE_MAX_COUT, FCL_ERR_SHAPE, "%s: cout must be 1 to %d (got %d)", who, HFE_MAX_COUT, a->cout);
    FCL_REQUIRE(a->ksize == 3 || a->ksize == 5 || a->ksize == 7 || a->ksize == 11, FCL_ERR_SHAPE, "%s: kernel size must be 3, 5, 7 or 11 (got %d)", who,
                a->ksize);
    FCL_REQUIRE(a->rows >= 1 && a->rows < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= rows < 2^31 expected (got %lld)", who, (long long)a->rows);
    FCL_REQUIRE(a->seg_lo && a->seg_hi, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi", who);
    return FCL_OK;
}

#define HFE_COUT(CALL)          \
    switch (a->cout) {          \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        default: CALL(4); break; \
    }

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_hfe_workspace_bytes(int64_t rows, int cin, int cout, int ksize) {
    if (rows < 1 || cin < 1 || cout < 1 || ksize < 1) return 0;
    return (size_t)pwr_chunks(rows) * ((size_t)ksize * cin + 1) * cout * sizeof(float);
}

int fcl_hfe_fwd(const fcl_hfe_t* a, fcl_stream_t stream) {
    const int rc = hfe_check(a, "hfe_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->bias && a->wav, FCL_ERR_INVALID, "hfe_fwd: null x / w / bias / wav");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w), FCL_ERR_ALIGN, "hfe_fwd: x and w must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows;
    const dim3 grid((unsigned)((n + HFE_ROWS - 1) / HFE_ROWS));
    ProfScope ps("hfe_fwd_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
#define HFE_CALL(CO) \
    hipLaunchKernelGGL(hfe_fwd_kernel<CO>, grid, dim3(256), 0, s, a->x, a->w, a->bias, a->cin, a->ksize, a->slope, a->seg_lo, a->seg_hi, a->wav, n)
    HFE_COUT(HFE_CALL)
#undef HFE_CALL
    return check_hip(hipGetLastError(), "hfe_fwd");
}

int fcl_hfe_dx(const fcl_hfe_t* a, fcl_stream_t stream) {
    const int rc = hfe_check(a, "hfe_dx");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->wav && a->dwav && a->dx, FCL_ERR_INVALID, "hfe_dx: null x / w / wav / dwav / dx");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w) && aligned16(a->dx), FCL_ERR_ALIGN, "hfe_dx: x, w and dx must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows, lanes = n * (a->cin / 4);
    const dim3 grid((unsigned)((lanes + 255) / 256));
    ProfScope ps("hfe_dx_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
#define HFE_CALL(CO) \
    hipLaunchKernelGGL(hfe_dx_kernel<CO>, grid, dim3(256), 0, s, a->x, a->w, a->wav, a->dwav, a->cin, a->ksize, a->slope, a->seg_lo, a->seg_hi, a->dx, n)
    HFE_COUT(HFE_CALL)
#undef HFE_CALL
    return check_hip(hipGetLastError(), "hfe_dx");
}

int fcl_hfe_dw(const fcl_hfe_t* a, fcl_stream_t stream) {
    const int rc = hfe_check(a, "hfe_dw");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->wav && a->dwav && a->dw && a->db && a->workspace, FCL_ERR_INVALID, "hfe_dw: null x / wav / dwav / dw / db / workspace");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->workspace), FCL_ERR_ALIGN, "hfe_dw: x and workspace must be 16-byte aligned");
    const size_t need = fcl_hfe_workspace_bytes(a->rows, a->cin, a->cout, a->ksize);
    FCL_REQUIRE(a->workspace_bytes >= need, FCL_ERR_WORKSPACE, "hfe_dw: the workspace holds %zu bytes, fcl_hfe_workspace_bytes asks for %zu",
                a->workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows;
    const int chunks = (int)pwr_chunks(n), nw = a->ksize * a->cout * a->cin;
    {
        const dim3 grid((unsigned)chunks, (unsigned)a->ksize);
        ProfScope ps("hfe_dw_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
#define HFE_CALL(CO) \
    hipLaunchKernelGGL(hfe_dw_kernel<CO>, grid, dim3(256), 0, s, a->x, a->wav, a->dwav, a->cin, a->ksize, a->slope, a->seg_lo, a->seg_hi, a->workspace, n)
        HFE_COUT(HFE_CALL)
#undef HFE_CALL
    }
    ProfScope ps("hfe_dw_reduce_kernel", 0.0, (double)chunks, s);
    hipLaunchKernelGGL(pwr_dw_reduce_kernel, dim3((unsigned)((nw + a->cout + 255) / 256)), dim3(256), 0, s, a->workspace, chunks, nw, a->cout, a->dw, a->db);
    return check_hip(hipGetLastError(), "hfe_dw");
}

}  // extern "C"
