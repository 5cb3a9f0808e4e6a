// hfd_rows.h -- what the two HiFi-GAN discriminator files share, once, on top of pwg_rows.h: hifigan_disc.hip (the period discriminator) and
// hifigan_sdisc.hip (the scale discriminator) keep their C -> C' kernels, their layer rules and their entries and take from here the
// table-driven row descriptor, the LeakyReLU mask, the width rules, the common argument checks, the pipelined MFMA loop (the scale file's two kernels; the
// period file's measured slower through it and keep theirs), the 1 -> C forward, the C -> 1 strided adjoint, the small weight-gradient kernel and the
// launch of the chunk-order reduce (which also says why the chunked C -> C' weight gradient stays one kernel per file).
//
// Layout as pwg_rows.h: float32, channel-last, packed [rows, C].  The segments of a level lie back to back and every level has its own row count, so the
// geometry is table-driven, per OUTPUT row t: src[t] is the input row under the centre of the kernel (in_lo + stride x the row's index in its segment) and
// [in_lo[t], in_hi[t]) the input segment.  Tap j reads input row src[t] + j - pad; a tap outside the segment contributes zero.  The output segment follows
// from the three tables: it holds (in_hi - in_lo + 2 pad - k) / stride + 1 rows and starts (src - in_lo) / stride rows before t.
// The kernels are static (or templates of internal linkage): one copy per including file, launched under that file's record names.
#pragma once
#include "pwg_rows.h"

namespace fcl {

constexpr int HFD_SMALL_GROUPS = 8;  // row groups of hfd_dw_small_kernel (1024 threads)

// d LeakyReLU / d pre-activation from the stored post-activation; h == 0 takes the slope, as torch does
__device__ __forceinline__ float hfd_mask(float h, float slope) { return h > 0.f ? 1.f : slope; }

// what a row kernel needs to know about output row t (all zero past the end, so that every tap is masked away and nothing is stored)
struct HfdRow {
    long long src, lo, hi;  // the input row under tap `pad`, the input segment (clamped to [0, rows_in])
    long long olo, ohi;     // the output segment
};

__device__ __forceinline__ HfdRow hfd_row(const int32_t* __restrict__ src, const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi, long long t,
                                          long long n, long long rows_in, int ksize, int stride, int pad) {
    HfdRow R = {0, 0, 0, 0, 0};
    if (t < n) {
        const long long lo = in_lo[t], hi = in_hi[t];
        R.src = src[t];
        R.lo = max(0LL, lo);
        R.hi = min(rows_in, hi);
        R.olo = max(0LL, t - (R.src - lo) / stride);
        R.ohi = min(n, R.olo + (hi - lo + 2 * pad - ksize) / stride + 1);
    }
    return R;
}

// The pipelined contraction of a wave's 32 rows x 16 NT columns: fetch(step, a, ok, b) requests the operands of one step of 16 contraction rows (a[mt]: 4
// consecutive channels of the lane's row of tile mt, ok[mt]: whether that row counts, b[s][nt]: the weights of MFMA s).  The operands of step s + 1 are
// requested before the MFMAs of step s (the last step requests itself again); every load is unconditional, from a clamped row, and what an outside row
// loaded is replaced by zero.  steps == 0 requests step 0 and runs nothing.
template <int NT, class Fetch>
__device__ __forceinline__ void hfd_mma_loop(int steps, const Fetch& fetch, f32x4 (&acc)[2][NT]) {
    f32x4 a0[2];
    bool ok0[2];
    float b0[4][NT];
    fetch(0, a0, ok0, b0);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int s = 0; s < 4; ++s) a0[mt][s] = pwr_keep(a0[mt][s], ok0[mt]);
    for (int step = 0; step < steps; ++step) {
        f32x4 a1[2];
        bool ok1[2];
        float b1[4][NT];
        fetch(min(step + 1, steps - 1), a1, ok1, b1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[mt][s], b0[s][nt], acc[mt][nt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int s = 0; s < 4; ++s) a0[mt][s] = pwr_keep(a1[mt][s], ok1[mt]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b0[s][nt] = b1[s][nt];
    }
}

// ---- 1 -> C forward (the first layer): y[t, c] = lrelu(bias[c] + sum_j s[src[t] + j - pad] w[j][c]); an item is (output row, 4 channels)
static __global__ __launch_bounds__(256) void hfd_expand_fwd_kernel(const float* __restrict__ s, const float* __restrict__ w, const float* __restrict__ bias,
                                                                    const int32_t* __restrict__ src, const int32_t* __restrict__ in_lo,
                                                                    const int32_t* __restrict__ in_hi, float* __restrict__ y, long long n, long long rows_in,
                                                                    int c, int ksize, int stride, int pad, float slope) {
    const int cq = c >> 2;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n * cq) return;
    const long long t = i / cq;
    const int ch = (int)(i - t * cq) * 4;
    const HfdRow R = hfd_row(src, in_lo, in_hi, t, n, rows_in, ksize, stride, pad);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < ksize; ++j) {
        const long long rr = R.src + j - pad;
        const float sv = (rr >= R.lo && rr < R.hi) ? s[rr] : 0.f;
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)j * c + ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(sv, wv[e], v[e]);
    }
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float u = v[e] + (bias ? bias[ch + e] : 0.f);
        o[e] = u > 0.f ? u : u * slope;
    }
    *reinterpret_cast<f32x4*>(y + t * c + ch) = o;
}

// ---- C -> 1 adjoint (the first layer's input gradient: the waveform gradient) with the strided adjoint's tap rule: 16 lanes per (output row t, phase ph);
// y[src[t] + ph] = sum_i sum_c g[t + c0 - i, c] w[j0 + stride i][c], j0 = (ph + pad) % stride, c0 = (ph + pad) / stride
static __global__ __launch_bounds__(256) void hfd_reduce_dx_kernel(const float* __restrict__ g, const float* __restrict__ w, const int32_t* __restrict__ src,
                                                                   const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi,
                                                                   float* __restrict__ y, long long n, long long rows_in, int c, int ksize, int stride,
                                                                   int pad) {
    const int sub = threadIdx.x & 15;
    const long long item = blockIdx.x * 16LL + (threadIdx.x >> 4);
    const long long t = item / stride;
    const int ph = (int)(item - t * stride);
    const HfdRow R = hfd_row(src, in_lo, in_hi, t, n, rows_in, ksize, stride, pad);
    const int c0 = (ph + pad) / stride, j0 = (ph + pad) - c0 * stride;
    float acc = 0.f;
    for (int j = j0, i = 0; j < ksize; j += stride, ++i) {
        const long long rr = t + c0 - i;
        if (rr < R.olo || rr >= R.ohi) continue;
        for (int ch = 4 * sub; ch < c; ch += 64) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + rr * c + ch), wv = *reinterpret_cast<const f32x4*>(w + (size_t)j * c + ch);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(gv[e], wv[e], acc);
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    const long long row = R.src + ph;
    if (sub == 0 && row >= R.lo && row < R.hi) y[row] = acc;
}

// ---- weight gradient of the 1 -> C and C -> 1 layers, one chunk's partial per (workgroup, block of 128 channels) in the forward layout.
// VEC_SHIFTED = 0 (first layer, cin 1): vec = g [n, c], sc = x [rows_in]: partial[j][ch] = sum_t sc[src[t] + j - pad] vec[t, ch], row k = sum_t vec[t, ch].
// VEC_SHIFTED = 1 (score layer, cout 1): vec = x [rows_in, c], sc = g [n]: partial[j c + ch] = sum_t vec[src[t] + j - pad, ch] sc[t], element k c = sum_t sc[t].
// Thread = (channel, one of 8 row groups taking every 8th row); the groups' sums meet in LDS and are added in ascending group order.
template <int VEC_SHIFTED, int KSIZE>
static __global__ __launch_bounds__(1024) void hfd_dw_small_kernel(const float* __restrict__ vec, const float* __restrict__ sc, const int32_t* __restrict__ src,
                                                                   const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi,
                                                                   float* __restrict__ partial, long long n, long long rows_in, int c, int pad) {
    constexpr int UNROLL = KSIZE > 5 ? 2 : 4;  // rows per register set: the taps of a row are registers too
    __shared__ float red[HFD_SMALL_GROUPS - 1][(KSIZE + 1) * 128];
    const int lch = threadIdx.x & 127, grp = threadIdx.x >> 7;
    const int ch = blockIdx.y * 128 + lch;
    const int chc = min(ch, c - 1);  // (the threads past the width load a valid channel and store nothing)
    const long long t_begin = (long long)blockIdx.x * PWR_DW_CHUNK, t_end = min(n, t_begin + PWR_DW_CHUNK);
    const long long last = t_end - 1, alast = rows_in - 1;
    float acc[KSIZE + 1];
#pragma unroll
    for (int j = 0; j <= KSIZE; ++j) acc[j] = 0.f;
    for (int it0 = 0; it0 < PWR_DW_CHUNK / HFD_SMALL_GROUPS; it0 += UNROLL) {
        int at[UNROLL], lo[UNROLL], hi[UNROLL];
        float ov[UNROLL], xv[UNROLL][KSIZE];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long long t = t_begin + (long long)(it0 + u) * HFD_SMALL_GROUPS + grp, tc = min(t, last);
            at[u] = src[tc];
            lo[u] = in_lo[tc];
            hi[u] = in_hi[tc];
            ov[u] = VEC_SHIFTED ? sc[tc] : vec[tc * c + chc];
#pragma unroll
            for (int j = 0; j < KSIZE; ++j) {
                const long long rc = min(max((long long)at[u] + j - pad, 0LL), alast);
                xv[u][j] = VEC_SHIFTED ? vec[rc * c + chc] : sc[rc];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long long t = t_begin + (long long)(it0 + u) * HFD_SMALL_GROUPS + grp;
            const bool live = t <= last;
            const long long l = max(0, lo[u]), h = min(rows_in, (long long)hi[u]);
            const float own = pwr_keep(ov[u], live);
#pragma unroll
            for (int j = 0; j < KSIZE; ++j) {
                const long long rr = (long long)at[u] + j - pad;
                acc[j] = fmaf(pwr_keep(xv[u][j], live && rr >= l && rr < h), own, acc[j]);
            }
            acc[KSIZE] += own;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (grp > 0) {
#pragma unroll
        for (int j = 0; j <= KSIZE; ++j) red[grp - 1][j * 128 + lch] = acc[j];
    }
    __syncthreads();
    if (grp == 0 && ch < c) {
#pragma unroll
        for (int j = 0; j <= KSIZE; ++j)
#pragma unroll
            for (int k = 0; k < HFD_SMALL_GROUPS - 1; ++k) acc[j] += red[k][j * 128 + lch];
        float* out = partial + (size_t)blockIdx.x * (VEC_SHIFTED ? (size_t)KSIZE * c + 1 : ((size_t)KSIZE + 1) * c);
#pragma unroll
        for (int j = 0; j < KSIZE; ++j) out[(size_t)j * c + ch] = acc[j];
        if (!VEC_SHIFTED || ch == 0) out[(size_t)KSIZE * c + (VEC_SHIFTED ? 0 : ch)] = acc[KSIZE];
    }
}

static bool hfd_width_ok(int c) { return c >= 16 && c <= 1024 && c % 16 == 0; }
static int hfd_nt(int cols) { return cols % 64 == 0 ? 4 : cols % 32 == 0 ? 2 : 1; }

#define HFD_TILES(NTV, CALL)     \
    switch (NTV) {               \
        case 1: CALL(1); break;  \
        case 2: CALL(2); break;  \
        default: CALL(4); break; \
    }

// what every layer entry of both files checks, in this order: the struct, the file's own rules (`rules(a, who)`: the layer class, the groups, the kernel
// size, the stride, the padding), the rows, the slope, the tables
template <class Args, class Rules>
static int hfd_check(const Args* a, const char* who, Rules rules) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    const int rc = rules(a, who);
    if (rc) return rc;
    FCL_REQUIRE(a->rows_in >= 1 && a->rows_in < 0x7fffffffLL && a->rows_out >= 1 && a->rows_out < 0x7fffffffLL, FCL_ERR_SHAPE,
                "%s: 1 <= rows < 2^31 expected (got %lld in, %lld out)", who, (long long)a->rows_in, (long long)a->rows_out);
    FCL_REQUIRE(a->slope >= 0.f && a->slope < 1.f, FCL_ERR_INVALID, "%s: 0 <= slope < 1 expected (got %g)", who, (double)a->slope);
    FCL_REQUIRE(a->src && a->in_lo && a->in_hi, FCL_ERR_INVALID, "%s: null src / in_lo / in_hi", who);
    return FCL_OK;
}

// the chunk-order reduce of a layer's weight-gradient partials, under the calling file's record name
template <class Args>
static void hfd_launch_dw_reduce(const Args* a, int cig, const char* name, hipStream_t s) {
    const int chunks = (int)pwr_chunks(a->rows_out), nw = a->ksize * cig * a->cout, nb = a->cout;
    ProfScope ps(name, 0.0, (double)chunks, s);
    hipLaunchKernelGGL(pwr_dw_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, a->workspace, chunks, nw, nb, a->dw, a->db);
}

}  // namespace fcl
