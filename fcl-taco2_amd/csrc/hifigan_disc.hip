// hifigan_disc.hip -- the HiFi-GAN period discriminator: a stack of strided (k, 1) convolutions + LeakyReLU on the waveform folded by its period, forward
// and backward (include/fcl_hip.h "HiFi-GAN period discriminator"; fcl_taco2_amd/hifigan_discriminator.py; restated in float64 numpy in
// tests/hfgd_ref.py).
//
// Layout and table-driven row geometry as hfd_rows.h: float32, channel-last, packed [rows, C].  A period p turns an utterance into p segments (one per
// phase of the period), the segments lie back to back, and the (k, 1) convolution is a plain 1-D convolution along each segment; no value crosses a
// segment boundary.
// Exact fp32, the C -> C contractions on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain), unconditional loads from clamped rows masked with pwr_keep,
// tile counts as template arguments, 64-bit row arithmetic, no atomics.  The row descriptor, the first layer's forward and waveform gradient and the
// small weight-gradient kernel are those of hfd_rows.h, shared with hifigan_sdisc.hip; the C -> C loops here are local forms of hft_conv_kernel /
// hft_dw_kernel with the table-driven row geometry: through hfd_mma_loop, and through the grouped weight-gradient kernel with one group, they measured
// slower (as 6n found for the neighbours' kernels).
#include "hfd_rows.h"

namespace fcl {

enum { HPD_BIAS = 0, HPD_NOBIAS = 1 };

// ---- C -> C forward: y[t, co] = lrelu(bias[co] + sum_j sum_ci x[src[t] + j - pad, ci] w[j][ci][co]).  The shape of hft_conv_kernel: a workgroup owns 128
// output rows x 16 NT columns (blockIdx.y: the column block), a wave 32 rows: 2 x NT accumulator tiles.  A lane loads 4 consecutive input channels of
// its row at once and feeds them to 4 MFMAs, so the contraction index of MFMA s of a 16-channel block is block + 4 (lane >> 4) + s on both operands.
template <int NT, int EPI>
__global__ __launch_bounds__(256) void hpd_conv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const int32_t* __restrict__ src, const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi,
                                                       float* __restrict__ y, long long n, long long rows_in, int cin, int cout, int ksize, int stride, int pad,
                                                       float slope) {
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    const int col0 = blockIdx.y * NT * 16;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    long long centre[2], lo[2], hi[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const HfdRow R = hfd_row(src, in_lo, in_hi, t0 + mt * 16 + r, n, rows_in, ksize, stride, pad);
        centre[mt] = R.src - pad, lo[mt] = R.lo, hi[mt] = R.hi;
    }
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int ncb = cin >> 4, steps = ksize * ncb;
    const long long last = rows_in - 1;
    // as pwr_contract: a step is 16 contraction rows; the operands of step s + 1 are requested before the MFMAs of step s (the last step requests itself
    // again); every load is unconditional, from a clamped row, and what an outside row loaded is replaced by zero
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const int j = step / ncb, cb = (step - j * ncb) << 4;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = centre[mt] + j;
            a[mt] = *reinterpret_cast<const f32x4*>(x + min(max(arow, 0LL), last) * cin + cb + 4 * q);
            ok[mt] = arow >= lo[mt] && arow < hi[mt];
        }
        const float* wr = w + ((size_t)step * 16 + 4 * q) * cout + col0 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[s][nt] = wr[(size_t)s * cout + nt * 16];
    };
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
    // results in the C / D layout: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = col0 + nt * 16 + r;
        const float bv = EPI == HPD_BIAS ? bias[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long row = t0 + mt * 16 + 4 * q + reg;
                if (row >= n) continue;
                const float v = acc[mt][nt][reg] + bv;
                y[row * cout + col] = v > 0.f ? v : v * slope;
            }
    }
}

// ---- C -> C input gradient, the adjoint of the strided convolution in gather form: input row h = stride m + ph of a segment collects
// g[m + c - i] Wb[ph][i] over i = 0 .. ceil((k - j0) / stride) - 1, where j0 = (ph + pad) % stride is the phase's first tap, c = (ph + pad) / stride, and
// Wb[ph][i][co][ci] = W[co][ci][j0 + stride i] (slots past the kernel are zero and never read beyond slot 0).  The rows run at the coarse (output) rate:
// row t of the tables is m of its segment, blockIdx.z the phase ph, and the stored row is src[t] + ph where that lies inside the input segment.
// y = m(hin) (acc + extra): hin [rows_in, cin] the stored post-activation of the layer's input, extra [rows_in, cin] (or null) the gradient that arrives
// at that feature map directly.  Here cg = the forward's cout is the contraction width and cw = the forward's cin the output width.
template <int NT>
__global__ __launch_bounds__(256) void hpd_conv_dx_kernel(const float* __restrict__ g, const float* __restrict__ wb, const float* __restrict__ hin,
                                                          const float* __restrict__ extra, const int32_t* __restrict__ src,
                                                          const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi, float* __restrict__ y,
                                                          long long n, long long rows_in, int cg, int cw, int ksize, int stride, int pad, int slots,
                                                          float slope) {
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    const int col0 = blockIdx.y * NT * 16;
    const int ph = blockIdx.z;
    const int c = (ph + pad) / stride, j0 = (ph + pad) - c * stride;
    const int ntaps = j0 < ksize ? (ksize - j0 + stride - 1) / stride : 0;
    wb += (size_t)ph * slots * cg * cw + col0;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    long long top[2], lo[2], hi[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const long long t = t0 + mt * 16 + r;
        const HfdRow R = hfd_row(src, in_lo, in_hi, t, n, rows_in, ksize, stride, pad);
        top[mt] = t + c, lo[mt] = R.olo, hi[mt] = R.ohi;
    }
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int ncb = cg >> 4, steps = ntaps * ncb;
    const long long last = n - 1;
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const int i = step / ncb, cb = (step - i * ncb) << 4;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = top[mt] - i;
            a[mt] = *reinterpret_cast<const f32x4*>(g + min(max(arow, 0LL), last) * cg + cb + 4 * q);
            ok[mt] = arow >= lo[mt] && arow < hi[mt];
        }
        const float* wr = wb + ((size_t)step * 16 + 4 * q) * cw + r;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[s][nt] = wr[(size_t)s * cw + nt * 16];
    };
    f32x4 a0[2];
    bool ok0[2];
    float b0[4][NT];
    fetch(0, a0, ok0, b0);  // (a phase without taps: slot 0 exists, holds zeros, and the loop below does not run)
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
    // the rows this lane stores are those of its accumulator registers, not the one it loaded for: their geometry is read again
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const long long t = t0 + mt * 16 + 4 * q + reg;
            const HfdRow R = hfd_row(src, in_lo, in_hi, t, n, rows_in, ksize, stride, pad);
            const long long row = R.src + ph;
            if (row < R.lo || row >= R.hi) continue;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const size_t at = (size_t)row * cw + col0 + nt * 16 + r;
                float v = acc[mt][nt][reg];
                if (extra) v += extra[at];
                y[at] = v * hfd_mask(hin[at], slope);
            }
        }
}

// ---- C -> C weight gradients, as hft_dw_kernel with the table-driven A row and a column block per blockIdx.z:
// partial[chunk][j cin + ci][co] = sum over the chunk's output rows t of x[src[t] + j - pad, ci] g[t, co], followed by one row sum_t g[t, co] for the bias (an
// A operand of ones in row 0 of a tile).  A wave owns 16 contraction rows x 16 NT columns; blockIdx.x is the chunk of PWR_DW_CHUNK output rows,
// blockIdx.y * 4 + wave the contraction tile.  No barrier in the kernel: an idle wave returns.
template <int NT>
__global__ __launch_bounds__(256) void hpd_dw_kernel(const float* __restrict__ x, const float* __restrict__ g, const int32_t* __restrict__ src,
                                                     const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi, float* __restrict__ partial,
                                                     long long n, long long rows_in, int cin, int cout, int ksize, int pad) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int mt1 = cin >> 4, tiles = ksize * mt1;
    const int combo = blockIdx.y * 4 + wave;
    if (combo > tiles) return;
    const bool ones = combo == tiles;
    const int j = ones ? 0 : combo / mt1, mt = ones ? 0 : combo - j * mt1;
    const int col0 = blockIdx.z * NT * 16;
    const long long shift = j - pad;
    const long long t_begin = (long long)blockIdx.x * PWR_DW_CHUNK, t_end = min(n, t_begin + PWR_DW_CHUNK);
    const long long last = t_end - 1, alast = rows_in - 1;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    struct Group {
        int at[PWR_DW_GROUP], lo[PWR_DW_GROUP], hi[PWR_DW_GROUP];
        float av[PWR_DW_GROUP], bv[PWR_DW_GROUP][NT];
    };
    // groups of PWR_DW_GROUP steps, two register sets: the loads of group i + 1 are all issued before the MFMAs of group i.  The A row depends on the
    // table, so the table entry is loaded first and the activation from it; every load is unconditional, from a clamped row, and masked afterwards.
    auto issue = [&](int grp, Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, tc = min(tq, last);
            G.at[u] = src[tc];
            G.lo[u] = in_lo[tc];
            G.hi[u] = in_hi[tc];
            G.av[u] = x[min(max(G.at[u] + shift, 0LL), alast) * cin + mt * 16 + r];
            const float* bs = g + tc * cout + col0 + r;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) G.bv[u][nt] = bs[nt * 16];
        }
    };
    auto compute = [&](int grp, const Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, ar = G.at[u] + shift;
            const bool live = tq <= last;
            const long long lo = max(0, G.lo[u]), hi = min(rows_in, (long long)G.hi[u]);
            // (branch-free: the row of ones OR the masked activation, never a select between a loaded value and a constant)
            const float a = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, pwr_keep(G.av[u], !ones && live && ar >= lo && ar < hi)) |
                                                          ((ones && live && r == 0) ? 0x3F800000u : 0u));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pwr_keep(G.bv[u][nt], live), acc[nt], 0, 0, 0);
        }
    };
    constexpr int groups = PWR_DW_CHUNK / 4 / PWR_DW_GROUP;  // even
    Group G0, G1;
    issue(0, G0);
    for (int grp = 0; grp < groups; grp += 2) {
        issue(grp + 1, G1);
        __builtin_amdgcn_sched_barrier(0);
        compute(grp, G0);
        __builtin_amdgcn_sched_barrier(0);
        issue(grp + 2, G0);  // (past the last group: clamped rows, never used)
        __builtin_amdgcn_sched_barrier(0);
        compute(grp + 1, G1);
        __builtin_amdgcn_sched_barrier(0);
    }
    float* out = partial + (size_t)blockIdx.x * ((size_t)tiles * 16 + 1) * cout + col0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int m = 4 * q + reg;
            if (ones) {
                if (m == 0) out[(size_t)tiles * 16 * cout + nt * 16 + r] = acc[nt][reg];
            } else {
                out[((size_t)combo * 16 + m) * cout + nt * 16 + r] = acc[nt][reg];
            }
        }
    }
}

// ---- 1 -> C adjoint (the score layer's input gradient, stride 1): y[h, c] = m(hin[h, c]) (sum_j g[t + pad - j] w[j][c] + extra[h, c]) for h = src[t] where
// that lies inside the input segment (the score map may have more rows than its input); an item is (output row, 4 channels)
__global__ __launch_bounds__(256) void hpd_expand_dx_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ hin,
                                                            const float* __restrict__ extra, const int32_t* __restrict__ src,
                                                            const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi, float* __restrict__ y,
                                                            long long n, long long rows_in, int c, int ksize, int pad, float slope) {
    const int cq = c >> 2;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n * cq) return;
    const long long t = i / cq;
    const int ch = (int)(i - t * cq) * 4;
    const HfdRow R = hfd_row(src, in_lo, in_hi, t, n, rows_in, ksize, 1, pad);
    if (R.src < R.lo || R.src >= R.hi) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < ksize; ++j) {
        const long long rr = t + pad - j;
        const float gv = (rr >= R.olo && rr < R.ohi) ? g[rr] : 0.f;
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)j * c + ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(gv, wv[e], v[e]);
    }
    const size_t at = (size_t)R.src * c + ch;
    const f32x4 hv = *reinterpret_cast<const f32x4*>(hin + at);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e];
    if (extra) {
        const f32x4 ev = *reinterpret_cast<const f32x4*>(extra + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += ev[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] *= hfd_mask(hv[e], slope);
    *reinterpret_cast<f32x4*>(y + at) = o;
}

// ---- C -> 1 forward (the score layer): y[t] = bias + sum_j sum_c x[src[t] + j - pad, c] w[j][c]; 16 lanes per output row, a fixed butterfly
__global__ __launch_bounds__(256) void hpd_reduce_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             const int32_t* __restrict__ src, const int32_t* __restrict__ in_lo,
                                                             const int32_t* __restrict__ in_hi, float* __restrict__ y, long long n, long long rows_in, int c,
                                                             int ksize, int stride, int pad) {
    const int sub = threadIdx.x & 15;
    const long long t = blockIdx.x * 16LL + (threadIdx.x >> 4);
    const HfdRow R = hfd_row(src, in_lo, in_hi, t, n, rows_in, ksize, stride, pad);
    float acc = 0.f;
    for (int j = 0; j < ksize; ++j) {
        const long long rr = R.src + j - pad;
        if (rr < R.lo || rr >= R.hi) continue;
        for (int ch = 4 * sub; ch < c; ch += 64) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + rr * c + ch), wv = *reinterpret_cast<const f32x4*>(w + (size_t)j * c + ch);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(xv[e], wv[e], acc);
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (sub == 0 && t < n) y[t] = acc + (bias ? bias[0] : 0.f);
}

// the period discriminator's own rules inside hfd_check: the layer class (1 -> C, C -> C, C -> 1), the kernel size, the stride, the padding
static int hpd_rules(const fcl_hpd_t* a, const char* who) {
    const bool first = a->cin == 1 && hfd_width_ok(a->cout), mid = hfd_width_ok(a->cin) && hfd_width_ok(a->cout), last = a->cout == 1 && hfd_width_ok(a->cin);
    FCL_REQUIRE(first || mid || last, FCL_ERR_SHAPE, "%s: a layer is 1 -> C, C -> C' or C -> 1 with the widths multiples of 16 from 16 to 1024 (got cin %d, cout %d)",
                who, a->cin, a->cout);
    if (last)
        FCL_REQUIRE((a->ksize == 2 || a->ksize == 3) && a->stride == 1 && a->pad == 1, FCL_ERR_SHAPE,
                    "%s: the score layer has 2 or 3 taps, stride 1 and padding 1 (got %d, %d, %d)", who, a->ksize, a->stride, a->pad);
    else
        FCL_REQUIRE((a->ksize == 3 || a->ksize == 5) && a->stride >= 1 && a->stride <= 4 && a->pad == (a->ksize - 1) / 2, FCL_ERR_SHAPE,
                    "%s: kernel size 3 or 5, stride 1 to 4 and padding (k - 1) / 2 expected (got %d, %d, %d)", who, a->ksize, a->stride, a->pad);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_hpd_dw_workspace_bytes(int64_t rows_out, int cin, int cout, int ksize) {
    if (rows_out < 1 || cin < 1 || cout < 1 || ksize < 1) return 0;
    return (size_t)pwr_chunks(rows_out) * ((size_t)ksize * cin + 1) * cout * sizeof(float);
}

int fcl_hpd_layer_fwd(const fcl_hpd_t* a, fcl_stream_t stream) {
    const int rc = hfd_check(a, "hpd_layer_fwd", hpd_rules);
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->y, FCL_ERR_INVALID, "hpd_layer_fwd: null x / w / y");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w) && aligned16(a->y), FCL_ERR_ALIGN, "hpd_layer_fwd: x, w and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows_out, ni = a->rows_in;
    if (a->cin == 1) {
        ProfScope ps("hpd_expand_kernel<fwd>", 2.0 * a->ksize * a->cout * (double)n, (double)n, s);
        hipLaunchKernelGGL(hfd_expand_fwd_kernel, dim3((unsigned)((n * (a->cout / 4) + 255) / 256)), dim3(256), 0, s, a->x, a->w, a->bias, a->src, a->in_lo,
                           a->in_hi, a->y, n, ni, a->cout, a->ksize, a->stride, a->pad, a->slope);
    } else if (a->cout == 1) {
        ProfScope ps("hpd_reduce_kernel<fwd>", 2.0 * a->ksize * a->cin * (double)n, (double)n, s);
        hipLaunchKernelGGL(hpd_reduce_fwd_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, a->x, a->w, a->bias, a->src, a->in_lo, a->in_hi, a->y, n, ni,
                           a->cin, a->ksize, a->stride, a->pad);
    } else {
        const int nt = hfd_nt(a->cout);
        const dim3 grid((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS), (unsigned)(a->cout / (16 * nt)));
        ProfScope ps("hpd_conv_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
#define HPD_FWD_B(NN) \
    hipLaunchKernelGGL((hpd_conv_kernel<NN, HPD_BIAS>), grid, dim3(256), 0, s, a->x, a->w, a->bias, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cin, a->cout, a->ksize, a->stride, a->pad, a->slope)
#define HPD_FWD_N(NN) \
    hipLaunchKernelGGL((hpd_conv_kernel<NN, HPD_NOBIAS>), grid, dim3(256), 0, s, a->x, a->w, a->bias, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cin, a->cout, a->ksize, a->stride, a->pad, a->slope)
        if (a->bias) {
            HFD_TILES(nt, HPD_FWD_B)
        } else {
            HFD_TILES(nt, HPD_FWD_N)
        }
#undef HPD_FWD_B
#undef HPD_FWD_N
    }
    return check_hip(hipGetLastError(), "hpd_layer_fwd");
}

int fcl_hpd_layer_dx(const fcl_hpd_t* a, fcl_stream_t stream) {
    const int rc = hfd_check(a, "hpd_layer_dx", hpd_rules);
    if (rc) return rc;
    FCL_REQUIRE(a->g && a->w && a->y, FCL_ERR_INVALID, "hpd_layer_dx: null g / w / y");
    FCL_REQUIRE(a->cin == 1 ? (a->h == nullptr && a->extra == nullptr) : a->h != nullptr, FCL_ERR_INVALID,
                "hpd_layer_dx: h (the stored activation of the layer's input) is needed for cin > 1; h and extra have no meaning for the first layer");
    FCL_REQUIRE(aligned16(a->g) && aligned16(a->w) && aligned16(a->y) && aligned16(a->h) && aligned16(a->extra), FCL_ERR_ALIGN,
                "hpd_layer_dx: g, w, h, extra and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows_out, ni = a->rows_in;
    if (a->cin == 1) {
        const long long items = n * a->stride;
        ProfScope ps("hpd_reduce_kernel<dx>", 2.0 * a->ksize * a->cout * (double)n, (double)ni, s);
        hipLaunchKernelGGL(hfd_reduce_dx_kernel, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, s, a->g, a->w, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cout,
                           a->ksize, a->stride, a->pad);
    } else if (a->cout == 1) {
        ProfScope ps("hpd_expand_kernel<dx>", 2.0 * a->ksize * a->cin * (double)n, (double)ni, s);
        hipLaunchKernelGGL(hpd_expand_dx_kernel, dim3((unsigned)((n * (a->cin / 4) + 255) / 256)), dim3(256), 0, s, a->g, a->w, a->h, a->extra, a->src, a->in_lo,
                           a->in_hi, a->y, n, ni, a->cin, a->ksize, a->pad, a->slope);
    } else {
        const int nt = hfd_nt(a->cin), slots = (a->ksize + a->stride - 1) / a->stride;
        const dim3 grid((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS), (unsigned)(a->cin / (16 * nt)), (unsigned)a->stride);
        ProfScope ps("hpd_conv_dx_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)ni, s);
#define HPD_DX(NN) \
    hipLaunchKernelGGL((hpd_conv_dx_kernel<NN>), grid, dim3(256), 0, s, a->g, a->w, a->h, a->extra, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cout, a->cin, a->ksize, a->stride, a->pad, slots, a->slope)
        HFD_TILES(nt, HPD_DX)
#undef HPD_DX
    }
    return check_hip(hipGetLastError(), "hpd_layer_dx");
}

int fcl_hpd_layer_dw(const fcl_hpd_t* a, fcl_stream_t stream) {
    const int rc = hfd_check(a, "hpd_layer_dw", hpd_rules);
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->g && a->dw && a->workspace, FCL_ERR_INVALID, "hpd_layer_dw: null x / g / dw / workspace");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->g) && aligned16(a->workspace), FCL_ERR_ALIGN, "hpd_layer_dw: x, g and workspace must be 16-byte aligned");
    const size_t need = fcl_hpd_dw_workspace_bytes(a->rows_out, a->cin, a->cout, a->ksize);
    FCL_REQUIRE(a->workspace_bytes >= need, FCL_ERR_WORKSPACE, "hpd_layer_dw: the workspace holds %zu bytes, fcl_hpd_dw_workspace_bytes asks for %zu",
                a->workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows_out, ni = a->rows_in;
    const unsigned chunks = (unsigned)pwr_chunks(n);
    if (a->cin == 1 || a->cout == 1) {
        const bool first = a->cin == 1;
        const int c = first ? a->cout : a->cin;
        const float *vec = first ? a->g : a->x, *sc = first ? a->x : a->g;
        const dim3 grid(chunks, (unsigned)((c + 127) / 128));
        ProfScope ps(first ? "hpd_dw_small_kernel<first>" : "hpd_dw_small_kernel<score>", 2.0 * (a->ksize + 1) * c * (double)n, (double)n, s);
#define HPD_SMALL(V, K) hipLaunchKernelGGL((hfd_dw_small_kernel<V, K>), grid, dim3(1024), 0, s, vec, sc, a->src, a->in_lo, a->in_hi, a->workspace, n, ni, c, a->pad)
        if (first) {
            if (a->ksize == 3)
                HPD_SMALL(0, 3);
            else
                HPD_SMALL(0, 5);
        } else {
            if (a->ksize == 2)
                HPD_SMALL(1, 2);
            else
                HPD_SMALL(1, 3);
        }
#undef HPD_SMALL
    } else {
        const int nt = hfd_nt(a->cout), combos = a->ksize * (a->cin / 16) + 1;
        const dim3 grid(chunks, (unsigned)((combos + 3) / 4), (unsigned)(a->cout / (16 * nt)));
        ProfScope ps("hpd_dw_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
#define HPD_DW(NN) \
    hipLaunchKernelGGL((hpd_dw_kernel<NN>), grid, dim3(256), 0, s, a->x, a->g, a->src, a->in_lo, a->in_hi, a->workspace, n, ni, a->cin, a->cout, a->ksize, a->pad)
        HFD_TILES(nt, HPD_DW)
#undef HPD_DW
    }
    hfd_launch_dw_reduce(a, a->cin, "hpd_dw_reduce_kernel", s);
    return check_hip(hipGetLastError(), "hpd_layer_dw");
}

}  // extern "C"
