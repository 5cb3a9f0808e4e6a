// hifigan_sdisc.hip -- the HiFi-GAN scale discriminator: grouped, strided 1-D convolutions + LeakyReLU on the waveform pooled 0, 1, 2, .. times, forward and
// backward, its 1 -> C first layer with up to 15 taps, and the average pooling with its adjoint (include/fcl_hip.h "HiFi-GAN scale discriminator";
// fcl_taco2_amd/hifigan_scale_discriminator.py; restated in float64 numpy in tests/hfgs_ref.py).
//
// Layout and geometry as hifigan_disc.hip: float32, channel-last, packed [rows, C], the three int32 tables per layer at the rate of its OUTPUT rows (a segment
// is an utterance), tap j of output row t reads input row src[t] + j - pad and a tap outside the utterance contributes zero.  Output channel co of a grouped
// layer belongs to group co / cog (cog = cout / groups) and reads the input channels [g cig, (g + 1) cig), cig = cin / groups; cog is a multiple of 16, so a
// workgroup's column block lies inside one group, and cig a multiple of 8.  The contraction runs over the flattened (tap, in-group channel) index in units of
// 4, so cig = 8 feeds no MFMA with zeros but in the last step of a kernel whose 8 ksize cig is no multiple of 16.
// Exact fp32 on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain), unconditional loads from clamped rows masked with pwr_keep, tile counts as template
// arguments, 64-bit row arithmetic, no atomics.  The row descriptor and the first layer's three kernels are those of hfd_rows.h, shared with
// hifigan_disc.hip; the grouped forward and input gradient run their fetch through its hfd_mma_loop; hsd_dw_kernel is the grouped form of
// hpd_dw_kernel.  The dense ksize 5 layer and the score layer of a scale discriminator are period-1 layers of hifigan_disc.hip and are launched
// through its entries.
#include "hfd_rows.h"

namespace fcl {

// ---- grouped forward: y[t, co] = lrelu(bias[co] + sum_j sum_c x[src[t] + j - pad, g cig + c] w[j][c][co]).  A workgroup owns 128 output rows x 16 NT columns of
// one group (blockIdx.y: the column block), a wave 32 rows.  A step is 16 rows of the flattened contraction index kk = j cig + c: a lane loads the 4
// consecutive in-group channels kk .. kk + 3 of its row (one tap, since cig is a multiple of 4) and feeds them to 4 MFMAs.  The lanes of the last step
// whose kk lies past ksize cig load the last valid unit and are masked.
template <int NT>
__global__ __launch_bounds__(256) void hsd_conv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const int32_t* __restrict__ src, const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi,
                                                       float* __restrict__ y, long long n, long long rows_in, int cin, int cout, int cig, int cog, int ksize,
                                                       int stride, int pad, float slope) {
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    const int col0 = blockIdx.y * NT * 16;
    const int ch0 = (col0 / cog) * cig;
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
    const int K = ksize * cig, steps = (K + 15) >> 4;
    const long long last = rows_in - 1;
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const int kk = step * 16 + 4 * q, kc = min(kk, K - 4);
        const int j = kc / cig, c = kc - j * cig;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = centre[mt] + j;
            a[mt] = *reinterpret_cast<const f32x4*>(x + min(max(arow, 0LL), last) * cin + ch0 + c);
            ok[mt] = kk < K && arow >= lo[mt] && arow < hi[mt];
        }
        const float* wr = w + (size_t)kc * cout + col0 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[s][nt] = wr[(size_t)s * cout + nt * 16];
    };
    hfd_mma_loop<NT>(steps, fetch, acc);
    // results in the C / D layout: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = col0 + nt * 16 + r;
        const float bv = bias ? bias[col] : 0.f;
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

// ---- grouped input gradient, the gather form of hpd_conv_dx_kernel: input row h = stride m + ph of an utterance collects g[m + c - i] Wb[ph][i] over the
// phase's taps; blockIdx.z is the phase ph, the rows run at the output rate and the stored row is src[t] + ph where that lies inside the utterance, so every
// input row is written exactly once.  The columns are INPUT channels: a tile of 16 NT columns from col0 reads, per group it touches, the cog gradient
// channels of that group.  NT > 1 is launched only where 16 NT divides cig (one group); a 16-column tile with cig below 16 (or no multiple of 16) spans two
// groups and loops over them, the weight of a column that belongs to the other group masked to zero: per such tile the MFMA work of a zero-padded
// block-diagonal operand, without storing one.  wb [stride][slots][cog][cin], y = m(hin) (acc + extra).
template <int NT>
__global__ __launch_bounds__(256) void hsd_conv_dx_kernel(const float* __restrict__ g, const float* __restrict__ wb, const float* __restrict__ hin,
                                                          const float* __restrict__ extra, const int32_t* __restrict__ src,
                                                          const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi, float* __restrict__ y,
                                                          long long n, long long rows_in, int cin, int cout, int cig, int cog, int ksize, int stride, int pad,
                                                          int slots, float slope) {
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    const int col0 = blockIdx.y * NT * 16;
    const int ph = blockIdx.z;
    const int c = (ph + pad) / stride, j0 = (ph + pad) - c * stride;
    const int ntaps = j0 < ksize ? (ksize - j0 + stride - 1) / stride : 0;
    wb += (size_t)ph * slots * cog * cin + col0;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int g_first = col0 / cig, g_last = (col0 + NT * 16 - 1) / cig;
    int colgrp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) colgrp[nt] = (col0 + nt * 16 + r) / cig;
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
    const int ncb = cog >> 4, per = max(ntaps, 1) * ncb, steps = (g_last - g_first + 1) * ntaps * ncb;
    const long long last = n - 1;
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const int gi = step / per, rem = step - gi * per;
        const int i = rem / ncb, cb = (rem - i * ncb) << 4, grp = g_first + gi;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = top[mt] - i;
            a[mt] = *reinterpret_cast<const f32x4*>(g + min(max(arow, 0LL), last) * cout + grp * cog + cb + 4 * q);
            ok[mt] = arow >= lo[mt] && arow < hi[mt];
        }
        const float* wr = wb + ((size_t)i * cog + cb + 4 * q) * cin + r;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[s][nt] = pwr_keep(wr[(size_t)s * cin + nt * 16], colgrp[nt] == grp);
    };
    hfd_mma_loop<NT>(steps, fetch, acc);  // (a phase without taps: slot 0 exists, holds zeros, and the loop does not run)
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
                const size_t at = (size_t)row * cin + col0 + nt * 16 + r;
                float v = acc[mt][nt][reg];
                if (extra) v += extra[at];
                y[at] = v * hfd_mask(hin[at], slope);
            }
        }
}

// ---- grouped weight gradients, as hpd_dw_kernel: partial[chunk][kk][co] = sum over the chunk's output rows t of x[src[t] + j - pad, g(co) cig + c] g[t, co],
// kk = j cig + c, followed by one row sum_t g[t, co] for the bias.  A wave owns 16 rows of kk x 16 NT columns of one group (blockIdx.z: the column block);
// a lane's tap follows from its own kk, so cig = 8 puts two taps into one tile.  blockIdx.x is the chunk of PWR_DW_CHUNK output rows, blockIdx.y * 4 + wave
// the contraction tile.  The partial is `groups` times smaller than a dense layer's.  No barrier in the kernel: an idle wave returns.  As in
// hpd_dw_kernel a wave reads its B rows once per contraction tile; the input rows are not reused across taps (DESIGN 6r says what that leaves).
template <int NT>
__global__ __launch_bounds__(256) void hsd_dw_kernel(const float* __restrict__ x, const float* __restrict__ g, const int32_t* __restrict__ src,
                                                     const int32_t* __restrict__ in_lo, const int32_t* __restrict__ in_hi, float* __restrict__ partial,
                                                     long long n, long long rows_in, int cin, int cout, int cig, int cog, int ksize, int pad) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int K = ksize * cig, tiles = (K + 15) >> 4;
    const int combo = blockIdx.y * 4 + wave;
    if (combo > tiles) return;
    const bool ones = combo == tiles;
    const int col0 = blockIdx.z * NT * 16;
    const int kk = combo * 16 + r;
    const bool arow_live = !ones && kk < K;
    const int kc = arow_live ? kk : 0;
    const int j = kc / cig;
    const int ach = (col0 / cog) * cig + (kc - j * cig);
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
    auto issue = [&](int grp, Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, tc = min(tq, last);
            G.at[u] = src[tc];
            G.lo[u] = in_lo[tc];
            G.hi[u] = in_hi[tc];
            G.av[u] = x[min(max(G.at[u] + shift, 0LL), alast) * cin + ach];
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
            const float a = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, pwr_keep(G.av[u], arow_live && live && ar >= lo && ar < hi)) |
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
    float* out = partial + (size_t)blockIdx.x * ((size_t)K + 1) * cout + col0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int m = combo * 16 + 4 * q + reg;
            if (ones) {
                if (4 * q + reg == 0) out[(size_t)K * cout + nt * 16 + r] = acc[nt][reg];
            } else if (m < K) {
                out[(size_t)m * cout + nt * 16 + r] = acc[nt][reg];
            }
        }
    }
}

// the utterance of row t: the largest b with off[b] <= t (off [n_utt + 1] ascending, off[0] = 0, t < off[n_utt])
__device__ __forceinline__ int hsd_utterance(const int32_t* __restrict__ off, int n_utt, long long t) {
    int lo = 0, hi = n_utt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---- AvgPool1d(4, 2, padding 2) per utterance, one thread per output row (DX 0): y[n] = (x[2n - 2] + x[2n - 1] + x[2n] + x[2n + 1]) / 4, zeros outside the
// utterance, added left to right; and its adjoint in gather form, one thread per input row (DX 1): dx[m] = (g[m / 2] + g[m / 2 + 1]) / 4, the second term
// where the utterance has that output (m / 2 + 1 <= T / 2).  in_off / out_off: the utterances' first rows at the fine and at the pooled rate.
template <int DX>
__global__ __launch_bounds__(256) void hsd_pool_kernel(const float* __restrict__ in, float* __restrict__ out, const int32_t* __restrict__ in_off,
                                                       const int32_t* __restrict__ out_off, int n_utt, long long rows_in, long long rows_out) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= (DX ? rows_in : rows_out)) return;
    const int b = hsd_utterance(DX ? in_off : out_off, n_utt, t);
    const long long lo = in_off[b], hi = min(rows_in, (long long)in_off[b + 1]), olo = out_off[b];
    if (DX) {
        const long long m = t - lo, n1 = m >> 1, count = ((hi - lo) >> 1) + 1;
        float v = in[min(olo + n1, rows_out - 1)];
        if (n1 + 1 < count && olo + n1 + 1 < rows_out) v += in[olo + n1 + 1];
        out[t] = 0.25f * v;
    } else {
        const long long first = lo + 2 * (t - olo) - 2;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rr = first + j;
            v += (rr >= lo && rr < hi) ? in[rr] : 0.f;
        }
        out[t] = 0.25f * v;
    }
}

// the scale discriminator's own rules inside hfd_check: the layer class (first or grouped), the groups, the kernel size, the stride, the padding
static int hsd_rules(const fcl_hsd_t* a, const char* who) {
    const bool first = a->cin == 1 && hfd_width_ok(a->cout), mid = hfd_width_ok(a->cin) && hfd_width_ok(a->cout);
    FCL_REQUIRE(first || mid, FCL_ERR_SHAPE,
                "%s: a layer is 1 -> C or C -> C' with the widths multiples of 16 from 16 to 1024; the score layer is an fcl_hpd layer (got cin %d, cout %d)", who,
                a->cin, a->cout);
    if (first)
        FCL_REQUIRE(a->groups == 1, FCL_ERR_SHAPE, "%s: the first layer has one group (got groups %d)", who, a->groups);
    else
        FCL_REQUIRE(a->groups >= 1 && a->cin % a->groups == 0 && a->cout % a->groups == 0 && (a->cout / a->groups) % 16 == 0 && (a->cin / a->groups) % 8 == 0,
                    FCL_ERR_SHAPE, "%s: groups must divide both widths with cout / groups a multiple of 16 and cin / groups a multiple of 8 (got %d -> %d in %d groups)",
                    who, a->cin, a->cout, a->groups);
    const int kmax = first ? 15 : 41;
    FCL_REQUIRE(a->ksize >= 3 && a->ksize <= kmax && a->ksize % 2 == 1 && a->stride >= 1 && a->stride <= 4 && a->pad == (a->ksize - 1) / 2, FCL_ERR_SHAPE,
                "%s: an odd kernel size from 3 to %d, stride 1 to 4 and padding (k - 1) / 2 expected (got %d, %d, %d)", who, kmax, a->ksize, a->stride, a->pad);
    return FCL_OK;
}

static int hsd_pool_check(const void* in, const void* out, const int32_t* in_off, const int32_t* out_off, int n_utt, int64_t rows_in, int64_t rows_out,
                          const char* who) {
    FCL_REQUIRE(in && out && in_off && out_off, FCL_ERR_INVALID, "%s: null input / output / in_off / out_off", who);
    FCL_REQUIRE(n_utt >= 1 && rows_in >= n_utt && rows_in < 0x7fffffffLL && rows_out >= n_utt && rows_out <= rows_in / 2 + n_utt, FCL_ERR_SHAPE,
                "%s: n_utt >= 1, n_utt <= rows_in < 2^31 and n_utt <= rows_out <= rows_in / 2 + n_utt expected (got %d, %lld, %lld)", who, n_utt,
                (long long)rows_in, (long long)rows_out);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_hsd_dw_workspace_bytes(int64_t rows_out, int cin, int cout, int groups, int ksize) {
    if (rows_out < 1 || cin < 1 || cout < 1 || groups < 1 || ksize < 1 || cin % groups) return 0;
    return (size_t)pwr_chunks(rows_out) * ((size_t)ksize * (cin / groups) + 1) * cout * sizeof(float);
}

int fcl_hsd_layer_fwd(const fcl_hsd_t* a, fcl_stream_t stream) {
    const int rc = hfd_check(a, "hsd_layer_fwd", hsd_rules);
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->y, FCL_ERR_INVALID, "hsd_layer_fwd: null x / w / y");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w) && aligned16(a->y), FCL_ERR_ALIGN, "hsd_layer_fwd: x, w and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows_out, ni = a->rows_in;
    if (a->cin == 1) {
        ProfScope ps("hsd_first_kernel<fwd>", 2.0 * a->ksize * a->cout * (double)n, (double)n, s);
        hipLaunchKernelGGL(hfd_expand_fwd_kernel, dim3((unsigned)((n * (a->cout / 4) + 255) / 256)), dim3(256), 0, s, a->x, a->w, a->bias, a->src, a->in_lo,
                           a->in_hi, a->y, n, ni, a->cout, a->ksize, a->stride, a->pad, a->slope);
    } else {
        const int cig = a->cin / a->groups, cog = a->cout / a->groups, nt = hfd_nt(cog);
        const dim3 grid((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS), (unsigned)(a->cout / (16 * nt)));
        ProfScope ps("hsd_conv_kernel", 2.0 * a->ksize * cig * a->cout * (double)n, (double)n, s);
#define HSD_FWD(NN) \
    hipLaunchKernelGGL((hsd_conv_kernel<NN>), grid, dim3(256), 0, s, a->x, a->w, a->bias, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cin, a->cout, cig, cog, a->ksize, a->stride, a->pad, a->slope)
        HFD_TILES(nt, HSD_FWD)
#undef HSD_FWD
    }
    return check_hip(hipGetLastError(), "hsd_layer_fwd");
}

int fcl_hsd_layer_dx(const fcl_hsd_t* a, fcl_stream_t stream) {
    const int rc = hfd_check(a, "hsd_layer_dx", hsd_rules);
    if (rc) return rc;
    FCL_REQUIRE(a->g && a->w && a->y, FCL_ERR_INVALID, "hsd_layer_dx: null g / w / y");
    FCL_REQUIRE(a->cin == 1 ? (a->h == nullptr && a->extra == nullptr) : a->h != nullptr, FCL_ERR_INVALID,
                "hsd_layer_dx: h (the stored activation of the layer's input) is needed for cin > 1; h and extra have no meaning for the first layer");
    FCL_REQUIRE(aligned16(a->g) && aligned16(a->w) && aligned16(a->y) && aligned16(a->h) && aligned16(a->extra), FCL_ERR_ALIGN,
                "hsd_layer_dx: g, w, h, extra and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows_out, ni = a->rows_in;
    if (a->cin == 1) {
        const long long items = n * a->stride;
        ProfScope ps("hsd_first_kernel<dx>", 2.0 * a->ksize * a->cout * (double)n, (double)ni, s);
        hipLaunchKernelGGL(hfd_reduce_dx_kernel, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, s, a->g, a->w, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cout,
                           a->ksize, a->stride, a->pad);
    } else {
        const int cig = a->cin / a->groups, cog = a->cout / a->groups, nt = hfd_nt(cig), slots = (a->ksize + a->stride - 1) / a->stride;
        const dim3 grid((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS), (unsigned)(a->cin / (16 * nt)), (unsigned)a->stride);
        ProfScope ps("hsd_conv_dx_kernel", 2.0 * a->ksize * cig * a->cout * (double)n, (double)ni, s);
#define HSD_DX(NN) \
    hipLaunchKernelGGL((hsd_conv_dx_kernel<NN>), grid, dim3(256), 0, s, a->g, a->w, a->h, a->extra, a->src, a->in_lo, a->in_hi, a->y, n, ni, a->cin, a->cout, cig, cog, a->ksize, a->stride, a->pad, slots, a->slope)
        HFD_TILES(nt, HSD_DX)
#undef HSD_DX
    }
    return check_hip(hipGetLastError(), "hsd_layer_dx");
}

int fcl_hsd_layer_dw(const fcl_hsd_t* a, fcl_stream_t stream) {
    const int rc = hfd_check(a, "hsd_layer_dw", hsd_rules);
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->g && a->dw && a->workspace, FCL_ERR_INVALID, "hsd_layer_dw: null x / g / dw / workspace");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->g) && aligned16(a->workspace), FCL_ERR_ALIGN, "hsd_layer_dw: x, g and workspace must be 16-byte aligned");
    const size_t need = fcl_hsd_dw_workspace_bytes(a->rows_out, a->cin, a->cout, a->groups, a->ksize);
    FCL_REQUIRE(a->workspace_bytes >= need, FCL_ERR_WORKSPACE, "hsd_layer_dw: the workspace holds %zu bytes, fcl_hsd_dw_workspace_bytes asks for %zu",
                a->workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->rows_out, ni = a->rows_in;
    const int cig = a->cin / a->groups, cog = a->cout / a->groups;
    if (a->cin == 1) {
        const dim3 grid((unsigned)pwr_chunks(n), (unsigned)((a->cout + 127) / 128));
        ProfScope ps("hsd_first_kernel<dw>", 2.0 * (a->ksize + 1) * a->cout * (double)n, (double)n, s);
#define HSD_FIRST(K) \
    case K: hipLaunchKernelGGL((hfd_dw_small_kernel<0, K>), grid, dim3(1024), 0, s, a->g, a->x, a->src, a->in_lo, a->in_hi, a->workspace, n, ni, a->cout, a->pad); break
        switch (a->ksize) {
            HSD_FIRST(3);
            HSD_FIRST(5);
            HSD_FIRST(7);
            HSD_FIRST(9);
            HSD_FIRST(11);
            HSD_FIRST(13);
            default: hipLaunchKernelGGL((hfd_dw_small_kernel<0, 15>), grid, dim3(1024), 0, s, a->g, a->x, a->src, a->in_lo, a->in_hi, a->workspace, n, ni, a->cout, a->pad);
        }
#undef HSD_FIRST
    } else {
        const int nt = hfd_nt(cog), combos = (a->ksize * cig + 15) / 16 + 1;
        const dim3 grid((unsigned)pwr_chunks(n), (unsigned)((combos + 3) / 4), (unsigned)(a->cout / (16 * nt)));
        ProfScope ps("hsd_dw_kernel", 2.0 * a->ksize * cig * a->cout * (double)n, (double)n, s);
#define HSD_DW(NN) \
    hipLaunchKernelGGL((hsd_dw_kernel<NN>), grid, dim3(256), 0, s, a->x, a->g, a->src, a->in_lo, a->in_hi, a->workspace, n, ni, a->cin, a->cout, cig, cog, a->ksize, a->pad)
        HFD_TILES(nt, HSD_DW)
#undef HSD_DW
    }
    hfd_launch_dw_reduce(a, cig, "hsd_dw_reduce_kernel", s);
    return check_hip(hipGetLastError(), "hsd_layer_dw");
}

int fcl_hsd_pool_fwd(const float* x, float* y, const int32_t* in_off, const int32_t* out_off, int n_utt, int64_t rows_in, int64_t rows_out, fcl_stream_t stream) {
    const int rc = hsd_pool_check(x, y, in_off, out_off, n_utt, rows_in, rows_out, "hsd_pool_fwd");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("hsd_pool_kernel<fwd>", 4.0 * (double)rows_out, (double)rows_out, s);
    hipLaunchKernelGGL((hsd_pool_kernel<0>), dim3((unsigned)((rows_out + 255) / 256)), dim3(256), 0, s, x, y, in_off, out_off, n_utt, (long long)rows_in,
                       (long long)rows_out);
    return check_hip(hipGetLastError(), "hsd_pool_fwd");
}

int fcl_hsd_pool_dx(const float* g, float* dx, const int32_t* in_off, const int32_t* out_off, int n_utt, int64_t rows_in, int64_t rows_out, fcl_stream_t stream) {
    const int rc = hsd_pool_check(g, dx, in_off, out_off, n_utt, rows_in, rows_out, "hsd_pool_dx");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("hsd_pool_kernel<dx>", 2.0 * (double)rows_in, (double)rows_in, s);
    hipLaunchKernelGGL((hsd_pool_kernel<1>), dim3((unsigned)((rows_in + 255) / 256)), dim3(256), 0, s, g, dx, in_off, out_off, n_utt, (long long)rows_in,
                       (long long)rows_out);
    return check_hip(hipGetLastError(), "hsd_pool_dx");
}

}  // extern "C"
