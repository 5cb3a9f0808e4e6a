// hifigan_train.hip -- the HiFi-GAN generator's upsampling stages in their training form: the transposed convolution and the multi-receptive-field
// residual units forward with the pre-activations kept, and backward to every input, weight and bias gradient (include/fcl_hip.h "HiFi-GAN generator,
// training form"; fcl_taco2_amd/hifigan_generator.py; restated in float64 numpy in tests/hfgt_ref.py).  The inference form is hifigan.hip;
// nothing is shared with it.
//
// Layout as pwg_rows.h: float32, channel-last, packed [rows, C], the utterances back to back, row t's utterance is [seg_lo[t], seg_hi[t]) and a tap outside
// it contributes zero; exact fp32 on v_mfma_f32_16x16x4_f32, unconditional loads from clamped rows masked with pwr_keep, tile counts as template arguments,
// 64-bit row arithmetic, no atomics.  pwr_contract takes the whole output width in one workgroup and reads its operand at the output's own rate; the loop
// here is a local form of it (the neighbours' kernels are not routed through a more general loop) with three additions: a column block per
// blockIdx.y (widths to 512), LeakyReLU formed on load, and a row geometry  A row = rs t + j dil - back,  output row = os t + blockIdx.z,  which makes the
// transposed convolution (os = s, two taps, one weight matrix per phase) and its adjoint in gather form (rs = s, 2 s taps) the same contraction.
#include "pwg_rows.h"

namespace fcl {

enum { HFT_PLAIN = 0, HFT_LRELU = 1 };              // the A operand as stored / v > 0 ? v : slope v formed on load
enum { HFT_BIAS = 0, HFT_BIAS_RES = 1, HFT_MASK = 2 };  // y = acc + bias / acc + bias + res / m(pre) acc + res   (pre, res: null = 1, 0)
constexpr int HFT_MAX_TERMS = 4;

// tables at the rate of t (n rows); the source p has n rs rows
struct HftA {
    const float* p;
    int ld, c1, taps, dil, rs;
    long long back;
    float slope;
};

__device__ __forceinline__ float hft_lrelu(float v, float slope) { return v * (v > 0.f ? 1.f : slope); }

template <int MODE, int NT, int EPI>
__global__ __launch_bounds__(256) void hft_conv_kernel(HftA A, const float* __restrict__ w, int ldw, long long w_phase, int os, int pad,
                                                       const float* __restrict__ bias, const float* res, const float* __restrict__ pre, float slope,
                                                       const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* y, long long n) {
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    const int col0 = blockIdx.y * NT * 16;
    // the output phase (os > 1: the transposed convolution): output row os t + z reads the inputs t + carry - 1 and t + carry with the taps ph + os and ph
    int ph = blockIdx.z + pad, carry = 0;
    if (ph >= os) {
        ph -= os;
        carry = 1;
    }
    const long long back = A.back - carry;
    w += (size_t)ph * w_phase + col0;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    long long trow[2], lo[2], hi[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        trow[mt] = t0 + mt * 16 + r;
        pwr_bounds(seg_lo, seg_hi, trow[mt], n, lo[mt], hi[mt]);
        lo[mt] *= A.rs;
        hi[mt] *= A.rs;
    }
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nb1 = A.c1 >> 4, steps = A.taps * nb1;
    const long long last = n * A.rs - 1;
    // as pwr_contract: a step is 16 contraction rows; the operands of step s + 1 are requested before the MFMAs of step s
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const int j = step / nb1, cb = (step - j * nb1) << 4;
        const long long shift = (long long)j * A.dil - back;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = trow[mt] * A.rs + shift;
            const f32x4 v = *reinterpret_cast<const f32x4*>(A.p + min(max(arow, 0LL), last) * A.ld + cb + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s) a[mt][s] = MODE == HFT_LRELU ? hft_lrelu(v[s], A.slope) : v[s];
            ok[mt] = arow >= lo[mt] && arow < hi[mt];
        }
        const float* wr = w + ((size_t)step * 16 + 4 * q) * ldw + r;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[s][nt] = wr[(size_t)s * ldw + nt * 16];
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
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long row = t0 + mt * 16 + 4 * q + reg;
                if (row >= n) continue;
                const size_t at = (size_t)(row * os + blockIdx.z) * ldw + col0 + nt * 16 + r;
                float v = acc[mt][nt][reg];
                if (EPI == HFT_MASK) {
                    if (pre) v *= pre[at] > 0.f ? 1.f : slope;
                    if (res) v += res[at];
                } else {
                    v += bias[col0 + nt * 16 + r];
                    if (EPI == HFT_BIAS_RES) v += res[at];
                }
                y[at] = v;
            }
}

// ---- weight gradients, as pwr_dw_kernel, with the row geometry on both operands and a column block per blockIdx.z:
// partial[chunk][j c1 + ci][co] = sum over the chunk's rows t of A[rs t + j dil - back, ci] B[rsb t + j bdil - bback, co], followed by `nones` rows
// sum_t B[rsb t + (ones_tap + o) bdil - bback, co] for the bias.  The chunk is `chunk` rows (a multiple of 32) of the tables' rate.
template <int MODE, int NT>
__global__ __launch_bounds__(256) void hft_dw_kernel(HftA A, const float* __restrict__ b, int ldb, int rsb, int bdil, long long bback, int nones, int ones_tap,
                                                     int chunk, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                     float* __restrict__ partial, long long n) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int mt1 = A.c1 >> 4, tiles = A.taps * mt1;
    const int combo = blockIdx.y * 4 + wave;
    if (combo >= tiles + nones) return;
    const bool ones = combo >= tiles;
    const int j = ones ? ones_tap + (combo - tiles) : combo / mt1, mt = ones ? 0 : combo - j * mt1;
    const int col0 = blockIdx.z * NT * 16;
    const long long shift = ones ? 0 : (long long)j * A.dil - A.back, bshift = (long long)j * bdil - bback;
    const long long t_begin = (long long)blockIdx.x * chunk, t_end = min(n, t_begin + chunk);
    const long long last = t_end - 1, alast = n * A.rs - 1, blast = n * rsb - 1;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    struct Group {
        int lo[PWR_DW_GROUP], hi[PWR_DW_GROUP];
        float av[PWR_DW_GROUP], bv[PWR_DW_GROUP][NT];
    };
    auto issue = [&](int grp, Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, tc = min(tq, last);
            G.lo[u] = seg_lo[tc];
            G.hi[u] = seg_hi[tc];
            const float av = A.p[min(max(tq * A.rs + shift, 0LL), alast) * A.ld + mt * 16 + r];
            G.av[u] = MODE == HFT_LRELU ? hft_lrelu(av, A.slope) : av;
            const float* src = b + min(max(tq * rsb + bshift, 0LL), blast) * ldb + col0 + r;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) G.bv[u][nt] = src[nt * 16];
        }
    };
    auto compute = [&](int grp, const Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, ar = tq * A.rs + shift, br = tq * rsb + bshift;
            const bool live = tq <= last;
            const long long lo = max(0, G.lo[u]), hi = min(n, (long long)G.hi[u]);
            const bool bok = live && br >= lo * rsb && br < hi * rsb;
            const float a = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, pwr_keep(G.av[u], !ones && live && ar >= lo * A.rs && ar < hi * A.rs)) |
                                                          ((ones && live && r == 0) ? 0x3F800000u : 0u));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pwr_keep(G.bv[u][nt], bok), acc[nt], 0, 0, 0);
        }
    };
    const int groups = chunk / 4 / PWR_DW_GROUP;  // even
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
    const int ldo = gridDim.z * NT * 16;
    float* out = partial + (size_t)blockIdx.x * ((size_t)tiles * 16 + nones) * ldo + col0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int m = 4 * q + reg;
            if (ones) {
                if (m == 0) out[((size_t)tiles * 16 + (combo - tiles)) * ldo + nt * 16 + r] = acc[nt][reg];
            } else {
                out[((size_t)combo * 16 + m) * ldo + nt * 16 + r] = acc[nt][reg];
            }
        }
    }
}

// the partials added in ascending chunk order (the bias: chunk-major over its `nones` rows)
__global__ __launch_bounds__(256) void hft_dw_reduce_kernel(const float* __restrict__ partial, int chunks, int nw, int cout, int nones,
                                                            float* __restrict__ dw, float* __restrict__ db) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nw + cout) return;
    const size_t stride = (size_t)nw + (size_t)nones * cout;
    float s = 0.f;
    if (e < nw) {
#pragma unroll 8
        for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * stride + e];
        dw[e] = s;
    } else {
        for (int k = 0; k < chunks; ++k)
            for (int o = 0; o < nones; ++o) s += partial[(size_t)k * stride + nw + (size_t)o * cout + (e - nw)];
        db[e - nw] = s;
    }
}

// out = scale (p0 + p1 + ..) in ascending order, 4 floats per lane: the stage's output (1 / nk) sum x_last, the backward seed dc / nk, and du = sum dx
struct HftTerms {
    const float* p[HFT_MAX_TERMS];
};
__global__ __launch_bounds__(256) void hft_sum_kernel(HftTerms T, int count, float scale, float* __restrict__ out, long long quads) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= quads) return;
    f32x4 s = reinterpret_cast<const f32x4*>(T.p[0])[e];
    for (int k = 1; k < count; ++k) {
        const f32x4 v = reinterpret_cast<const f32x4*>(T.p[k])[e];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] *= scale;
    reinterpret_cast<f32x4*>(out)[e] = s;
}

static bool hft_ksize(int k) { return k == 1 || k == 3 || k == 5 || k == 7 || k == 11; }
static int hft_nt(int cout) { return cout % 64 == 0 ? 4 : cout % 32 == 0 ? 2 : 1; }
// rows of the input rate per partial of the transposed convolution's weight gradient: 1 024 output rows, a multiple of 32
static int hft_tchunk(int s) { return (PWR_DW_CHUNK / s) & ~31; }  // (s <= 16: at least 64)
static long long hft_chunks(long long rows, int chunk) { return (rows + chunk - 1) / chunk; }

static int hft_check_conv(const fcl_hft_conv_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->slope >= 0.f && a->slope < 1.f, FCL_ERR_INVALID, "%s: slope must be in [0, 1) (got %g)", who, (double)a->slope);
    FCL_REQUIRE(a->cin >= 16 && a->cin <= 512 && a->cin % 16 == 0, FCL_ERR_SHAPE, "%s: cin must be a multiple of 16 from 16 to 512 (got %d)", who, a->cin);
    FCL_REQUIRE(a->cout >= 16 && a->cout <= 512 && a->cout % 16 == 0, FCL_ERR_SHAPE, "%s: cout must be a multiple of 16 from 16 to 512 (got %d)", who,
                a->cout);
    FCL_REQUIRE(hft_ksize(a->ksize), FCL_ERR_SHAPE, "%s: kernel size must be 1, 3, 5, 7 or 11 (got %d)", who, a->ksize);
    FCL_REQUIRE(a->dilation >= 1 && a->dilation <= (1 << 20), FCL_ERR_SHAPE, "%s: dilation must be 1 to 2^20 (got %d)", who, a->dilation);
    FCL_REQUIRE(a->rows >= 1 && a->rows < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= rows < 2^31 expected (got %lld)", who, (long long)a->rows);
    FCL_REQUIRE(a->seg_lo && a->seg_hi, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi", who);
    return FCL_OK;
}

static int hft_check_tconv(const fcl_hft_tconv_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->slope >= 0.f && a->slope < 1.f, FCL_ERR_INVALID, "%s: slope must be in [0, 1) (got %g)", who, (double)a->slope);
    FCL_REQUIRE(a->cin >= 16 && a->cin <= 512 && a->cin % 16 == 0, FCL_ERR_SHAPE, "%s: cin must be a multiple of 16 from 16 to 512 (got %d)", who, a->cin);
    FCL_REQUIRE(a->cout >= 16 && a->cout <= 512 && a->cout % 16 == 0, FCL_ERR_SHAPE, "%s: cout must be a multiple of 16 from 16 to 512 (got %d)", who,
                a->cout);
    FCL_REQUIRE(a->stride >= 2 && a->stride <= 16, FCL_ERR_SHAPE, "%s: stride must be 2 to 16 (got %d)", who, a->stride);
    FCL_REQUIRE(a->rows >= 1 && a->rows * a->stride < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= rows, rows x stride < 2^31 expected (got %lld)", who,
                (long long)a->rows);
    FCL_REQUIRE(a->seg_lo && a->seg_hi, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi", who);
    return FCL_OK;
}

#define HFT_TILES(NTV, CALL)  \
    switch (NTV) {            \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        default: CALL(4); break; \
    }

// one launch of the row contraction: MODE and EPI are runtime here, template arguments in the kernel
static void hft_launch_rows(int lrelu, int epi, const HftA& A, const float* w, int cout, long long w_phase, int os, int pad, const float* bias,
                            const float* res, const float* pre, float slope, const int32_t* lo, const int32_t* hi, float* y, long long n, hipStream_t s) {
    const int nt = hft_nt(cout);
    const dim3 grid((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS), (unsigned)(cout / (16 * nt)), (unsigned)os);
#define HFT_GO(M, E, NN) hipLaunchKernelGGL((hft_conv_kernel<M, NN, E>), grid, dim3(256), 0, s, A, w, cout, w_phase, os, pad, bias, res, pre, slope, lo, hi, y, n)
#define HFT_PLAIN_BIAS(NN) HFT_GO(HFT_PLAIN, HFT_BIAS, NN)
#define HFT_LRELU_BIAS(NN) HFT_GO(HFT_LRELU, HFT_BIAS, NN)
#define HFT_LRELU_RES(NN) HFT_GO(HFT_LRELU, HFT_BIAS_RES, NN)
#define HFT_PLAIN_RES(NN) HFT_GO(HFT_PLAIN, HFT_BIAS_RES, NN)
#define HFT_PLAIN_MASK(NN) HFT_GO(HFT_PLAIN, HFT_MASK, NN)
    if (epi == HFT_MASK) {
        HFT_TILES(nt, HFT_PLAIN_MASK)
    } else if (epi == HFT_BIAS_RES) {
        if (lrelu) {
            HFT_TILES(nt, HFT_LRELU_RES)
        } else {
            HFT_TILES(nt, HFT_PLAIN_RES)
        }
    } else if (lrelu) {
        HFT_TILES(nt, HFT_LRELU_BIAS)
    } else {
        HFT_TILES(nt, HFT_PLAIN_BIAS)
    }
#undef HFT_GO
}

static void hft_launch_dw(int lrelu, const HftA& A, const float* b, int cout, int rsb, int bdil, long long bback, int nones, int ones_tap, int chunk,
                          const int32_t* lo, const int32_t* hi, float* partial, long long n, hipStream_t s) {
    const int nt = hft_nt(cout), combos = A.taps * (A.c1 / 16) + nones;
    const dim3 grid((unsigned)hft_chunks(n, chunk), (unsigned)((combos + 3) / 4), (unsigned)(cout / (16 * nt)));
#define HFT_DW_L(NN) hipLaunchKernelGGL((hft_dw_kernel<HFT_LRELU, NN>), grid, dim3(256), 0, s, A, b, cout, rsb, bdil, bback, nones, ones_tap, chunk, lo, hi, partial, n)
#define HFT_DW_P(NN) hipLaunchKernelGGL((hft_dw_kernel<HFT_PLAIN, NN>), grid, dim3(256), 0, s, A, b, cout, rsb, bdil, bback, nones, ones_tap, chunk, lo, hi, partial, n)
    if (lrelu) {
        HFT_TILES(nt, HFT_DW_L)
    } else {
        HFT_TILES(nt, HFT_DW_P)
    }
}

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_hft_workspace_bytes(int64_t rows, int cin, int cout, int taps, int stride) {
    if (rows < 1 || cin < 1 || cout < 1 || taps < 1 || stride < 1 || stride > 16) return 0;
    const bool tc = stride > 1;
    const long long chunks = hft_chunks(rows, tc ? hft_tchunk(stride) : PWR_DW_CHUNK);
    return (size_t)chunks * ((size_t)taps * cin + (tc ? stride : 1)) * cout * sizeof(float);
}

int fcl_hft_conv_fwd(const fcl_hft_conv_t* a, fcl_stream_t stream) {
    const int rc = hft_check_conv(a, "hft_conv_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->bias && a->y, FCL_ERR_INVALID, "hft_conv_fwd: null x / w / bias / y");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w) && aligned16(a->res) && aligned16(a->y), FCL_ERR_ALIGN,
                "hft_conv_fwd: x, w, res and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const HftA in = {a->x, a->cin, a->cin, a->ksize, a->dilation, 1, (long long)((a->ksize - 1) / 2) * a->dilation, a->slope};
    ProfScope ps("hft_conv_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)a->rows, (double)a->rows, s);
    hft_launch_rows(a->lrelu, a->res ? HFT_BIAS_RES : HFT_BIAS, in, a->w, a->cout, 0, 1, 0, a->bias, a->res, nullptr, a->slope, a->seg_lo, a->seg_hi, a->y,
                    a->rows, s);
    return check_hip(hipGetLastError(), "hft_conv_fwd");
}

int fcl_hft_conv_dx(const fcl_hft_conv_t* a, fcl_stream_t stream) {
    const int rc = hft_check_conv(a, "hft_conv_dx");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->y, FCL_ERR_INVALID, "hft_conv_dx: null x / w / y");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w) && aligned16(a->res) && aligned16(a->pre) && aligned16(a->y), FCL_ERR_ALIGN,
                "hft_conv_dx: x, w, res, pre and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const HftA in = {a->x, a->cin, a->cin, a->ksize, a->dilation, 1, (long long)((a->ksize - 1) / 2) * a->dilation, a->slope};
    ProfScope ps("hft_conv_dx_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)a->rows, (double)a->rows, s);
    hft_launch_rows(0, HFT_MASK, in, a->w, a->cout, 0, 1, 0, nullptr, a->res, a->pre, a->slope, a->seg_lo, a->seg_hi, a->y, a->rows, s);
    return check_hip(hipGetLastError(), "hft_conv_dx");
}

int fcl_hft_conv_dw(const fcl_hft_conv_t* a, fcl_stream_t stream) {
    const int rc = hft_check_conv(a, "hft_conv_dw");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->g && a->dw && a->db && a->workspace, FCL_ERR_INVALID, "hft_conv_dw: null x / g / dw / db / workspace");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->g) && aligned16(a->workspace), FCL_ERR_ALIGN, "hft_conv_dw: x, g and workspace must be 16-byte aligned");
    const size_t need = fcl_hft_workspace_bytes(a->rows, a->cin, a->cout, a->ksize, 1);
    FCL_REQUIRE(a->workspace_bytes >= need, FCL_ERR_WORKSPACE, "hft_conv_dw: the workspace holds %zu bytes, fcl_hft_workspace_bytes asks for %zu",
                a->workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const HftA in = {a->x, a->cin, a->cin, a->ksize, a->dilation, 1, (long long)((a->ksize - 1) / 2) * a->dilation, a->slope};
    {
        ProfScope ps("hft_dw_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)a->rows, (double)a->rows, s);
        hft_launch_dw(a->lrelu, in, a->g, a->cout, 1, 0, 0, 1, 0, PWR_DW_CHUNK, a->seg_lo, a->seg_hi, a->workspace, a->rows, s);
    }
    const int chunks = (int)hft_chunks(a->rows, PWR_DW_CHUNK), nw = a->ksize * a->cin * a->cout;
    ProfScope ps("hft_dw_reduce_kernel", 0.0, (double)chunks, s);
    hipLaunchKernelGGL(hft_dw_reduce_kernel, dim3((unsigned)((nw + a->cout + 255) / 256)), dim3(256), 0, s, a->workspace, chunks, nw, a->cout, 1, a->dw, a->db);
    return check_hip(hipGetLastError(), "hft_conv_dw");
}

int fcl_hft_tconv_fwd(const fcl_hft_tconv_t* a, fcl_stream_t stream) {
    const int rc = hft_check_tconv(a, "hft_tconv_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->c && a->w && a->bias && a->u, FCL_ERR_INVALID, "hft_tconv_fwd: null c / w / bias / u");
    FCL_REQUIRE(aligned16(a->c) && aligned16(a->w) && aligned16(a->u), FCL_ERR_ALIGN, "hft_tconv_fwd: c, w and u must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int st = a->stride;
    const HftA in = {a->c, a->cin, a->cin, 2, 1, 1, 1, a->slope};
    ProfScope ps("hft_tconv_kernel", 2.0 * 2 * a->cin * a->cout * (double)a->rows * st, (double)a->rows * st, s);
    hft_launch_rows(1, HFT_BIAS, in, a->w, a->cout, 2LL * a->cin * a->cout, st, st / 2 + st % 2, a->bias, nullptr, nullptr, a->slope, a->seg_lo, a->seg_hi,
                    a->u, a->rows, s);
    return check_hip(hipGetLastError(), "hft_tconv_fwd");
}

int fcl_hft_tconv_dx(const fcl_hft_tconv_t* a, fcl_stream_t stream) {
    const int rc = hft_check_tconv(a, "hft_tconv_dx");
    if (rc) return rc;
    FCL_REQUIRE(a->c && a->w && a->du && a->dc, FCL_ERR_INVALID, "hft_tconv_dx: null c / w / du / dc");
    FCL_REQUIRE(aligned16(a->c) && aligned16(a->w) && aligned16(a->du) && aligned16(a->dc), FCL_ERR_ALIGN,
                "hft_tconv_dx: c, w, du and dc must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int st = a->stride;
    // the adjoint in gather form: input row q collects du[s q + j - padding] W[:, :, j]^T over the 2 s taps
    const HftA in = {a->du, a->cout, a->cout, 2 * st, 1, st, st / 2 + st % 2, a->slope};
    ProfScope ps("hft_tconv_dx_kernel", 2.0 * 2 * a->cin * a->cout * (double)a->rows * st, (double)a->rows, s);
    hft_launch_rows(0, HFT_MASK, in, a->w, a->cin, 0, 1, 0, nullptr, nullptr, a->c, a->slope, a->seg_lo, a->seg_hi, a->dc, a->rows, s);
    return check_hip(hipGetLastError(), "hft_tconv_dx");
}

int fcl_hft_tconv_dw(const fcl_hft_tconv_t* a, fcl_stream_t stream) {
    const int rc = hft_check_tconv(a, "hft_tconv_dw");
    if (rc) return rc;
    FCL_REQUIRE(a->c && a->du && a->dw && a->db && a->workspace, FCL_ERR_INVALID, "hft_tconv_dw: null c / du / dw / db / workspace");
    FCL_REQUIRE(aligned16(a->c) && aligned16(a->du) && aligned16(a->workspace), FCL_ERR_ALIGN, "hft_tconv_dw: c, du and workspace must be 16-byte aligned");
    const int st = a->stride;
    const size_t need = fcl_hft_workspace_bytes(a->rows, a->cin, a->cout, 2 * st, st);
    FCL_REQUIRE(a->workspace_bytes >= need, FCL_ERR_WORKSPACE, "hft_tconv_dw: the workspace holds %zu bytes, fcl_hft_workspace_bytes asks for %zu",
                a->workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int pad = st / 2 + st % 2, chunk = hft_tchunk(st);
    // dW[:, :, j] = sum over the input rows q of lrelu(c[q])^T du[s q + j - padding]; the bias sums du over the s taps from `padding`, every row once
    const HftA in = {a->c, a->cin, a->cin, 2 * st, 0, 1, 0, a->slope};
    {
        ProfScope ps("hft_tconv_dw_kernel", 2.0 * 2 * a->cin * a->cout * (double)a->rows * st, (double)a->rows, s);
        hft_launch_dw(1, in, a->du, a->cout, st, 1, pad, st, pad, chunk, a->seg_lo, a->seg_hi, a->workspace, a->rows, s);
    }
    const int chunks = (int)hft_chunks(a->rows, chunk), nw = 2 * st * a->cin * a->cout;
    ProfScope ps("hft_dw_reduce_kernel", 0.0, (double)chunks, s);
    hipLaunchKernelGGL(hft_dw_reduce_kernel, dim3((unsigned)((nw + a->cout + 255) / 256)), dim3(256), 0, s, a->workspace, chunks, nw, a->cout, st, a->dw,
                       a->db);
    return check_hip(hipGetLastError(), "hft_tconv_dw");
}

int fcl_hft_sum(float* out, const float* const* terms, int count, float scale, int64_t elems, fcl_stream_t stream) {
    FCL_REQUIRE(out && terms, FCL_ERR_INVALID, "hft_sum: null out / terms");
    FCL_REQUIRE(count >= 1 && count <= HFT_MAX_TERMS, FCL_ERR_SHAPE, "hft_sum: 1 to %d terms expected (got %d)", HFT_MAX_TERMS, count);
    FCL_REQUIRE(elems >= 4 && elems % 4 == 0, FCL_ERR_SHAPE, "hft_sum: the element count must be a positive multiple of 4 (got %lld)", (long long)elems);
    HftTerms T;
    for (int k = 0; k < HFT_MAX_TERMS; ++k) T.p[k] = terms[k < count ? k : 0];
    for (int k = 0; k < count; ++k) FCL_REQUIRE(T.p[k], FCL_ERR_INVALID, "hft_sum: term %d is null", k);
    FCL_REQUIRE(aligned16(out), FCL_ERR_ALIGN, "hft_sum: out must be 16-byte aligned");
    for (int k = 0; k < count; ++k) FCL_REQUIRE(aligned16(T.p[k]), FCL_ERR_ALIGN, "hft_sum: term %d must be 16-byte aligned", k);
    hipStream_t s = (hipStream_t)stream;
    const long long quads = elems / 4;
    ProfScope ps("hft_sum_kernel", 0.0, (double)elems, s);
    hipLaunchKernelGGL(hft_sum_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, T, count, scale, out, quads);
    return check_hip(hipGetLastError(), "hft_sum");
}

}  // extern "C"
