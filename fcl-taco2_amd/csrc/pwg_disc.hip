// pwg_disc.hip -- the Parallel WaveGAN discriminator: a stack of dilated Conv1d + LeakyReLU, forward and backward (include/fcl_hip.h "Parallel
// WaveGAN discriminator"; fcl_taco2_amd/pwg_discriminator.py; restated in float64 numpy in tests/pwgd_ref.py).
//
// Layout: activations and gradients are float32, channel-last [samples, C]; a batch is packed, one row per sample, the utterances back to back.
// Rows get their utterance bounds from seg_lo / seg_hi [samples] (as fcl_conv1d_fwd): a tap of row t reads row r only where seg_lo[t] <= r <
// seg_hi[t], anything else contributes zero, so no value crosses an utterance boundary.  Both tables are clamped to [0, samples].
// Weights are tap-major: the forward form [k][cin][cout]; the input-gradient form [k][cout][cin] with the taps reversed, so that the input
// gradient is the forward contraction on it.  Weight gradients come out in the forward form.
//
// One launch per layer and one arithmetic mode: exact fp32, the C -> C contractions on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain).  The
// shifted row blocks come straight from global memory / L2 (no halo in LDS), so there is no dilation limit.  No atomics: the weight gradients are
// per-chunk partials added in ascending chunk order by a second launch; a batch is bit for bit its per-utterance runs.
// The keep mask, the bounds lookup, the C -> C weight-gradient kernel and the reduce are pwg_rows.h's, shared with pwg_train.hip.  pwd_conv_kernel keeps
// its own two-operand form of the header's pipelined loop: through the general one it ran 6 - 9 % slower.
#include "pwg_rows.h"

namespace fcl {

constexpr int PWD_SMALL_GROUPS = 8; // row groups of pwd_dw_small_kernel (1024 threads)
constexpr int PWD_SMALL_UNROLL = 4; // samples per register set of pwd_dw_small_kernel

enum { PWD_FWD = 0, PWD_DX = 1 };

// d LeakyReLU / d pre-activation from the stored post-activation (the activation keeps the sign); h == 0 takes the slope, as torch does
__device__ __forceinline__ float pwd_mask(float h, float slope) { return h > 0.f ? 1.f : slope; }

// ---- C -> C: y[t, co] = epi(sum_j sum_ci x[t + (j - (k - 1) / 2) d, ci] w[j][ci][co]).  A workgroup owns 128 rows x 16 NT columns (blockIdx.y: the column
// block; pwd_tiles: NT = 1 .. 5 or 7, the whole width or half of it), a wave 32 rows: 2 x NT accumulator tiles of v_mfma_f32_16x16x4_f32.  A lane loads
// 4 consecutive input channels of its row at once and feeds them to 4 MFMAs; the contraction index of MFMA s of a 16-channel block is therefore
// ci = block + 4 (lane >> 4) + s on both operands.
// EPI PWD_FWD: + bias, LeakyReLU.  PWD_DX: x is the gradient, w the reversed / transposed form, and the result is multiplied by the LeakyReLU derivative
// read from the stored activation h [samples, cout] (null: no mask).
template <int EPI, int NT>
__global__ __launch_bounds__(256) void pwd_conv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ h, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                       float* __restrict__ y, long long n, int cin, int cout, int ksize, int dil, float slope) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + wave * 32;
    const int n0 = blockIdx.y * (NT * 16);
    long long trow[2], lo[2], hi[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        trow[mt] = t0 + mt * 16 + r;
        pwr_bounds(seg_lo, seg_hi, trow[mt], n, lo[mt], hi[mt]);
    }
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int half = (ksize - 1) >> 1;
    // a step is (tap, 16 input channels): 2 row loads and 4 NT weight loads feed 8 NT MFMAs.  The operands of step s + 1 are requested before the
    // MFMAs of step s, so their latency runs under the matrix pipe (the last step requests itself again).  Every load is unconditional -- a row outside
    // the utterance is loaded from a clamped row and replaced by zero -- and the tile count is a template argument: a runtime condition around a load
    // makes the compiler wait for each load where it stands.
    const int ncb = cin >> 4, steps = ksize * ncb;
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const int j = step / ncb, cb = (step - j * ncb) << 4;
        const long long shift = (long long)(j - half) * dil;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = trow[mt] + shift;
            a[mt] = *reinterpret_cast<const f32x4*>(x + min(max(arow, 0LL), n - 1) * cin + cb + 4 * q);
            ok[mt] = arow >= lo[mt] && arow < hi[mt];
        }
        const float* wr = w + ((size_t)j * cin + cb + 4 * q) * cout + n0 + r;
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
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[mt][s], b0[s][nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int s = 0; s < 4; ++s) a0[mt][s] = pwr_keep(a1[mt][s], ok1[mt]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b0[s][nt] = b1[s][nt];
    }
    // C / D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + nt * 16 + r;
        const float bv = (EPI == PWD_FWD && bias) ? bias[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long row = t0 + mt * 16 + 4 * q + reg;
                if (row >= n) continue;
                float v = acc[mt][nt][reg];
                if (EPI == PWD_FWD) {
                    v += bv;
                    v = v > 0.f ? v : v * slope;
                } else if (h) {
                    v *= pwd_mask(h[row * cout + col], slope);
                }
                y[row * cout + col] = v;
            }
        }
    }
}

// ---- 1 -> C: y[t, c] = epi(sum_j s[t + (j - (k - 1) / 2) d] w[j][c]); an item is (sample, 4 channels).  PWD_FWD: the first layer (+ bias, LeakyReLU);
// PWD_DX: the last layer's input gradient (times the mask of h).
template <int EPI>
__global__ __launch_bounds__(256) void pwd_expand_kernel(const float* __restrict__ s, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ h, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                         float* __restrict__ y, long long n, int c, int ksize, int dil, float slope) {
    const int cq = c >> 2;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n * cq) return;
    const long long t = i / cq;
    const int ch = (int)(i - t * cq) * 4;
    long long lo, hi;
    pwr_bounds(seg_lo, seg_hi, t, n, lo, hi);
    const int half = (ksize - 1) >> 1;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < ksize; ++j) {
        const long long rr = t + (long long)(j - half) * dil;
        const float sv = (rr >= lo && rr < hi) ? s[rr] : 0.f;
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)j * c + ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(sv, wv[e], v[e]);
    }
    f32x4 o;
    if (EPI == PWD_FWD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = v[e] + (bias ? bias[ch + e] : 0.f);
            o[e] = u > 0.f ? u : u * slope;
        }
    } else {
        const f32x4 hv = *reinterpret_cast<const f32x4*>(h + t * c + ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e] * pwd_mask(hv[e], slope);
    }
    *reinterpret_cast<f32x4*>(y + t * c + ch) = o;
}

// ---- C -> 1: y[t] = bias + sum_j sum_c x[t + (j - (k - 1) / 2) d, c] w[j][c]; 16 lanes per sample, a fixed butterfly.  DX = 0: the last layer (the
// scores); DX = 1: the first layer's input gradient (the waveform gradient) -- the same arithmetic under its own name in the launch record.
template <int DX>
__global__ __launch_bounds__(256) void pwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* __restrict__ y,
                                                         long long n, int c, int ksize, int dil) {
    const int sub = threadIdx.x & 15;
    const long long t = blockIdx.x * 16LL + (threadIdx.x >> 4);
    long long lo, hi;
    pwr_bounds(seg_lo, seg_hi, t, n, lo, hi);
    const int half = (ksize - 1) >> 1;
    float acc = 0.f;
    for (int j = 0; j < ksize; ++j) {
        const long long rr = t + (long long)(j - half) * dil;
        if (rr < lo || rr >= hi) continue;
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

// ---- weight gradient of the 1 -> C and C -> 1 layers, one chunk's partial per workgroup in the same layout.  vec [samples, c], sc [samples].
// VEC_SHIFTED = 0 (first layer, cin 1): partial[j][ch] = sum_t sc[t + shift_j] vec[t, ch], row k = sum_t vec[t, ch].
// VEC_SHIFTED = 1 (last layer, cout 1): partial[j c + ch] = sum_t vec[t + shift_j, ch] sc[t], element k c = sum_t sc[t].
// Thread = (channel, one of 8 row groups taking every 8th sample); the groups' sums meet in LDS and are added in ascending group order.
template <int VEC_SHIFTED, int KSIZE>
__global__ __launch_bounds__(1024) void pwd_dw_small_kernel(const float* __restrict__ vec, const float* __restrict__ sc, const int32_t* __restrict__ seg_lo,
                                                            const int32_t* __restrict__ seg_hi, float* __restrict__ partial, long long n, int c, int dil) {
    __shared__ float red[PWD_SMALL_GROUPS - 1][(KSIZE + 1) * 128];
    const int ch = threadIdx.x & 127, grp = threadIdx.x >> 7;
    const int chc = min(ch, c - 1);  // (the threads past the width load a valid channel and store nothing)
    const long long t_begin = (long long)blockIdx.x * PWR_DW_CHUNK, t_end = min(n, t_begin + PWR_DW_CHUNK);
    const long long last = t_end - 1;
    constexpr int half = (KSIZE - 1) >> 1;
    float acc[KSIZE + 1];
#pragma unroll
    for (int j = 0; j <= KSIZE; ++j) acc[j] = 0.f;
    // loads first (unconditional, clamped rows), a scheduling barrier, then the arithmetic: as pwr_dw_kernel, one register set
    for (int it0 = 0; it0 < PWR_DW_CHUNK / PWD_SMALL_GROUPS; it0 += PWD_SMALL_UNROLL) {
        int lo[PWD_SMALL_UNROLL], hi[PWD_SMALL_UNROLL];
        float ov[PWD_SMALL_UNROLL], xv[PWD_SMALL_UNROLL][KSIZE];
#pragma unroll
        for (int u = 0; u < PWD_SMALL_UNROLL; ++u) {
            const long long t = t_begin + (long long)(it0 + u) * PWD_SMALL_GROUPS + grp, tc = min(t, last);
            lo[u] = seg_lo[tc];
            hi[u] = seg_hi[tc];
            ov[u] = VEC_SHIFTED ? sc[tc] : vec[tc * c + chc];
#pragma unroll
            for (int j = 0; j < KSIZE; ++j) {
                const long long rc = min(max(t + (long long)(j - half) * dil, 0LL), n - 1);
                xv[u][j] = VEC_SHIFTED ? vec[rc * c + chc] : sc[rc];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < PWD_SMALL_UNROLL; ++u) {
            const long long t = t_begin + (long long)(it0 + u) * PWD_SMALL_GROUPS + grp;
            const bool live = t <= last;
            const long long l = max(0, lo[u]), h = min(n, (long long)hi[u]);
            const float own = pwr_keep(ov[u], live);
#pragma unroll
            for (int j = 0; j < KSIZE; ++j) {
                const long long rr = t + (long long)(j - half) * dil;
                acc[j] = fmaf(pwr_keep(xv[u][j], live && rr >= l && rr < h), own, acc[j]);
            }
            acc[KSIZE] += own;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (grp > 0) {
#pragma unroll
        for (int j = 0; j <= KSIZE; ++j) red[grp - 1][j * 128 + ch] = acc[j];
    }
    __syncthreads();
    if (grp == 0 && ch < c) {
#pragma unroll
        for (int j = 0; j <= KSIZE; ++j)
#pragma unroll
            for (int k = 0; k < PWD_SMALL_GROUPS - 1; ++k) acc[j] += red[k][j * 128 + ch];
        float* out = partial + (size_t)blockIdx.x * (VEC_SHIFTED ? (size_t)KSIZE * c + 1 : ((size_t)KSIZE + 1) * c);
#pragma unroll
        for (int j = 0; j < KSIZE; ++j) out[(size_t)j * c + ch] = acc[j];
        if (!VEC_SHIFTED || ch == 0) out[(size_t)KSIZE * c + (VEC_SHIFTED ? 0 : ch)] = acc[KSIZE];
    }
}

static bool pwd_width_ok(int c) { return c >= 16 && c <= 128 && c % 16 == 0; }

// column tiles per workgroup of pwd_conv_kernel for c / 16 tiles in all: the whole width up to 5 tiles and at 7, half of it at 6 and 8
static int pwd_tiles(int c) {
    const int t = c / 16;
    return (t == 6 || t == 8) ? t / 2 : t;
}

template <int EPI>
static void pwd_launch_conv(const float* x, const float* w, const float* bias, const float* h, const int32_t* seg_lo, const int32_t* seg_hi, float* y, long long n,
                            int cin, int cout, int ksize, int dil, float slope, hipStream_t s) {
    const int nt = pwd_tiles(cout);
    const dim3 grid((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS), (unsigned)(cout / 16 / nt));
#define PWD_CONV(NN)                                                                                                                                  \
    case NN:                                                                                                                                          \
        hipLaunchKernelGGL((pwd_conv_kernel<EPI, NN>), grid, dim3(256), 0, s, x, w, bias, h, seg_lo, seg_hi, y, n, cin, cout, ksize, dil, slope);    \
        break;
    switch (nt) {
        PWD_CONV(1) PWD_CONV(2) PWD_CONV(3) PWD_CONV(4) PWD_CONV(5) PWD_CONV(7)
    }
#undef PWD_CONV
}

// what every entry checks: the struct, the layer class (1 -> C, C -> C, C -> 1), the kernel size, the dilation, the slope, the tables
static int pwd_check(const fcl_pwd_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    const bool first = a->cin == 1 && pwd_width_ok(a->cout), mid = a->cin == a->cout && pwd_width_ok(a->cin), last = a->cout == 1 && pwd_width_ok(a->cin);
    FCL_REQUIRE(first || mid || last, FCL_ERR_SHAPE,
                "%s: a layer is 1 -> C, C -> C or C -> 1 with C a multiple of 16 from 16 to 128 (got cin %d, cout %d)", who, a->cin, a->cout);
    FCL_REQUIRE(a->ksize == 3 || a->ksize == 5, FCL_ERR_SHAPE, "%s: kernel size must be 3 or 5 (got %d)", who, a->ksize);
    FCL_REQUIRE(a->dilation >= 1, FCL_ERR_SHAPE, "%s: dilation must be positive (got %d)", who, a->dilation);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->slope >= 0.f && a->slope < 1.f, FCL_ERR_INVALID, "%s: 0 <= negative_slope < 1 expected (got %g)", who, (double)a->slope);
    FCL_REQUIRE(a->seg_lo && a->seg_hi, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi", who);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_pwd_dw_workspace_bytes(int64_t samples, int cin, int cout, int ksize) {
    if (samples < 1 || cin < 1 || cout < 1 || ksize < 1) return 0;
    return (size_t)pwr_chunks(samples) * ((size_t)ksize * cin + 1) * cout * sizeof(float);
}

int fcl_pwd_layer_fwd(const fcl_pwd_t* a, fcl_stream_t stream) {
    const int rc = pwd_check(a, "pwd_layer_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->w && a->y, FCL_ERR_INVALID, "pwd_layer_fwd: null x / w / y");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->w) && aligned16(a->y), FCL_ERR_ALIGN, "pwd_layer_fwd: x, w and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    if (a->cin == 1) {
        ProfScope ps("pwd_expand_kernel<fwd>", 2.0 * a->ksize * a->cout * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwd_expand_kernel<PWD_FWD>, dim3((unsigned)((n * (a->cout / 4) + 255) / 256)), dim3(256), 0, s, a->x, a->w, a->bias, (const float*)nullptr,
                           a->seg_lo, a->seg_hi, a->y, n, a->cout, a->ksize, a->dilation, a->slope);
    } else if (a->cout == 1) {
        ProfScope ps("pwd_reduce_kernel<fwd>", 2.0 * a->ksize * a->cin * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwd_reduce_kernel<0>, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, a->x, a->w, a->bias, a->seg_lo, a->seg_hi, a->y, n, a->cin,
                           a->ksize, a->dilation);
    } else {
        ProfScope ps("pwd_conv_kernel<fwd>", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
        pwd_launch_conv<PWD_FWD>(a->x, a->w, a->bias, nullptr, a->seg_lo, a->seg_hi, a->y, n, a->cin, a->cout, a->ksize, a->dilation, a->slope, s);
    }
    return check_hip(hipGetLastError(), "pwd_layer_fwd");
}

int fcl_pwd_layer_dx(const fcl_pwd_t* a, fcl_stream_t stream) {
    const int rc = pwd_check(a, "pwd_layer_dx");
    if (rc) return rc;
    FCL_REQUIRE(a->g && a->w && a->y, FCL_ERR_INVALID, "pwd_layer_dx: null g / w / y");
    FCL_REQUIRE(a->cin == 1 ? a->h == nullptr : a->h != nullptr, FCL_ERR_INVALID,
                "pwd_layer_dx: h (the stored activation of the layer's input) is needed for cin > 1 and has no meaning for the first layer");
    FCL_REQUIRE(aligned16(a->g) && aligned16(a->w) && aligned16(a->y) && aligned16(a->h), FCL_ERR_ALIGN, "pwd_layer_dx: g, w, h and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    if (a->cin == 1) {
        ProfScope ps("pwd_reduce_kernel<dx>", 2.0 * a->ksize * a->cout * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwd_reduce_kernel<1>, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, a->g, a->w, (const float*)nullptr, a->seg_lo, a->seg_hi, a->y, n,
                           a->cout, a->ksize, a->dilation);
    } else if (a->cout == 1) {
        ProfScope ps("pwd_expand_kernel<dx>", 2.0 * a->ksize * a->cin * (double)n, (double)n, s);
        hipLaunchKernelGGL(pwd_expand_kernel<PWD_DX>, dim3((unsigned)((n * (a->cin / 4) + 255) / 256)), dim3(256), 0, s, a->g, a->w, (const float*)nullptr, a->h,
                           a->seg_lo, a->seg_hi, a->y, n, a->cin, a->ksize, a->dilation, a->slope);
    } else {
        ProfScope ps("pwd_conv_kernel<dx>", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
        pwd_launch_conv<PWD_DX>(a->g, a->w, nullptr, a->h, a->seg_lo, a->seg_hi, a->y, n, a->cout, a->cin, a->ksize, a->dilation, a->slope, s);
    }
    return check_hip(hipGetLastError(), "pwd_layer_dx");
}

int fcl_pwd_layer_dw(const fcl_pwd_t* a, fcl_stream_t stream) {
    const int rc = pwd_check(a, "pwd_layer_dw");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->g && a->dw && a->workspace, FCL_ERR_INVALID, "pwd_layer_dw: null x / g / dw / workspace");
    FCL_REQUIRE(a->workspace_bytes >= fcl_pwd_dw_workspace_bytes(a->samples, a->cin, a->cout, a->ksize), FCL_ERR_WORKSPACE,
                "pwd_layer_dw: the workspace holds %zu bytes, fcl_pwd_dw_workspace_bytes asks for %zu", a->workspace_bytes,
                fcl_pwd_dw_workspace_bytes(a->samples, a->cin, a->cout, a->ksize));
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const unsigned chunks = (unsigned)pwr_chunks(n);
    if (a->cin == 1) {
        ProfScope ps("pwd_dw_small_kernel<first>", 2.0 * (a->ksize + 1) * a->cout * (double)n, (double)n, s);
        if (a->ksize == 3)
            hipLaunchKernelGGL((pwd_dw_small_kernel<0, 3>), dim3(chunks), dim3(1024), 0, s, a->g, a->x, a->seg_lo, a->seg_hi, a->workspace, n, a->cout, a->dilation);
        else
            hipLaunchKernelGGL((pwd_dw_small_kernel<0, 5>), dim3(chunks), dim3(1024), 0, s, a->g, a->x, a->seg_lo, a->seg_hi, a->workspace, n, a->cout, a->dilation);
    } else if (a->cout == 1) {
        ProfScope ps("pwd_dw_small_kernel<last>", 2.0 * (a->ksize + 1) * a->cin * (double)n, (double)n, s);
        if (a->ksize == 3)
            hipLaunchKernelGGL((pwd_dw_small_kernel<1, 3>), dim3(chunks), dim3(1024), 0, s, a->x, a->g, a->seg_lo, a->seg_hi, a->workspace, n, a->cin, a->dilation);
        else
            hipLaunchKernelGGL((pwd_dw_small_kernel<1, 5>), dim3(chunks), dim3(1024), 0, s, a->x, a->g, a->seg_lo, a->seg_hi, a->workspace, n, a->cin, a->dilation);
    } else {
        const int combos = a->ksize * (a->cin / 16) + 1;
        const PwrA in = {a->x, a->cin, a->cin, a->ksize, a->dilation, 1.f, nullptr, 0, 0};  // B = g alone: no b1 tile
        ProfScope ps("pwd_dw_kernel", 2.0 * a->ksize * a->cin * a->cout * (double)n, (double)n, s);
        const dim3 grid(chunks, (unsigned)((combos + 3) / 4));
#define PWD_DW(NN)                                                                                                                                         \
    case NN:                                                                                                                                               \
        hipLaunchKernelGGL((pwr_dw_kernel<PWR_PLAIN, NN, 0>), grid, dim3(256), 0, s, in, a->g, a->g, a->cout, 1.f, 1, a->seg_lo, a->seg_hi, a->workspace, n); \
        break;
        switch (a->cout / 16) {
            PWD_DW(1) PWD_DW(2) PWD_DW(3) PWD_DW(4) PWD_DW(5) PWD_DW(6) PWD_DW(7) PWD_DW(8)
        }
#undef PWD_DW
    }
    {
        const int nw = a->ksize * a->cin * a->cout, nb = a->cout;
        ProfScope ps("pwd_dw_reduce_kernel", 0.0, (double)chunks, s);
        hipLaunchKernelGGL(pwr_dw_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, a->workspace, (int)chunks, nw, nb, a->dw, a->db);
    }
    return check_hip(hipGetLastError(), "pwd_layer_dw");
}

}  // extern "C"
