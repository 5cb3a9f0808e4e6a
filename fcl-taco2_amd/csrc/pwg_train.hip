// pwg_train.hip -- the Parallel WaveGAN generator's residual block in its training form: forward with the gate activations kept, and backward (input,
// conditioning and weight gradients) (include/fcl_hip.h "Parallel WaveGAN generator, training form"; fcl_taco2_amd/pwg_generator.py; restated
// in float64 numpy in tests/pwgt_ref.py).  The inference form is pwg.hip; nothing is shared with it.
//
// Layout as pwg_disc.hip: float32, channel-last, packed [samples, C]; row t's utterance is [seg_lo[t], seg_hi[t]) and a tap outside it contributes zero.
// Every contraction is one shape -- rows x (a few shifted or plain row sources) x a tap-major weight matrix -- on v_mfma_f32_16x16x4_f32 (exact fp32, a
// k-ordered fmaf chain), after pwd_conv_kernel / pwd_dw_kernel: unconditional loads from clamped rows masked with a bitwise AND, tile counts as template
// arguments, the next step's operands requested before this step's MFMAs, 64-bit row arithmetic, no atomics (weight gradients: per-chunk partials added in
// ascending order by a second launch).
#include "fcl_common.h"

namespace fcl {

constexpr int PWT_ROWS = 128;       // rows per workgroup of the row kernels: 4 waves x 2 tiles of 16 rows
constexpr int PWT_DW_CHUNK = 1024;  // samples per partial of the weight gradients
constexpr int PWT_DW_GROUP = 4;     // MFMA steps (of 4 samples) per register set of pwt_dw_kernel
constexpr float PWT_SQRT_HALF = 0.70710678118654752440f;

enum { PWT_PLAIN = 0, PWT_GATED = 1 };  // the A operand as stored / g = a * b formed on load from ab [samples, 2 R]

// The gate with accurate functions: tanhf, and the sigmoid with a true division.  The inference path's clamped pwg_gate and lstm_epilogue.h's rcpf forms
// are not used: the backward pass takes 1 - a^2 and b (1 - b), differences near saturation, where an absolute error of a few ulp of 1 in a or b is a
// large relative error of the derivative.
__device__ __forceinline__ float pwt_tanh(float z) { return tanhf(z); }
__device__ __forceinline__ float pwt_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// v where keep, else +0.0, as a bitwise AND (pwd_keep): the load is used whatever keep says, and a NaN in an unused lane leaves no trace
__device__ __forceinline__ float pwt_keep(float v, bool keep) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & (keep ? 0xFFFFFFFFu : 0u));
}

__device__ __forceinline__ void pwt_bounds(const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, long long t, long long n, long long& lo,
                                           long long& hi) {
    lo = hi = 0;
    if (t < n) {
        lo = max(0, seg_lo[t]);
        hi = min(n, (long long)seg_hi[t]);
    }
}

// The A operand of a contraction: `taps` shifted views of p1 [samples, ld1] (c1 channels each, tap j at (j - (taps - 1) / 2) dil, times s1), followed by
// p2 [samples, ld2] (c2 channels, unshifted).  Contraction row of the weight matrix: j c1 + channel, then taps c1 + channel of p2.  taps == 0 or c2 == 0
// leaves a source out (its pointer is then never used).  PWT_GATED: p1 is ab [samples, 2 c1] and the value is ab[:, ch] * ab[:, c1 + ch].
struct PwtA {
    const float* p1;
    int ld1, c1, taps, dil;
    float s1;
    const float* p2;
    int ld2, c2;
};

// acc[mt][nt] = A[t0 + 16 mt + .., :] W[:, 16 nt + ..] for the wave's 32 rows from t0 (the whole width: ldw = 16 NT).  A lane loads 4 consecutive channels of its row at once and feeds
// them to 4 MFMAs, so the contraction index of MFMA s of a 16-channel block is block + 4 (lane >> 4) + s on both operands (as pwd_conv_kernel).
template <int MODE, int NT>
__device__ __forceinline__ void pwt_contract(const PwtA& A, const float* __restrict__ w, const int32_t* __restrict__ seg_lo,
                                             const int32_t* __restrict__ seg_hi, long long n, long long t0, f32x4 (&acc)[2][NT]) {
    constexpr int ldw = NT * 16;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    long long trow[2], lo[2], hi[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        trow[mt] = t0 + mt * 16 + r;
        pwt_bounds(seg_lo, seg_hi, trow[mt], n, lo[mt], hi[mt]);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int half = (A.taps - 1) >> 1;
    const int nb1 = max(A.c1 >> 4, 1), steps1 = A.taps * (A.c1 >> 4), steps = steps1 + (A.c2 >> 4);
    // a step is 16 contraction rows: 2 row loads (4 when gated) and 4 NT weight loads feed 8 NT MFMAs.  The operands of step s + 1 are requested before the
    // MFMAs of step s (the last step requests itself again); every load is unconditional, a row outside the utterance comes from a clamped row and is
    // replaced by zero.  Which source a step reads is uniform over the workgroup.
    auto fetch = [&](int step, f32x4(&a)[2], bool(&ok)[2], float(&b)[4][NT]) {
        const bool one = step < steps1;
        const int j = one ? step / nb1 : 0, cb = (one ? step - j * nb1 : step - steps1) << 4;
        const float* p = one ? A.p1 : A.p2;
        const int ld = one ? A.ld1 : A.ld2;
        const long long shift = one ? (long long)(j - half) * A.dil : 0;
        const float sc = one ? A.s1 : 1.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const long long arow = trow[mt] + shift;
            const float* src = p + min(max(arow, 0LL), n - 1) * ld + cb + 4 * q;
            const f32x4 v = *reinterpret_cast<const f32x4*>(src);
            if (MODE == PWT_GATED) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(src + A.c1);
#pragma unroll
                for (int s = 0; s < 4; ++s) a[mt][s] = v[s] * u[s];
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) a[mt][s] = v[s] * sc;
            }
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
        for (int s = 0; s < 4; ++s) a0[mt][s] = pwt_keep(a0[mt][s], ok0[mt]);
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
            for (int s = 0; s < 4; ++s) a0[mt][s] = pwt_keep(a1[mt][s], ok1[mt]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b0[s][nt] = b1[s][nt];
    }
}

// The epilogues below visit the wave's results in the C / D layout: column = lane & 15, row = 4 (lane >> 4) + register.
#define PWT_FOR_RESULTS(NTILES)                                         \
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;    \
    _Pragma("unroll") for (int nt = 0; nt < (NTILES); ++nt)             \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                    \
    _Pragma("unroll") for (int reg = 0; reg < 4; ++reg)

// ---- gate forward: z = b_gate + (x taps | c) w_gate, K = k R + A, N = 2 R.  The wave holds both halves of every column pair (tiles nt and nt + NT / 2), so
// a and b of a channel meet in one lane.  ab = (tanh | sigmoid); z_out (tests only) = z.
template <int NT>
__global__ __launch_bounds__(256) void pwt_gate_kernel(PwtA A, const float* __restrict__ w, const float* __restrict__ bias, const int32_t* __restrict__ seg_lo,
                                                       const int32_t* __restrict__ seg_hi, float* __restrict__ ab, float* __restrict__ z_out, long long n) {
    constexpr int NH = NT / 2, R = NH * 16;
    const long long t0 = (long long)blockIdx.x * PWT_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwt_contract<PWT_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NH) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float za = acc[mt][nt][reg] + bias[col], zb = acc[mt][nt + NH][reg] + bias[R + col];
        if (z_out) {
            z_out[row * (2 * R) + col] = za;
            z_out[row * (2 * R) + R + col] = zb;
        }
        ab[row * (2 * R) + col] = pwt_tanh(za);
        ab[row * (2 * R) + R + col] = pwt_sigmoid(zb);
    }
}

// ---- out forward: (o | s) = g w_out + b_out with g = a * b formed on load, K = R, N = 2 R; x_out = (o + x) sqrt(.5), skips = s or skips + s
template <int NT>
__global__ __launch_bounds__(256) void pwt_out_kernel(PwtA A, const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ x,
                                                      const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* __restrict__ x_out,
                                                      float* __restrict__ skips, long long n, int first) {
    constexpr int NH = NT / 2, R = NH * 16;
    const long long t0 = (long long)blockIdx.x * PWT_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwt_contract<PWT_GATED, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NH) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float o = acc[mt][nt][reg] + bias[col], sk = acc[mt][nt + NH][reg] + bias[R + col];
        x_out[row * R + col] = (o + x[row * R + col]) * PWT_SQRT_HALF;
        skips[row * R + col] = first ? sk : skips[row * R + col] + sk;
    }
}

// ---- out backward: dg = (sqrt(.5) dxo | ds) w_dz, K = 2 R (R without dxo), N = R; dz = (dg b (1 - a^2) | dg a b (1 - b)) from the stored ab
template <int NT>
__global__ __launch_bounds__(256) void pwt_dz_kernel(PwtA A, const float* __restrict__ w, const float* __restrict__ ab, const int32_t* __restrict__ seg_lo,
                                                     const int32_t* __restrict__ seg_hi, float* __restrict__ dz, long long n) {
    constexpr int R = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWT_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwt_contract<PWT_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NT) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float a = ab[row * (2 * R) + col], b = ab[row * (2 * R) + R + col], dg = acc[mt][nt][reg];
        dz[row * (2 * R) + col] = dg * b * (1.f - a * a);
        dz[row * (2 * R) + R + col] = dg * a * b * (1.f - b);
    }
}

// ---- conv backward: dx = dz taps w_dx (taps reversed in the weights) + sqrt(.5) dxo, K = 2 k R, N = R
template <int NT>
__global__ __launch_bounds__(256) void pwt_dx_kernel(PwtA A, const float* __restrict__ w, const float* __restrict__ dxo, const int32_t* __restrict__ seg_lo,
                                                     const int32_t* __restrict__ seg_hi, float* __restrict__ dx, long long n) {
    constexpr int R = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWT_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwt_contract<PWT_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NT) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        float v = acc[mt][nt][reg];
        if (dxo) v += dxo[row * R + col] * PWT_SQRT_HALF;
        dx[row * R + col] = v;
    }
}

// ---- aux backward: dc = dz w_dc or dc + that, K = 2 R, N = A
template <int NT>
__global__ __launch_bounds__(256) void pwt_dc_kernel(PwtA A, const float* __restrict__ w, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                     float* __restrict__ dc, long long n, int write) {
    constexpr int AUX = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWT_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwt_contract<PWT_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NT) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float v = acc[mt][nt][reg];
        dc[row * AUX + col] = write ? v : dc[row * AUX + col] + v;
    }
}

// ---- weight gradients: partial[chunk][m][co] = sum over the chunk's samples t of A[t, m] B[t, co], m the contraction rows of PwtA (so the partial has the
// forward weights' layout), and one more row m = rows for the bias gradient sum_t B[t, co] (an A operand of ones in row 0 of a tile).  B [samples, 16 NT] is
// (b1 s1b | b2), NT / 2 tiles each; b1_live == 0 makes the first half exactly zero (the last block has no dxo).  The contraction runs over the samples, 4
// per MFMA; a wave owns 16 contraction rows x all columns; blockIdx.x is the chunk.  No barrier in the kernel: an idle wave returns.  After pwd_dw_kernel.
template <int MODE, int NT>
__global__ __launch_bounds__(256) void pwt_dw_kernel(PwtA A, const float* __restrict__ b1, const float* __restrict__ b2, int ldb, float s1b, int b1_live,
                                                     const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* __restrict__ partial,
                                                     long long n) {
    constexpr int NH = NT / 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int mt1 = A.c1 >> 4, tiles1 = A.taps * mt1, tiles = tiles1 + (A.c2 >> 4);
    const int combo = blockIdx.y * 4 + wave;
    if (combo > tiles) return;
    const bool ones = combo == tiles, one = !ones && combo < tiles1;
    const int j = one ? combo / mt1 : 0, mt = ones ? 0 : (one ? combo - j * mt1 : combo - tiles1);
    const bool from1 = one || (ones && tiles1 > 0);  // (the wave of ones loads a valid address of a source that exists and masks it away)
    const float* ap = from1 ? A.p1 : A.p2;
    const int lda = from1 ? A.ld1 : A.ld2;
    const long long shift = one ? (long long)(j - ((A.taps - 1) >> 1)) * A.dil : 0;
    const long long t_begin = (long long)blockIdx.x * PWT_DW_CHUNK, t_end = min(n, t_begin + PWT_DW_CHUNK);
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const long long last = t_end - 1;
    struct Group {
        int lo[PWT_DW_GROUP], hi[PWT_DW_GROUP];
        float av[PWT_DW_GROUP], bv[PWT_DW_GROUP][NT];
    };
    // two register sets: the loads of group i + 1 are all issued before the MFMAs of group i; every load is unconditional, from a clamped row, and what a dead
    // lane loaded is masked to zero.  The trip count is fixed: the steps past the chunk's end are dead lanes.
    auto issue = [&](int grp, Group& G) {
#pragma unroll
        for (int u = 0; u < PWT_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWT_DW_GROUP + u) + q, tc = min(tq, last);
            G.lo[u] = seg_lo[tc];
            G.hi[u] = seg_hi[tc];
            const float* src = ap + min(max(tq + shift, 0LL), n - 1) * lda + mt * 16 + r;
            G.av[u] = MODE == PWT_GATED ? src[0] * src[A.c1] : src[0];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) G.bv[u][nt] = nt < NH ? b1[tc * ldb + nt * 16 + r] * s1b : b2[tc * ldb + (nt - NH) * 16 + r];
        }
    };
    auto compute = [&](int grp, const Group& G) {
#pragma unroll
        for (int u = 0; u < PWT_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWT_DW_GROUP + u) + q, rr = tq + shift;
            const bool live = tq <= last;
            const long long lo = max(0, G.lo[u]), hi = min(n, (long long)G.hi[u]);
            const float a = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, pwt_keep(G.av[u], !ones && live && rr >= lo && rr < hi)) |
                                                          ((ones && live && r == 0) ? 0x3F800000u : 0u));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pwt_keep(G.bv[u][nt], live && (nt >= NH || b1_live)), acc[nt], 0, 0, 0);
        }
    };
    constexpr int groups = PWT_DW_CHUNK / 4 / PWT_DW_GROUP;  // even
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
    constexpr int ldo = NT * 16;
    float* out = partial + (size_t)blockIdx.x * ((size_t)tiles * 16 + 1) * ldo;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int m = 4 * q + reg;
            if (ones) {
                if (m == 0) out[(size_t)tiles * 16 * ldo + nt * 16 + r] = acc[nt][reg];
            } else {
                out[((size_t)combo * 16 + m) * ldo + nt * 16 + r] = acc[nt][reg];
            }
        }
    }
}

// the partials added in ascending chunk order: elements [0, nw) are dw, [nw, nw + nb) db
__global__ __launch_bounds__(256) void pwt_dw_reduce_kernel(const float* __restrict__ partial, int chunks, int nw, int nb, float* __restrict__ dw,
                                                            float* __restrict__ db) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nw + nb) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * (nw + nb) + e];
    if (e < nw)
        dw[e] = s;
    else
        db[e - nw] = s;
}

static long long pwt_chunks(long long samples) { return (samples + PWT_DW_CHUNK - 1) / PWT_DW_CHUNK; }
static dim3 pwt_grid(long long n) { return dim3((unsigned)((n + PWT_ROWS - 1) / PWT_ROWS)); }

// what every entry checks: the struct, the widths, the kernel size, the dilation, the sample count, the tables
static int pwt_check(const fcl_pwt_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->residual >= 16 && a->residual <= 64 && a->residual % 16 == 0, FCL_ERR_SHAPE,
                "%s: residual (= skip) channels must be a multiple of 16 from 16 to 64 (got %d)", who, a->residual);
    FCL_REQUIRE(a->aux >= 16 && a->aux <= 128 && a->aux % 16 == 0, FCL_ERR_SHAPE, "%s: aux channels must be a multiple of 16 from 16 to 128 (got %d)", who,
                a->aux);
    FCL_REQUIRE(a->ksize == 3 || a->ksize == 5, FCL_ERR_SHAPE, "%s: kernel size must be 3 or 5 (got %d)", who, a->ksize);
    FCL_REQUIRE(a->dilation >= 1, FCL_ERR_SHAPE, "%s: dilation must be positive (got %d)", who, a->dilation);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->seg_lo && a->seg_hi, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi", who);
    return FCL_OK;
}

#define PWT_EVEN_TILES(CALL) \
    switch (R / 16) {        \
        case 1: CALL(2); break; \
        case 2: CALL(4); break; \
        case 3: CALL(6); break; \
        case 4: CALL(8); break; \
    }
#define PWT_R_TILES(CALL)    \
    switch (R / 16) {        \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
    }

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_pwt_dw_workspace_bytes(int64_t samples, int residual, int aux, int ksize) {
    if (samples < 1 || residual < 1 || aux < 1 || ksize < 1) return 0;
    return (size_t)pwt_chunks(samples) * ((size_t)ksize * residual + aux + 1) * 2 * residual * sizeof(float);
}

int fcl_pwt_block_fwd(const fcl_pwt_t* a, fcl_stream_t stream) {
    const int rc = pwt_check(a, "pwt_block_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->c && a->w_gate && a->b_gate && a->w_out && a->b_out && a->ab && a->x_out && a->skips, FCL_ERR_INVALID,
                "pwt_block_fwd: null x / c / w_gate / b_gate / w_out / b_out / ab / x_out / skips");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->c) && aligned16(a->w_gate) && aligned16(a->w_out) && aligned16(a->ab) && aligned16(a->x_out) &&
                    aligned16(a->skips) && aligned16(a->z_out),
                FCL_ERR_ALIGN, "pwt_block_fwd: x, c, w_gate, w_out, ab, x_out, skips and z_out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual, A = a->aux, k = a->ksize;
    {
        const PwtA in = {a->x, R, R, k, a->dilation, 1.f, a->c, A, A};
        ProfScope ps("pwt_gate_kernel", 2.0 * (k * R + A) * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) hipLaunchKernelGGL(pwt_gate_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_gate, a->b_gate, a->seg_lo, a->seg_hi, a->ab, a->z_out, n)
        PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
    }
    {
        const PwtA in = {a->ab, 2 * R, R, 1, 1, 1.f, nullptr, 0, 0};
        ProfScope ps("pwt_out_kernel", 2.0 * R * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    hipLaunchKernelGGL(pwt_out_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_out, a->b_out, a->x, a->seg_lo, a->seg_hi, a->x_out, a->skips, n, a->first)
        PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
    }
    return check_hip(hipGetLastError(), "pwt_block_fwd");
}

int fcl_pwt_block_dx(const fcl_pwt_t* a, fcl_stream_t stream) {
    const int rc = pwt_check(a, "pwt_block_dx");
    if (rc) return rc;
    FCL_REQUIRE(a->ds && a->ab && a->w_dz && a->dz, FCL_ERR_INVALID, "pwt_block_dx: null ds / ab / w_dz / dz");
    FCL_REQUIRE(a->last ? a->dxo == nullptr : a->dxo != nullptr, FCL_ERR_INVALID,
                "pwt_block_dx: dxo (the gradient of x_out) is needed for every block but the last, which has none");
    FCL_REQUIRE(!a->dx || a->w_dx, FCL_ERR_INVALID, "pwt_block_dx: dx needs w_dx");
    FCL_REQUIRE(!a->dc || a->w_dc, FCL_ERR_INVALID, "pwt_block_dx: dc needs w_dc");
    FCL_REQUIRE(aligned16(a->ds) && aligned16(a->dxo) && aligned16(a->ab) && aligned16(a->w_dz) && aligned16(a->w_dx) && aligned16(a->w_dc) &&
                    aligned16(a->dz) && aligned16(a->dx) && aligned16(a->dc),
                FCL_ERR_ALIGN, "pwt_block_dx: ds, dxo, ab, w_dz, w_dx, w_dc, dz, dx and dc must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual, A = a->aux, k = a->ksize;
    {
        // without dxo the contraction is over ds alone, on the Wskip rows of w_dz
        const PwtA in = {a->dxo, R, R, a->dxo ? 1 : 0, 1, PWT_SQRT_HALF, a->ds, R, R};
        const float* w = a->dxo ? a->w_dz : a->w_dz + (size_t)R * R;
        ProfScope ps("pwt_dz_kernel", 2.0 * (a->dxo ? 2 : 1) * R * R * (double)n, (double)n, s);
#define PWT_CALL(NN) hipLaunchKernelGGL(pwt_dz_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, w, a->ab, a->seg_lo, a->seg_hi, a->dz, n)
        PWT_R_TILES(PWT_CALL)
#undef PWT_CALL
    }
    if (a->dx) {
        const PwtA in = {a->dz, 2 * R, 2 * R, k, a->dilation, 1.f, nullptr, 0, 0};
        ProfScope ps("pwt_dx_kernel", 2.0 * k * 2 * R * R * (double)n, (double)n, s);
#define PWT_CALL(NN) hipLaunchKernelGGL(pwt_dx_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_dx, a->dxo, a->seg_lo, a->seg_hi, a->dx, n)
        PWT_R_TILES(PWT_CALL)
#undef PWT_CALL
    }
    if (a->dc) {
        const PwtA in = {a->dz, 2 * R, 2 * R, 1, 1, 1.f, nullptr, 0, 0};
        ProfScope ps("pwt_dc_kernel", 2.0 * 2 * R * A * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    case NN:         \
        hipLaunchKernelGGL(pwt_dc_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_dc, a->seg_lo, a->seg_hi, a->dc, n, a->last); \
        break;
        switch (A / 16) { PWT_CALL(1) PWT_CALL(2) PWT_CALL(3) PWT_CALL(4) PWT_CALL(5) PWT_CALL(6) PWT_CALL(7) PWT_CALL(8) }
#undef PWT_CALL
    }
    return check_hip(hipGetLastError(), "pwt_block_dx");
}

int fcl_pwt_block_dw(const fcl_pwt_t* a, fcl_stream_t stream) {
    const int rc = pwt_check(a, "pwt_block_dw");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->c && a->ab && a->dz && a->ds && a->dw_gate && a->db_gate && a->dw_out && a->db_out && a->workspace, FCL_ERR_INVALID,
                "pwt_block_dw: null x / c / ab / dz / ds / dw_gate / db_gate / dw_out / db_out / workspace");
    FCL_REQUIRE(a->last ? a->dxo == nullptr : a->dxo != nullptr, FCL_ERR_INVALID,
                "pwt_block_dw: dxo (the gradient of x_out) is needed for every block but the last, which has none");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->c) && aligned16(a->ab) && aligned16(a->dz) && aligned16(a->ds) && aligned16(a->dxo), FCL_ERR_ALIGN,
                "pwt_block_dw: x, c, ab, dz, ds and dxo must be 16-byte aligned");
    FCL_REQUIRE(a->workspace_bytes >= fcl_pwt_dw_workspace_bytes(a->samples, a->residual, a->aux, a->ksize), FCL_ERR_WORKSPACE,
                "pwt_block_dw: the workspace holds %zu bytes, fcl_pwt_dw_workspace_bytes asks for %zu", a->workspace_bytes,
                fcl_pwt_dw_workspace_bytes(a->samples, a->residual, a->aux, a->ksize));
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual, A = a->aux, k = a->ksize;
    const unsigned chunks = (unsigned)pwt_chunks(n);
    {
        const int rows = k * R + A, combos = rows / 16 + 1;
        const PwtA in = {a->x, R, R, k, a->dilation, 1.f, a->c, A, A};
        const dim3 grid(chunks, (unsigned)((combos + 3) / 4));
        {
            ProfScope ps("pwt_dw_kernel<gate>", 2.0 * rows * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    hipLaunchKernelGGL((pwt_dw_kernel<PWT_PLAIN, NN>), grid, dim3(256), 0, s, in, a->dz, a->dz + R, 2 * R, 1.f, 1, a->seg_lo, a->seg_hi, a->workspace, n)
            PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
        }
        const int nw = rows * 2 * R, nb = 2 * R;
        ProfScope ps("pwt_dw_reduce_kernel", 0.0, (double)chunks, s);
        hipLaunchKernelGGL(pwt_dw_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, a->workspace, (int)chunks, nw, nb, a->dw_gate,
                           a->db_gate);
    }
    {
        const int combos = R / 16 + 1;
        const PwtA in = {a->ab, 2 * R, R, 1, 1, 1.f, nullptr, 0, 0};
        const dim3 grid(chunks, (unsigned)((combos + 3) / 4));
        const float* b1 = a->dxo ? a->dxo : a->ds;  // (without dxo: a valid address, masked to zero)
        {
            ProfScope ps("pwt_dw_kernel<out>", 2.0 * R * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    hipLaunchKernelGGL((pwt_dw_kernel<PWT_GATED, NN>), grid, dim3(256), 0, s, in, b1, a->ds, R, PWT_SQRT_HALF, a->dxo ? 1 : 0, a->seg_lo, a->seg_hi, a->workspace, n)
            PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
        }
        const int nw = R * 2 * R, nb = 2 * R;
        ProfScope ps("pwt_dw_reduce_kernel", 0.0, (double)chunks, s);
        hipLaunchKernelGGL(pwt_dw_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, a->workspace, (int)chunks, nw, nb, a->dw_out,
                           a->db_out);
    }
    return check_hip(hipGetLastError(), "pwt_block_dw");
}

}  // extern "C"
