// pwg_rows.h -- the exact-fp32 row contraction of the Parallel WaveGAN training kernels, once: pwg_disc.hip (the discriminator) and pwg_train.hip
// (the generator's residual block) keep their epilogues, their small layers and their entries and take from here the keep mask, the utterance
// bounds, the A-operand descriptor, the pipelined MFMA loop (pwr_contract; pwd_conv_kernel keeps a two-operand form of it), the chunked
// weight-gradient kernel and the chunk-order reduce.
//
// Layout: float32, channel-last, packed [samples, C], the utterances back to back; row t's utterance is [seg_lo[t], seg_hi[t]) (both clamped to
// [0, samples]) and a tap outside it contributes zero.  Every contraction is rows x (a few shifted or plain row sources) x a tap-major weight matrix on
// v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain): unconditional loads from clamped rows masked with a bitwise AND, tile counts as template arguments, the
// next step's operands requested before this step's MFMAs, 64-bit row arithmetic, no atomics (weight gradients: per-chunk partials added in ascending chunk
// order by a second launch).
#pragma once
#include "fcl_common.h"

namespace fcl {

constexpr int PWR_ROWS = 128;       // rows per workgroup of the row kernels: 4 waves x 2 tiles of 16 rows
constexpr int PWR_DW_CHUNK = 1024;  // samples per partial of the weight gradients
constexpr int PWR_DW_GROUP = 4;     // MFMA steps (of 4 samples) per register set of pwr_dw_kernel

enum { PWR_PLAIN = 0, PWR_GATED = 1, PWR_RELU = 2 };  // the A operand as stored / g = a * b formed on load from ab [samples, 2 R] / max(s1 p1, 0)

// v where keep, else +0.0, as a bitwise AND: the loaded value is USED whatever keep says, so the compiler cannot move the load under the condition
// (where it would wait for each load on the spot), and whatever an unused lane loaded -- a NaN included -- leaves no trace
__device__ __forceinline__ float pwr_keep(float v, bool keep) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & (keep ? 0xFFFFFFFFu : 0u));
}

__device__ __forceinline__ void pwr_bounds(const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, long long t, long long n, long long& lo,
                                           long long& hi) {
    lo = hi = 0;
    if (t < n) {
        lo = max(0, seg_lo[t]);
        hi = min(n, (long long)seg_hi[t]);
    }
}

// The A operand of a contraction: `taps` shifted views of p1 [samples, ld1] (c1 channels each, tap j at (j - (taps - 1) / 2) dil, times s1), followed by
// p2 [samples, ld2] (c2 channels, unshifted).  Contraction row of the weight matrix: j c1 + channel, then taps c1 + channel of p2.  taps == 0 or c2 == 0
// leaves a source out (its pointer is then never used).  PWR_GATED: p1 is ab [samples, 2 c1] and the value is ab[:, ch] * ab[:, c1 + ch].  PWR_RELU: the
// value is max(s1 p1, 0) (the generator's output end, pwg_ends.hip), in pwr_dw_kernel too, which otherwise takes p1 as stored.
struct PwrA {
    const float* p1;
    int ld1, c1, taps, dil;
    float s1;
    const float* p2;
    int ld2, c2;
};

// acc[mt][nt] = A[t0 + 16 mt + .., :] W[:, 16 nt + ..] for the wave's 32 rows from t0 (the whole width: ldw = 16 NT).  A lane loads 4 consecutive channels
// of its row at once and feeds them to 4 MFMAs, so the contraction index of MFMA s of a 16-channel block is block + 4 (lane >> 4) + s on both operands.
template <int MODE, int NT>
__device__ __forceinline__ void pwr_contract(const PwrA& A, const float* __restrict__ w, const int32_t* __restrict__ seg_lo,
                                             const int32_t* __restrict__ seg_hi, long long n, long long t0, f32x4 (&acc)[2][NT]) {
    constexpr int ldw = NT * 16;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    long long trow[2], lo[2], hi[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        trow[mt] = t0 + mt * 16 + r;
        pwr_bounds(seg_lo, seg_hi, trow[mt], n, lo[mt], hi[mt]);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int half = (A.taps - 1) >> 1;
    const int nb1 = max(A.c1 >> 4, 1), steps1 = A.taps * (A.c1 >> 4), steps = steps1 + (A.c2 >> 4);
    // a step is 16 contraction rows: 2 row loads (4 when gated) and 4 NT weight loads feed 8 NT MFMAs.  The operands of step s + 1 are requested before the
    // MFMAs of step s, so their latency runs under the matrix pipe (the last step requests itself again).  Every load is unconditional -- a row outside the
    // utterance is loaded from a clamped row and replaced by zero -- and the tile count is a template argument: a runtime condition around a load makes the
    // compiler wait for each load where it stands.  Which source a step reads is uniform over the workgroup.
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
            if (MODE == PWR_GATED) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(src + A.c1);
#pragma unroll
                for (int s = 0; s < 4; ++s) a[mt][s] = v[s] * u[s];
            } else if (MODE == PWR_RELU) {
#pragma unroll
                for (int s = 0; s < 4; ++s) a[mt][s] = fmaxf(v[s] * sc, 0.f);
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

// ---- weight gradients: partial[chunk][m][co] = sum over the chunk's samples t of A[t, m] B[t, co], m the contraction rows of PwrA (so the partial has the
// forward weights' layout), and one more row m = rows for the bias gradient sum_t B[t, co] (an A operand of ones in row 0 of a tile).  B [samples, 16 NT] is
// (b1 s1b | b2): NB1 tiles of b1, the rest of b2, both with the leading dimension ldb; b1_live == 0 makes the b1 part exactly zero.  The contraction runs
// over the samples, 4 per MFMA; a wave owns 16 contraction rows x all columns; blockIdx.x is the chunk of PWR_DW_CHUNK samples, blockIdx.y * 4 + wave the
// contraction tile.  No barrier in the kernel: an idle wave returns.  The launch record names it pwd_dw_kernel (NB1 = 0: B = g alone) or
// pwt_dw_kernel<gate / out> (NB1 = NT / 2).  A kernel and not a device function under two wrappers: through a wrapper the generator's instances compile
// to other code than before and <out> ran 5 % slower.
template <int MODE, int NT, int NB1>
__global__ __launch_bounds__(256) void pwr_dw_kernel(PwrA A, const float* __restrict__ b1, const float* __restrict__ b2, int ldb, float s1b, int b1_live,
                                                     const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* __restrict__ partial,
                                                     long long n) {
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
    const long long t_begin = (long long)blockIdx.x * PWR_DW_CHUNK, t_end = min(n, t_begin + PWR_DW_CHUNK);
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const long long last = t_end - 1;
    struct Group {
        int lo[PWR_DW_GROUP], hi[PWR_DW_GROUP];
        float av[PWR_DW_GROUP], bv[PWR_DW_GROUP][NT];
    };
    // Groups of PWR_DW_GROUP steps, two register sets: the loads of group i + 1 are all issued before the MFMAs of group i, and scheduling barriers keep
    // the compiler from moving each load down to its use (where it would wait out one latency per load).  Every load is unconditional, from a clamped
    // row; what a dead lane loaded is masked to zero.  The trip count is fixed: the steps past the chunk's end are dead lanes.
    auto issue = [&](int grp, Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, tc = min(tq, last);
            G.lo[u] = seg_lo[tc];
            G.hi[u] = seg_hi[tc];
            const float* src = ap + min(max(tq + shift, 0LL), n - 1) * lda + mt * 16 + r;
            G.av[u] = MODE == PWR_GATED ? src[0] * src[A.c1] : MODE == PWR_RELU ? fmaxf(src[0] * A.s1, 0.f) : src[0];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) G.bv[u][nt] = nt < NB1 ? b1[tc * ldb + nt * 16 + r] * s1b : b2[tc * ldb + (nt - NB1) * 16 + r];
        }
    };
    auto compute = [&](int grp, const Group& G) {
#pragma unroll
        for (int u = 0; u < PWR_DW_GROUP; ++u) {
            const long long tq = t_begin + 4 * (grp * PWR_DW_GROUP + u) + q, rr = tq + shift;
            const bool live = tq <= last;
            const long long lo = max(0, G.lo[u]), hi = min(n, (long long)G.hi[u]);
            // (branch-free: the row of ones OR the masked activation, never a select between a loaded value and a constant)
            const float a = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, pwr_keep(G.av[u], !ones && live && rr >= lo && rr < hi)) |
                                                          ((ones && live && r == 0) ? 0x3F800000u : 0u));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pwr_keep(G.bv[u][nt], live && (nt >= NB1 || b1_live)), acc[nt], 0, 0, 0);
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

// the partials added in ascending chunk order: elements [0, nw) are dw, [nw, nw + nb) db (db may be null).  (static: one copy per including file)
static __global__ __launch_bounds__(256) void pwr_dw_reduce_kernel(const float* __restrict__ partial, int chunks, int nw, int nb, float* __restrict__ dw,
                                                                   float* __restrict__ db) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nw + nb) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * (nw + nb) + e];
    if (e < nw)
        dw[e] = s;
    else if (db)
        db[e - nw] = s;
}

static long long pwr_chunks(long long samples) { return (samples + PWR_DW_CHUNK - 1) / PWR_DW_CHUNK; }

}  // namespace fcl
