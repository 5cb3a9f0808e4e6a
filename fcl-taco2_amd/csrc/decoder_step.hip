// decoder_step.hip — latency-tuned kernels for the decoder's time loop (H6-H8), gfx950.
//
// The loop is a chain of small dependent contractions (SURVEY.md §7 "sequential dependence"): once the
// live row count drops, a 64-row LDS-staged GEMM tile spends its time in per-chunk barriers, not MFMAs.
// Every kernel here uses 16-row tiles whose activations (full K) sit in LDS once, while every wave takes
// its own W rows straight from L2 into MFMA fragments (no sharing between waves => no LDS round trip).
// Two launches per decoder step, each in several forms that launch_feat_prenet / launch_lstm_small pick:
//   feat/prenet: feat_out(t-1) -> [H10 scatter] -> prenet layer 0 -> prenet layer 1 of step t, three
//   row-local GEMMs chained through LDS in ONE launch
//     * feat_prenet_kernel                          fp32 operands, W streamed (any shape)
//     * feat_prenet_x3_kernel                       bf16x3 planes, W fragments streamed (any shape)
//     * feat_prenet_split_kernel<Ops, DROP, RT>     the student's shape, every W fragment register-resident:
//                                                   OpsX3 (RT = 1, 2 row tiles) and OpsF32 (exact, RT = 1)
//     * feat_prenet_walk_kernel<DROP>               the same on bf16x3 for launches with many row tiles: a workgroup walks several tiles and
//                                                   pulls the weights once (feat_out's fragments in LDS)
//   small LSTM step: one wave per gate (16 rows x 16 units each), gates exchanged through LDS, the LSTMCell +
//   zoneout epilogue one (row, unit) per thread
//     * lstm_small_kernel, lstm_small_pair_kernel   fp32 operands, W streamed; the pair: two steps in one launch
//     * lstm_small_x3_kernel                        bf16x3 planes, W fragments streamed (any K)
//     * lstm_small_resident_kernel<Ops>             K = 256 terms, every W fragment register-resident: OpsX3, OpsF32
// OpsX3 / OpsF32 are the operand policies of the register-resident bodies (below): each body exists once.
#include "fcl_common.h"
#include "lstm_epilogue.h"

namespace fcl {


// acc[t] = A_l[16 x K] . W_t[16 rows x K]^T for NT column tiles that share the A fragments.
// A_l: LDS, row stride lda_l floats.  wrow[t] = &W[(n_t + r16) * ldw] — ALWAYS a valid row (callers clamp the row
// index and discard the surplus columns), so every load is unconditional and stays in flight (guide §5 trap (c)).
// W fragments are fetched one 64-k chunk ahead of the MFMAs that consume them.
// rot: workgroups start the K walk at different 64-k chunks (chunk index rotated by rot) so that the ~150 workgroups
// of a launch do not all request the same weight lines from the same L2 channels at the same moment.
template <int NT>
__device__ __forceinline__ void rowtile_mma(const float* A_l, int lda_l, const float* const (&wrow)[NT], int K, int r16, int kq,
                                            f32x4 (&out)[NT], int rot = 0) {
    f32x4 acc0[NT], acc1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc0[t] = acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* ap = A_l + r16 * lda_l + kq * 4;
    const float* wp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wp[t] = wrow[t] + kq * 4;
    const int nfull = K >> 6;  // whole 64-k chunks
    f32x4 bn[NT][4];
    int cc = nfull > 0 ? rot % nfull : 0;
    if (nfull > 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) bn[t][i] = *reinterpret_cast<const f32x4*>(wp[t] + (cc << 6) + i * 16);
    }
    for (int c = 0; c < nfull; ++c) {
        const int k = cc << 6;
        const int cn = cc + 1 == nfull ? 0 : cc + 1;
        f32x4 b[NT][4], a[4];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) b[t][i] = bn[t][i];
        if (c + 1 < nfull) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) bn[t][i] = *reinterpret_cast<const f32x4*>(wp[t] + (cn << 6) + i * 16);
        }
        cc = cn;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(ap + k + i * 16);
        __builtin_amdgcn_sched_barrier(0);  // keep the next chunk's W loads ABOVE this chunk's MFMAs (hipcc sinks them otherwise)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][0], b[t][i][0], acc0[t], 0, 0, 0);
                acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][1], b[t][i][1], acc1[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][2], b[t][i][2], acc0[t], 0, 0, 0);
                acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][3], b[t][i][3], acc1[t], 0, 0, 0);
            }
        }
    }
    for (int k = nfull << 6; k < K; k += 16) {  // tail: K % 4 == 0, lanes past K contribute zeros
        const bool in = k + kq * 4 < K;
        // lanes past K: keep the address valid (the first float4 of the row -- `wp + 0` would still carry the lane's kq * 4 offset, i.e. up to 12 floats
        // past the end of a row shorter than 16, and past the end of the MATRIX in its last row: a fault when the weight ends a mapped segment) and
        // zero the operand instead of skipping the load
        f32x4 a = *reinterpret_cast<const f32x4*>(in ? ap + k : A_l + r16 * lda_l);
        if (!in) a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(in ? wp[t] + k : wrow[t]);
            acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bb[0], acc0[t], 0, 0, 0);
            acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bb[1], acc1[t], 0, 0, 0);
            acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bb[2], acc0[t], 0, 0, 0);
            acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bb[3], acc1[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) out[t] = acc0[t] + acc1[t];
}

// cooperative load of a [16 x K] row tile (rows m0.., zero beyond M) into LDS with row stride ld_l
__device__ __forceinline__ void load_rowtile(float* dst, int ld_l, const float* src, int ld, int K, int m0, int M) {
    const int per_row = K >> 2;
    for (int i = threadIdx.x; i < 16 * per_row; i += blockDim.x) {
        const int r = i / per_row, c = (i - r * per_row) * 4;
        const int m = min(m0 + r, M - 1);  // clamp (M >= 1): rows past M are computed on a copy and never stored
        *reinterpret_cast<f32x4*>(dst + r * ld_l + c) = *reinterpret_cast<const f32x4*>(src + (size_t)m * ld + c);
    }
}

__device__ __forceinline__ float drop_apply(float v, int mode, const uint8_t* keep, int ldkeep, int m, int n, int N,
                                            float scale, float p, unsigned int seed) {
    if (mode == 1) return keep[(size_t)m * ldkeep + n] ? v * scale : 0.f;
    if (mode == 2) {
        const unsigned int h = hash_u32(((unsigned int)m * (unsigned int)N + (unsigned int)n) ^ seed);
        return ((h >> 8) * (1.0f / 16777216.0f) >= p) ? v * scale : 0.f;
    }
    return v;
}

// Row bounds of a feat/prenet launch.  LOADS and the MFMA chains use the host's bounds a.M_feat / a.M_pre; the STORES are limited to Ms_feat / Ms_pre: the
// host's counts, or -- device-driven loop -- the smaller of the host's bounds and the device's live counts (rows between the two hold stale but finite
// state; the counts' scalar loads are off the kernel's critical path: first use in an epilogue).  Reports a live count above the host's bound in
// a.status; false = this workgroup's `rows` rows lie beyond the live rows (uniform per workgroup, before any barrier): the kernel returns at once.
__device__ __forceinline__ bool feat_prenet_rows(const FeatPrenetArgs& a, int rows, int& Ms_feat, int& Ms_pre) {
    Ms_feat = (a.live && a.t_prev >= 0) ? min(a.M_feat, a.live[a.t_prev]) : a.M_feat;
    Ms_pre = a.live ? min(a.M_pre, a.live[a.t_cur]) : a.M_pre;
    if (a.live && a.w0 && blockIdx.x == 0 && threadIdx.x == 0 && a.live[a.t_cur] > a.M_pre) atomicOr(a.status, (unsigned int)FCL_STATUS_ROWS_CAP);
    if ((int)blockIdx.x * rows >= (a.h1 ? Ms_feat : Ms_pre)) return false;
    return true;
}

__global__ __launch_bounds__(512) void feat_prenet_kernel(const FeatPrenetArgs a) {
    const int M_feat = a.M_feat, M_pre = a.M_pre;
    int Ms_feat, Ms_pre;
    if (!feat_prenet_rows(a, 16, Ms_feat, Ms_pre)) return;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ldU = a.U + 4, ldO = a.O + 4, ldP = a.P + 4;
    float* A1 = smem;            // [16, U]  h1 tile
    float* A2 = A1 + 16 * ldU;   // [16, O]  feat_out / prenet input
    float* A3 = A2 + 16 * ldO;   // [16, P]  prenet layer-0 output
    const int m0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int col = lane & 15, rq = lane >> 4;
    const unsigned int sbump = a.seed_dev ? *a.seed_dev * 0x9E3779B9u : 0u;
    const unsigned int seed0 = hash_u32(a.seed0 + sbump), seed1 = hash_u32(a.seed1 + sbump);

    // ---- H8 feat_out of the previous step (+ H10 scatter) ------------------------------------------
    if (a.h1) {
        load_rowtile(A1, ldU, a.h1, a.U, a.U, m0, M_feat);
        __syncthreads();
        for (int tile = wave; tile * 16 < a.O; tile += nwaves) {
            const float* const wr[1] = {a.wf_h + (size_t)min(tile * 16 + r16, a.O - 1) * a.U};
            const int nc = tile * 16 + col, ncc = min(nc, a.O - 1);
            float f0v[4];
            int fo[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // epilogue operands fetched before the MFMA chain (clamped, unconditional)
                const int mc = min(m0 + rq * 4 + r, M_feat - 1);
                f0v[r] = a.F0[(size_t)mc * a.O + ncc];
                fo[r] = a.frame_off[mc];
            }
            f32x4 accv[1];
            rowtile_mma<1>(A1, ldU, wr, a.U, r16, kq, accv, blockIdx.x);
            const f32x4 acc = accv[0];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rq * 4 + r, m = m0 + row;
                float v = 0.f;
                if (m < Ms_feat && nc < a.O) {
                    v = acc[r] + f0v[r];
                    a.before[(size_t)(fo[r] + a.t_prev) * a.O + nc] = v;
                }
                if (nc < a.O) A2[row * ldO + nc] = (a.out_act && m < Ms_feat) ? act_apply(v, a.out_act) : v;
            }
        }
    } else {
        for (int i = threadIdx.x; i < 16 * ldO; i += blockDim.x) A2[i] = 0.f;  // prev_out = 0 at t = 0
    }
    if (!a.w0 || m0 >= M_pre) return;  // last step: feat only / rows that just finished
    __syncthreads();
    if (a.teacher_in) {  // teacher forcing: prenet input is y_{t-1}, not the decoder's own output
        load_rowtile(A2, ldO, a.teacher_in, a.teacher_ld, a.O, m0, M_pre);
        __syncthreads();
    }
    // ---- H6 prenet layer 0 ---------------------------------------------------------------------------
    for (int tile = wave; tile * 16 < a.P; tile += 2 * nwaves) {
        const int tile2 = tile + nwaves;
        const float* const wr[2] = {a.w0 + (size_t)min(tile * 16 + r16, a.P - 1) * a.O, a.w0 + (size_t)min(tile2 * 16 + r16, a.P - 1) * a.O};
        f32x4 accv[2];
        rowtile_mma<2>(A2, ldO, wr, a.O, r16, kq, accv, blockIdx.x);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (tt ? tile2 : tile) * 16 + col;
            if (nc < a.P) {
                const float bn = a.b0[nc];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rq * 4 + r, m = m0 + row;
                    float v = fmaxf(accv[tt][r] + bn, 0.f);
                    if (m < M_pre) v = drop_apply(v, a.drop_mode, a.keep0, a.P, m, nc, a.P, a.keep_scale, a.drop_p, seed0);
                    A3[row * ldP + nc] = v;
                }
            }
        }
    }
    __syncthreads();
    // ---- H6 prenet layer 1 -> global (+ KD tap) --------------------------------------------------------
    for (int tile = wave; tile * 16 < a.P; tile += 2 * nwaves) {
        const int tile2 = tile + nwaves;
        const float* const wr[2] = {a.w1 + (size_t)min(tile * 16 + r16, a.P - 1) * a.P, a.w1 + (size_t)min(tile2 * 16 + r16, a.P - 1) * a.P};
        f32x4 accv[2];
        rowtile_mma<2>(A3, ldP, wr, a.P, r16, kq, accv, blockIdx.x);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (tt ? tile2 : tile) * 16 + col;
            if (nc < a.P) {
                const float bn = a.b1[nc];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + rq * 4 + r;
                    if (m >= Ms_pre) continue;
                    float v = fmaxf(accv[tt][r] + bn, 0.f);
                    v = drop_apply(v, a.drop_mode, a.keep1, a.P, m, nc, a.P, a.keep_scale, a.drop_p, seed1);
                    a.pre_out[(size_t)m * a.P + nc] = v;
                    if (a.tap_prenet) a.tap_prenet[(size_t)(a.frame_off[m] + a.t_cur) * a.P + nc] = v;
                }
            }
        }
    }
}

// =====================================================================================================
// bf16x3 variants of the two small-tile kernels: activations are split (hi/lo bf16 planes) when they enter LDS,
// weights arrive pre-split (fcl_split_bf16 at plan time) and stream from L2 straight into 16x16x32 bf16 MFMA fragments:
// 3 MFMAs of 16 cycles per 32-k step instead of 8 fp32 MFMAs of 32 cycles, same fp32 accumulators and epilogues.
__device__ __forceinline__ void split1(float x, u16& hi, u16& lo) {
    const __bf16 h = (__bf16)x;
    hi = __builtin_bit_cast(u16, h);
    lo = __builtin_bit_cast(u16, (__bf16)(x - (float)h));
}

// A planes: Ah/Al [16][ldk] bf16 in LDS.  fhi/flo[t]: this lane's slot in the first fragment block of column tile t
// (fragment-major planes, fcl_pack_frag_bf16): step st lives 512 elements further, zero-padded past K.
template <int NT>
__device__ __forceinline__ void rowtile_mma_x3(const u16* Ah, const u16* Al, int ldk, const u16* const (&fhi)[NT], const u16* const (&flo)[NT],
                                               int K, int r16, int kq, f32x4 (&out)[NT]) {
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const u16* ah = Ah + r16 * ldk + kq * 8;
    const u16* al = Al + r16 * ldk + kq * 8;
    const int nsteps = (K + 31) >> 5;
    s16x8 bhn[NT], bln[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        bhn[t] = *reinterpret_cast<const s16x8*>(fhi[t]);
        bln[t] = *reinterpret_cast<const s16x8*>(flo[t]);
    }
    for (int st = 0; st < nsteps; ++st) {
        const int k = st << 5;
        s16x8 bh[NT], bl[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { bh[t] = bhn[t]; bl[t] = bln[t]; }
        if (st + 1 < nsteps) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                bhn[t] = *reinterpret_cast<const s16x8*>(fhi[t] + (size_t)(st + 1) * 512);
                bln[t] = *reinterpret_cast<const s16x8*>(flo[t] + (size_t)(st + 1) * 512);
            }
        }
        s16x8 a_hi = {0, 0, 0, 0, 0, 0, 0, 0}, a_lo = {0, 0, 0, 0, 0, 0, 0, 0};
        if (k + kq * 8 < K) {  // K % 8 == 0; the LDS row holds exactly K valid elements
            a_hi = *reinterpret_cast<const s16x8*>(ah + k);
            a_lo = *reinterpret_cast<const s16x8*>(al + k);
        }
        __builtin_amdgcn_sched_barrier(0);  // next step's W loads stay above this step's MFMAs
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, bh[t], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bl[t], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, bh[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) out[t] = acc[t];
}

// cooperative load of a [16 x K] fp32 row tile, split into the two LDS planes (rows clamped to M-1)
__device__ __forceinline__ void load_rowtile_split(u16* Ah, u16* Al, int ldk, const float* src, int ld, int K, int m0, int M) {
    const int per_row = K >> 2;
    for (int i = threadIdx.x; i < 16 * per_row; i += blockDim.x) {
        const int r = i / per_row, c = (i - r * per_row) * 4;
        const int m = min(m0 + r, M - 1);
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)m * ld + c);
        u16 h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) split1(v[e], h[e], l[e]);
        *reinterpret_cast<uint2*>(Ah + r * ldk + c) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
        *reinterpret_cast<uint2*>(Al + r * ldk + c) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
    }
}

// A thread's share of a [16 x 256] fp32 row tile (rows m0.., clamped to M - 1), in two halves: request() issues the four float4 loads and nothing else,
// so that a caller can have several tiles and its weight fragments in flight before the first wait; the store halves then split into the two LDS planes
// (split_store, element mapping and rounding of load_rowtile_split) or copy (store).  256 threads.
struct RowTile256 {
    f32x4 v[4];
    __device__ __forceinline__ void request(const float* src, int ld, int m0, int M) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = threadIdx.x + j * 256, r = i >> 6, c = (i & 63) * 4;
            v[j] = *reinterpret_cast<const f32x4*>(src + (size_t)min(m0 + r, M - 1) * ld + c);
        }
    }
    __device__ __forceinline__ void split_store(u16* Ah, u16* Al, int ldk) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = threadIdx.x + j * 256, r = i >> 6, c = (i & 63) * 4;
            u16 h[4], l[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split1(v[j][e], h[e], l[e]);
            *reinterpret_cast<uint2*>(Ah + r * ldk + c) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
            *reinterpret_cast<uint2*>(Al + r * ldk + c) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
        }
    }
    __device__ __forceinline__ void store(float* dst, int ld_l) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = threadIdx.x + j * 256, r = i >> 6, c = (i & 63) * 4;
            *reinterpret_cast<f32x4*>(dst + r * ld_l + c) = v[j];
        }
    }
};

// The streaming bf16x3 form, for the shapes feat_prenet_split_kernel does not cover: any U / O / P (multiples of 8), every wave walking its column
// tiles' weight fragments from L2 one 32-k step ahead of the MFMAs (rowtile_mma_x3).
__global__ __launch_bounds__(512) void feat_prenet_x3_kernel(const FeatPrenetArgs a) {
    const int M_feat = a.M_feat, M_pre = a.M_pre;
    // feat_prenet_rows, spelled out: through the helper this kernel (alone) compiles to a different schedule
    const int Ms_feat = (a.live && a.t_prev >= 0) ? min(a.M_feat, a.live[a.t_prev]) : a.M_feat, Ms_pre = a.live ? min(a.M_pre, a.live[a.t_cur]) : a.M_pre;
    if (a.live && a.w0 && blockIdx.x == 0 && threadIdx.x == 0 && a.live[a.t_cur] > a.M_pre) atomicOr(a.status, (unsigned int)FCL_STATUS_ROWS_CAP);
    if ((int)blockIdx.x * (16) >= (a.h1 ? Ms_feat : Ms_pre)) return;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ldU = a.U + 8, ldO = a.O + 8, ldP = a.P + 8;  // bf16 elements per plane row
    u16* A1h = reinterpret_cast<u16*>(smem);
    u16* A1l = A1h + 16 * ldU;
    u16* A2h = A1l + 16 * ldU;
    u16* A2l = A2h + 16 * ldO;
    u16* A3h = A2l + 16 * ldO;
    u16* A3l = A3h + 16 * ldP;
    const int m0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int col = lane & 15, rq = lane >> 4;
    const unsigned int sbump = a.seed_dev ? *a.seed_dev * 0x9E3779B9u : 0u;
    const unsigned int seed0 = hash_u32(a.seed0 + sbump), seed1 = hash_u32(a.seed1 + sbump);

    const bool has_pre = a.w0 && m0 < M_pre;
    const int ptile = wave, ptile2 = wave + nwaves;  // this wave's column tiles in the first pass of the prenet layers' tile loops
    const int nsU = (a.U + 31) >> 5, nsO = (a.O + 31) >> 5, nsP = (a.P + 31) >> 5, ptmax = ((a.P + 15) >> 4) - 1;
    const size_t lane8 = (size_t)lane * 8;
    auto frag = [&](const u16* base, int tile, int ns) { return base + (size_t)tile * ns * 512 + lane8; };
    // epilogue biases of this wave's two prenet column tiles: requested now, consumed two / three barriers later (they used to be dependent
    // global loads behind each layer's MFMA chain: ~1 us of exposed latency each on the step's critical path)
    float pb0[2] = {0.f, 0.f}, pb1[2] = {0.f, 0.f};
    if (has_pre) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = min((tt ? ptile2 : ptile) * 16 + col, a.P - 1);
            pb0[tt] = a.b0[nc];
            pb1[tt] = a.b1[nc];
        }
    }
    if (a.h1) {
        f32x4 accv[1];
        load_rowtile_split(A1h, A1l, ldU, a.h1, a.U, a.U, m0, M_feat);
        __syncthreads();
        for (int tile = wave; tile * 16 < a.O; tile += nwaves) {
            const u16* const wh[1] = {frag(a.wf_hi, tile, nsU)};
            const u16* const wl[1] = {frag(a.wf_lo, tile, nsU)};
            const int nc = tile * 16 + col, ncc = min(nc, a.O - 1);
            float f0v[4];
            int fo[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mc = min(m0 + rq * 4 + r, M_feat - 1);
                f0v[r] = a.F0[(size_t)mc * a.O + ncc];
                fo[r] = a.frame_off[mc];
            }
            rowtile_mma_x3<1>(A1h, A1l, ldU, wh, wl, a.U, r16, kq, accv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rq * 4 + r, m = m0 + row;
                float v = 0.f;
                if (m < Ms_feat && nc < a.O) {
                    v = accv[0][r] + f0v[r];
                    a.before[(size_t)(fo[r] + a.t_prev) * a.O + nc] = v;
                    if (a.before_p) store_p32(a.before_p, (a.O + 31) >> 5, fo[r] + a.t_prev, nc, v);
                }
                if (nc < a.O) split1((a.out_act && m < Ms_feat) ? act_apply(v, a.out_act) : v, A2h[row * ldO + nc], A2l[row * ldO + nc]);
            }
        }
        if (a.before_p && (a.O & 31)) {  // zero padding of the last 32-column line of this tile's frames
            const int padc = 32 - (a.O & 31);
            for (int i = threadIdx.x; i < 16 * padc; i += blockDim.x) {
                const int m = m0 + i / padc;
                if (m < Ms_feat) store_p32(a.before_p, (a.O + 31) >> 5, a.frame_off[m] + a.t_prev, a.O + i % padc, 0.f);
            }
        }
    } else {
        for (int i = threadIdx.x; i < 16 * ldO; i += blockDim.x) { A2h[i] = 0; A2l[i] = 0; }  // prev_out = 0 at t = 0
    }
    if (!has_pre) return;
    lds_barrier();  // NOT __syncthreads(): its vmcnt(0) would wait for the prefetched biases, which nothing needs before an epilogue
    if (a.teacher_in) {
        load_rowtile_split(A2h, A2l, ldO, a.teacher_in, a.teacher_ld, a.O, m0, M_pre);
        __syncthreads();
    }
    for (int tile = wave; tile * 16 < a.P; tile += 2 * nwaves) {
        const int tile2 = tile + nwaves;
        const u16* const wh[2] = {frag(a.w0_hi, tile, nsO), frag(a.w0_hi, min(tile2, ptmax), nsO)};
        const u16* const wl[2] = {frag(a.w0_lo, tile, nsO), frag(a.w0_lo, min(tile2, ptmax), nsO)};
        f32x4 accv[2];
        rowtile_mma_x3<2>(A2h, A2l, ldO, wh, wl, a.O, r16, kq, accv);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (tt ? tile2 : tile) * 16 + col;
            if (nc < a.P) {
                const float bn = tile == ptile ? pb0[tt] : a.b0[nc];  // first pass of the tile loop: the prefetched value
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rq * 4 + r, m = m0 + row;
                    float v = fmaxf(accv[tt][r] + bn, 0.f);
                    if (m < M_pre) v = drop_apply(v, a.drop_mode, a.keep0, a.P, m, nc, a.P, a.keep_scale, a.drop_p, seed0);
                    split1(v, A3h[row * ldP + nc], A3l[row * ldP + nc]);
                }
            }
        }
    }
    lds_barrier();
    for (int tile = wave; tile * 16 < a.P; tile += 2 * nwaves) {
        const int tile2 = tile + nwaves;
        const u16* const wh[2] = {frag(a.w1_hi, tile, nsP), frag(a.w1_hi, min(tile2, ptmax), nsP)};
        const u16* const wl[2] = {frag(a.w1_lo, tile, nsP), frag(a.w1_lo, min(tile2, ptmax), nsP)};
        f32x4 accv[2];
        rowtile_mma_x3<2>(A3h, A3l, ldP, wh, wl, a.P, r16, kq, accv);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (tt ? tile2 : tile) * 16 + col;
            if (nc < a.P) {
                const float bn = tile == ptile ? pb1[tt] : a.b1[nc];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + rq * 4 + r;
                    if (m >= Ms_pre) continue;
                    float v = fmaxf(accv[tt][r] + bn, 0.f);
                    v = drop_apply(v, a.drop_mode, a.keep1, a.P, m, nc, a.P, a.keep_scale, a.drop_p, seed1);
                    if (a.pre_out) a.pre_out[(size_t)m * a.P + nc] = v;
                    if (a.pre_out_p) store_p32(a.pre_out_p, (a.P + 31) >> 5, m, nc, v);
                    if (a.tap_prenet) a.tap_prenet[(size_t)(a.frame_off[m] + a.t_cur) * a.P + nc] = v;
                }
            }
        }
    }
}

// ---- the same chain for the student's shape (U = P = 256, 64 < O <= 96) with every weight fragment register-resident and TRANSPOSED accumulators.
// With the activations as the MFMA's A operand a lane ends up with ONE column of FOUR rows, and every finished element costs its own bias / mask
// load, counter hash, fp32 -> (hi, lo) split, two 2-byte LDS stores and up to five scattered global stores.  Swapping the operands (weights as A,
// activations as B: the same fragments, the same products in the same order, D^T instead of D) gives a lane FOUR CONSECUTIVE COLUMNS of ONE row: one
// float4 bias / F0 load, one 4-byte mask load, two hashes (16 bits per decision), one packed split, two 8-byte LDS stores = the next layer's
// operand, and 8- / 16-byte global stores -- about a quarter of the instructions.
// A workgroup owns RT row tiles of 16 rows and all 256 columns (82 + 98 + 262 KB of fragments).  The layer-1 operand tile re-uses the h1 tile's LDS
// (96 KB at RT = 4).  The h1 rows, then feat_out's and layer 0's fragments are requested at entry, layer 1's once feat_out's registers are free; no
// __syncthreads (its vmcnt(0) would wait for every fragment before the first phase).
// RNG mode draws a different (equally distributed) stream than the other feat/prenet kernels: 16 bits of a counter hash per decision instead of 24.
// The exact fp32 form (OpsF32; launched with one row tile, without teacher input or plane outputs) replaces feat_prenet_kernel where the shape is covered:
// there the weights were re-streamed from L2 at every k-step, 19.2 us per launch at 2 400 rows, the largest item of the exact-mode pass.
__device__ __forceinline__ void p32_store4(unsigned short* __restrict__ p, int ld, long long m, int n, uint2 hi, uint2 lo) {
    unsigned short* line = p + ((size_t)m * ld + (n >> 5)) * 64 + (n & 31);
    *reinterpret_cast<uint2*>(line) = hi;
    *reinterpret_cast<uint2*>(line + 32) = lo;
}

// ---- operand policies of the register-resident kernels (feat_prenet_split_kernel and lstm_small_resident_kernel, below): everything that differs
// between the bf16x3 form (OpsX3: hi / lo bf16 planes in LDS and in the fragment-major weights, fcl_pack_frag_bf16) and the exact fp32 form (OpsF32:
// FCL_PRECISION=0, fp32 tiles and fragment-major fp32 weights, fcl_pack_frag_f32, v_mfma_f32_16x16x4_f32).  The kernel bodies exist once.
//   W     the fragment-major weights of one layer / term; at(): a (uniform, per-lane) element offset into each plane
//   Tile  an LDS row tile (rows PAD elements apart beyond K: 2 (mod 4) sixteen-byte slots, conflict-free fragment reads); carve(): the next n elements of the
//         dynamic LDS; fixed<N>(): static LDS
//   Frag  register-resident W fragments.  The weights do not depend on the activation chain, so a wave can request ALL the fragments it will need
//         (NS 32-k steps x NT column tiles) up front and pay the L2 / Infinity-Cache latency once per kernel instead of once per k-step; the MFMAs then
//         issue back to back from registers.  load<S0, S1>: k-steps S0 .. S1 - 1 (a caller short of registers requests the last steps later); every
//         wave-wide load is one contiguous 1 KB block (a lane's two float4 of an fp32 fragment are exactly the bytes of its hi + lo pair).
//         mma_t: the weight fragment as the MFMA's A operand -- transposed accumulators, four consecutive columns of one row per lane.
//   kPlanes        the plane outputs (before_p, pre_out_p) and the teacher input exist for this form: compiled out of the other
//   kUnitsInLane   the small step's accumulator layout (gates_to_cell): the bf16x3 step keeps the activations as the A operand (Frag::mma_small)
struct OpsX3 {
    static constexpr bool kPlanes = true, kUnitsInLane = false;
    static constexpr int PAD = 16, LDS_BYTES = 2 * sizeof(u16);  // (per tile element)
    struct W {
        const u16 *hi, *lo;
        __device__ __forceinline__ W at(size_t o, size_t o2 = 0) const { return {hi + o + o2, lo + o + o2}; }
    };
    struct Tile {
        u16 *h, *l;
        __device__ __forceinline__ Tile at(int o) const { return {h + o, l + o}; }
        static __device__ __forceinline__ Tile carve(u16*& p, int n) {
            u16* b = p;
            p += 2 * n;
            return {b, b + n};
        }
        template <int N>
        static __device__ __forceinline__ Tile fixed() {  // a tile of the workgroup's static LDS: two arrays (one array of both planes compiles to other code)
            __shared__ __attribute__((aligned(16))) u16 A_h[N];
            __shared__ __attribute__((aligned(16))) u16 A_lo[N];
            return {A_h, A_lo};
        }
    };
    template <int NT, int NS>
    struct Frag {
        s16x8 hi[NT][NS], lo[NT][NS];
        template <int S0 = 0, int S1 = NS>
        __device__ __forceinline__ void load(const W (&w)[NT]) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int st = S0; st < S1; ++st) {
                    hi[t][st] = *reinterpret_cast<const s16x8*>(w[t].hi + st * 512);
                    lo[t][st] = *reinterpret_cast<const s16x8*>(w[t].lo + st * 512);
                }
        }
        // out = A . W^T, hi / lo products in the order lo.hi, hi.lo, hi.hi.  W_IS_A: the weight fragment is the MFMA's A operand (D^T: a lane holds four
        // consecutive columns of one row); otherwise the activations are (four rows of one column).  Same products, same order, either way.
        template <bool W_IS_A>
        __device__ __forceinline__ void chain(Tile A, int ldk, int r16, int kq, f32x4 (&out)[NT]) const {
            auto mfma = [](s16x8 w, s16x8 a, f32x4 c) {
                return W_IS_A ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w, c, 0, 0, 0);
            };
            f32x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const u16* ah = A.h + r16 * ldk + kq * 8;
            const u16* al = A.l + r16 * ldk + kq * 8;
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const s16x8 a_hi = *reinterpret_cast<const s16x8*>(ah + st * 32);
                const s16x8 a_lo = *reinterpret_cast<const s16x8*>(al + st * 32);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = mfma(hi[t][st], a_lo, acc[t]);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = mfma(lo[t][st], a_hi, acc[t]);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = mfma(hi[t][st], a_hi, acc[t]);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) out[t] = acc[t];
        }
        __device__ __forceinline__ void mma_t(Tile A, int ldk, int r16, int kq, f32x4 (&out)[NT]) const { chain<true>(A, ldk, r16, kq, out); }
        __device__ __forceinline__ void mma_small(Tile A, int ldk, int r16, int kq, f32x4 (&out)[NT]) const { chain<false>(A, ldk, r16, kq, out); }
    };
    static __device__ __forceinline__ u16* dynamic_lds() {
        extern __shared__ __attribute__((aligned(16))) u16 x3_lds[];
        return x3_lds;
    }
    static __device__ __forceinline__ W wf(const FeatPrenetArgs& a) { return {a.wf_hi, a.wf_lo}; }
    static __device__ __forceinline__ W w0(const FeatPrenetArgs& a) { return {a.w0_hi, a.w0_lo}; }
    static __device__ __forceinline__ W w1(const FeatPrenetArgs& a) { return {a.w1_hi, a.w1_lo}; }
    static __device__ __forceinline__ W w(const GemmTerm& t) { return {t.Whi, t.Wlo}; }
    static __device__ __forceinline__ void store4(Tile t, int row, int ld, int col, const f32x4 v) {  // columns col .. col + 3 of a row
        uint2 h, l;
        split4(v, h, l);
        *reinterpret_cast<uint2*>(t.h + row * ld + col) = h;
        *reinterpret_cast<uint2*>(t.l + row * ld + col) = l;
    }
    static __device__ __forceinline__ void store_rows(const RowTile256& r, Tile t, int ld) { r.split_store(t.h, t.l, ld); }
    static __device__ __forceinline__ void zero(Tile t, int n) {  // n elements, 512 threads
        for (int i = threadIdx.x; i < n / 8; i += 512) {
            reinterpret_cast<uint4*>(t.h)[i] = make_uint4(0, 0, 0, 0);
            reinterpret_cast<uint4*>(t.l)[i] = make_uint4(0, 0, 0, 0);
        }
    }
};

struct OpsF32 {
    static constexpr bool kPlanes = false, kUnitsInLane = true;
    static constexpr int PAD = 8, LDS_BYTES = sizeof(float);
    struct W {
        const float* f;
        __device__ __forceinline__ W at(size_t o, size_t o2 = 0) const { return {f + o + o2}; }
    };
    struct Tile {
        float* p;
        __device__ __forceinline__ Tile at(int o) const { return {p + o}; }
        static __device__ __forceinline__ Tile carve(float*& p, int n) {
            float* b = p;
            p += n;
            return {b};
        }
        template <int N>
        static __device__ __forceinline__ Tile fixed() {
            __shared__ __attribute__((aligned(16))) float A_f[N];
            return {A_f};
        }
    };
    template <int NT, int NS>
    struct Frag {
        f32x4 w0[NT][NS], w1[NT][NS];
        template <int S0 = 0, int S1 = NS>
        __device__ __forceinline__ void load(const W (&w)[NT]) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int st = S0; st < S1; ++st) {
                    w0[t][st] = *reinterpret_cast<const f32x4*>(w[t].f + st * 512);
                    w1[t][st] = *reinterpret_cast<const f32x4*>(w[t].f + st * 512 + 4);
                }
        }
        __device__ __forceinline__ void mma_t(Tile A, int ldk, int r16, int kq, f32x4 (&out)[NT]) const {
            f32x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* a = A.p + r16 * ldk + kq * 4;
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + st * 32), a1 = *reinterpret_cast<const f32x4*>(a + st * 32 + 16);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[t][st][e], a0[e], acc[t], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[t][st][e], a1[e], acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) out[t] = acc[t];
        }
        __device__ __forceinline__ void mma_small(Tile A, int ldk, int r16, int kq, f32x4 (&out)[NT]) const { mma_t(A, ldk, r16, kq, out); }
    };
    static __device__ __forceinline__ float* dynamic_lds() {
        extern __shared__ __attribute__((aligned(16))) float f32_lds[];
        return f32_lds;
    }
    static __device__ __forceinline__ W wf(const FeatPrenetArgs& a) { return {a.wf_ff}; }
    static __device__ __forceinline__ W w0(const FeatPrenetArgs& a) { return {a.w0_ff}; }
    static __device__ __forceinline__ W w1(const FeatPrenetArgs& a) { return {a.w1_ff}; }
    static __device__ __forceinline__ W w(const GemmTerm& t) { return {t.Wff}; }
    static __device__ __forceinline__ void store4(Tile t, int row, int ld, int col, const f32x4 v) { *reinterpret_cast<f32x4*>(t.p + row * ld + col) = v; }
    static __device__ __forceinline__ void store_rows(const RowTile256& r, Tile t, int ld) { r.store(t.p, ld); }
    static __device__ __forceinline__ void zero(Tile t, int n) {
        for (int i = threadIdx.x; i < n / 4; i += 512) reinterpret_cast<f32x4*>(t.p)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
};

// Developer aid, compiled out unless the library is built with EXTRA=-DFCL_FP_TS (then FCL_FP_TS=1 at run time prints, after every register-resident
// bf16x3 feat/prenet launch, where its waves spent their cycles; synchronous, not usable under graph capture).  Eight s_memtime stamps per wave, kept in
// scalar registers and written once at exit to a buffer of their own:
//   0 entry   1 h1 rows arrived and split into LDS   2 the barrier after it   3 phase 1 done (feat_out: its MFMAs wait for feat_out's fragments)
//   4 the barrier(s) after it   5 phase 2 and its barrier (layer 0's fragments)   6 every request of the wave has landed (a vmcnt(0) that only this
//   build executes: from here on phase 3 waits for nothing)   7 exit.  The walker stamps 0 - 6 on its first tile.
#ifdef FCL_FP_TS
constexpr int kFpTsWorkgroups = 1024;
__device__ long long g_fp_ts[kFpTsWorkgroups * 8 * 8];
struct FpStamps {
    long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    template <int I>
    __device__ __forceinline__ void at(bool drain = false) {
        __builtin_amdgcn_sched_barrier(0);
        if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t[I])::"memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void flush() {
        at<7>();
        if ((threadIdx.x & 63) == 0 && blockIdx.x < kFpTsWorkgroups) {
#pragma unroll
            for (int i = 0; i < 8; ++i) g_fp_ts[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + i] = t[i];
        }
    }
};
#define FP_STAMP(ts, i, ...) ts.at<i>(__VA_ARGS__)
#define FP_STAMP_FLUSH(ts) ts.flush()
#else
struct FpStamps {};
#define FP_STAMP(ts, i, ...)
#define FP_STAMP_FLUSH(ts)
#endif

template <class Ops, int DROP, int RT>
__global__ __launch_bounds__(512) void feat_prenet_split_kernel(const FeatPrenetArgs a) {
    typedef typename Ops::Tile Tile;
    constexpr int SU = 8, SO = 3, SP = 8, U = 256, OP = 96, P = 256;
    const int M_feat = a.M_feat, M_pre = a.M_pre;
    int Ms_feat, Ms_pre;
    if (!feat_prenet_rows(a, 16 * RT, Ms_feat, Ms_pre)) return;
    [[maybe_unused]] FpStamps ts;
    FP_STAMP(ts, 0);
    constexpr int ldU = U + Ops::PAD, ldO = OP + Ops::PAD, ldP = P + Ops::PAD, ROWS = 16 * RT;
    static_assert(ldU == ldP, "the layer-1 operand tile re-uses the h1 tile's LDS");
    auto* lds = Ops::dynamic_lds();
    const Tile A1 = Tile::carve(lds, ROWS * ldU);  // h1 tile
    const Tile A2 = Tile::carve(lds, ROWS * ldO);  // feat_out / prenet input
    const Tile A3 = A1;  // layer 0's output: written in phase 2, when every wave is past its last read of the h1 tile (the barrier that ends phase 1)
    const int O = a.O;
    const int m0 = blockIdx.x * ROWS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kq = lane >> 4;   // operand fragments: row / column r16, k-group kq
    const int arow = lane & 15, cq = lane >> 4;  // transposed accumulators: activation row arow, columns cq * 4 .. cq * 4 + 3 of the column tile
    const bool has_feat = a.h1 != nullptr, has_pre = a.w0 != nullptr && m0 < M_pre;
    const bool feat_wave = has_feat && wave * 16 < O;
    const size_t lane8 = (size_t)lane * 8;
    auto frag = [&](const typename Ops::W w, int tile, int ns) { return w.at((size_t)tile * ns * 512, lane8); };  // (the uniform offset first: a scalar add)
    const int t0 = wave, t1 = wave + 8;  // this wave's layer-0 column tiles
    const int c1 = wave * 2;  // first of this wave's two layer-1 column tiles

    // ---- phase 0 operands first (loads return in order: the first wait then covers the h1 rows alone) ---------------------------------------
    constexpr int HV = RT * 2;  // float4 loads of h1 per thread: ROWS x 64 float4 over 512 threads
    f32x4 hreg[HV];
    if (has_feat) {
#pragma unroll
        for (int j = 0; j < HV; ++j) {
            const int i = threadIdx.x + j * 512, r = i >> 6, c = (i & 63) * 4;
            hreg[j] = *reinterpret_cast<const f32x4*>(a.h1 + (size_t)min(m0 + r, M_feat - 1) * U + c);
        }
    }
    // The CU's address path serves its 8 waves' requests in ISSUE order (one 1 KB wave-load per 16 clocks): a wave that runs ahead and queues its 30 - 44
    // fragment loads puts them in front of the other waves' h1 loads, and phase 0 ends at a barrier -- so the phase used to wait for ~2 us of weight
    // traffic it does not need (r4).  An s_barrier (no data wait: ~100 clocks) between the request groups makes the queue's order the order of use:
    // every wave's h1 rows, then feat_out's fragments, then layer 0's, then layer 1's.
    asm volatile("s_barrier" ::: "memory");
    // ---- weight fragments and epilogue operands of phases 1 and 2, requested now ------------------------------------------------------------------
    typename Ops::template Frag<1, SU> ff;
    typename Ops::template Frag<2, SO> f0;
    typename Ops::template Frag<2, SP> f1;
    const int fnc = wave * 16 + cq * 4;  // feat_out columns fnc .. fnc + 3 of this lane (whole groups of four: O % 4 == 0)
    f32x4 f0v[RT];
    int fo[RT];
    if (feat_wave) {
        const typename Ops::W w[1] = {frag(Ops::wf(a), wave, SU)};
        ff.load(w);
    }
#pragma unroll
    for (int q = 0; q < RT; ++q) {
        f0v[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        fo[q] = 0;
        if (feat_wave && fnc < O) {
            const int mc = min(m0 + q * 16 + arow, M_feat - 1);
            f0v[q] = *reinterpret_cast<const f32x4*>(a.F0 + (size_t)mc * O + fnc);
            fo[q] = a.frame_off[mc];
        }
    }
    unsigned int seed0 = 0, seed1 = 0;
    const unsigned int thr16 = (unsigned int)(a.drop_p * 65536.0f);
    if (DROP == 2) {
        const unsigned int sbump = a.seed_dev ? *a.seed_dev * 0x9E3779B9u : 0u;
        seed0 = hash_u32(a.seed0 + sbump);
        seed1 = hash_u32(a.seed1 + sbump);
    }
    f32x4 pb0[2], pb1[2];
    unsigned int k0[RT][2], k1[RT][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) pb0[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (has_feat) asm volatile("s_barrier" ::: "memory");  // (feat_out's fragments are queued before anybody's layer-0 fragments)
    if (has_pre) {
        const typename Ops::W w[2] = {frag(Ops::w0(a), t0, SO), frag(Ops::w0(a), t1, SO)};
        f0.load(w);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (tt ? t1 : t0) * 16 + cq * 4;
            pb0[tt] = *reinterpret_cast<const f32x4*>(a.b0 + nc);
            if (DROP == 1) {
#pragma unroll
                for (int q = 0; q < RT; ++q) k0[q][tt] = *reinterpret_cast<const unsigned int*>(a.keep0 + (size_t)min(m0 + q * 16 + arow, M_pre - 1) * P + nc);
            }
        }
    }
    // ---- phase 0: h1 tiles -> LDS planes; prenet-input tiles zeroed (prev_out = 0 at t = 0; zero padding past O otherwise) ------------------
    Ops::zero(A2, ROWS * ldO);
    if (has_feat) {
#pragma unroll
        for (int j = 0; j < HV; ++j) {
            const int i = threadIdx.x + j * 512, r = i >> 6, c = (i & 63) * 4;
            Ops::store4(A1, r, ldU, c, hreg[j]);
        }
    }
    FP_STAMP(ts, 1);
    // layer-1 fragments (all 16 column tiles: 128 VGPRs) and epilogue operands: requested after phase 1, once feat_out's fragments are dead
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) pb1[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto request_l1 = [&]() {
        if (has_pre) {
            typename Ops::W w[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) w[tt] = frag(Ops::w1(a), c1 + tt, SP);
            f1.load(w);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int nc = (c1 + tt) * 16 + cq * 4;
                pb1[tt] = *reinterpret_cast<const f32x4*>(a.b1 + nc);
                if (DROP == 1) {
#pragma unroll
                    for (int q = 0; q < RT; ++q) k1[q][tt] = *reinterpret_cast<const unsigned int*>(a.keep1 + (size_t)min(m0 + q * 16 + arow, M_pre - 1) * P + nc);
                }
            }
        }
    };
    lds_barrier();
    FP_STAMP(ts, 2);
    // ---- phase 1: H8 feat_out of the previous step (+ H10 scatter) ---------------------------------------------------------------------------
    if (feat_wave) {
#pragma unroll
        for (int q = 0; q < RT; ++q) {
            f32x4 accv[1];
            ff.mma_t(A1.at(q * 16 * ldU), ldU, r16, kq, accv);
            const int row = q * 16 + arow, m = m0 + row;
            if (fnc < O) {
                f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (m < Ms_feat) {
                    v = accv[0] + f0v[q];
                    const long long fr = (long long)fo[q] + a.t_prev;
                    *reinterpret_cast<f32x4*>(a.before + (size_t)fr * O + fnc) = v;
                    if constexpr (Ops::kPlanes) {
                        if (a.before_p) {
                            uint2 h, l;
                            split4(v, h, l);
                            p32_store4(a.before_p, (O + 31) >> 5, fr, fnc, h, l);
                        }
                    }
                    if (a.out_act) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = act_apply(v[r], a.out_act);
                    }
                }
                Ops::store4(A2, row, ldO, fnc, v);
            }
        }
    }
    if (Ops::kPlanes && has_feat && a.before_p && (O & 31)) {  // zero padding of the last 32-column line of this tile's frames
        const int padc = 32 - (O & 31);
        for (int i = threadIdx.x; i < ROWS * padc; i += 512) {
            const int m = m0 + i / padc;
            if (m < Ms_feat) store_p32(a.before_p, (O + 31) >> 5, a.frame_off[m] + a.t_prev, O + i % padc, 0.f);
        }
    }
    FP_STAMP(ts, 3);
    if (!has_pre) {
        FP_STAMP_FLUSH(ts);
        return;
    }
    request_l1();
    lds_barrier();
    if constexpr (Ops::kPlanes) {
        if (a.teacher_in) {  // teacher forcing: prenet input is y_{t-1}, not the decoder's own output
#pragma unroll
            for (int q = 0; q < RT; ++q) load_rowtile_split(A2.h + q * 16 * ldO, A2.l + q * 16 * ldO, ldO, a.teacher_in, a.teacher_ld, O, m0 + q * 16, M_pre);
            lds_barrier();
        }
    }
    FP_STAMP(ts, 4);
    // ---- phase 2: H6 prenet layer 0 -> LDS (over the h1 tile) ----------------------------------------------------------------------------------
#pragma unroll
    for (int q = 0; q < RT; ++q) {
        f32x4 accv[2];
        f0.mma_t(A2.at(q * 16 * ldO), ldO, r16, kq, accv);
        const int row = q * 16 + arow, m = m0 + row;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (tt ? t1 : t0) * 16 + cq * 4;
            f32x4 v = accv[tt] + pb0[tt];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            v = drop4<DROP>(v, DROP == 1 ? k0[q][tt] : 0u, (unsigned int)m * (unsigned int)P + (unsigned int)nc, seed0, thr16, a.keep_scale);
            Ops::store4(A3, row, ldP, nc, v);
        }
    }
    lds_barrier();
    FP_STAMP(ts, 5);
    FP_STAMP(ts, 6, true);
    // ---- phase 3: H6 prenet layer 1 -> global (+ KD tap, + P32 planes) --------------------------------------------------------------------------
#pragma unroll
    for (int q = 0; q < RT; ++q) {
        f32x4 accv[2];
        f1.mma_t(A3.at(q * 16 * ldP), ldP, r16, kq, accv);
        const int m = m0 + q * 16 + arow;
        if (m >= Ms_pre) continue;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int nc = (c1 + tt) * 16 + cq * 4;
            f32x4 v = accv[tt] + pb1[tt];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            v = drop4<DROP>(v, DROP == 1 ? k1[q][tt] : 0u, (unsigned int)m * (unsigned int)P + (unsigned int)nc, seed1, thr16, a.keep_scale);
            if (a.pre_out) *reinterpret_cast<f32x4*>(a.pre_out + (size_t)m * P + nc) = v;
            if constexpr (Ops::kPlanes) {
                if (a.pre_out_p) {
                    uint2 h, l;
                    split4(v, h, l);
                    p32_store4(a.pre_out_p, SP, m, nc, h, l);
                }
            }
            if (a.tap_prenet) *reinterpret_cast<f32x4*>(a.tap_prenet + (size_t)(a.frame_off[m] + a.t_cur) * P + nc) = v;
        }
    }
    FP_STAMP_FLUSH(ts);
}

// ---- the row-walking form of feat_prenet_split_kernel<OpsX3, DROP, 1>: a workgroup takes `ntw` consecutive row tiles and pulls the weights ONCE.
// The one-tile kernel loads all 430 KB of fragments to use them on 16 rows; at 50 - 160 row tiles a launch that is 40 - 70 MB through the per-CU
// vector-memory path.  Here
//   * layer 0's and layer 1's fragments stay register-resident (48 + 128 VGPRs) and are requested at entry, together: feat_out's fragments are not in
//     registers any more, so layer 1's need not wait for them to die;
//   * feat_out's fragments go to LDS once, by LDS-DMA (a wave's fragment-major loads are contiguous 1 KB blocks, so the image is lane-linear: the
//     fragment of k-step st is one 16-byte read at lane * 16; wave w reads only what wave w requested); the biases go to LDS too (16 registers);
//   * the first tile is a copy of the tile body of its own, in front of the loop: its phases 0 - 2 run while layer 1's fragments are still landing
//     (counted waits), and in the loop the only loads ever in flight are the NEXT tile's operands, so that no wait there takes in anything else;
//   * the h1 / prenet-input tiles are double-buffered.  The next tile's h1 rows, F0 rows and frame offsets are requested right after phase 1 (into
//     the registers phase 1 has just read for the last time; the keep bytes likewise after phases 2 and 3) and are taken in at ONE point, between
//     phase 3's MFMAs and its stores -- a wait placed after those stores would wait for them too, stores and loads retiring in issue order.  So an
//     extra tile costs its MFMAs, epilogues and three barriers, not a memory round trip.
// Per tile the phases, products, their order, the hash inputs and every epilogue are those of the one-tile kernel: every output is bit-identical.
// Dynamic LDS: ceil(O / 16) x 16 KB of fragments + 2 x 24 KB of tiles + 2 KB of biases = 130 KB at O = 80.  The launch keeps the rows below 4 096
// (32-bit element offsets).
// One LDS-DMA wave-load (64 x 16 bytes from the lanes' addresses g to LDS at the wave-uniform address l, lane * 16 apart) that the COMPILER DOES NOT
// SEE: after the builtin form hipcc drains vmcnt(0) before the kernel's next LDS store -- here with every weight fragment in flight -- because
// that store might alias the pending LDS write.  The caller orders the reads of the image itself (feat_prenet_walk: how).  M0 is saved and
// restored inside the statement: the compiler keeps values of its own in it.
__device__ __forceinline__ void glds16_unseen(const void* g, const void* l) {
    typedef const __attribute__((address_space(3))) void* lds_t;
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_t)l);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
}

// FEAT / PRE: the workgroup has a feat_out part (h1 given) / a prenet part (w0 given and its first row below M_pre).  Template arguments, and the
// next tile's requests and phase 0 run whether or not there is a next tile (rows clamped as everywhere, into the buffer nobody reads): the
// compiler's wait counts do not follow a condition from a request to its use, and with either in a branch of its own it would wait for
// "possibly pending" loads at the next request -- which takes in the stores of phase 3.
template <int DROP, bool FEAT, bool PRE>
__device__ __forceinline__ void feat_prenet_walk(const FeatPrenetArgs& a, const int ntw, const int Ms_feat, const int Ms_pre) {
    typedef OpsX3 Ops;
    typedef Ops::Tile Tile;
    constexpr int SU = 8, SO = 3, SP = 8, U = 256, OP = 96, P = 256;
    constexpr int ldU = U + Ops::PAD, ldO = OP + Ops::PAD, ldP = P + Ops::PAD;
    constexpr int BUF = 2 * 16 * (ldU + ldO);  // elements of one buffer: both planes of an h1 tile and of a prenet-input tile
    static_assert(ldU == ldP, "the layer-1 operand tile re-uses the h1 tile's LDS");
    const int M_feat = a.M_feat, M_pre = a.M_pre;
    [[maybe_unused]] FpStamps ts;
    FP_STAMP(ts, 0);
    const int O = a.O;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kq = lane >> 4;   // operand fragments: row / column r16, k-group kq
    const int arow = lane & 15, cq = lane >> 4;  // transposed accumulators: activation row arow, columns cq * 4 .. cq * 4 + 3 of the column tile
    constexpr bool has_feat = FEAT, pre_any = PRE;
    const bool feat_wave = has_feat && wave * 16 < O;
    const int mbeg = blockIdx.x * 16 * ntw;
    // the tiles of this workgroup that the one-tile launch would not have left at entry (feat_prenet_rows): at least one
    const int nt = min(ntw, ((has_feat ? Ms_feat : Ms_pre) - mbeg + 15) >> 4);
    u16* lds = Ops::dynamic_lds();
    u16* const WF = lds + wave * (2 * SU * 512);  // this wave's feat_out fragments: hi plane, k-steps 0 .. SU - 1, then the lo plane
    lds += ((O + 15) >> 4) * (2 * SU * 512);
    const Tile A1 = Tile::carve(lds, 16 * ldU);  // h1 tile; layer 0's output from phase 2 on      } of buffer 0; buffer 1: BUF elements further
    const Tile A2 = Tile::carve(lds, 16 * ldO);  // feat_out / prenet input                        }
    float* const BL = reinterpret_cast<float*>(lds + BUF);  // b0 [P], b1 [P]
    const size_t lane8 = (size_t)lane * 8;
    auto frag = [&](const Ops::W w, int tile, int ns) { return w.at((size_t)tile * ns * 512, lane8); };
    const int t0 = wave, t1 = wave + 8;  // this wave's layer-0 column tiles
    const int c1 = wave * 2;             // first of this wave's two layer-1 column tiles
    const int fnc = wave * 16 + cq * 4;  // feat_out columns fnc .. fnc + 3 of this lane
    // zero padding of before_p's last 32-column line (O % 8 == 0: 8, 16 or 24 columns): four columns per lane of the first two waves, beside the
    // lane's own row of feat_out (the same frame offset)
    const int padc = O + wave * 16 + cq * 4;
    const bool pad_lane = wave < 2 && padc < ((O + 31) & ~31);

    // what a tile needs besides the weights
    f32x4 hrow[2];                    // this thread's share of the h1 rows
    f32x4 f0v = (f32x4){0.f, 0.f, 0.f, 0.f};  // F0 row (feat waves)
    int fo = 0;                       // frame offset of the accumulator's row
    unsigned int k0[2] = {0u, 0u}, k1[2] = {0u, 0u};  // keep bytes (mask mode)
    auto request_rows = [&](int m0) {
        if (has_feat) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = threadIdx.x + j * 512, r = i >> 6, c = (i & 63) * 4;
                hrow[j] = *reinterpret_cast<const f32x4*>(a.h1 + (unsigned)(min(m0 + r, M_feat - 1) * U + c));
            }
        }
    };
    auto request_feat = [&](int m0) {  // phase 1's epilogue operands
        if (feat_wave && fnc < O) {
            const int mc = min(m0 + arow, M_feat - 1);
            f0v = *reinterpret_cast<const f32x4*>(a.F0 + (unsigned)(mc * O + fnc));
            fo = a.frame_off[(unsigned)mc];
        }
    };
    auto request_keep = [&](unsigned int (&k)[2], const uint8_t* keep, int m0, int ca, int cb) {  // column tiles ca, cb of a layer's mask
        if (DROP == 1 && pre_any && m0 < M_pre) {
            const unsigned mk = (unsigned)(min(m0 + arow, M_pre - 1) * P);
            k[0] = *reinterpret_cast<const unsigned int*>(keep + mk + ca * 16 + cq * 4);
            k[1] = *reinterpret_cast<const unsigned int*>(keep + mk + cb * 16 + cq * 4);
        }
    };
    auto store_rows = [&](int buf) {  // phase 0 of a tile: its h1 rows -> LDS planes, its prenet-input tile zeroed
        Ops::zero(A2.at(buf * BUF), 16 * ldO);
        if (has_feat) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = threadIdx.x + j * 512, r = i >> 6, c = (i & 63) * 4;
                Ops::store4(A1.at(buf * BUF), r, ldU, c, hrow[j]);
            }
        }
    };

    // ---- every request of the entry, in the order of use (the CU's address path serves its waves' requests in issue order).  feat_out's LDS-DMA goes
    // FIRST: vmcnt retires in issue order, so a wave's wait for its h1 rows in phase 0 is also the wait for its own LDS-DMA, and the barrier that
    // ends phase 0 (a memory clobber) keeps its reads of the image behind that wait.
    if (feat_wave) {
        const Ops::W w = frag(Ops::wf(a), wave, SU);
#pragma unroll
        for (int st = 0; st < SU; ++st) {
            glds16_unseen(w.hi + st * 512, WF + st * 512);
            glds16_unseen(w.lo + st * 512, WF + (SU + st) * 512);
        }
    }
    request_rows(mbeg);
    asm volatile("s_barrier" ::: "memory");  // no data wait: no wave's fragments in front of another wave's rows
    request_feat(mbeg);
    request_keep(k0, a.keep0, mbeg, t0, t1);
    request_keep(k1, a.keep1, mbeg, c1, c1 + 1);
    Ops::Frag<2, SO> f0;
    Ops::Frag<2, SP> f1;
    unsigned int seed0 = 0, seed1 = 0;
    const unsigned int thr16 = (unsigned int)(a.drop_p * 65536.0f);
    if (DROP == 2) {
        const unsigned int sbump = a.seed_dev ? *a.seed_dev * 0x9E3779B9u : 0u;
        seed0 = hash_u32(a.seed0 + sbump);
        seed1 = hash_u32(a.seed1 + sbump);
    }
    f32x4 bias = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool bias_thread = pre_any && threadIdx.x < 2 * (P / 4);
    if (pre_any) {
        if (bias_thread) bias = *reinterpret_cast<const f32x4*>((threadIdx.x < P / 4 ? a.b0 : a.b1 - P) + threadIdx.x * 4);
        const Ops::W w0[2] = {frag(Ops::w0(a), t0, SO), frag(Ops::w0(a), t1, SO)};
        f0.load(w0);
        const Ops::W w1[2] = {frag(Ops::w1(a), c1, SP), frag(Ops::w1(a), c1 + 1, SP)};
        f1.load(w1);
    }
    store_rows(0);
    if (bias_thread) *reinterpret_cast<f32x4*>(BL + threadIdx.x * 4) = bias;
    FP_STAMP(ts, 1);

    auto tile = [&](const int q) {
        const int buf = q & 1, m0 = mbeg + q * 16;
        const Tile T1 = A1.at(buf * BUF), T2 = A2.at(buf * BUF);
        const bool has_pre = pre_any && m0 < M_pre;
        lds_barrier();  // this tile's buffer is written; every wave is done with the other buffer (the tile before)
        if (q == 0) FP_STAMP(ts, 2);
        // ---- phase 1: H8 feat_out of the previous step (+ H10 scatter), feat_out's fragments from LDS -----------------------------------------------
        if (feat_wave) {
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
            const u16* ah = T1.h + r16 * ldU + kq * 8;
            const u16* al = T1.l + r16 * ldU + kq * 8;
            // WF IS WRITTEN BY THIS WAVE'S OWN LDS-DMA, WHICH THE COMPILER DOES NOT SEE (glds16_unseen).  These reads are ordered behind it by exactly
            // this: the wave issued the DMA before its h1 loads (the entry, above), it has waited for those loads in store_rows(0) (vmcnt retires
            // in issue order), and a barrier with a memory clobber lies between that wait and here.  Whoever moves request_rows() in front of the
            // DMA, drops the h1 loads of a feat wave, or lets a wave read another wave's part of the image must put an s_waitcnt vmcnt here.
            const u16* wf = WF + lane8;
#pragma unroll
            for (int st = 0; st < SU; ++st) {  // (Frag::chain<true>, NT = 1)
                const s16x8 a_hi = *reinterpret_cast<const s16x8*>(ah + st * 32), a_lo = *reinterpret_cast<const s16x8*>(al + st * 32);
                const s16x8 w_hi = *reinterpret_cast<const s16x8*>(wf + st * 512), w_lo = *reinterpret_cast<const s16x8*>(wf + (SU + st) * 512);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w_hi, a_lo, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w_lo, a_hi, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w_hi, a_hi, acc, 0, 0, 0);
            }
            const int m = m0 + arow;
            if (fnc < O) {
                f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (m < Ms_feat) {
                    v = acc + f0v;
                    const long long fr = (long long)fo + a.t_prev;
                    *reinterpret_cast<f32x4*>(a.before + (size_t)fr * O + fnc) = v;
                    if (a.before_p) {
                        uint2 h, l;
                        split4(v, h, l);
                        p32_store4(a.before_p, (O + 31) >> 5, fr, fnc, h, l);
                        if (pad_lane) p32_store4(a.before_p, (O + 31) >> 5, fr, padc, make_uint2(0u, 0u), make_uint2(0u, 0u));
                    }
                    if (a.out_act) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = act_apply(v[r], a.out_act);
                    }
                }
                Ops::store4(T2, arow, ldO, fnc, v);
            }
        }
        request_rows(m0 + 16);  // the next tile's rows and phase-1 operands: in flight during phases 2 and 3
        request_feat(m0 + 16);
        if (q == 0) FP_STAMP(ts, 3);
        f32x4 out1[2];
        if (has_pre) {
            lds_barrier();
            if (a.teacher_in) {  // teacher forcing: prenet input is y_{t-1}, not the decoder's own output
                load_rowtile_split(T2.h, T2.l, ldO, a.teacher_in, a.teacher_ld, O, m0, M_pre);
                lds_barrier();
            }
            if (q == 0) FP_STAMP(ts, 4);
            // ---- phase 2: H6 prenet layer 0 -> LDS (over the h1 tile) ------------------------------------------------------------------------------
            {
                f32x4 accv[2];
                f0.mma_t(T2, ldO, r16, kq, accv);
                const int m = m0 + arow;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const int nc = (tt ? t1 : t0) * 16 + cq * 4;
                    f32x4 v = accv[tt] + *reinterpret_cast<const f32x4*>(BL + nc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                    v = drop4<DROP>(v, DROP == 1 ? k0[tt] : 0u, (unsigned int)m * (unsigned int)P + (unsigned int)nc, seed0, thr16, a.keep_scale);
                    Ops::store4(T1, arow, ldP, nc, v);
                }
            }
            request_keep(k0, a.keep0, m0 + 16, t0, t1);
            lds_barrier();
            if (q == 0) {
                FP_STAMP(ts, 5);
                FP_STAMP(ts, 6, true);
            }
            // ---- phase 3: H6 prenet layer 1 -> global (+ KD tap, + P32 planes): the MFMAs here, the stores below --------------------------------
            f1.mma_t(T1, ldP, r16, kq, out1);
        }
        // phase 0 of the next tile, into the buffer every wave left before this tile's first barrier -- and the one point of the tile at which
        // loads are waited for (the asm makes the compiler take the other operands in here as well, not at their use behind phase 3's stores)
        store_rows(buf ^ 1);
        asm volatile("" : "+v"(f0v), "+v"(fo), "+v"(k0[0]), "+v"(k0[1]));
        if (has_pre) {
            const int m = m0 + arow;
            if (m < Ms_pre) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const int nc = (c1 + tt) * 16 + cq * 4;
                    f32x4 v = out1[tt] + *reinterpret_cast<const f32x4*>(BL + P + nc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                    v = drop4<DROP>(v, DROP == 1 ? k1[tt] : 0u, (unsigned int)m * (unsigned int)P + (unsigned int)nc, seed1, thr16, a.keep_scale);
                    if (a.pre_out) *reinterpret_cast<f32x4*>(a.pre_out + (size_t)m * P + nc) = v;
                    if (a.pre_out_p) {
                        uint2 h, l;
                        split4(v, h, l);
                        p32_store4(a.pre_out_p, SP, m, nc, h, l);
                    }
                    if (a.tap_prenet) *reinterpret_cast<f32x4*>(a.tap_prenet + (size_t)(a.frame_off[m] + a.t_cur) * P + nc) = v;
                }
            }
            request_keep(k1, a.keep1, m0 + 16, c1, c1 + 1);
        }
    };
    tile(0);
#pragma unroll 1
    for (int q = 1; q < nt; ++q) tile(q);
    FP_STAMP_FLUSH(ts);
}

template <int DROP>
__global__ __launch_bounds__(512) void feat_prenet_walk_kernel(const FeatPrenetArgs a, const int ntw) {
    int Ms_feat, Ms_pre;
    if (!feat_prenet_rows(a, 16 * ntw, Ms_feat, Ms_pre)) return;
    const bool pre = a.w0 != nullptr && (int)blockIdx.x * 16 * ntw < a.M_pre;  // (the later tiles of the workgroup start at higher rows)
    if (a.h1 != nullptr) {
        if (pre) feat_prenet_walk<DROP, true, true>(a, ntw, Ms_feat, Ms_pre);
        else feat_prenet_walk<DROP, true, false>(a, ntw, Ms_feat, Ms_pre);
    } else if (pre) {
        feat_prenet_walk<DROP, false, true>(a, ntw, Ms_feat, Ms_pre);
    }
}

// Tail of the small LSTM steps with prefetched cell operands: wave g's accumulators (gate g of the tile's 16 rows x 16 units) go to LDS, then thread
// (row, unit) of the workgroup collects its four gate pre-activations and runs the cell.  units_in_lane: the accumulator layout -- false: four rows
// (hi * 4 ..) of unit lo, the activations being the MFMA's A operand (x3 form); true: four units (hi * 4 ..) of row lo, the weight fragment being the
// A operand (ff form).  valid: the thread's (m, u) exists; rows from Ms on are beyond the live rows and not stored.
__device__ __forceinline__ void gates_to_cell(const LstmStepArgs& a, int g, int lane, const f32x4& acc, bool units_in_lane, int m, int u, bool valid, int Ms,
                                              const CellIn& ci) {
    __shared__ float g_l[4][16][17];
    const int lo = lane & 15, hi = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (units_in_lane) g_l[g][lo][hi * 4 + i] = acc[i];
        else g_l[g][hi * 4 + i][lo] = acc[i];
    }
    __syncthreads();
    if (!valid || m >= Ms) return;
    const int row = threadIdx.x >> 4, uc = threadIdx.x & 15;
    const float pre[4] = {g_l[0][row][uc], g_l[1][row][uc], g_l[2][row][uc], g_l[3][row][uc]};
    cell_finish(a, m, u, pre, ci);
}

constexpr int kSmallStepsAtEntry = 4;  // of term 1's eight k-steps of weight fragments, in the register-resident small steps (below)

// The K walk of the register-resident small steps, NT = 1 or 2 terms of K = 256 (a template, not a run-time count: where the two forms share code the
// compiler's wait counts are those of the form with fewer loads in flight).  Request order = order of use: every wave's activation rows (term 0 to
// columns 0 - 255 of the K = 512 tile, term 1 to columns 256 - 511), an s_barrier (no data wait; as in feat_prenet_split_kernel: no wave's fragments in
// front of another wave's rows), the weight fragments.  The rows' 32 registers are free once they are split into LDS (that wait covers the rows alone:
// loads return in order); term 1's last k-steps then take their place, queued right behind the other fragments and first used ~40 MFMAs after the
// barrier -- with all 16 steps requested at entry the kernel needs 184 VGPRs, two waves per SIMD instead of three.
template <class Ops, int NT>
__device__ __forceinline__ f32x4 small_walk(const LstmStepArgs& a, typename Ops::Tile A, int ldk, int m0, int M, int g, int u0, int lane) {
    const int r16 = lane & 15, kq = lane >> 4;
    RowTile256 rows[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) rows[t].request(a.term[t].A, a.term[t].lda, m0, M);
    asm volatile("s_barrier" ::: "memory");
    const size_t fo = (size_t)((g * a.U + u0) >> 4) * 8 * 512 + (size_t)lane * 8;  // W rows g*U + u0.. form fragment tile (g*U + u0)/16 (U % 16 == 0); 8 steps per row tile
    typename Ops::template Frag<1, 8> wf[NT];
    const typename Ops::W w0[1] = {Ops::w(a.term[0]).at(fo)}, w1[1] = {Ops::w(a.term[NT - 1]).at(fo)};  // (both formed before the first request)
    wf[0].load(w0);
    if (NT > 1) wf[NT - 1].template load<0, kSmallStepsAtEntry>(w1);
    __builtin_amdgcn_sched_barrier(0);  // (hipcc otherwise starts the stores -- and their wait for the first row -- above the fragment requests)
#pragma unroll
    for (int t = 0; t < NT; ++t) Ops::store_rows(rows[t], A.at(t * 256), ldk);
    asm volatile("" ::: "memory");  // (the late requests stay below the rows' last use)
    if (NT > 1) wf[NT - 1].template load<kSmallStepsAtEntry, 8>(w1);
    __syncthreads();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {  // the partial sums are formed and added as the one-term-at-a-time kernel did: 0 + term 0 + term 1
        f32x4 part[1];
        wf[t].mma_small(A.at(t * 256), ldk, r16, kq, part);
        acc += part[0];
    }
    return acc;
}

// The register-resident small step, in either operand form.  Every term has K = 256 (the student's decoder LSTMs: two terms, or the input term alone in
// the zero-state form of step 0) -> the activation rows of every term and the weight fragments are requested at kernel entry (small_walk; both terms'
// rows side by side in one K = 512 tile), ONE barrier, then the two terms' k-walks back to back.  (Until round 8 term 1's rows were requested after term
// 0's MFMAs, into term 0's columns: a global round trip and two barriers exposed in every small step.)
template <class Ops>
__global__ __launch_bounds__(256) void lstm_small_resident_kernel(const LstmStepArgs a) {
    // device-driven loops: loads and MFMAs run on the host's row bound, only the final store is limited to the device's live-row count (its scalar
    // load is then off the critical path: first use after the K walk)
    const int M = a.M, Ms = live_rows_of(a.M, a.m_dev);
    if ((int)blockIdx.y * 16 >= Ms) return;  // tile beyond the device's live rows (uniform per workgroup, before any barrier): a step of a loose bound costs a launch, not a pass
    constexpr int LD = 512 + Ops::PAD;
    const typename Ops::Tile A = Ops::Tile::template fixed<16 * LD>();
    const int m0 = blockIdx.y * 16, u0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    // epilogue operands first (latency hides under the K walk)
    const int erow = threadIdx.x >> 4, euc = threadIdx.x & 15;
    const int em = m0 + erow, eu = u0 + euc;
    const bool evalid = em < M && eu < a.U;
    CellIn ci;
    if (evalid) ci = cell_prefetch(a, em, eu);
    const f32x4 acc = a.nterms == 2 ? small_walk<Ops, 2>(a, A, LD, m0, M, g, u0, lane) : small_walk<Ops, 1>(a, A, LD, m0, M, g, u0, lane);
    gates_to_cell(a, g, lane, acc, Ops::kUnitsInLane, em, eu, evalid, Ms, ci);
}

// The streaming bf16x3 small step, for every other K: the row tile enters LDS one 512-k chunk at a time, the weight fragments stream from L2 one 32-k
// step ahead of the MFMAs (rowtile_mma_x3).
__global__ __launch_bounds__(256) void lstm_small_x3_kernel(const LstmStepArgs a) {
    const int M = a.M, Ms = live_rows_of(a.M, a.m_dev);
    if ((int)blockIdx.y * 16 >= Ms) return;  // (as above)
    constexpr int KC = 512;
    __shared__ __attribute__((aligned(16))) u16 A_h[16 * (KC + 16)];  // row stride = 2 (mod 4) sixteen-byte slots: conflict-free fragment reads
    __shared__ __attribute__((aligned(16))) u16 A_lo[16 * (KC + 16)];
    const int m0 = blockIdx.y * 16, u0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    // epilogue operands first (latency hides under the K walk)
    const int erow = threadIdx.x >> 4, euc = threadIdx.x & 15;
    const int em = m0 + erow, eu = u0 + euc;
    const bool evalid = em < M && eu < a.U;
    CellIn ci;
    if (evalid) ci = cell_prefetch(a, em, eu);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < a.nterms; ++t) {
        const GemmTerm T = a.term[t];
        for (int k0 = 0; k0 < T.K; k0 += KC) {
            const int kc = min(KC, T.K - k0);
            __syncthreads();
            load_rowtile_split(A_h, A_lo, kc + 16, T.A + k0, T.lda, kc, m0, M);
            __syncthreads();
            const size_t fo = ((size_t)((g * a.U + u0) >> 4) * ((T.K + 31) >> 5) + (k0 >> 5)) * 512 + (size_t)lane * 8;
            const u16* const wh[1] = {T.Whi + fo};
            const u16* const wl[1] = {T.Wlo + fo};
            f32x4 part[1];
            rowtile_mma_x3<1>(A_h, A_lo, kc + 16, wh, wl, kc, r16, kq, part);
            acc += part[0];
        }
    }
    gates_to_cell(a, g, lane, acc, false, em, eu, evalid, Ms, ci);
}


// ---- small-M LSTM step: wave g owns gate g of 16 units x 16 rows ------------------------------------
constexpr int SMALL_KC = 512;  // K chunk resident in LDS

__device__ __forceinline__ void lstm_small_body(const LstmStepArgs& a) {
    // device-driven loops: loads and MFMAs run on the host's row bound, only the final store is limited to the device's live-row count (its scalar
    // load is then off the critical path: first use after the K walk)
    const int M = a.M, Ms = live_rows_of(a.M, a.m_dev);
    if ((int)blockIdx.y * 16 >= Ms) return;  // tile beyond the device's live rows (uniform per workgroup, before any barrier): a step of a loose bound costs a launch, not a pass
    __shared__ __attribute__((aligned(16))) float A_l[16 * (SMALL_KC + 4)];
    __shared__ float g_l[4][16][17];
    const int m0 = blockIdx.y * 16, u0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int u = u0 + r16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < a.nterms; ++t) {
        const GemmTerm T = a.term[t];
        for (int k0 = 0; k0 < T.K; k0 += SMALL_KC) {
            const int kc = min(SMALL_KC, T.K - k0);
            __syncthreads();  // previous chunk fully consumed
            load_rowtile(A_l, kc + 4, T.A + k0, T.lda, kc, m0, M);
            __syncthreads();
            const float* const wr[1] = {T.W + (size_t)(g * a.U + min(u, a.U - 1)) * T.ldw + k0};
            f32x4 part[1];
            rowtile_mma<1>(A_l, kc + 4, wr, kc, r16, kq, part, blockIdx.y);
            acc += part[0];
        }
    }
    {
        const int col = lane & 15, rq = lane >> 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) g_l[g][rq * 4 + r][col] = acc[r];
    }
    __syncthreads();
    // cell epilogue: thread -> (row, unit); the cell operands are fetched HERE, for the live cells only (not gates_to_cell's prefetched form)
    const int row = threadIdx.x >> 4, uc = threadIdx.x & 15;
    const int m = m0 + row, uu = u0 + uc;
    if (m >= Ms || uu >= a.U) return;
    const CellIn ci = cell_prefetch(a, m, uu);
    const float pre[4] = {g_l[0][row][uc], g_l[1][row][uc], g_l[2][row][uc], g_l[3][row][uc]};
    cell_finish(a, m, uu, pre, ci);
}

__global__ __launch_bounds__(256) void lstm_small_kernel(const LstmStepArgs a) { lstm_small_body(a); }

// Two independent steps of the same shape in one launch (blockIdx.z picks the problem): the forward and the backward direction of a BiLSTM time
// step (bilstm.hip algo 1) -- half the dependent launches of the per-step path.
__global__ __launch_bounds__(256) void lstm_small_pair_kernel(const LstmStepArgs a0, const LstmStepArgs a1) {
    if (blockIdx.z == 0) lstm_small_body(a0);
    else lstm_small_body(a1);
}

int launch_lstm_small(const LstmStepArgs& a, hipStream_t s) {
    const double fl = lstm_step_flops(a);
    dim3 grid((a.U + 15) / 16, (a.M + 15) / 16);
    bool planes = true;
    for (int i = 0; i < a.nterms; ++i) planes = planes && a.term[i].Whi && a.term[i].Wlo && (a.term[i].K & 7) == 0 && a.term[i].ldw == a.term[i].K;
    planes = planes && (a.U & 15) == 0;
    // the register-resident forms: two K = 256 terms, or the zero-state step's single one (its h . W_hh^T term is dropped, not contracted with zeros)
    bool pre256 = a.nterms == 2 || (a.nterms == 1 && !a.h_in), ff = true;
    for (int i = 0; i < a.nterms; ++i) {
        pre256 = pre256 && a.term[i].K == 256;
        ff = ff && a.term[i].Wff != nullptr;
    }
    if (planes) {
        ProfScope ps("lstm_small_kernel/bf16x3", fl, a.M, s);
        if (pre256) hipLaunchKernelGGL(lstm_small_resident_kernel<OpsX3>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(lstm_small_x3_kernel, grid, dim3(256), 0, s, a);
    } else if (pre256 && ff && (a.U & 15) == 0) {
        ProfScope ps("lstm_small_ff_kernel/f32", fl, a.M, s);
        hipLaunchKernelGGL(lstm_small_resident_kernel<OpsF32>, grid, dim3(256), 0, s, a);
    } else {
        ProfScope ps("lstm_small_kernel", fl, a.M, s);
        hipLaunchKernelGGL(lstm_small_kernel, grid, dim3(256), 0, s, a);
    }
    return check_hip(hipGetLastError(), "lstm_small launch");
}

int launch_lstm_small_pair(const LstmStepArgs& a0, const LstmStepArgs& a1, hipStream_t s) {
    const double fl = lstm_step_flops(a0) + lstm_step_flops(a1);
    const int mmax = a0.M > a1.M ? a0.M : a1.M;  // (tiles beyond a problem's own rows exit at once)
    dim3 grid((a0.U + 15) / 16, (mmax + 15) / 16, 2);
    ProfScope ps("lstm_small_pair_kernel", fl, a0.M + a1.M, s);
    hipLaunchKernelGGL(lstm_small_pair_kernel, grid, dim3(256), 0, s, a0, a1);
    return check_hip(hipGetLastError(), "lstm_small_pair launch");
}

// two independent small steps that launch_lstm_step would both send to lstm_small_kernel (fp32 operands, no fragment-major weights): one launch;
// *handled = false when either step has another form (the caller launches them one after the other)
int launch_lstm_small_pair_any(const LstmStepArgs& a0, const LstmStepArgs& a1, hipStream_t s, bool* handled) {
    *handled = false;
    if (a0.U != a1.U || a0.m_dev || a1.m_dev) return 0;
    for (const LstmStepArgs* a : {&a0, &a1})
        for (int i = 0; i < a->nterms; ++i)
            if (!a->term[i].A || !a->term[i].W || a->term[i].Whi || a->term[i].Wff) return 0;
    *handled = true;
    return launch_lstm_small_pair(a0, a1, s);
}

// One of a kernel's three dropout forms (FCL_DROP_*: none, mask, rng), opted in for `lds` bytes of dynamic LDS and launched on 512 threads.
// ntw: the walker's second argument (row tiles per workgroup); 0 = the kernel takes the argument block alone.
static int launch_fp_drop(const void* const (&fn)[3], int drop_mode, dim3 grid, size_t lds, const FeatPrenetArgs& a, hipStream_t s, int ntw = 0) {
    const void* f = fn[drop_mode == 1 || drop_mode == 2 ? drop_mode : 0];
    const int rc = ensure_dyn_lds(f, (int)lds);
    if (rc) return rc;
    void* args1[] = {const_cast<FeatPrenetArgs*>(&a)};
    void* args2[] = {const_cast<FeatPrenetArgs*>(&a), &ntw};
    return check_hip(hipLaunchKernel(f, grid, dim3(512), ntw ? args2 : args1, lds, s), "feat_prenet launch");
}

#ifdef FCL_FP_TS
// developer aid (see FpStamps): the launch just enqueued on s, synchronously -- per stamp, the cycles since the wave's entry, mean and maximum over the
// waves that ran (feat waves alone for stamp 3: the others pass phase 1 at once)
static void print_fp_stamps(const char* form, int rows, int wgs) {
    static const int want = tunable("FP_TS", 0);
    if (!want) return;
    if (hipDeviceSynchronize() != hipSuccess) return;
    static long long h[kFpTsWorkgroups * 64];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fp_ts), sizeof(h)) != hipSuccess) return;
    double sum[8] = {}, mx[8] = {};
    int cnt[8] = {};
    for (int w = 0; w < (wgs < kFpTsWorkgroups ? wgs : kFpTsWorkgroups) * 8; ++w) {
        const long long* t = &h[(size_t)w * 8];
        if (!t[0]) continue;  // (a workgroup beyond the live rows left at entry)
        for (int i = 1; i < 8; ++i) {
            if (!t[i] || (i == 3 && (w & 7) >= 5)) continue;
            const double d = (double)(t[i] - t[0]);
            sum[i] += d; cnt[i]++;
            if (d > mx[i]) mx[i] = d;
        }
    }
    fprintf(stderr, "fp_ts %s rows %d workgroups %d: cycles since entry, mean (max):", form, rows, wgs);
    static const char* const name[8] = {"", "rows->LDS", "barrier0", "phase1", "barrier1", "phase2+barrier2", "all landed", "exit"};
    for (int i = 1; i < 8; ++i) fprintf(stderr, "  %s %.0f (%.0f)", name[i], cnt[i] ? sum[i] / cnt[i] : 0.0, mx[i]);
    fprintf(stderr, "\n");
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_fp_ts)) == hipSuccess) (void)hipMemset(p, 0, sizeof(h));
}
#else
static void print_fp_stamps(const char*, int, int) {}
#endif

// The walker: ceil(tiles / ntw) workgroups of feat_prenet_walk_kernel, each on ntw consecutive row tiles.
static int launch_feat_prenet_walk(const FeatPrenetArgs& a, int rows, int ntw, hipStream_t s) {
    const size_t lds_w = sizeof(u16) * ((size_t)((a.O + 15) / 16) * 2 * 8 * 512 + 2 * 2 * 16 * ((256 + OpsX3::PAD) + (96 + OpsX3::PAD))) + 2 * 256 * sizeof(float);
    static const void* const fn[3] = {reinterpret_cast<const void*>(feat_prenet_walk_kernel<0>), reinterpret_cast<const void*>(feat_prenet_walk_kernel<1>),
                                      reinterpret_cast<const void*>(feat_prenet_walk_kernel<2>)};
    const int tiles = (rows + 15) / 16, wgs = (tiles + ntw - 1) / ntw;
    const int rc = launch_fp_drop(fn, a.drop_mode, dim3(wgs, 1), lds_w, a, s, ntw);
    if (!rc) print_fp_stamps("walk", rows, wgs);
    return rc;
}

// feat_prenet_split_kernel with RT row tiles per workgroup.  Measured on one box, 2 400 live rows, rocprofv3 durations: the kernel it replaced (RT = 2)
// 14.1 us; this one at RT = 1 9.5, at RT = 2 11.9.  The 4-stream bench line does not move with either (44.5 - 45.7 M frames/s, same box): with four
// passes in flight the pass is bound by the sum of workgroup-time, which RT = 1 doubles while it halves the latency.  RT = 1 has the lowest single-pass
// latency (339 -> 269 us of a 1.38 ms eager pass).  Which launch takes which form: launch_feat_prenet, below.
template <class Ops, int RT>
static int launch_feat_prenet_split(const FeatPrenetArgs& a, int rows, hipStream_t s) {
    constexpr size_t lds_s = (size_t)Ops::LDS_BYTES * 16 * RT * ((256 + Ops::PAD) + (96 + Ops::PAD));
    static const void* const fn[3] = {reinterpret_cast<const void*>(feat_prenet_split_kernel<Ops, 0, RT>), reinterpret_cast<const void*>(feat_prenet_split_kernel<Ops, 1, RT>),
                                      reinterpret_cast<const void*>(feat_prenet_split_kernel<Ops, 2, RT>)};
    const int wgs = (rows + 16 * RT - 1) / (16 * RT);
    const int rc = launch_fp_drop(fn, a.drop_mode, dim3(wgs, 1), lds_s, a, s);
    if (!rc && Ops::kPlanes) print_fp_stamps(RT == 2 ? "split RT=2" : "split RT=1", rows, wgs);
    return rc;
}

int launch_feat_prenet(const FeatPrenetArgs& a, hipStream_t s) {
    const int rows = a.h1 ? a.M_feat : a.M_pre;
    if (rows <= 0) return 0;
    FCL_REQUIRE(!(a.U & 3) && !(a.O & 3) && !(a.P & 3), FCL_ERR_SHAPE, "feat_prenet: U/O/P must be multiples of 4");
    const size_t lds = sizeof(float) * 16 * ((size_t)(a.U + 4) + (a.O + 4) + (a.P + 4));
    FCL_REQUIRE(lds <= 160 * 1024, FCL_ERR_SHAPE, "feat_prenet: tile does not fit LDS (%zu B)", lds);
    double fl = 0;
    if (a.h1) fl += 2.0 * a.M_feat * a.O * a.U;
    if (a.w0) fl += 2.0 * a.M_pre * ((double)a.P * a.O + (double)a.P * a.P);
    const bool planes = a.wf_hi && a.wf_lo && a.w0_hi && a.w0_lo && a.w1_hi && a.w1_lo && !(a.U & 7) && !(a.O & 7) && !(a.P & 7);
    FCL_REQUIRE(planes || (!a.pre_out_p && !a.before_p), FCL_ERR_INVALID, "feat_prenet: P32 outputs need the bf16x3 weight planes");
    FCL_REQUIRE(!a.w0 || a.pre_out || a.pre_out_p, FCL_ERR_INVALID, "feat_prenet: no prenet output buffer");
    FCL_REQUIRE(!a.pre_out_p || !(a.P & 31), FCL_ERR_SHAPE, "feat_prenet: P32 prenet output needs P %% 32 == 0");
    if (planes) {
        const bool resident = a.U == 256 && a.O > 64 && a.O <= 96 && a.P == 256;
        // The register-resident forms by row count: below FCL_FP_WALK_MIN_TILES row tiles (default 112 = 1 792 rows) one row tile per workgroup, the
        // lowest latency; from there up to 4 095 rows the walker with FCL_FP_WALK_TILES tiles per workgroup (default 2; 0 = walker off: one tile
        // per workgroup); from 4 096 rows on two tiles per workgroup as before (the walker was not measured against that route).  Defaults from
        // the same-box scans of profiles/r12_fp_walk_ab.log.
        static const int walk_tiles = tunable("FP_WALK_TILES", 2), walk_min = tunable("FP_WALK_MIN_TILES", 112);
        const bool walk = resident && walk_tiles > 0 && rows < 4096 && (rows + 15) / 16 >= walk_min;
        ProfScope ps(walk ? "feat_prenet_walk_kernel/bf16x3" : "feat_prenet_kernel/bf16x3", fl, rows, s);
        if (walk) {
            const int rc = launch_feat_prenet_walk(a, rows, walk_tiles, s);
            if (rc) return rc;
        } else if (resident) {
            const int rc = rows >= 4096 ? launch_feat_prenet_split<OpsX3, 2>(a, rows, s) : launch_feat_prenet_split<OpsX3, 1>(a, rows, s);
            if (rc) return rc;
        } else {
            const size_t lds3 = 2 * sizeof(unsigned short) * 16 * ((size_t)(a.U + 8) + (a.O + 8) + (a.P + 8));
            const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(feat_prenet_x3_kernel), 160 * 1024);
            if (rc) return rc;
            hipLaunchKernelGGL(feat_prenet_x3_kernel, dim3((rows + 15) / 16), dim3(512), lds3, s, a);
        }
    } else if (a.wf_ff && a.w0_ff && a.w1_ff && a.U == 256 && a.P == 256 && a.O > 64 && a.O <= 96 && !a.teacher_in && !a.pre_out_p && !a.before_p &&
               (!a.w0 || a.pre_out)) {
        // exact-fp32 mode with fragment-major fp32 weights: the register-resident form (19.2 -> ~9 us per launch at 2 400 rows)
        ProfScope ps("feat_prenet_split_kernel/f32", fl, rows, s);
        const int rc = launch_feat_prenet_split<OpsF32, 1>(a, rows, s);
        if (rc) return rc;
    } else {
        ProfScope ps("feat_prenet_kernel", fl, rows, s);
        const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(feat_prenet_kernel), 160 * 1024);
        if (rc) return rc;
        hipLaunchKernelGGL(feat_prenet_kernel, dim3((rows + 15) / 16), dim3(512), lds, s, a);
    }
    return check_hip(hipGetLastError(), "feat_prenet launch");
}

}  // namespace fcl
