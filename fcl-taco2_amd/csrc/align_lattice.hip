// align_lattice.hip — forced alignment over a lattice: Viterbi over an utterance whose rows name up to 8 predecessors each and carry START / FINAL
// flags, with the choice of the end row and the backtrack on the device (include/fcl_hip.h "Forced alignment, lattice graphs").  gfx950 only.
//   al_lattice_viterbi_kernel  the shape of al_viterbi_kernel (csrc/align.hip): ONE workgroup of 256 threads per utterance, thread i owns the rows
//                      i, i + 256, i + 512, i + 768; two rolling V columns in LDS, one barrier per frame; the gather ll[t][row_state[r]] of a chunk of
//                      8 frames sits in registers and the next chunk's is requested before the current one is worked through.  A row's eight
//                      predecessor distances (16 bits each: S <= 1024) stay in four registers of its thread; an unusable slot is stored as 0.  Almost
//                      every row has slot 0 alone, so slot 0 is tried first and the other seven sit behind one flag per row: a row without them pays
//                      what a chain row pays, two LDS reads per frame.  The same sanitised table lies in LDS for the backtrack.  One back-pointer
//                      byte per cell (0 stay, 1 + slot otherwise), frame-major.  The end row is the FINAL row with the largest finite V(r, T - 1), the
//                      lowest row on ties: every thread reduces its own rows, then a tree over LDS whose combiner (larger value, then lower row) is
//                      commutative and associative, so the order of the reduction cannot show.  The backtrack is al_viterbi_kernel's: the workgroup
//                      loads the 16 x 16 window of back-pointers that ends at the current cell, thread 0 walks until it leaves the window (a move
//                      over a word boundary leaves it at once: one round trip per such move).  A move is taken only by the row's own usable slot;
//                      anything else, or a row without START in frame 0, fails the utterance.
// Every offset, state, slot and flag read from a device table is clamped, and an utterance whose slices do not fit its lengths fails (ok 0) without
// touching anything outside its clamped slices.  No atomics; nothing depends on the batch.
#include <math.h>

#include "fcl_common.h"

namespace fcl {

constexpr int LT_TMAX = 4096, LT_SMAX = 1024, LT_MMAX = 1024, LT_UTT_MAX = 65535;
constexpr int LT_NP = 8;                 // predecessor slots per row
constexpr int LT_NT = 256;               // threads
constexpr int LT_NR = LT_SMAX / LT_NT;   // rows per thread
constexpr int LT_CH = 8;                 // frames per staging chunk
constexpr int LT_W = 16;                 // the backtrack's window is LT_W frames x LT_W rows (LT_W * LT_W == LT_NT)

__device__ __forceinline__ long long lt_clamp(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

struct LtUtt {
    int f0, r0, nf, nr;
    long long c0;
};
__device__ __forceinline__ bool lt_utt(const fcl_al_lattice_t& a, int u, LtUtt& g) {
    const long long f0 = lt_clamp(a.frame_off[u], 0, a.frames), f1 = lt_clamp(a.frame_off[u + 1], f0, a.frames);
    const long long r0 = lt_clamp(a.row_off[u], 0, a.rows), r1 = lt_clamp(a.row_off[u + 1], r0, a.rows);
    const long long c0 = lt_clamp(a.cell_off[u], 0, a.cells), c1 = lt_clamp(a.cell_off[u + 1], c0, a.cells);
    g.f0 = (int)f0, g.r0 = (int)r0, g.c0 = c0;
    g.nf = (int)min(f1 - f0, (long long)LT_TMAX), g.nr = (int)min(r1 - r0, (long long)LT_SMAX);
    return f1 - f0 >= 1 && f1 - f0 <= min(a.max_t, LT_TMAX) && r1 - r0 >= 1 && r1 - r0 <= min(a.max_s, LT_SMAX) && (f1 - f0) * (r1 - r0) <= c1 - c0;
}

// the utterance has no alignment: frame_row -1, row_frames 0 (row_begin: the utterance's first frame), score -inf, ok 0
__device__ __forceinline__ void lt_fail(const fcl_al_lattice_t& a, int u, const LtUtt& g, int tid) {
    for (int t = tid; t < g.nf; t += LT_NT) a.frame_row[g.f0 + t] = -1;
    for (int r = tid; r < g.nr; r += LT_NT) a.row_begin[g.r0 + r] = g.f0, a.row_frames[g.r0 + r] = 0;
    if (tid == 0) a.score[u] = -INFINITY, a.ok[u] = 0;
}

// the better end row of two: the larger value, the lower row on equal values; row -1 is "none" (its value is -inf and every real candidate is finite)
__device__ __forceinline__ void lt_better(float& v, int& r, float v2, int r2) {
    if (r2 >= 0 && (r < 0 || v2 > v || (v2 == v && r2 < r))) v = v2, r = r2;
}

__global__ __launch_bounds__(LT_NT) void al_lattice_viterbi_kernel(const fcl_al_lattice_t a) {
    __shared__ float vcol[2][LT_SMAX];
    __shared__ unsigned short fr[LT_TMAX];
    __shared__ short seg_b[LT_SMAX], seg_e[LT_SMAX];              // first frame and end of each row's run, -1: no frames
    __shared__ __align__(16) unsigned short pd[LT_SMAX * LT_NP];  // the usable predecessor distances, 0: the slot does not count
    __shared__ unsigned char flg[LT_SMAX];                        // bit 0 START, bit 1 FINAL
    __shared__ unsigned char win[LT_NT];
    __shared__ float red_v[LT_NT];
    __shared__ int red_r[LT_NT];
    __shared__ int st[4];  // the backtrack's state: row, frame, done, failed
    const int u = blockIdx.x, tid = threadIdx.x;
    LtUtt g;
    if (!lt_utt(a, u, g)) {
        lt_fail(a, u, g, tid);
        return;
    }
    const int T = g.nf, S = g.nr, M = min(max(a.n_states, 1), LT_MMAX);
    const float* __restrict__ LL = a.ll + (long long)g.f0 * M;
    unsigned char* __restrict__ ws = reinterpret_cast<unsigned char*>(a.workspace) + g.c0;

    int state[LT_NR], p0[LT_NR], flags[LT_NR];
    unsigned pk[LT_NR][LT_NP / 2];  // slots 2i and 2i + 1 in the halves of pk[k][i]
    bool more[LT_NR];               // any usable slot beyond slot 0
#pragma unroll
    for (int k = 0; k < LT_NR; ++k) {
        const int r = tid + k * LT_NT;
        state[k] = 0, p0[k] = 0, flags[k] = 0, more[k] = false;
#pragma unroll
        for (int i = 0; i < LT_NP / 2; ++i) pk[k][i] = 0u;
        if (r < S) {
            state[k] = min(max(a.row_state[g.r0 + r], 0), M - 1);
            flags[k] = a.row_flags[g.r0 + r] & 3;
            flg[r] = (unsigned char)flags[k];
            const int* __restrict__ rp = a.row_pred + (long long)(g.r0 + r) * LT_NP;
#pragma unroll
            for (int s = 0; s < LT_NP; ++s) {
                const int j = rp[s];
                const unsigned d = (j >= 1 && j <= r) ? (unsigned)j : 0u;  // j <= r < 1024: 16 bits hold it
                pd[r * LT_NP + s] = (unsigned short)d;
                pk[k][s >> 1] |= d << (16 * (s & 1));
                if (s > 0 && d) more[k] = true;
            }
            p0[k] = (int)(pk[k][0] & 0xffffu);
        }
    }

    // ---- forward: column after column, the ll values of a chunk of frames in registers one chunk ahead ----
    float nxt[LT_NR][LT_CH];
#pragma unroll
    for (int k = 0; k < LT_NR; ++k)
#pragma unroll
        for (int i = 0; i < LT_CH; ++i) nxt[k][i] = (tid + k * LT_NT < S && i < T) ? LL[(long long)i * M + state[k]] : 0.f;
    for (int c0 = 0; c0 < T; c0 += LT_CH) {
        float cur[LT_NR][LT_CH];
#pragma unroll
        for (int k = 0; k < LT_NR; ++k)
#pragma unroll
            for (int i = 0; i < LT_CH; ++i) {
                cur[k][i] = nxt[k][i];
                const int t = c0 + LT_CH + i;
                nxt[k][i] = (tid + k * LT_NT < S && t < T) ? LL[(long long)t * M + state[k]] : 0.f;
            }
#pragma unroll
        for (int i = 0; i < LT_CH; ++i) {
            const int t = c0 + i;
            if (t < T) {  // uniform over the workgroup
                const float* vp = vcol[(t - 1) & 1];
                float* vn = vcol[t & 1];
#pragma unroll
                for (int k = 0; k < LT_NR; ++k) {
                    const int r = tid + k * LT_NT;
                    if (r < S) {
                        float v;
                        int bp = 0;
                        if (t == 0) {
                            v = (flags[k] & 1) ? cur[k][i] : -INFINITY;
                        } else {
                            // stay wins; the usable slots in slot order, each replaces the winner only when strictly greater
                            float best = vp[r];
                            if (p0[k]) {
                                const float c = vp[r - p0[k]];
                                if (c > best) best = c, bp = 1;
                            }
                            if (more[k]) {
#pragma unroll
                                for (int s = 1; s < LT_NP; ++s) {
                                    const int d = (int)((pk[k][s >> 1] >> (16 * (s & 1))) & 0xffffu);
                                    if (d) {
                                        const float c = vp[r - d];
                                        if (c > best) best = c, bp = 1 + s;
                                    }
                                }
                            }
                            v = cur[k][i] + best;
                        }
                        vn[r] = v;
                        ws[(long long)t * S + r] = (unsigned char)bp;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- the end row: the FINAL row with the largest finite V(r, T - 1), the lowest row on ties ----
    {
        const float* vl = vcol[(T - 1) & 1];
        float bv = -INFINITY;
        int br = -1;
#pragma unroll
        for (int k = 0; k < LT_NR; ++k) {
            const int r = tid + k * LT_NT;
            if (r < S && (flags[k] & 2)) {
                const float v = vl[r];
                if (isfinite(v)) lt_better(bv, br, v, r);
            }
        }
        red_v[tid] = bv, red_r[tid] = br;
        __syncthreads();
        for (int h = LT_NT / 2; h >= 1; h >>= 1) {
            if (tid < h) {
                float v = red_v[tid];
                int r = red_r[tid];
                lt_better(v, r, red_v[tid + h], red_r[tid + h]);
                red_v[tid] = v, red_r[tid] = r;
            }
            __syncthreads();
        }
    }
    const int end_row = red_r[0];
    const float score = red_v[0];
    if (end_row < 0) {  // uniform: no FINAL row was reached
        lt_fail(a, u, g, tid);
        return;
    }

    // ---- backtrack: from (end_row, T - 1) down to frame 0 ----
    for (int r = tid; r < S; r += LT_NT) seg_b[r] = -1, seg_e[r] = -1;
    if (tid == 0) st[0] = end_row, st[1] = T - 1, st[2] = 0, st[3] = 0;
    __syncthreads();
    for (int round = 0; round < T; ++round) {
        if (st[2]) break;
        const int r0 = min(max(st[0], 0), S - 1), t0 = min(max(st[1], 0), T - 1);
        const int wt = t0 - (tid / LT_W), wr = r0 - (tid % LT_W);
        win[tid] = (wt >= 0 && wr >= 0) ? ws[(long long)wt * S + wr] : (unsigned char)0;
        __syncthreads();
        if (tid == 0) {
            int r = r0, t = t0, done = 0, bad = 0;
            while (t0 - t < LT_W && r0 - r < LT_W) {
                fr[t] = (unsigned short)r;
                if (t == 0) {
                    done = 1, bad = !(flg[r] & 1);
                    break;
                }
                const int mv = win[(t0 - t) * LT_W + (r0 - r)];
                int step = 0;
                if (mv != 0) {
                    step = mv <= LT_NP ? (int)pd[r * LT_NP + mv - 1] : 0;
                    if (step < 1 || r - step < 0) {
                        done = 1, bad = 1;
                        break;
                    }
                }
                r -= step;
                --t;
            }
            st[0] = r, st[1] = t, st[2] = done, st[3] = bad;
        }
        __syncthreads();
    }
    if (!st[2] || st[3]) {
        lt_fail(a, u, g, tid);
        return;
    }

    // ---- frame_row, and each row's run from the places where frame_row changes ----
    for (int t = tid; t < T; t += LT_NT) {
        const int r = fr[t];  // < S: every entry was written by the walk
        a.frame_row[g.f0 + t] = r;
        if (t == 0 || fr[t - 1] != r) seg_b[r] = (short)t;
        if (t == T - 1 || fr[t + 1] != r) seg_e[r] = (short)(t + 1);
    }
    __syncthreads();
    for (int r = tid; r < S; r += LT_NT) {
        const int b = seg_b[r];
        a.row_begin[g.r0 + r] = g.f0 + (b >= 0 ? b : 0);  // a row off the path: 0 frames at the utterance's first frame
        a.row_frames[g.r0 + r] = b >= 0 ? seg_e[r] - b : 0;
    }
    if (tid == 0) a.score[u] = score, a.ok[u] = 1;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_al_lattice_viterbi_fwd(const fcl_al_lattice_t* a, fcl_stream_t stream) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "al_lattice_viterbi_fwd: null argument");
    FCL_REQUIRE(a->n_utt >= 0 && a->n_utt <= LT_UTT_MAX, FCL_ERR_SHAPE, "al_lattice_viterbi_fwd: 0 <= n_utt <= %d expected (got %d)", LT_UTT_MAX, a->n_utt);
    FCL_REQUIRE(a->n_states >= 1 && a->n_states <= LT_MMAX, FCL_ERR_SHAPE, "al_lattice_viterbi_fwd: 1 <= M <= %d expected (got %d)", LT_MMAX, a->n_states);
    if (a->n_utt == 0) return FCL_OK;
    FCL_REQUIRE(a->max_t >= 1 && a->max_t <= LT_TMAX && a->max_s >= 1 && a->max_s <= LT_SMAX, FCL_ERR_SHAPE,
                "al_lattice_viterbi_fwd: 1 <= max_t <= %d and 1 <= max_s <= %d expected (got %d, %d)", LT_TMAX, LT_SMAX, a->max_t, a->max_s);
    FCL_REQUIRE(a->frames >= 1 && a->rows >= 1 && a->cells >= 1 && a->frames * a->n_states < 0x7fffffffLL && a->rows * LT_NP < 0x7fffffffLL, FCL_ERR_SHAPE,
                "al_lattice_viterbi_fwd: 1 <= frames, rows, cells, frames x M < 2^31 and rows x 8 < 2^31 expected (got %lld, %lld, %lld)",
                (long long)a->frames, (long long)a->rows, (long long)a->cells);
    FCL_REQUIRE(a->ll && a->frame_off && a->row_off && a->cell_off && a->row_state && a->row_pred && a->row_flags && a->workspace && a->frame_row &&
                    a->row_begin && a->row_frames && a->score && a->ok,
                FCL_ERR_INVALID, "al_lattice_viterbi_fwd: null ll / frame_off / row_off / cell_off / row_state / row_pred / row_flags / workspace / "
                                 "frame_row / row_begin / row_frames / score / ok");
    FCL_REQUIRE(a->workspace_bytes >= fcl_al_workspace_bytes(a->cells, a->n_utt), FCL_ERR_WORKSPACE,
                "al_lattice_viterbi_fwd: the workspace has %zu bytes, %lld cells need %zu (fcl_al_workspace_bytes)", a->workspace_bytes,
                (long long)a->cells, fcl_al_workspace_bytes(a->cells, a->n_utt));
    ProfScope ps("al_lattice_viterbi_kernel", 6.0 * (double)a->cells, (double)a->cells, (hipStream_t)stream);
    hipLaunchKernelGGL(al_lattice_viterbi_kernel, dim3((unsigned)a->n_utt), dim3(LT_NT), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "al_lattice_viterbi_fwd");
}

}  // extern "C"
