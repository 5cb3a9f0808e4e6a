// align_common.h -- what the three forced-alignment files share, once: align.hip (single Gaussians over a chain of rows), align_gmm.hip
// (Gaussian-mixture states) and align_lattice.hip (rows that name their predecessors) keep their kernels, their entries and what
// is particular to each and take from here the limits, the clamped utterance geometry, the phases of the Viterbi kernels, the row-list walk of the
// statistics kernels and the argument checks of a Viterbi batch.  (The log-likelihood kernels keep their staging and their fma chain in their own
// files: shared through functions they compiled to other instruction schedules, which the mixture kernel's timing showed.)  gfx950 only.
//   Viterbi         ONE workgroup of AL_NT = 256 threads per utterance; thread i owns the rows i, i + 256, i + 512, i + 768.  Column t depends on
//                   column t - 1 alone: two rolling V columns in LDS, one barrier per frame.  The gather ll[t][row_state[r]] does not depend on V, so a
//                   thread holds the values of its rows for a chunk of AL_CH = 8 frames in registers and requests the next chunk's before it works
//                   through the current one: no step of the serial loop waits on memory it has only just asked for.  One back-pointer byte per cell
//                   goes to the utterance's slice of the workspace, frame-major ([t][S]: the stores of a frame are consecutive).  Then the backtrack,
//                   in the same launch: the workgroup loads the AL_W x AL_W window of back-pointers that ends at the current cell, thread 0 walks
//                   until it leaves the window (at least one frame per round trip to memory, 16 on a path that advances a row per frame or slower),
//                   writing frame_row into LDS.  The workgroup then writes frame_row and finds each row's run from the places where frame_row
//                   changes: no atomics.  What differs between the kernels comes in as callables (lambdas of the kernel): the value in frame 0 and
//                   the transition of the forward pass, the end row, the decoding of a back-pointer byte and the rows a path may begin in.
//   statistics      one float64 chain per thread over a state's rows in list order, frames ascending (al_state_frames).
// Every offset read from a device table is clamped, and an utterance whose slices do not fit its lengths fails (ok 0) without touching anything
// outside its clamped slices: the kernels stay inside their buffers whatever the tables hold.  No atomics; nothing depends on the batch.
#pragma once
#include <math.h>

#include "fcl_common.h"

namespace fcl {

constexpr int AL_TMAX = 4096, AL_SMAX = 1024, AL_DMAX = 40, AL_MMAX = 1024, AL_UTT_MAX = 65535;
constexpr int AL_LF = 16, AL_LS = 64;    // frames per workgroup and slots per tile of the log-likelihood kernels
constexpr int AL_NT = 256;               // threads of a Viterbi kernel
constexpr int AL_NR = AL_SMAX / AL_NT;   // rows per thread
constexpr int AL_CH = 8;                 // frames per staging chunk
constexpr int AL_W = 16;                 // the backtrack's window is AL_W frames x AL_W rows (AL_W * AL_W == AL_NT)

__device__ __forceinline__ long long al_clamp(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// ---- the utterance (Args: fcl_al_t or fcl_al_lattice_t, which name these fields alike) ----
// its clamped geometry: f0 / r0 and nf / nr are its slices' starts and (capped) lengths whatever the tables hold; false: the utterance cannot be run
// inside its slices
struct AlUtt {
    int f0, r0, nf, nr;
    long long c0;
};
template <class Args>
__device__ __forceinline__ bool al_utt(const Args& a, int u, AlUtt& g) {
    const long long f0 = al_clamp(a.frame_off[u], 0, a.frames), f1 = al_clamp(a.frame_off[u + 1], f0, a.frames);
    const long long r0 = al_clamp(a.row_off[u], 0, a.rows), r1 = al_clamp(a.row_off[u + 1], r0, a.rows);
    const long long c0 = al_clamp(a.cell_off[u], 0, a.cells), c1 = al_clamp(a.cell_off[u + 1], c0, a.cells);
    g.f0 = (int)f0, g.r0 = (int)r0, g.c0 = c0;
    g.nf = (int)min(f1 - f0, (long long)AL_TMAX), g.nr = (int)min(r1 - r0, (long long)AL_SMAX);
    return f1 - f0 >= 1 && f1 - f0 <= min(a.max_t, AL_TMAX) && r1 - r0 >= 1 && r1 - r0 <= min(a.max_s, AL_SMAX) && (f1 - f0) * (r1 - r0) <= c1 - c0;
}

// the utterance has no alignment: frame_row -1, row_frames 0 (row_begin: the utterance's first frame), score -inf, ok 0
template <class Args>
__device__ __forceinline__ void al_fail(const Args& a, int u, const AlUtt& g, int tid) {
    for (int t = tid; t < g.nf; t += AL_NT) a.frame_row[g.f0 + t] = -1;
    for (int r = tid; r < g.nr; r += AL_NT) a.row_begin[g.r0 + r] = g.f0, a.row_frames[g.r0 + r] = 0;
    if (tid == 0) a.score[u] = -INFINITY, a.ok[u] = 0;
}

// ---- the Viterbi phases; the LDS arrays are the calling kernel's: vcol[2][AL_SMAX], fr[AL_TMAX], seg_b / seg_e[AL_SMAX], win[AL_NT], st[4] ----
// forward: column after column, the ll values of a chunk of frames in registers one chunk ahead.  LL: the utterance's ll rows, state[k]: the model
// state of the thread's row k, ws: the utterance's back-pointer bytes.  first(k, r, ll) is V(r, 0); best(k, r, vp, bp) is the best predecessor value
// of row r in the previous column vp and sets the cell's back-pointer byte bp (0 on entry: stay).  Ends behind the last column's barrier.
// T, S and M are al_utt's and the kernel's clamped values; the function says so because the code generated for gfx950 depends on it: with the line
// a chunk waits for memory in its first frame alone (as it does when the loop stands in the kernel itself), without it the chain kernel's other
// seven frames each wait for the back-pointer stores of the frame before (s_waitcnt vmcnt(0) in every row's block; checked in the disassembly).
template <class First, class Best>
__device__ __forceinline__ void al_forward(const float* LL, unsigned char* ws, float (*vcol)[AL_SMAX], const int (&state)[AL_NR], int T, int S, int M,
                                           int tid, const First& first, const Best& best) {
    __builtin_assume(T >= 1 && T <= AL_TMAX && S >= 1 && S <= AL_SMAX && M >= 1 && M <= AL_MMAX);
    float nxt[AL_NR][AL_CH];
#pragma unroll
    for (int k = 0; k < AL_NR; ++k)
#pragma unroll
        for (int i = 0; i < AL_CH; ++i) nxt[k][i] = (tid + k * AL_NT < S && i < T) ? LL[(long long)i * M + state[k]] : 0.f;
    for (int c0 = 0; c0 < T; c0 += AL_CH) {
        float cur[AL_NR][AL_CH];
#pragma unroll
        for (int k = 0; k < AL_NR; ++k)
#pragma unroll
            for (int i = 0; i < AL_CH; ++i) {
                cur[k][i] = nxt[k][i];
                const int t = c0 + AL_CH + i;
                nxt[k][i] = (tid + k * AL_NT < S && t < T) ? LL[(long long)t * M + state[k]] : 0.f;
            }
#pragma unroll
        for (int i = 0; i < AL_CH; ++i) {
            const int t = c0 + i;
            if (t < T) {  // uniform over the workgroup
                const float* vp = vcol[(t - 1) & 1];
                float* vn = vcol[t & 1];
#pragma unroll
                for (int k = 0; k < AL_NR; ++k) {
                    const int r = tid + k * AL_NT;
                    if (r < S) {
                        float v;
                        int bp = 0;
                        if (t == 0) {
                            v = first(k, r, cur[k][i]);
                        } else {
                            v = cur[k][i] + best(k, r, vp, bp);
                        }
                        vn[r] = v;
                        ws[(long long)t * S + r] = (unsigned char)bp;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// backtrack: from (end_row, T - 1) down to frame 0, fr[t] = the path's row in frame t.  step(r, mv) is how many rows the back-pointer byte mv of row r
// goes down, < 0 for a byte the row cannot have; start_ok(r): the path may begin in row r.  A move is taken only if it stays in [0, S).  false: no
// alignment (an illegal byte, a move out of the rows, a start that is not one).  Also resets seg_b / seg_e for al_runs.
template <class Step, class StartOk>
__device__ __forceinline__ bool al_backtrack(const unsigned char* ws, unsigned short* fr, short* seg_b, short* seg_e, unsigned char* win, int* st,
                                             int end_row, int T, int S, int tid, const Step& step, const StartOk& start_ok) {
    for (int r = tid; r < S; r += AL_NT) seg_b[r] = -1, seg_e[r] = -1;
    if (tid == 0) st[0] = end_row, st[1] = T - 1, st[2] = 0, st[3] = 0;  // the walk's state: row, frame, done, failed
    __syncthreads();
    for (int round = 0; round < T; ++round) {
        if (st[2]) break;
        const int r0 = min(max(st[0], 0), S - 1), t0 = min(max(st[1], 0), T - 1);
        const int wt = t0 - (tid / AL_W), wr = r0 - (tid % AL_W);
        win[tid] = (wt >= 0 && wr >= 0) ? ws[(long long)wt * S + wr] : (unsigned char)0;
        __syncthreads();
        if (tid == 0) {
            int r = r0, t = t0, done = 0, bad = 0;
            while (t0 - t < AL_W && r0 - r < AL_W) {
                fr[t] = (unsigned short)r;
                if (t == 0) {
                    done = 1, bad = !start_ok(r);
                    break;
                }
                const int s = step(r, (int)win[(t0 - t) * AL_W + (r0 - r)]);
                if (s < 0 || r - s < 0) {
                    done = 1, bad = 1;
                    break;
                }
                r -= s;
                --t;
            }
            st[0] = r, st[1] = t, st[2] = done, st[3] = bad;
        }
        __syncthreads();
    }
    return st[2] && !st[3];
}

// runs: frame_row (the utterance's slice), and each row's run from the places where fr changes: seg_b the first frame, seg_e the end, -1: no frames
__device__ __forceinline__ void al_runs(int* frame_row, const unsigned short* fr, short* seg_b, short* seg_e, int T, int tid) {
    for (int t = tid; t < T; t += AL_NT) {
        const int r = fr[t];  // < S: every entry was written by the walk
        frame_row[t] = r;
        if (t == 0 || fr[t - 1] != r) seg_b[r] = (short)t;
        if (t == T - 1 || fr[t + 1] != r) seg_e[r] = (short)(t + 1);
    }
    __syncthreads();
}

// ---- the statistics kernels' walk: frame(f) for the frames of state m's rows in list order, frames ascending; -> the number of frames.  The row
// list and the runs are clamped to [0, rows) and [0, frames] whatever the tables hold.
template <class Frame>
__device__ __forceinline__ long long al_state_frames(int m, const int* __restrict__ state_off, const int* __restrict__ state_rows,
                                                     const int* __restrict__ row_begin, const int* __restrict__ row_frames, long long frames, long long rows,
                                                     const Frame& frame) {
    const long long e0 = al_clamp(state_off[m], 0, rows), e1 = al_clamp(state_off[m + 1], e0, rows);
    long long n = 0;
    for (long long e = e0; e < e1; ++e) {
        const long long r = al_clamp(state_rows[e], 0, rows - 1);
        const long long b = al_clamp(row_begin[r], 0, frames), cnt = al_clamp(row_frames[r], 0, frames - b);
        for (long long f = b; f < b + cnt; ++f) frame(f);
        n += cnt;
    }
    return n;
}

// ---- what the two Viterbi entries check, in this order: the struct, n_utt, M, the entry's own fields (`own(a)`: an error code or FCL_OK), -- an empty
// batch ends here, FCL_OK --, max_t / max_s, the totals (row_words: the int32 words of the widest per-row table, rows_text its name in the message),
// the entry's pointers (`ptrs(a)`: all there; ptr_names for the message), the workspace
template <class Args, class Own, class Ptrs>
static int al_check_batch(const char* who, const Args* a, int row_words, const char* rows_text, Own own, Ptrs ptrs, const char* ptr_names) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n_utt >= 0 && a->n_utt <= AL_UTT_MAX, FCL_ERR_SHAPE, "%s: 0 <= n_utt <= %d expected (got %d)", who, AL_UTT_MAX, a->n_utt);
    FCL_REQUIRE(a->n_states >= 1 && a->n_states <= AL_MMAX, FCL_ERR_SHAPE, "%s: 1 <= M <= %d expected (got %d)", who, AL_MMAX, a->n_states);
    if (int rc = own(a)) return rc;
    if (a->n_utt == 0) return FCL_OK;
    FCL_REQUIRE(a->max_t >= 1 && a->max_t <= AL_TMAX && a->max_s >= 1 && a->max_s <= AL_SMAX, FCL_ERR_SHAPE,
                "%s: 1 <= max_t <= %d and 1 <= max_s <= %d expected (got %d, %d)", who, AL_TMAX, AL_SMAX, a->max_t, a->max_s);
    FCL_REQUIRE(a->frames >= 1 && a->rows >= 1 && a->cells >= 1 && a->frames * a->n_states < 0x7fffffffLL && a->rows * row_words < 0x7fffffffLL, FCL_ERR_SHAPE,
                "%s: 1 <= frames, rows, cells, frames x M < 2^31 and %s < 2^31 expected (got %lld, %lld, %lld)", who, rows_text, (long long)a->frames,
                (long long)a->rows, (long long)a->cells);
    FCL_REQUIRE(ptrs(a), FCL_ERR_INVALID, "%s: null %s", who, ptr_names);
    FCL_REQUIRE(a->workspace_bytes >= fcl_al_workspace_bytes(a->cells, a->n_utt), FCL_ERR_WORKSPACE,
                "%s: the workspace has %zu bytes, %lld cells need %zu (fcl_al_workspace_bytes)", who, a->workspace_bytes, (long long)a->cells,
                fcl_al_workspace_bytes(a->cells, a->n_utt));
    return FCL_OK;
}

}  // namespace fcl
