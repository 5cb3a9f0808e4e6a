// align_lattice.hip — forced alignment over a lattice: Viterbi over an utterance whose rows name up to 8 predecessors each and carry START / FINAL
// flags, with the choice of the end row and the backtrack on the device (include/fcl_hip.h "Forced alignment, lattice graphs").  gfx950 only.
//   al_lattice_viterbi_kernel  the shape of align_common.h's Viterbi; here: V(r, 0) is ll for the START rows.  A row's eight predecessor distances (16
//                      bits each: S <= 1024) stay in four registers of its thread; an unusable slot is stored as 0.  Almost every row has slot 0
//                      alone, so slot 0 is tried first and the other seven sit behind one flag per row: a row without them pays what a chain row
//                      pays, two LDS reads per frame.  The same sanitised table lies in LDS for the backtrack.  A back-pointer byte is 0 stay, 1 +
//                      slot otherwise.  The end row is the FINAL row with the largest finite V(r, T - 1), the lowest row on ties: every thread
//                      reduces its own rows, then a tree over LDS whose combiner (larger value, then lower row) is commutative and associative, so
//                      the order of the reduction cannot show.  In the backtrack a move over a word boundary leaves the window at once: one round
//                      trip per such move.  A move is taken only by the row's own usable slot; anything else, or a row without START in frame 0,
//                      fails the utterance.  States, slots and flags read from the device tables are clamped like the offsets.
#include "align_common.h"

namespace fcl {

constexpr int LT_NP = 8;  // predecessor slots per row

// the better end row of two: the larger value, the lower row on equal values; row -1 is "none" (its value is -inf and every real candidate is finite)
__device__ __forceinline__ void lt_better(float& v, int& r, float v2, int r2) {
    if (r2 >= 0 && (r < 0 || v2 > v || (v2 == v && r2 < r))) v = v2, r = r2;
}

__global__ __launch_bounds__(AL_NT) void al_lattice_viterbi_kernel(const fcl_al_lattice_t a) {
    __shared__ float vcol[2][AL_SMAX];
    __shared__ unsigned short fr[AL_TMAX];
    __shared__ short seg_b[AL_SMAX], seg_e[AL_SMAX];              // first frame and end of each row's run, -1: no frames
    __shared__ __align__(16) unsigned short pd[AL_SMAX * LT_NP];  // the usable predecessor distances, 0: the slot does not count
    __shared__ unsigned char flg[AL_SMAX];                        // bit 0 START, bit 1 FINAL
    __shared__ unsigned char win[AL_NT];
    __shared__ float red_v[AL_NT];
    __shared__ int red_r[AL_NT];
    __shared__ int st[4];  // the backtrack's state: row, frame, done, failed
    const int u = blockIdx.x, tid = threadIdx.x;
    AlUtt g;
    if (!al_utt(a, u, g)) {
        al_fail(a, u, g, tid);
        return;
    }
    const int T = g.nf, S = g.nr, M = min(max(a.n_states, 1), AL_MMAX);
    const float* __restrict__ LL = a.ll + (long long)g.f0 * M;
    unsigned char* __restrict__ ws = reinterpret_cast<unsigned char*>(a.workspace) + g.c0;

    int state[AL_NR], p0[AL_NR], flags[AL_NR];
    unsigned pk[AL_NR][LT_NP / 2];  // slots 2i and 2i + 1 in the halves of pk[k][i]
    bool more[AL_NR];               // any usable slot beyond slot 0
#pragma unroll
    for (int k = 0; k < AL_NR; ++k) {
        const int r = tid + k * AL_NT;
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

    al_forward(
        LL, ws, vcol, state, T, S, M, tid, [&](int k, int, float ll) { return (flags[k] & 1) ? ll : -INFINITY; },
        [&](int k, int r, const float* vp, int& bp) {
            // stay wins; the usable slots in slot order, each replaces the winner only when strictly greater
            float best = vp[r];
            int b = 0;
            if (p0[k]) {
                const float c = vp[r - p0[k]];
                if (c > best) best = c, b = 1;
            }
            if (more[k]) {
#pragma unroll
                for (int s = 1; s < LT_NP; ++s) {
                    const int d = (int)((pk[k][s >> 1] >> (16 * (s & 1))) & 0xffffu);
                    if (d) {
                        const float c = vp[r - d];
                        if (c > best) best = c, b = 1 + s;
                    }
                }
            }
            bp = b;
            return best;
        });

    // ---- the end row: the FINAL row with the largest finite V(r, T - 1), the lowest row on ties ----
    {
        const float* vl = vcol[(T - 1) & 1];
        float bv = -INFINITY;
        int br = -1;
#pragma unroll
        for (int k = 0; k < AL_NR; ++k) {
            const int r = tid + k * AL_NT;
            if (r < S && (flags[k] & 2)) {
                const float v = vl[r];
                if (isfinite(v)) lt_better(bv, br, v, r);
            }
        }
        red_v[tid] = bv, red_r[tid] = br;
        __syncthreads();
        for (int h = AL_NT / 2; h >= 1; h >>= 1) {
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
        al_fail(a, u, g, tid);
        return;
    }

    const auto step = [&](int r, int mv) {
        if (mv == 0) return 0;
        const int d = mv <= LT_NP ? (int)pd[r * LT_NP + mv - 1] : 0;
        return d >= 1 ? d : -1;
    };
    if (!al_backtrack(ws, fr, seg_b, seg_e, win, st, end_row, T, S, tid, step, [&](int r) { return (flg[r] & 1) != 0; })) {
        al_fail(a, u, g, tid);
        return;
    }
    al_runs(a.frame_row + g.f0, fr, seg_b, seg_e, T, tid);
    for (int r = tid; r < S; r += AL_NT) {
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
    const int rc = al_check_batch(
        "al_lattice_viterbi_fwd", a, LT_NP, "rows x 8", [](const fcl_al_lattice_t*) -> int { return FCL_OK; },
        [](const fcl_al_lattice_t* a) {
            return a->ll && a->frame_off && a->row_off && a->cell_off && a->row_state && a->row_pred && a->row_flags && a->workspace && a->frame_row &&
                   a->row_begin && a->row_frames && a->score && a->ok;
        },
        "ll / frame_off / row_off / cell_off / row_state / row_pred / row_flags / workspace / frame_row / row_begin / row_frames / score / ok");
    if (rc || a->n_utt == 0) return rc;
    ProfScope ps("al_lattice_viterbi_kernel", 6.0 * (double)a->cells, (double)a->cells, (hipStream_t)stream);
    hipLaunchKernelGGL(al_lattice_viterbi_kernel, dim3((unsigned)a->n_utt), dim3(AL_NT), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "al_lattice_viterbi_fwd");
}

}  // extern "C"
