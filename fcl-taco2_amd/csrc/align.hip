// align.hip — forced alignment: Gaussian log-likelihoods, Viterbi over an utterance's row graph with a device-side backtrack, and the sufficient
// statistics of an alignment (include/fcl_hip.h "Forced alignment").  gfx950 only.
//   al_loglik_kernel   a workgroup of 256 threads owns 16 consecutive frames.  It stages their x rows (pitch D4) and, tile after tile, the mean and
//                      ivar rows of 64 states (pitch D4 | 1: lanes that differ in the state hit different banks) in LDS, D4 = D rounded up to a
//                      multiple of 4 with zero x / mean / ivar.  A wave owns 4 of the frames and lane l the state tile + l: the x values are wave
//                      broadcasts, each mean / ivar value read from LDS serves 4 frames.  q is ONE fma chain in ascending d from 0:
//                      df = x - mean, q = fma(df * df, ivar, q);  ll = fma(-0.5, q, gconst).
//   al_viterbi_kernel  ONE workgroup of 256 threads per utterance; thread i owns the rows i, i + 256, i + 512, i + 768.  Column t depends on column
//                      t - 1 alone: two rolling V columns in LDS, one barrier per frame.  The gather ll[t][row_state[r]] does not depend on V, so a
//                      thread holds the values of its rows for a chunk of 8 frames in registers and requests the next chunk's before it works
//                      through the current one: no step of the serial loop waits on memory it has only just asked for.  One back-pointer byte per
//                      cell (0 stay, 1 advance, 2 skip) goes to the utterance's slice of the workspace, frame-major ([t][S]: the stores of a frame
//                      are consecutive).  Then the backtrack, in the same launch: the workgroup loads the 16 x 16 window of back-pointers that ends
//                      at the current cell, thread 0 walks until it leaves the window (at least one frame per round trip to memory, 16 on a path
//                      that advances a row per frame or slower), writing frame_row into LDS.  A move is taken only if it stays in [0, S) and, for
//                      a skip, only by the row's own row_skip; anything else, or another row than 0 in frame 0, fails the utterance.  The
//                      workgroup then writes frame_row, and row_begin / row_frames from the places where frame_row changes: no atomics.
//   al_stats_kernel    one workgroup of 64 threads per model state, thread d owns coefficient d: one float64 chain per (state, coefficient) over
//                      the state's rows in list order, frames ascending, x and x * x widened to double before the add; added to acc_s / acc_q.
// Every offset read from a device table is clamped, and an utterance whose slices do not fit its lengths fails (ok 0) without touching anything
// outside its clamped slices: the kernels stay inside their buffers whatever the tables hold.  No atomics; nothing depends on the batch.
#include <math.h>

#include "fcl_common.h"

namespace fcl {

constexpr int AL_TMAX = 4096, AL_SMAX = 1024, AL_DMAX = 40, AL_MMAX = 1024, AL_UTT_MAX = 65535, AL_SKIP_MAX = 4;
constexpr int AL_LF = 16, AL_LS = 64;    // frames per workgroup and states per tile of al_loglik_kernel
constexpr int AL_NT = 256;               // threads of al_viterbi_kernel
constexpr int AL_NR = AL_SMAX / AL_NT;   // rows per thread
constexpr int AL_CH = 8;                 // frames per staging chunk
constexpr int AL_W = 16;                 // the backtrack's window is AL_W frames x AL_W rows (AL_W * AL_W == AL_NT)

__global__ __launch_bounds__(256) void al_loglik_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ ivar,
                                                        const float* __restrict__ gconst, float* __restrict__ ll, long long frames, int D, int M) {
    __shared__ float xs[AL_LF * AL_DMAX];
    __shared__ float ms[AL_LS * (AL_DMAX + 1)];
    __shared__ float vs[AL_LS * (AL_DMAX + 1)];
    const int tid = threadIdx.x, D4 = (D + 3) & ~3, pitch = D4 | 1;
    const long long f0 = (long long)blockIdx.x * AL_LF;
    const int nf = (int)min((long long)AL_LF, frames - f0);
    for (int e = tid; e < AL_LF * D4; e += 256) {
        const int f = e / D4, d = e - f * D4;
        xs[e] = (f < nf && d < D) ? x[(f0 + f) * D + d] : 0.f;
    }
    const int lane = tid & (AL_LS - 1), fg = (tid >> 6) * 4;
    for (int m0 = 0; m0 < M; m0 += AL_LS) {
        __syncthreads();  // the x rows are there; the last tile's readers are done
        const int ns = min(AL_LS, M - m0);
        for (int e = tid; e < AL_LS * D4; e += 256) {
            const int s = e / D4, d = e - s * D4;
            const bool in = s < ns && d < D;
            ms[s * pitch + d] = in ? mean[(long long)(m0 + s) * D + d] : 0.f;
            vs[s * pitch + d] = in ? ivar[(long long)(m0 + s) * D + d] : 0.f;
        }
        __syncthreads();
        if (lane < ns) {
            const float* mr = ms + lane * pitch;
            const float* vr = vs + lane * pitch;
            const float* xr = xs + fg * D4;
            float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
            for (int d = 0; d < D4; ++d) {
                const float mu = mr[d], iv = vr[d];
                const float d0 = xr[d] - mu, d1 = xr[D4 + d] - mu, d2 = xr[2 * D4 + d] - mu, d3 = xr[3 * D4 + d] - mu;
                q0 = fmaf(d0 * d0, iv, q0);
                q1 = fmaf(d1 * d1, iv, q1);
                q2 = fmaf(d2 * d2, iv, q2);
                q3 = fmaf(d3 * d3, iv, q3);
            }
            const float gc = gconst[m0 + lane];
            float* out = ll + (f0 + fg) * M + m0 + lane;
            if (fg + 0 < nf) out[0] = fmaf(-0.5f, q0, gc);
            if (fg + 1 < nf) out[M] = fmaf(-0.5f, q1, gc);
            if (fg + 2 < nf) out[2LL * M] = fmaf(-0.5f, q2, gc);
            if (fg + 3 < nf) out[3LL * M] = fmaf(-0.5f, q3, gc);
        }
    }
}

__device__ __forceinline__ long long al_clamp(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// the utterance's clamped geometry: f0 / r0 and nf / nr are its slices' starts and (capped) lengths whatever the tables hold; false: the utterance
// cannot be run inside its slices
struct AlUtt {
    int f0, r0, nf, nr;
    long long c0;
};
__device__ __forceinline__ bool al_utt(const fcl_al_t& a, int u, AlUtt& g) {
    const long long f0 = al_clamp(a.frame_off[u], 0, a.frames), f1 = al_clamp(a.frame_off[u + 1], f0, a.frames);
    const long long r0 = al_clamp(a.row_off[u], 0, a.rows), r1 = al_clamp(a.row_off[u + 1], r0, a.rows);
    const long long c0 = al_clamp(a.cell_off[u], 0, a.cells), c1 = al_clamp(a.cell_off[u + 1], c0, a.cells);
    g.f0 = (int)f0, g.r0 = (int)r0, g.c0 = c0;
    g.nf = (int)min(f1 - f0, (long long)AL_TMAX), g.nr = (int)min(r1 - r0, (long long)AL_SMAX);
    return f1 - f0 >= 1 && f1 - f0 <= min(a.max_t, AL_TMAX) && r1 - r0 >= 1 && r1 - r0 <= min(a.max_s, AL_SMAX) && (f1 - f0) * (r1 - r0) <= c1 - c0;
}

// the utterance has no alignment: frame_row -1, row_frames 0 (row_begin: the utterance's first frame), score -inf, ok 0
__device__ __forceinline__ void al_fail(const fcl_al_t& a, int u, const AlUtt& g, int tid) {
    for (int t = tid; t < g.nf; t += AL_NT) a.frame_row[g.f0 + t] = -1;
    for (int r = tid; r < g.nr; r += AL_NT) a.row_begin[g.r0 + r] = g.f0, a.row_frames[g.r0 + r] = 0;
    if (tid == 0) a.score[u] = -INFINITY, a.ok[u] = 0;
}

__global__ __launch_bounds__(AL_NT) void al_viterbi_kernel(const fcl_al_t a) {
    __shared__ float vcol[2][AL_SMAX];
    __shared__ unsigned short fr[AL_TMAX];
    __shared__ short seg_b[AL_SMAX], seg_e[AL_SMAX];  // first frame and end of each row's run, -1: no frames
    __shared__ unsigned char skb[AL_SMAX];            // the row's skip, 0 where it has none (or an unusable one)
    __shared__ unsigned char win[AL_NT];
    __shared__ int st[4];  // the backtrack's state: row, frame, done, failed
    const int u = blockIdx.x, tid = threadIdx.x;
    AlUtt g;
    if (!al_utt(a, u, g)) {
        al_fail(a, u, g, tid);
        return;
    }
    const int T = g.nf, S = g.nr, M = min(max(a.n_states, 1), AL_MMAX), max_skip = min(a.max_skip, AL_SKIP_MAX);
    const float* __restrict__ LL = a.ll + (long long)g.f0 * M;
    unsigned char* __restrict__ ws = reinterpret_cast<unsigned char*>(a.workspace) + g.c0;

    int state[AL_NR], skip[AL_NR];
#pragma unroll
    for (int k = 0; k < AL_NR; ++k) {
        const int r = tid + k * AL_NT;
        state[k] = 0, skip[k] = 0;
        if (r < S) {
            state[k] = min(max(a.row_state[g.r0 + r], 0), M - 1);
            const int j = a.row_skip[g.r0 + r];
            skip[k] = (j >= 2 && j <= max_skip && r - j >= 0) ? j : 0;
            skb[r] = (unsigned char)skip[k];
        }
    }

    // ---- forward: column after column, the ll values of a chunk of frames in registers one chunk ahead ----
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
                            v = r == 0 ? cur[k][i] : -INFINITY;
                        } else {
                            // stay wins; advance replaces it only when strictly greater, then skip only when strictly greater
                            float best = vp[r];
                            if (r > 0) {
                                const float adv = vp[r - 1];
                                if (adv > best) best = adv, bp = 1;
                            }
                            if (skip[k]) {
                                const float sk = vp[r - skip[k]];
                                if (sk > best) best = sk, bp = 2;
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
    const float score = vcol[(T - 1) & 1][S - 1];

    // ---- backtrack: from (S - 1, T - 1) down to frame 0 ----
    for (int r = tid; r < S; r += AL_NT) seg_b[r] = -1, seg_e[r] = -1;
    if (tid == 0) st[0] = S - 1, st[1] = T - 1, st[2] = 0, st[3] = 0;
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
                    done = 1, bad = r != 0;
                    break;
                }
                const int mv = win[(t0 - t) * AL_W + (r0 - r)];
                const int step = mv == 0 ? 0 : (mv == 1 ? 1 : (mv == 2 ? (int)skb[r] : -1));
                if (step < 0 || (mv == 2 && step < 2) || r - step < 0) {
                    done = 1, bad = 1;
                    break;
                }
                r -= step;
                --t;
            }
            st[0] = r, st[1] = t, st[2] = done, st[3] = bad;
        }
        __syncthreads();
    }
    if (!st[2] || st[3]) {
        al_fail(a, u, g, tid);
        return;
    }

    // ---- frame_row, and each row's run from the places where frame_row changes ----
    for (int t = tid; t < T; t += AL_NT) {
        const int r = fr[t];  // < S: every entry was written by the walk
        a.frame_row[g.f0 + t] = r;
        if (t == 0 || fr[t - 1] != r) seg_b[r] = (short)t;
        if (t == T - 1 || fr[t + 1] != r) seg_e[r] = (short)(t + 1);
    }
    __syncthreads();
    for (int r = tid; r < S; r += AL_NT) {
        int b = seg_b[r], n = 0;
        if (b >= 0) {
            n = seg_e[r] - b;
        } else {  // a skipped row begins where the next row with frames does (at most max_skip - 1 rows on)
            b = T;
            for (int j = 1; j < AL_SKIP_MAX && r + j < S; ++j)
                if (seg_b[r + j] >= 0) {
                    b = seg_b[r + j];
                    break;
                }
        }
        a.row_begin[g.r0 + r] = g.f0 + b;
        a.row_frames[g.r0 + r] = n;
    }
    if (tid == 0) a.score[u] = score, a.ok[u] = 1;
}

__global__ __launch_bounds__(64) void al_stats_kernel(const float* __restrict__ x, const int* __restrict__ row_begin, const int* __restrict__ row_frames,
                                                      const int* __restrict__ state_off, const int* __restrict__ state_rows, long long* __restrict__ acc_n,
                                                      double* __restrict__ acc_s, double* __restrict__ acc_q, long long frames, long long rows, int D) {
    const int m = blockIdx.x, d = threadIdx.x;
    if (d >= D) return;
    const long long e0 = al_clamp(state_off[m], 0, rows), e1 = al_clamp(state_off[m + 1], e0, rows);
    double s = 0.0, q = 0.0;
    long long n = 0;
    for (long long e = e0; e < e1; ++e) {
        const long long r = al_clamp(state_rows[e], 0, rows - 1);
        const long long b = al_clamp(row_begin[r], 0, frames), cnt = al_clamp(row_frames[r], 0, frames - b);
        for (long long f = b; f < b + cnt; ++f) {
            const float v = x[f * D + d];
            s += (double)v;
            q += (double)v * (double)v;  // exact: the product of two floats fits a double
        }
        n += cnt;
    }
    acc_s[(long long)m * D + d] += s;
    acc_q[(long long)m * D + d] += q;
    if (d == 0) acc_n[m] += n;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_al_workspace_bytes(int64_t total_cells, int n_utt) {
    (void)n_utt;  // one back-pointer byte per cell, the utterances' slices back to back
    return total_cells <= 0 ? 0 : (((size_t)total_cells + 255) & ~(size_t)255);
}

int fcl_al_loglik_fwd(const float* x, const float* mean, const float* ivar, const float* gconst, float* ll, int64_t frames, int d, int n_states,
                      fcl_stream_t stream) {
    FCL_REQUIRE(d >= 1 && d <= AL_DMAX && n_states >= 1 && n_states <= AL_MMAX, FCL_ERR_SHAPE,
                "al_loglik_fwd: 1 <= D <= %d and 1 <= M <= %d expected (got %d, %d)", AL_DMAX, AL_MMAX, d, n_states);
    FCL_REQUIRE(frames >= 0 && frames * n_states < 0x7fffffffLL, FCL_ERR_SHAPE, "al_loglik_fwd: 0 <= frames and frames x M < 2^31 expected (got %lld)",
                (long long)frames);
    if (frames == 0) return FCL_OK;
    FCL_REQUIRE(x && mean && ivar && gconst && ll, FCL_ERR_INVALID, "al_loglik_fwd: null x / mean / ivar / gconst / ll");
    ProfScope ps("al_loglik_kernel", 4.0 * d * n_states * (double)frames, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(al_loglik_kernel, dim3((unsigned)((frames + AL_LF - 1) / AL_LF)), dim3(256), 0, (hipStream_t)stream, x, mean, ivar, gconst, ll,
                       (long long)frames, d, n_states);
    return check_hip(hipGetLastError(), "al_loglik_fwd");
}

int fcl_al_viterbi_fwd(const fcl_al_t* a, fcl_stream_t stream) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "al_viterbi_fwd: null argument");
    FCL_REQUIRE(a->n_utt >= 0 && a->n_utt <= AL_UTT_MAX, FCL_ERR_SHAPE, "al_viterbi_fwd: 0 <= n_utt <= %d expected (got %d)", AL_UTT_MAX, a->n_utt);
    FCL_REQUIRE(a->n_states >= 1 && a->n_states <= AL_MMAX, FCL_ERR_SHAPE, "al_viterbi_fwd: 1 <= M <= %d expected (got %d)", AL_MMAX, a->n_states);
    FCL_REQUIRE(a->max_skip == 0 || (a->max_skip >= 2 && a->max_skip <= AL_SKIP_MAX), FCL_ERR_SHAPE,
                "al_viterbi_fwd: max_skip (the largest row_skip, K + 1) must be 0 or 2 .. %d (got %d)", AL_SKIP_MAX, a->max_skip);
    if (a->n_utt == 0) return FCL_OK;
    FCL_REQUIRE(a->max_t >= 1 && a->max_t <= AL_TMAX && a->max_s >= 1 && a->max_s <= AL_SMAX, FCL_ERR_SHAPE,
                "al_viterbi_fwd: 1 <= max_t <= %d and 1 <= max_s <= %d expected (got %d, %d)", AL_TMAX, AL_SMAX, a->max_t, a->max_s);
    FCL_REQUIRE(a->frames >= 1 && a->rows >= 1 && a->cells >= 1 && a->frames * a->n_states < 0x7fffffffLL && a->rows < 0x7fffffffLL, FCL_ERR_SHAPE,
                "al_viterbi_fwd: 1 <= frames, rows, cells, frames x M < 2^31 and rows < 2^31 expected (got %lld, %lld, %lld)", (long long)a->frames,
                (long long)a->rows, (long long)a->cells);
    FCL_REQUIRE(a->ll && a->frame_off && a->row_off && a->cell_off && a->row_state && a->row_skip && a->workspace && a->frame_row && a->row_begin &&
                    a->row_frames && a->score && a->ok,
                FCL_ERR_INVALID, "al_viterbi_fwd: null ll / frame_off / row_off / cell_off / row_state / row_skip / workspace / frame_row / row_begin / "
                                 "row_frames / score / ok");
    FCL_REQUIRE(a->workspace_bytes >= fcl_al_workspace_bytes(a->cells, a->n_utt), FCL_ERR_WORKSPACE,
                "al_viterbi_fwd: the workspace has %zu bytes, %lld cells need %zu (fcl_al_workspace_bytes)", a->workspace_bytes, (long long)a->cells,
                fcl_al_workspace_bytes(a->cells, a->n_utt));
    ProfScope ps("al_viterbi_kernel", 6.0 * (double)a->cells, (double)a->cells, (hipStream_t)stream);
    hipLaunchKernelGGL(al_viterbi_kernel, dim3((unsigned)a->n_utt), dim3(AL_NT), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "al_viterbi_fwd");
}

int fcl_al_stats_fwd(const float* x, const int32_t* row_begin, const int32_t* row_frames, const int32_t* state_off, const int32_t* state_rows,
                     int64_t* acc_n, double* acc_s, double* acc_q, int64_t frames, int64_t rows, int d, int n_states, fcl_stream_t stream) {
    FCL_REQUIRE(d >= 1 && d <= AL_DMAX && n_states >= 1 && n_states <= AL_MMAX, FCL_ERR_SHAPE,
                "al_stats_fwd: 1 <= D <= %d and 1 <= M <= %d expected (got %d, %d)", AL_DMAX, AL_MMAX, d, n_states);
    FCL_REQUIRE(frames >= 0 && rows >= 0 && frames * d < 0x7fffffffLL && rows < 0x7fffffffLL, FCL_ERR_SHAPE,
                "al_stats_fwd: 0 <= frames, rows, frames x D < 2^31 and rows < 2^31 expected (got %lld, %lld)", (long long)frames, (long long)rows);
    if (frames == 0 || rows == 0) return FCL_OK;
    FCL_REQUIRE(x && row_begin && row_frames && state_off && state_rows && acc_n && acc_s && acc_q, FCL_ERR_INVALID,
                "al_stats_fwd: null x / row_begin / row_frames / state_off / state_rows / acc_n / acc_s / acc_q");
    ProfScope ps("al_stats_kernel", 3.0 * d * (double)frames, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(al_stats_kernel, dim3((unsigned)n_states), dim3(64), 0, (hipStream_t)stream, x, row_begin, row_frames, state_off, state_rows,
                       (long long*)acc_n, acc_s, acc_q, (long long)frames, (long long)rows, d);
    return check_hip(hipGetLastError(), "al_stats_fwd");
}

}  // extern "C"
