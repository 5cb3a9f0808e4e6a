// align.hip — forced alignment: Gaussian log-likelihoods, Viterbi over an utterance's chain of rows with a device-side backtrack, and the sufficient
// statistics of an alignment (include/fcl_hip.h "Forced alignment").  gfx950 only.  The shape of the Viterbi kernel is align_common.h's; here:
//   al_loglik_kernel   a workgroup of 256 threads owns 16 consecutive frames.  It stages their x rows (pitch D4) and, tile after tile, the mean and
//                      ivar rows of 64 states (pitch D4 | 1: lanes that differ in the state hit different banks) in LDS, D4 = D rounded up to a
//                      multiple of 4 with zero x / mean / ivar.  A wave owns 4 of the frames and lane l the state tile + l: the x values are wave
//                      broadcasts, each mean / ivar value read from LDS serves 4 frames.  q is ONE fma chain in ascending d from 0:
//                      df = x - mean, q = fma(df * df, ivar, q);  ll = fma(-0.5, q, gconst).
//   al_viterbi_kernel  V(r, 0) is ll for row 0 alone.  A back-pointer byte is 0 stay, 1 advance, 2 skip: stay wins, advance replaces it only when
//                      strictly greater, then skip.  The path ends in row S - 1 and begins in row 0; a skip is taken only by the row's own row_skip.
//   al_stats_kernel    one workgroup of 64 threads per model state, thread d owns coefficient d: one float64 chain per (state, coefficient) over
//                      the state's frames, x and x * x widened to double before the add; added to acc_s / acc_q.
#include "align_common.h"

namespace fcl {

constexpr int AL_SKIP_MAX = 4;

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

__global__ __launch_bounds__(AL_NT) void al_viterbi_kernel(const fcl_al_t a) {
    __shared__ float vcol[2][AL_SMAX];
    __shared__ unsigned short fr[AL_TMAX];
    __shared__ short seg_b[AL_SMAX], seg_e[AL_SMAX];
    __shared__ unsigned char skb[AL_SMAX];  // the row's skip, 0 where it has none (or an unusable one)
    __shared__ unsigned char win[AL_NT];
    __shared__ int st[4];
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

    al_forward(
        LL, ws, vcol, state, T, S, M, tid, [&](int, int r, float ll) { return r == 0 ? ll : -INFINITY; },
        [&](int k, int r, const float* vp, int& bp) {
            float best = vp[r];
            int b = 0;
            if (r > 0) {
                const float adv = vp[r - 1];
                if (adv > best) best = adv, b = 1;
            }
            if (skip[k]) {
                const float sk = vp[r - skip[k]];
                if (sk > best) best = sk, b = 2;
            }
            bp = b;
            return best;
        });
    const float score = vcol[(T - 1) & 1][S - 1];

    const auto step = [&](int r, int mv) { return mv == 0 ? 0 : (mv == 1 ? 1 : (mv == 2 && skb[r] >= 2 ? (int)skb[r] : -1)); };
    if (!al_backtrack(ws, fr, seg_b, seg_e, win, st, S - 1, T, S, tid, step, [](int r) { return r == 0; })) {
        al_fail(a, u, g, tid);
        return;
    }
    al_runs(a.frame_row + g.f0, fr, seg_b, seg_e, T, tid);
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
    double s = 0.0, q = 0.0;
    const long long n = al_state_frames(m, state_off, state_rows, row_begin, row_frames, frames, rows, [&](long long f) {
        const float v = x[f * D + d];
        s += (double)v;
        q += (double)v * (double)v;  // exact: the product of two floats fits a double
    });
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
    const int rc = al_check_batch(
        "al_viterbi_fwd", a, 1, "rows",
        [](const fcl_al_t* a) -> int {
            FCL_REQUIRE(a->max_skip == 0 || (a->max_skip >= 2 && a->max_skip <= AL_SKIP_MAX), FCL_ERR_SHAPE,
                        "al_viterbi_fwd: max_skip (the largest row_skip, K + 1) must be 0 or 2 .. %d (got %d)", AL_SKIP_MAX, a->max_skip);
            return FCL_OK;
        },
        [](const fcl_al_t* a) {
            return a->ll && a->frame_off && a->row_off && a->cell_off && a->row_state && a->row_skip && a->workspace && a->frame_row && a->row_begin &&
                   a->row_frames && a->score && a->ok;
        },
        "ll / frame_off / row_off / cell_off / row_state / row_skip / workspace / frame_row / row_begin / row_frames / score / ok");
    if (rc || a->n_utt == 0) return rc;
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
