// pyin.hip — probabilistic YIN on the d' rows of px_yin_kernel (include/fcl_hip.h "Probabilistic YIN"; Mauch & Dixon 2014).  gfx950 only.
//   pyin_obs_kernel      a workgroup of ONE wave walks PYIN_FPB consecutive frames; the threshold, weight and edge tables sit in LDS for all of them.
//                        Per frame: the d' row into LDS (coalesced), lane l owns the lags tau_min + 64 r + l.  A lag is a candidate when it is a
//                        strict record (below the minimum of every earlier lag of the range: a wave prefix-minimum per r, the carry handed on) and
//                        its successor is not lower -- exactly the lags the contract's serial walk stops at.  The candidates come out of ballots in
//                        ascending lag; lane 0 alone runs the rare serial part (threshold count and bin by binary search in LDS, the parabola, the
//                        masses, ov / bf0 in LDS in candidate order) and the sum of ov over ascending bins.  Then all lanes write lv, lu, bf0.
//   pyin_viterbi_kernel  ONE workgroup of 256 threads per utterance, thread i owns the states i, i + 256, i + 512, i + 768 of (voicing, bin).  Two
//                        rolling V columns in LDS, each voicing's bins between W_MAX words of -inf on either side, so that a predecessor outside
//                        [0, nb) loses every comparison without a test; neighbouring lanes read neighbouring words for every k.  One barrier per
//                        frame; the next frame's observations are requested before the current frame's band loop.  One back-pointer byte per cell
//                        (v1 (2 W + 1) + k) goes to the utterance's slice of the workspace, frame-major.  The backtrack, in the same launch: the
//                        workgroup loads the back-pointers of 32 frames into LDS, thread 0 walks them, 32 threads write state and f0.  The walk
//                        clamps every bin into [0, nb) and counts frames down from T: it ends whatever the workspace or the tables hold.
// Every sum, product and quotient below is one rounded float32 operation (no contraction): tests/pyin_ref.py restates both kernels in numpy float32
// and the results agree bit for bit, logf aside.  No atomics; a batch is its per-frame / per-utterance runs.
#include <math.h>

#include "fcl_common.h"

#pragma clang fp contract(off)

namespace fcl {

constexpr int PYIN_NB_MAX = 512, PYIN_W_MAX = 63, PYIN_LAG_MAX = 520, PYIN_NTHR = 100, PYIN_UTT_MAX = 65535;
constexpr int PYIN_FPB = 8;                            // frames per workgroup of pyin_obs_kernel
constexpr int PYIN_NT = 256;                           // threads of pyin_viterbi_kernel
constexpr int PYIN_SPT = 2 * PYIN_NB_MAX / PYIN_NT;    // states per thread
constexpr int PYIN_VS = PYIN_NB_MAX + 2 * PYIN_W_MAX;  // one voicing's padded V row
constexpr int PYIN_CH = 32;                            // frames per round of the backtrack
constexpr float PYIN_PA = 0.01f, PYIN_FLOOR = 1e-30f;

__global__ __launch_bounds__(64) void pyin_obs_kernel(const fcl_pyin_t a) {
    __shared__ float row[PYIN_LAG_MAX], thr[PYIN_NTHR], cw[PYIN_NTHR + 1], edge[PYIN_NB_MAX], ov[PYIN_NB_MAX], best[PYIN_NB_MAX], bf[PYIN_NB_MAX];
    __shared__ unsigned long long msk[8];  // the candidates' ballots: written and read by lane 0 alone
    const int lane = threadIdx.x, nb = a.nb, tau_min = a.tau_min, tau_max = a.tau_max, n_lag = a.n_lag;
    for (int i = lane; i < PYIN_NTHR; i += 64) thr[i] = a.thr[i];
    for (int i = lane; i <= PYIN_NTHR; i += 64) cw[i] = a.cw[i];
    for (int i = lane; i < nb - 1; i += 64) edge[i] = a.edge[i];
    const long long fbase = (long long)blockIdx.x * PYIN_FPB;
    for (int s = 0; s < PYIN_FPB; ++s) {
        const long long f = fbase + s;
        if (f >= a.frames) break;  // uniform over the workgroup
        __syncthreads();           // the tables are there; the last frame's readers are done
        const float* __restrict__ dp = a.cmnd + (size_t)f * n_lag;
        for (int i = lane; i < n_lag; i += 64) row[i] = dp[i];
        for (int i = lane; i < nb; i += 64) ov[i] = 0.f, best[i] = 0.f, bf[i] = 0.f;
        __syncthreads();
        // candidates: strict records whose successor is not lower
        float carry = INFINITY;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int t = tau_min + 64 * r + lane;
            const bool in = t <= tau_max;
            const float v = in ? row[t] : INFINITY;
            float inc = v < INFINITY ? v : INFINITY;  // a NaN is never a record and never lowers the minimum
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float up = __shfl_up(inc, o);
                if (lane >= o) inc = up < inc ? up : inc;
            }
            float before = __shfl_up(inc, 1);  // the minimum of the lanes below, then of everything before
            before = lane == 0 ? carry : (carry < before ? carry : before);
            const float nxt = in ? row[t + 1] : 0.f;  // t + 1 <= tau_max + 1 < n_lag
            const unsigned long long mk = __ballot(in && v < before && !(t < tau_max && nxt < v));
            if (lane == 0) msk[r] = mk;
            const float all = __shfl(inc, 63);
            carry = all < carry ? all : carry;
        }
        if (lane == 0) {
            int last = -1;  // the global record: it takes the mass of the thresholds below it as well
            for (int r = 0; r < 8; ++r)
                if (msk[r]) last = tau_min + 64 * r + 63 - __clzll((long long)msk[r]);
            int rec_i = PYIN_NTHR;
            for (int r = 0; r < 8; ++r) {
                unsigned long long mk = msk[r];
                while (mk) {
                    const int m = tau_min + 64 * r + __ffsll((long long)mk) - 1;
                    mk &= mk - 1;
                    const float pa = row[m - 1], pb = row[m], pc = row[m + 1];  // tau_min >= 2
                    int lo = 0, hi = PYIN_NTHR;  // lo_i = #{i : thr[i - 1] <= d'(m)}: thr ascends
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (thr[mid] <= pb) lo = mid + 1;
                        else hi = mid;
                    }
                    const int lo_i = lo;
                    float mass = cw[rec_i] - cw[lo_i];
                    if (m == last) {
                        const float tail = PYIN_PA * cw[lo_i];
                        mass = mass + tail;
                    }
                    rec_i = lo_i;
                    const float D = (pa - (pb + pb)) + pc;
                    float dl = 0.f;
                    if (D > 0.f) {
                        dl = (0.5f * (pa - pc)) / D;
                        dl = dl < -0.5f ? -0.5f : (dl > 0.5f ? 0.5f : dl);
                    }
                    const float p = (float)m + dl;
                    lo = 0, hi = nb - 1;  // b = #{j : edge[j] >= p}: edge descends
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (edge[mid] >= p) lo = mid + 1;
                        else hi = mid;
                    }
                    ov[lo] = ov[lo] + mass;
                    if (mass > best[lo]) best[lo] = mass, bf[lo] = a.fs / p;
                }
            }
            float pv = 0.f;
            for (int b = 0; b < nb; ++b) pv = pv + ov[b];
            const float u = (1.f - pv) / (float)nb;
            a.lu[f] = logf(u > PYIN_FLOOR ? u : PYIN_FLOOR);
        }
        __syncthreads();
        for (int b = lane; b < nb; b += 64) {
            const float v = ov[b];
            const size_t o = (size_t)f * nb + b;
            a.lv[o] = logf(v > PYIN_FLOOR ? v : PYIN_FLOOR);
            a.bf0[o] = bf[b];
            if (a.ov_out) a.ov_out[o] = v;
        }
    }
}

__global__ __launch_bounds__(PYIN_NT) void pyin_viterbi_kernel(const fcl_pyin_t a) {
    __shared__ float vcol[2][2][PYIN_VS];
    __shared__ float tri[2 * PYIN_W_MAX + 1];
    __shared__ unsigned char bpw[PYIN_CH * 2 * PYIN_NB_MAX];
    __shared__ float redv[PYIN_NT];
    __shared__ int redi[PYIN_NT], walk[PYIN_CH], cur[1];
    const int u = blockIdx.x, tid = threadIdx.x, nb = a.nb, W = a.w, K = 2 * W + 1, S = 2 * nb;
    const long long frames = a.frames;
    const long long f0 = min(max((long long)a.utt_off[u], 0LL), frames), f1 = min(max((long long)a.utt_off[u + 1], 0LL), frames);
    if (f1 <= f0) {  // an empty or descending slice: no frames of its own
        if (tid == 0) a.score[u] = -INFINITY;
        return;
    }
    const int T = (int)(f1 - f0);
    const float* __restrict__ LV = a.lv + (size_t)f0 * nb;
    const float* __restrict__ LU = a.lu + f0;
    unsigned char* __restrict__ ws = reinterpret_cast<unsigned char*>(a.workspace) + (size_t)f0 * S;
    const float la00 = a.la[0], la01 = a.la[1], la10 = a.la[2], la11 = a.la[3];

    for (int i = tid; i < 2 * 2 * PYIN_VS; i += PYIN_NT) (&vcol[0][0][0])[i] = -INFINITY;
    for (int i = tid; i < K; i += PYIN_NT) tri[i] = a.tri[i];
    int vo[PYIN_SPT], bo[PYIN_SPT], br[PYIN_SPT];  // the owned states' voicing and bin; br: the bin the band loop reads at
    float obs[PYIN_SPT];
#pragma unroll
    for (int j = 0; j < PYIN_SPT; ++j) {
        const int s = tid + j * PYIN_NT;
        vo[j] = s >= nb ? 1 : 0;
        bo[j] = s - vo[j] * nb;
        br[j] = s < S ? bo[j] : 0;  // a slot past the last state runs the loop on bin 0 and drops the result: its reads stay inside the row
        obs[j] = s < S ? (vo[j] ? LU[0] : LV[bo[j]]) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PYIN_SPT; ++j)
        if (tid + j * PYIN_NT < S) vcol[0][vo[j]][PYIN_W_MAX + bo[j]] = obs[j];
#pragma unroll
    for (int j = 0; j < PYIN_SPT; ++j) {
        const int s = tid + j * PYIN_NT;
        obs[j] = (s < S && T > 1) ? (vo[j] ? LU[1] : LV[(size_t)nb + bo[j]]) : 0.f;
    }
    __syncthreads();

    // ---- forward: column after column ----
    for (int t = 1; t < T; ++t) {
        const float* vp0 = vcol[(t - 1) & 1][0] + (PYIN_W_MAX - W);
        const float* vp1 = vcol[(t - 1) & 1][1] + (PYIN_W_MAX - W);
        float now[PYIN_SPT], m0[PYIN_SPT], m1[PYIN_SPT];
        int k0[PYIN_SPT], k1[PYIN_SPT];
#pragma unroll
        for (int j = 0; j < PYIN_SPT; ++j) {
            const int s = tid + j * PYIN_NT;
            now[j] = obs[j];
            obs[j] = (s < S && t + 1 < T) ? (vo[j] ? LU[t + 1] : LV[(size_t)(t + 1) * nb + bo[j]]) : 0.f;
            m0[j] = m1[j] = -INFINITY, k0[j] = k1[j] = W;
        }
#pragma unroll 8
        for (int k = 0; k < K; ++k) {  // ascending k: a later k wins only when strictly greater.  No branch: several k's reads are in flight together
            const float tk = tri[k];
#pragma unroll
            for (int j = 0; j < PYIN_SPT; ++j) {
                const float c0 = vp0[br[j] + k] + tk, c1 = vp1[br[j] + k] + tk;
                if (c0 > m0[j]) m0[j] = c0, k0[j] = k;
                if (c1 > m1[j]) m1[j] = c1, k1[j] = k;
            }
        }
#pragma unroll
        for (int j = 0; j < PYIN_SPT; ++j) {
            const int s = tid + j * PYIN_NT;
            if (s < S) {
                const float c0 = m0[j] + (vo[j] ? la01 : la00), c1 = m1[j] + (vo[j] ? la11 : la10);
                const bool one = c1 > c0;
                vcol[t & 1][vo[j]][PYIN_W_MAX + bo[j]] = (one ? c1 : c0) + now[j];
                ws[(size_t)t * S + s] = (unsigned char)(one ? K + k1[j] : k0[j]);
            }
        }
        __syncthreads();
    }

    // ---- the end: the largest V, the lowest index among equals ----
    {
        const float* v0 = vcol[(T - 1) & 1][0] + PYIN_W_MAX;
        const float* v1 = vcol[(T - 1) & 1][1] + PYIN_W_MAX;
        float bv = -INFINITY;
        int bi = S;  // S: nothing found yet
#pragma unroll
        for (int j = 0; j < PYIN_SPT; ++j) {
            const int s = tid + j * PYIN_NT;
            if (s < S) {
                const float v = vo[j] ? v1[bo[j]] : v0[bo[j]];
                if (bi == S || v > bv) bv = v, bi = s;
            }
        }
        redv[tid] = bv, redi[tid] = bi;
        __syncthreads();
        for (int o = PYIN_NT / 2; o >= 1; o >>= 1) {
            if (tid < o) {
                const float ov = redv[tid + o];
                const int oi = redi[tid + o];
                if (oi < S && (redi[tid] >= S || ov > redv[tid] || (ov == redv[tid] && oi < redi[tid]))) redv[tid] = ov, redi[tid] = oi;
            }
            __syncthreads();
        }
        if (tid == 0) {
            cur[0] = min(max(redi[0], 0), S - 1);
            a.score[u] = redv[0];
        }
    }

    // ---- backtrack: rounds of PYIN_CH frames, from T - 1 down ----
    __threadfence_block();
    __syncthreads();  // every back-pointer of this workgroup is written
    for (int hi = T - 1; hi >= 0; hi -= PYIN_CH) {
        const int lo = max(hi - PYIN_CH + 1, 0), n = hi - lo + 1;
        const unsigned char* src = ws + (size_t)lo * S;
        for (int i = tid; i < n * S; i += PYIN_NT) bpw[i] = src[i];
        __syncthreads();
        if (tid == 0) {
            int s = cur[0];
            for (int t = hi; t >= lo; --t) {
                walk[t - lo] = s;
                if (t > 0) {  // frame 0 has no predecessor (and no back-pointer)
                    const int code = bpw[(t - lo) * S + s], v1 = code >= K ? 1 : 0, k = code - v1 * K;
                    const int b = s >= nb ? s - nb : s;
                    s = v1 * nb + min(max(b + min(k, K - 1) - W, 0), nb - 1);
                }
            }
            cur[0] = s;
        }
        __syncthreads();
        if (tid < n) {
            const int t = lo + tid, s = walk[tid];
            float hz = 0.f;
            if (s < nb) {
                const float c = a.bf0[((size_t)f0 + t) * nb + s];
                hz = c > 0.f ? c : a.f_bin[s];
            }
            a.state[f0 + t] = s;
            a.f0[f0 + t] = hz;
        }
        __syncthreads();
    }
}

static int pyin_check(const fcl_pyin_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->nb >= 1 && a->nb <= PYIN_NB_MAX, FCL_ERR_SHAPE, "%s: 1 <= nb <= %d pitch bins expected (got %d)", who, PYIN_NB_MAX, a->nb);
    FCL_REQUIRE(a->frames >= 0 && a->frames * (int64_t)(2 * a->nb) < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: frames >= 0 and frames x 2 nb below 2^31 expected (got %lld)",
                who, (long long)a->frames);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_px_pyin_obs_fwd(const fcl_pyin_t* a, fcl_stream_t stream) {
    const int rc = pyin_check(a, "px_pyin_obs_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->tau_min >= 2 && a->tau_min < a->tau_max && a->tau_max <= 511 && a->n_lag >= a->tau_max + 2 && a->n_lag <= PYIN_LAG_MAX, FCL_ERR_SHAPE,
                "px_pyin_obs_fwd: 2 <= tau_min < tau_max <= 511 and tau_max + 2 <= n_lag <= %d expected (got tau_min %d, tau_max %d, n_lag %d)", PYIN_LAG_MAX,
                a->tau_min, a->tau_max, a->n_lag);
    FCL_REQUIRE(a->frames * (int64_t)a->n_lag < 0x7fffffffLL, FCL_ERR_SHAPE, "px_pyin_obs_fwd: frames x n_lag must stay below 2^31 (got %lld frames)",
                (long long)a->frames);
    FCL_REQUIRE(a->fs > 0.f, FCL_ERR_SHAPE, "px_pyin_obs_fwd: fs > 0 expected (got %g)", (double)a->fs);
    if (a->frames == 0) return FCL_OK;
    FCL_REQUIRE(a->cmnd && a->thr && a->cw && a->edge && a->lv && a->lu && a->bf0, FCL_ERR_INVALID, "px_pyin_obs_fwd: null cmnd / thr / cw / edge / lv / lu / bf0");
    ProfScope ps("pyin_obs_kernel", 4.0 * a->n_lag * (double)a->frames, (double)a->frames, (hipStream_t)stream);
    hipLaunchKernelGGL(pyin_obs_kernel, dim3((unsigned)((a->frames + PYIN_FPB - 1) / PYIN_FPB)), dim3(64), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "px_pyin_obs_fwd");
}

int fcl_px_pyin_viterbi_fwd(const fcl_pyin_t* a, fcl_stream_t stream) {
    const int rc = pyin_check(a, "px_pyin_viterbi_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->w >= 1 && a->w <= PYIN_W_MAX, FCL_ERR_SHAPE, "px_pyin_viterbi_fwd: 1 <= W <= %d (the band's half width in bins) expected (got %d)", PYIN_W_MAX,
                a->w);
    FCL_REQUIRE(a->n_utt >= 0 && a->n_utt <= PYIN_UTT_MAX, FCL_ERR_SHAPE, "px_pyin_viterbi_fwd: 0 <= n_utt <= %d expected (got %d)", PYIN_UTT_MAX, a->n_utt);
    if (a->n_utt == 0 || a->frames == 0) return FCL_OK;
    FCL_REQUIRE(a->lv && a->lu && a->bf0 && a->f_bin && a->tri && a->la && a->utt_off && a->workspace && a->state && a->f0 && a->score, FCL_ERR_INVALID,
                "px_pyin_viterbi_fwd: null lv / lu / bf0 / f_bin / tri / la / utt_off / workspace / state / f0 / score");
    FCL_REQUIRE(a->workspace_bytes >= (size_t)a->frames * 2 * (size_t)a->nb, FCL_ERR_WORKSPACE,
                "px_pyin_viterbi_fwd: the workspace has %zu bytes, %lld frames of %d bins need %zu (one byte per frame and state)", a->workspace_bytes,
                (long long)a->frames, a->nb, (size_t)a->frames * 2 * (size_t)a->nb);
    ProfScope ps("pyin_viterbi_kernel", 8.0 * (2 * a->w + 1) * a->nb * (double)a->frames, (double)a->frames, (hipStream_t)stream);
    hipLaunchKernelGGL(pyin_viterbi_kernel, dim3((unsigned)a->n_utt), dim3(PYIN_NT), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "px_pyin_viterbi_fwd");
}

}  // extern "C"
