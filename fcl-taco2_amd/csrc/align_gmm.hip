// align_gmm.hip — forced alignment with Gaussian-mixture states: mixture log-likelihoods, the component posteriors of an alignment and their
// sufficient statistics (include/fcl_hip.h "Forced alignment", the mixture entries).  gfx950 only.  The single-Gaussian kernels of
// align.hip are untouched; the per-component chain here is theirs, operation for operation.
//   al_gmm_loglik_kernel  al_loglik_kernel's shape: a workgroup of 256 threads owns 16 consecutive frames, their x rows staged in LDS (pitch D4), and
//                         walks the model in tiles of at most 64 COMPONENT slots.  A tile takes whole states: every wave reads the component counts
//                         of the 64 states from the tile's first on, scans them (shuffles, no LDS, no barrier) and the tile is the longest prefix
//                         whose counts sum to at most 64 -- at least 8 states, so no state ever straddles a tile and none needs a carry.  Wave 0
//                         writes the slot tables; the mean / ivar rows of the slots are staged at pitch D4 | 1; a wave owns 4 frames and lane l the
//                         slot l (x values are wave broadcasts, 4 independent chains per thread) and leaves l_c = fma(-0.5, q_c, cconst_c) in LDS
//                         ([16][64]); then thread p owns the pair (frame p / ns, state p % ns): mx, the sum of expf(l_c - mx) in ascending c from 0,
//                         ll = mx + logf(sum); a one-component state is l_0 itself, a non-finite mx is the value.
//   al_gmm_post_kernel    frames x 8: 8 consecutive lanes own a frame, lane c the component c of the state the alignment gave it.  Each lane runs
//                         its own chain on global memory (x is a broadcast inside the group), the groups exchange l and expf(l - mx) by shuffles
//                         of width 8, every lane forms the sum in ascending c itself.  Branch-free up to the store: every lane of a wave takes
//                         part in every shuffle.
//   al_gmm_stats_kernel   al_stats_kernel's layout with a component axis: one workgroup of 64 x 8 threads per model state, thread (d, c) owns
//                         coefficient d of the state's component c and runs the plain float64 chains over the state's frames, every product and sum
//                         a statement of its own under `#pragma clang fp contract(off)`: nothing is fused (the disassembly has v_mul_f64 and
//                         v_add_f64 only, no v_fma_f64 / v_fmac_f64).
// A state's components are read as g0 = clamp(comp_off[m], 0, G - 1), count = clamp(comp_off[m + 1] - g0, 1, min(max_comp, G - g0)); frame_state is
// clamped to M - 1, the row lists by al_state_frames (align_common.h): the kernels stay inside their buffers whatever the tables hold.  No atomics.
#include "align_common.h"

namespace fcl {

constexpr int ALG_CMAX = 8, ALG_GMAX = 8192;
constexpr int ALG_PF = 32;  // frames per workgroup of al_gmm_post_kernel

// the components of state m, inside [0, G) whatever comp_off holds: 1 <= cnt <= max_comp <= 8
__device__ __forceinline__ void alg_state(const int* __restrict__ comp_off, int m, int G, int max_comp, int& g0, int& cnt) {
    g0 = (int)al_clamp(comp_off[m], 0, G - 1);
    cnt = (int)al_clamp((long long)comp_off[m + 1] - g0, 1, min(max_comp, G - g0));
}

// NaN wins, then the larger value
__device__ __forceinline__ float alg_max(float mx, float l) { return (l > mx || __builtin_isnan(l)) ? l : mx; }

__global__ __launch_bounds__(256) void al_gmm_loglik_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ ivar,
                                                            const float* __restrict__ cconst, const int* __restrict__ comp_off, float* __restrict__ ll,
                                                            long long frames, int D, int M, int G, int max_comp) {
    __shared__ float xs[AL_LF * AL_DMAX];
    __shared__ float ms[AL_LS * (AL_DMAX + 1)];
    __shared__ float vs[AL_LS * (AL_DMAX + 1)];
    __shared__ float lv[AL_LF * AL_LS];  // l_c of the tile: [frame][slot]
    __shared__ int slot_g[AL_LS];        // the component of each slot
    __shared__ unsigned char st_start[AL_LS], st_cnt[AL_LS];  // the first slot and the count of each state of the tile
    const int tid = threadIdx.x, D4 = (D + 3) & ~3, pitch = D4 | 1;
    const long long f0 = (long long)blockIdx.x * AL_LF;
    const int nf = (int)min((long long)AL_LF, frames - f0);
    for (int e = tid; e < AL_LF * D4; e += 256) {
        const int f = e / D4, d = e - f * D4;
        xs[e] = (f < nf && d < D) ? x[(f0 + f) * D + d] : 0.f;
    }
    const int lane = tid & (AL_LS - 1), fg = (tid >> 6) * 4;
    for (int m0 = 0; m0 < M;) {
        // the tile: the longest run of states from m0 whose components fit 64 slots.  Every wave finds it for itself, lane i looking at state m0 + i.
        int g0 = 0, cnt = 0;
        if (m0 + lane < M) alg_state(comp_off, m0 + lane, G, max_comp, g0, cnt);
        int end = cnt;  // inclusive scan: the slot this state ends at
#pragma unroll
        for (int o = 1; o < AL_LS; o <<= 1) {
            const int v = __shfl_up(end, o);
            if (lane >= o) end += v;
        }
        const int ns = __popcll(__ballot(m0 + lane < M && end <= AL_LS));  // >= 1: lane 0 ends at cnt <= 8
        const int nslots = __shfl(end, ns - 1);
        __syncthreads();  // the x rows are there; the last tile's readers are done
        if (tid < ns) {
            st_start[tid] = (unsigned char)(end - cnt), st_cnt[tid] = (unsigned char)cnt;
            for (int c = 0; c < cnt; ++c) slot_g[end - cnt + c] = g0 + c;
        }
        __syncthreads();
        for (int e = tid; e < AL_LS * D4; e += 256) {
            const int s = e / D4, d = e - s * D4;
            const bool in = s < nslots && d < D;
            const long long g = in ? slot_g[s] : 0;
            ms[s * pitch + d] = in ? mean[g * D + d] : 0.f;
            vs[s * pitch + d] = in ? ivar[g * D + d] : 0.f;
        }
        __syncthreads();
        if (lane < nslots) {
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
            const float cc = cconst[slot_g[lane]];
            float* out = lv + fg * AL_LS + lane;  // the rows past nf hold the values of zero frames: finite, never read
            out[0] = fmaf(-0.5f, q0, cc);
            out[AL_LS] = fmaf(-0.5f, q1, cc);
            out[2 * AL_LS] = fmaf(-0.5f, q2, cc);
            out[3 * AL_LS] = fmaf(-0.5f, q3, cc);
        }
        __syncthreads();
        for (int p = tid; p < ns * nf; p += 256) {
            const int f = p / ns, s = p - f * ns, cn = st_cnt[s];
            const float* lr = lv + f * AL_LS + st_start[s];
            float v = lr[0];
            if (cn > 1) {
                float mx = v;
                for (int c = 1; c < cn; ++c) mx = alg_max(mx, lr[c]);
                v = mx;
                if (isfinite(mx)) {
                    float sum = 0.f;
                    for (int c = 0; c < cn; ++c) sum += expf(lr[c] - mx);
                    v = mx + logf(sum);
                }
            }
            ll[(f0 + f) * M + m0 + s] = v;
        }
        m0 += ns;
    }
}

__global__ __launch_bounds__(256) void al_gmm_post_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ ivar,
                                                          const float* __restrict__ cconst, const int* __restrict__ comp_off,
                                                          const int* __restrict__ frame_state, float* __restrict__ gamma, long long frames, int D, int M,
                                                          int G, int max_comp) {
    const int tid = threadIdx.x, c = tid & (ALG_CMAX - 1);
    const long long fr = (long long)blockIdx.x * ALG_PF + (tid >> 3);
    const bool valid = fr < frames;
    const long long f = valid ? fr : frames - 1;
    const int fs = frame_state[f];
    int g0, cnt;
    alg_state(comp_off, min(max(fs, 0), M - 1), G, max_comp, g0, cnt);
    const bool mine = c < cnt;
    const long long g = g0 + (mine ? c : 0);
    const float* xr = x + f * D;
    const float* mr = mean + g * D;
    const float* vr = ivar + g * D;
    float q = 0.f;  // the padding of D to a multiple of 4 adds exactly 0: the chain over d < D is the padded one
    for (int d = 0; d < D; ++d) {
        const float df = xr[d] - mr[d];
        q = fmaf(df * df, vr[d], q);
    }
    const float l = fmaf(-0.5f, q, cconst[g]);
    float mx = __shfl(l, 0, ALG_CMAX);
#pragma unroll
    for (int k = 1; k < ALG_CMAX; ++k) {
        const float lk = __shfl(l, k, ALG_CMAX);
        if (k < cnt) mx = alg_max(mx, lk);
    }
    const float e = mine ? expf(l - mx) : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < ALG_CMAX; ++k) {
        const float ek = __shfl(e, k, ALG_CMAX);
        if (k < cnt) sum += ek;
    }
    float out = 0.f;
    if (fs >= 0 && mine) out = cnt == 1 ? 1.f : __fdiv_rn(e, sum);
    if (valid) gamma[f * ALG_CMAX + c] = out;
}

__global__ __launch_bounds__(512) void al_gmm_stats_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const int* __restrict__ row_begin,
                                                           const int* __restrict__ row_frames, const int* __restrict__ state_off,
                                                           const int* __restrict__ state_rows, const int* __restrict__ comp_off, double* __restrict__ acc_w,
                                                           double* __restrict__ acc_s, double* __restrict__ acc_q, long long frames, long long rows, int D,
                                                           int G, int max_comp) {
    // Whether a step is fused is part of the contract.  hipcc's __dmul_rn / __dadd_rn are inline functions of a plain * and + that carry the
    // translation unit's contraction mode with them (q + p v came out as v_fmac_f64 through them), so the steps are plain operators under this pragma.
#pragma clang fp contract(off)
    const int m = blockIdx.x, d = threadIdx.x, c = threadIdx.y;
    int g0, cnt;
    alg_state(comp_off, m, G, max_comp, g0, cnt);
    if (d >= D || c >= cnt) return;
    double w = 0.0, s = 0.0, q = 0.0;
    al_state_frames(m, state_off, state_rows, row_begin, row_frames, frames, rows, [&](long long f) {
        const double gm = (double)gamma[f * ALG_CMAX + c], v = (double)x[f * D + d];
        const double p = gm * v;  // exact: the product of two floats fits a double
        const double pv = p * v;
        w = w + gm;
        s = s + p;
        q = q + pv;
    });
    const long long o = (long long)(g0 + c) * D + d;
    acc_s[o] = acc_s[o] + s;
    acc_q[o] = acc_q[o] + q;
    if (d == 0) acc_w[g0 + c] = acc_w[g0 + c] + w;
}

// what the three entries share: D, M, G and max_comp
static int alg_check_model(const char* who, int d, int n_states, int n_comp, int max_comp) {
    FCL_REQUIRE(d >= 1 && d <= AL_DMAX && n_states >= 1 && n_states <= AL_MMAX, FCL_ERR_SHAPE, "%s: 1 <= D <= %d and 1 <= M <= %d expected (got %d, %d)", who,
                AL_DMAX, AL_MMAX, d, n_states);
    FCL_REQUIRE(max_comp >= 1 && max_comp <= ALG_CMAX, FCL_ERR_SHAPE, "%s: max_comp (the largest component count of a state) must lie in 1 .. %d (got %d)", who,
                ALG_CMAX, max_comp);
    FCL_REQUIRE(n_comp >= n_states && n_comp <= ALG_GMAX && (long long)n_comp <= (long long)n_states * max_comp, FCL_ERR_SHAPE,
                "%s: M <= G <= min(%d, M x max_comp) expected (got G %d, M %d, max_comp %d)", who, ALG_GMAX, n_comp, n_states, max_comp);
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_al_gmm_loglik_fwd(const float* x, const float* mean, const float* ivar, const float* cconst, const int32_t* comp_off, float* ll, int64_t frames,
                          int d, int n_states, int n_comp, int max_comp, fcl_stream_t stream) {
    if (int rc = alg_check_model("al_gmm_loglik_fwd", d, n_states, n_comp, max_comp)) return rc;
    FCL_REQUIRE(frames >= 0 && frames * n_states < 0x7fffffffLL, FCL_ERR_SHAPE, "al_gmm_loglik_fwd: 0 <= frames and frames x M < 2^31 expected (got %lld)",
                (long long)frames);
    if (frames == 0) return FCL_OK;
    FCL_REQUIRE(x && mean && ivar && cconst && comp_off && ll, FCL_ERR_INVALID, "al_gmm_loglik_fwd: null x / mean / ivar / cconst / comp_off / ll");
    ProfScope ps("al_gmm_loglik_kernel", (4.0 * d + 4.0) * n_comp * (double)frames, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(al_gmm_loglik_kernel, dim3((unsigned)((frames + AL_LF - 1) / AL_LF)), dim3(256), 0, (hipStream_t)stream, x, mean, ivar, cconst,
                       comp_off, ll, (long long)frames, d, n_states, n_comp, max_comp);
    return check_hip(hipGetLastError(), "al_gmm_loglik_fwd");
}

int fcl_al_gmm_post_fwd(const float* x, const float* mean, const float* ivar, const float* cconst, const int32_t* comp_off, const int32_t* frame_state,
                        float* gamma, int64_t frames, int d, int n_states, int n_comp, int max_comp, fcl_stream_t stream) {
    if (int rc = alg_check_model("al_gmm_post_fwd", d, n_states, n_comp, max_comp)) return rc;
    FCL_REQUIRE(frames >= 0 && frames * AL_DMAX < 0x7fffffffLL, FCL_ERR_SHAPE, "al_gmm_post_fwd: 0 <= frames and frames x 40 < 2^31 expected (got %lld)",
                (long long)frames);
    if (frames == 0) return FCL_OK;
    FCL_REQUIRE(x && mean && ivar && cconst && comp_off && frame_state && gamma, FCL_ERR_INVALID,
                "al_gmm_post_fwd: null x / mean / ivar / cconst / comp_off / frame_state / gamma");
    ProfScope ps("al_gmm_post_kernel", (4.0 * d + 6.0) * ALG_CMAX * (double)frames, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(al_gmm_post_kernel, dim3((unsigned)((frames + ALG_PF - 1) / ALG_PF)), dim3(256), 0, (hipStream_t)stream, x, mean, ivar, cconst, comp_off,
                       frame_state, gamma, (long long)frames, d, n_states, n_comp, max_comp);
    return check_hip(hipGetLastError(), "al_gmm_post_fwd");
}

int fcl_al_gmm_stats_fwd(const float* x, const float* gamma, const int32_t* row_begin, const int32_t* row_frames, const int32_t* state_off,
                         const int32_t* state_rows, const int32_t* comp_off, double* acc_w, double* acc_s, double* acc_q, int64_t frames, int64_t rows, int d,
                         int n_states, int n_comp, int max_comp, fcl_stream_t stream) {
    if (int rc = alg_check_model("al_gmm_stats_fwd", d, n_states, n_comp, max_comp)) return rc;
    FCL_REQUIRE(frames >= 0 && rows >= 0 && frames * AL_DMAX < 0x7fffffffLL && rows < 0x7fffffffLL, FCL_ERR_SHAPE,
                "al_gmm_stats_fwd: 0 <= frames, rows, frames x 40 < 2^31 and rows < 2^31 expected (got %lld, %lld)", (long long)frames, (long long)rows);
    if (frames == 0 || rows == 0) return FCL_OK;
    FCL_REQUIRE(x && gamma && row_begin && row_frames && state_off && state_rows && comp_off && acc_w && acc_s && acc_q, FCL_ERR_INVALID,
                "al_gmm_stats_fwd: null x / gamma / row_begin / row_frames / state_off / state_rows / comp_off / acc_w / acc_s / acc_q");
    ProfScope ps("al_gmm_stats_kernel", 5.0 * d * max_comp * (double)frames, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(al_gmm_stats_kernel, dim3((unsigned)n_states), dim3(64, ALG_CMAX), 0, (hipStream_t)stream, x, gamma, row_begin, row_frames, state_off,
                       state_rows, comp_off, acc_w, acc_s, acc_q, (long long)frames, (long long)rows, d, n_comp, max_comp);
    return check_hip(hipGetLastError(), "al_gmm_stats_fwd");
}

}  // extern "C"
