// evaluate.hip — objective evaluation: mel cepstra, dynamic time warping and the F0 figures over the warping path (include/fcl_hip.h "Evaluation",
// DESIGN 6h).  gfx950 only.
//   ev_cepstra_kernel     a workgroup of 256 threads owns 16 consecutive frames.  It stages the table [D][N] (row pitch N | 1: lanes that differ in k hit
//                         different banks) and its 16 mel rows in LDS; each thread then runs whole outputs c[f][k] = (sum_m table[k][m] x[f][m]) + bias[k],
//                         ONE fma chain in ascending m from 0, the bias added last.
//   ev_dtw_kernel         ONE workgroup of 128 threads per pair.  The cost matrix is swept in strips of 128 rows; inside a strip thread t owns row
//                         i = strip + t, keeps its cepstrum a_i in registers, and at step q works on the cell (i, q - t): the 128 threads sit on one
//                         anti-diagonal, which moves one column per step.  C(i, j - 1) and C(i - 1, j - 1) are the thread's own values of the last two
//                         steps (registers); C(i - 1, j) is its neighbour's value of the last step, handed over through the two rolling anti-diagonals
//                         xc[2][128] in LDS (one barrier per step); the strip's last row goes to edge[Tb] in LDS, from which thread 0 of the next strip
//                         reads.  b's cepstra are staged in LDS as a ring of 256 columns, TRANSPOSED (bs[k][column & 255]: the lanes of a wave read
//                         consecutive words), refilled 128 columns at a time.  The local distance sqrt(sum_k (a_i[k] - b_j[k])^2) is one fma chain in
//                         ascending k over D rounded up to a multiple of 4 (the padding is zero on both sides and adds exactly 0).  One back-pointer
//                         byte per cell (0 diagonal, 1 (i - 1, j), 2 (i, j - 1)) goes to the pair's slice of the workspace, row-major.  Then the
//                         backtrack, in the same launch: the workgroup loads the 8 x 16 window of back-pointers that ends at the current cell, thread 0
//                         walks until it leaves the window (at least 8 cells per round trip to memory), writing the path backwards from the end of the
//                         pair's slice; the workgroup then moves it to the front and fills the rest of the slice with -1.  A move is taken only if it
//                         stays inside the matrix (otherwise diagonal, up, left, whichever exists), so that the path is a valid warping path whatever
//                         the workspace or the inputs hold, and the walk ends after at most Ta + Tb - 1 cells.
//   ev_path_pitch_kernel  one workgroup of 256 threads per pair: thread t sums the path cells t, t + 256, ... in ascending order, then a fixed tree over
//                         the 256 partial results.
// Every offset read from a device table is clamped, and a pair whose slices are too small for its lengths is skipped (path_len 0, cost NaN): the
// kernels stay inside their buffers whatever the tables hold.  No atomics; nothing depends on the batch.
#include <math.h>

#include "fcl_common.h"

namespace fcl {

constexpr int EV_TMAX = 4096, EV_DMAX = 40, EV_NMAX = 256, EV_PAIRS_MAX = 65535;
constexpr int EV_CF = 16;               // frames per workgroup of ev_cepstra_kernel
constexpr int EV_R = 128;               // rows per strip = threads of ev_dtw_kernel
constexpr int EV_RING = 2 * EV_R;       // columns of b in LDS
constexpr int EV_WR = 8, EV_WC = 16;    // the backtrack's window (EV_WR * EV_WC == EV_R)

__global__ __launch_bounds__(256) void ev_cepstra_kernel(const float* __restrict__ x, const float* __restrict__ table, const float* __restrict__ bias,
                                                         float* __restrict__ c, long long frames, int N, int D) {
    __shared__ float tab[EV_DMAX * (EV_NMAX + 1)];
    __shared__ float xs[EV_CF * (EV_NMAX + 1)];
    const int tid = threadIdx.x, pitch = N | 1;
    const long long f0 = (long long)blockIdx.x * EV_CF;
    const int nf = (int)min((long long)EV_CF, frames - f0);
    for (int e = tid; e < D * N; e += 256) tab[(e / N) * pitch + e % N] = table[e];
    for (int e = tid; e < nf * N; e += 256) xs[(e / N) * pitch + e % N] = x[f0 * N + e];
    __syncthreads();
    for (int o = tid; o < nf * D; o += 256) {
        const int f = o / D, k = o - f * D;
        const float* tr = tab + k * pitch;
        const float* xr = xs + f * pitch;
        float acc = 0.f;
#pragma unroll 4
        for (int m = 0; m < N; ++m) acc = fmaf(tr[m], xr[m], acc);
        c[f0 * D + o] = acc + bias[k];
    }
}

__device__ __forceinline__ long long ev_clamp(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// the pair's clamped geometry; false: the pair cannot be run inside its slices
struct EvPair {
    int a0, b0, ta, tb, p0;
    long long c0;
};
__device__ __forceinline__ bool ev_pair(const fcl_ev_t& a, int p, EvPair& g) {
    const long long a0 = ev_clamp(a.a_off[p], 0, a.frames_a), a1 = ev_clamp(a.a_off[p + 1], a0, a.frames_a);
    const long long b0 = ev_clamp(a.b_off[p], 0, a.frames_b), b1 = ev_clamp(a.b_off[p + 1], b0, a.frames_b);
    const long long c0 = ev_clamp(a.cell_off[p], 0, a.cells), c1 = ev_clamp(a.cell_off[p + 1], c0, a.cells);
    const long long p0 = ev_clamp(a.path_off[p], 0, a.path_rows), p1 = ev_clamp(a.path_off[p + 1], p0, a.path_rows);
    g.a0 = (int)a0, g.b0 = (int)b0, g.p0 = (int)p0, g.c0 = c0;
    g.ta = (int)min(a1 - a0, (long long)min(a.max_ta, EV_TMAX));
    g.tb = (int)min(b1 - b0, (long long)min(a.max_tb, EV_TMAX));
    return g.ta >= 1 && g.tb >= 1 && (long long)g.ta * g.tb <= c1 - c0 && (long long)g.ta + g.tb - 1 <= p1 - p0;
}

__global__ __launch_bounds__(EV_R) void ev_dtw_kernel(const fcl_ev_t a) {
    __shared__ float bs[EV_DMAX * EV_RING];
    __shared__ float edge[EV_TMAX];
    __shared__ float xc[2][EV_R];
    __shared__ unsigned char win[EV_R];
    __shared__ int st[4];  // the backtrack's state: i, j, cells written, done
    const int p = blockIdx.x, t = threadIdx.x;
    EvPair g;
    if (!ev_pair(a, p, g)) {
        if (t == 0) a.path_len[p] = 0, a.cost[p] = __builtin_nanf("");
        return;
    }
    const int ta = g.ta, tb = g.tb, D = min(max(a.d, 1), EV_DMAX), D4 = (D + 3) & ~3;
    const float* __restrict__ A = a.a + (long long)g.a0 * D;
    const float* __restrict__ B = a.b + (long long)g.b0 * D;
    unsigned char* __restrict__ ws = reinterpret_cast<unsigned char*>(a.workspace) + g.c0;
    for (int e = t; e < (D4 - D) * EV_RING; e += EV_R) bs[D * EV_RING + e] = 0.f;  // the padding rows stay zero

    for (int s0 = 0; s0 < ta; s0 += EV_R) {
        const int i = s0 + t;
        const bool row = i < ta;
        float ar[EV_DMAX];
#pragma unroll
        for (int k = 0; k < EV_DMAX; ++k) ar[k] = (row && k < D) ? A[(long long)i * D + k] : 0.f;
        float left = 0.f, prev_up = 0.f;
        const int nq = tb + min(EV_R, ta - s0) - 1;
        for (int q = 0; q < nq; ++q) {
            if ((q & (EV_R - 1)) == 0 && q < tb) {  // columns q .. q + 127 enter the ring; the slots they take were last read 128 steps ago
                const int ne = min(EV_R, tb - q) * D;
                for (int e = t; e < ne; e += EV_R) {
                    const int col = e / D, k = e - col * D;
                    bs[k * EV_RING + ((q + col) & (EV_RING - 1))] = B[(long long)q * D + e];
                }
                __syncthreads();
            }
            const int j = q - t;
            if (row && j >= 0 && j < tb) {
                const float up = t == 0 ? edge[j] : xc[(q - 1) & 1][t - 1];  // C(i - 1, j): read only where i > 0 makes it one
                const float* bc = bs + (j & (EV_RING - 1));
                float acc = 0.f;
#pragma unroll
                for (int k4 = 0; k4 < EV_DMAX; k4 += 4) {
                    if (k4 < D) {
#pragma unroll
                        for (int k = k4; k < k4 + 4; ++k) {
                            const float df = ar[k] - bc[k * EV_RING];
                            acc = fmaf(df, df, acc);
                        }
                    }
                }
                const float dist = __fsqrt_rn(acc);
                // the diagonal wins; (i - 1, j) replaces it only when strictly smaller, then (i, j - 1) only when strictly smaller
                float best = 0.f;
                int bp = -1;
                if (i > 0 && j > 0) best = prev_up, bp = 0;
                if (i > 0 && (bp < 0 || up < best)) best = up, bp = 1;
                if (j > 0 && (bp < 0 || left < best)) best = left, bp = 2;
                const float cv = bp < 0 ? dist : dist + best;
                ws[(long long)i * tb + j] = (unsigned char)max(bp, 0);
                prev_up = up;
                left = cv;
                xc[q & 1][t] = cv;
                if (t == EV_R - 1) edge[j] = cv;
                if (i == ta - 1 && j == tb - 1) a.cost[p] = cv;
            }
            __syncthreads();
        }
    }

    // ---- backtrack: from (Ta - 1, Tb - 1) to (0, 0), written backwards from the end of the pair's slice ----
    const int cap = ta + tb - 1;
    int* __restrict__ path = a.path + 2LL * g.p0;
    if (t == 0) st[0] = ta - 1, st[1] = tb - 1, st[2] = 0, st[3] = 0;
    __syncthreads();
    for (int round = 0; round < cap; ++round) {
        const int i0 = min(max(st[0], 0), ta - 1), j0 = min(max(st[1], 0), tb - 1);
        if (st[3]) break;
        const int wi = i0 - (t / EV_WC), wj = j0 - (t % EV_WC);
        win[t] = (wi >= 0 && wj >= 0) ? ws[(long long)wi * tb + wj] : (unsigned char)0;
        __syncthreads();
        if (t == 0) {
            int i = i0, j = j0, n = st[2], done = 0;
            while (i0 - i < EV_WR && j0 - j < EV_WC && n < cap) {
                path[2 * (cap - 1 - n)] = i;
                path[2 * (cap - 1 - n) + 1] = j;
                ++n;
                if (i == 0 && j == 0) {
                    done = 1;
                    break;
                }
                int mv = win[(i0 - i) * EV_WC + (j0 - j)];
                if (mv > 2 || (mv == 0 && (i == 0 || j == 0)) || (mv == 1 && i == 0) || (mv == 2 && j == 0)) mv = (i > 0 && j > 0) ? 0 : (i > 0 ? 1 : 2);
                i -= mv != 2;
                j -= mv != 1;
            }
            st[0] = i, st[1] = j, st[2] = n, st[3] = done | (n >= cap);
        }
        __syncthreads();
    }
    const int n = min(max(st[2], 0), cap), gap = cap - n;
    if (gap > 0) {  // to the front, in chunks: a chunk is read, then written below every entry still unread
        for (int base = 0; base < n; base += EV_R) {
            const int m = base + t;
            int vi = 0, vj = 0;
            if (m < n) vi = path[2 * (gap + m)], vj = path[2 * (gap + m) + 1];
            __syncthreads();
            if (m < n) path[2 * m] = vi, path[2 * m + 1] = vj;
            __syncthreads();
        }
        for (int m = n + t; m < cap; m += EV_R) path[2 * m] = -1, path[2 * m + 1] = -1;
    }
    if (t == 0) a.path_len[p] = n;
}

__global__ __launch_bounds__(256) void ev_path_pitch_kernel(const fcl_ev_t a) {
    __shared__ int s_vv[256], s_vuv[256];
    __shared__ float s_sum[256];
    const int p = blockIdx.x, t = threadIdx.x;
    EvPair g;
    const bool ok = ev_pair(a, p, g);
    int vv = 0, vuv = 0;
    float sum = 0.f;
    if (ok) {
        const int n = min(max(a.path_len[p], 0), g.ta + g.tb - 1);
        const int* __restrict__ path = a.path + 2LL * g.p0;
        for (int m = t; m < n; m += 256) {
            const int i = min(max(path[2 * m], 0), g.ta - 1), j = min(max(path[2 * m + 1], 0), g.tb - 1);
            const float pa = a.pitch_a[g.a0 + i], pb = a.pitch_b[g.b0 + j];
            const bool va = pa > 0.f, vb = pb > 0.f;
            if (va && vb) {
                const float df = pa - pb;
                sum += df * df;
                ++vv;
            } else if (va != vb) {
                ++vuv;
            }
        }
    }
    s_vv[t] = vv, s_vuv[t] = vuv, s_sum[t] = sum;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s_vv[t] += s_vv[t + h], s_vuv[t] += s_vuv[t + h], s_sum[t] += s_sum[t + h];
        __syncthreads();
    }
    if (t == 0) a.counts[2 * p] = s_vv[0], a.counts[2 * p + 1] = s_vuv[0], a.sums[p] = s_sum[0];
}

// the checks the two entries on fcl_ev_t share; *launch = false: an empty batch
static int ev_check(const fcl_ev_t* a, const char* who, bool* launch) {
    *launch = false;
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->n_pairs >= 0 && a->n_pairs <= EV_PAIRS_MAX, FCL_ERR_SHAPE, "%s: 0 <= n_pairs <= %d expected (got %d)", who, EV_PAIRS_MAX, a->n_pairs);
    FCL_REQUIRE(a->d >= 1 && a->d <= EV_DMAX, FCL_ERR_SHAPE, "%s: 1 <= D <= %d expected (got %d)", who, EV_DMAX, a->d);
    if (a->n_pairs == 0) return FCL_OK;
    FCL_REQUIRE(a->max_ta >= 1 && a->max_ta <= EV_TMAX && a->max_tb >= 1 && a->max_tb <= EV_TMAX, FCL_ERR_SHAPE,
                "%s: 1 <= max_ta, max_tb <= %d expected (got %d, %d)", who, EV_TMAX, a->max_ta, a->max_tb);
    FCL_REQUIRE(a->frames_a >= 1 && a->frames_b >= 1 && a->frames_a < 0x7fffffffLL && a->frames_b < 0x7fffffffLL && a->cells >= 1 && a->path_rows >= 1 &&
                    a->path_rows < 0x7fffffffLL,
                FCL_ERR_SHAPE, "%s: 1 <= frames_a, frames_b, path_rows < 2^31 and cells >= 1 expected (got %lld, %lld, %lld, %lld)", who, (long long)a->frames_a,
                (long long)a->frames_b, (long long)a->path_rows, (long long)a->cells);
    FCL_REQUIRE(a->a_off && a->b_off && a->cell_off && a->path_off && a->path && a->path_len, FCL_ERR_INVALID,
                "%s: null a_off / b_off / cell_off / path_off / path / path_len", who);
    *launch = true;
    return FCL_OK;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_ev_dtw_workspace_bytes(int64_t total_cells, int n_pairs) {
    (void)n_pairs;  // one back-pointer byte per cell, the pairs' slices back to back
    return total_cells <= 0 ? 0 : (((size_t)total_cells + 255) & ~(size_t)255);
}

int fcl_ev_cepstra_fwd(const float* x, const float* table, const float* bias, float* c, int64_t frames, int n_mels, int d, fcl_stream_t stream) {
    FCL_REQUIRE(n_mels >= 2 && n_mels <= EV_NMAX && d >= 1 && d <= EV_DMAX && d <= n_mels - 1, FCL_ERR_SHAPE,
                "ev_cepstra_fwd: 2 <= n_mels <= %d and 1 <= D <= min(n_mels - 1, %d) expected (got %d, %d)", EV_NMAX, EV_DMAX, n_mels, d);
    FCL_REQUIRE(frames >= 0 && frames * n_mels < 0x7fffffffLL, FCL_ERR_SHAPE, "ev_cepstra_fwd: 0 <= frames and frames x n_mels < 2^31 expected (got %lld)",
                (long long)frames);
    if (frames == 0) return FCL_OK;
    FCL_REQUIRE(x && table && bias && c, FCL_ERR_INVALID, "ev_cepstra_fwd: null x / table / bias / c");
    ProfScope ps("ev_cepstra_kernel", 2.0 * n_mels * d * (double)frames, (double)frames, (hipStream_t)stream);
    hipLaunchKernelGGL(ev_cepstra_kernel, dim3((unsigned)((frames + EV_CF - 1) / EV_CF)), dim3(256), 0, (hipStream_t)stream, x, table, bias, c, (long long)frames,
                       n_mels, d);
    return check_hip(hipGetLastError(), "ev_cepstra_fwd");
}

int fcl_ev_dtw_fwd(const fcl_ev_t* a, fcl_stream_t stream) {
    bool launch;
    const int rc = ev_check(a, "ev_dtw_fwd", &launch);
    if (rc != FCL_OK || !launch) return rc;
    FCL_REQUIRE(a->a && a->b && a->workspace && a->cost, FCL_ERR_INVALID, "ev_dtw_fwd: null a / b / workspace / cost");
    FCL_REQUIRE(a->workspace_bytes >= fcl_ev_dtw_workspace_bytes(a->cells, a->n_pairs), FCL_ERR_WORKSPACE,
                "ev_dtw_fwd: the workspace has %zu bytes, %lld cells need %zu (fcl_ev_dtw_workspace_bytes)", a->workspace_bytes, (long long)a->cells,
                fcl_ev_dtw_workspace_bytes(a->cells, a->n_pairs));
    ProfScope ps("ev_dtw_kernel", (3.0 * a->d + 8.0) * (double)a->cells, (double)a->cells, (hipStream_t)stream);
    hipLaunchKernelGGL(ev_dtw_kernel, dim3((unsigned)a->n_pairs), dim3(EV_R), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "ev_dtw_fwd");
}

int fcl_ev_path_pitch_fwd(const fcl_ev_t* a, fcl_stream_t stream) {
    bool launch;
    const int rc = ev_check(a, "ev_path_pitch_fwd", &launch);
    if (rc != FCL_OK || !launch) return rc;
    FCL_REQUIRE(a->pitch_a && a->pitch_b && a->counts && a->sums, FCL_ERR_INVALID, "ev_path_pitch_fwd: null pitch_a / pitch_b / counts / sums");
    ProfScope ps("ev_path_pitch_kernel", 4.0 * (double)a->path_rows, (double)a->path_rows, (hipStream_t)stream);
    hipLaunchKernelGGL(ev_path_pitch_kernel, dim3((unsigned)a->n_pairs), dim3(256), 0, (hipStream_t)stream, *a);
    return check_hip(hipGetLastError(), "ev_path_pitch_fwd");
}

}  // extern "C"
