// resample.hip — band-limited resampling of a packed batch of waveforms (include/fcl_hip.h "Resampling").  gfx950 only.
//   rs_resample_kernel  a workgroup of 256 threads owns `tile` consecutive outputs of ONE utterance (blockIdx.y; blockIdx.x counts the tiles of the
//                       longest one, the others' surplus blocks leave at once).  It stages the tile's input span x[n0 - K .. n1 + K] in LDS, zero where
//                       the index lies outside the utterance, and each thread then runs whole outputs: y[t] = sum_j c[p][j] x[n - j] as ONE fma chain
//                       in ascending j, the sample from LDS, the coefficient from the transposed table table[(j + K) L + p] (a few hundred KB: L2).
//                       Slot -> output: with `period` = L (the tile holds whole periods of L outputs) slot i of a period takes the output whose
//                       phase p is i, r = i * minv mod L with minv = M^-1 mod L, so that the 64 lanes of a wave read 64 consecutive floats of a
//                       table row; with period = 1 (L above the tile) the slots take the outputs in order.  Either way every output is computed by
//                       one thread from the same staged values in the same order: a batch is bit for bit its per-utterance runs.
#include <algorithm>

#include "fcl_common.h"

namespace fcl {

constexpr int RS_SPAN_CAP = 12288;  // floats of LDS a tile's input span may take (48 KB)
constexpr int RS_TILE_MAX = 1024;

__global__ __launch_bounds__(256) void rs_resample_kernel(const float* __restrict__ x, const int* __restrict__ smp_off_in, const int* __restrict__ smp_off_out,
                                                          const float* __restrict__ table, int L, int M, int K, int tile, int period, int minv,
                                                          int samples_in, int samples_out, float* __restrict__ y) {
    __shared__ float xs[RS_SPAN_CAP];
    const int u = blockIdx.y, tid = threadIdx.x;
    // every offset read from a device table is clamped: the kernel stays inside x and y whatever the tables hold
    const int i0 = min(max(smp_off_in[u], 0), samples_in), n_in = min(max(smp_off_in[u + 1], i0), samples_in) - i0;
    const int o0 = min(max(smp_off_out[u], 0), samples_out), n_out = min(max(smp_off_out[u + 1], o0), samples_out) - o0;
    const long long t0 = (long long)blockIdx.x * tile;
    if (t0 >= n_out) return;
    const int t_end = (int)min(t0 + tile, (long long)n_out);           // the tile's outputs: t0 .. t_end - 1
    const long long n0 = t0 * M / L, n1 = (long long)(t_end - 1) * M / L;  // their positions n: n0 .. n1
    const int span = min((int)(n1 - n0) + 2 * K + 1, RS_SPAN_CAP);     // (the launcher's tile keeps it below the cap: no effect)
    const long long base = n0 - K;
    for (int i = tid; i < span; i += 256) {
        const long long q = base + i;
        xs[i] = (q >= 0 && q < n_in) ? x[(long long)i0 + q] : 0.f;
    }
    __syncthreads();
    const int taps = 2 * K + 1;
    for (int s = tid; s < tile; s += 256) {
        const int q = s / period, i = s - q * period;
        const int r = period > 1 ? (int)((long long)i * minv % period) : i;
        const long long t = t0 + (long long)q * period + r;
        if (t >= t_end) continue;
        const long long pos = t * M;
        const int p = (int)(pos % L), d = (int)(pos / L - n0);  // x[n - j] = xs[d + 2 K - (j + K)]
        const float* c = table + p;
        const float* xv = xs + min(d, RS_SPAN_CAP - taps) + 2 * K;
        float acc = 0.f;
#pragma unroll 4
        for (int jj = 0; jj < taps; ++jj) acc = fmaf(c[(size_t)jj * L], xv[-jj], acc);
        y[(long long)o0 + t] = acc;
    }
}

// the extended Euclidean algorithm on (m mod l, l), l >= 2: returns gcd(m, l) and, when that is 1, *inv = M^-1 mod L
static int rs_gcd_inverse(int m, int l, int* inv) {
    long long a = m % l, b = l, u0 = 1, u1 = 0;
    while (b) {
        const long long q = a / b, r = a - q * b, w = u0 - q * u1;
        a = b, b = r, u0 = u1, u1 = w;
    }
    *inv = (int)((u0 % l + l) % l);
    return (int)a;
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_rs_resample_fwd(const fcl_rs_t* a, fcl_stream_t stream) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "rs_resample_fwd: null argument");
    FCL_REQUIRE(a->l >= 1 && a->m >= 1 && a->k >= 1, FCL_ERR_SHAPE, "rs_resample_fwd: L, M, K >= 1 expected (got %d, %d, %d)", a->l, a->m, a->k);
    FCL_REQUIRE(a->n_utt >= 0 && a->n_utt <= 65535 && a->max_out >= 0 && a->samples_in >= 0 && a->samples_out >= 0 && a->samples_in < 0x7fffffffLL &&
                    a->samples_out < 0x7fffffffLL,
                FCL_ERR_SHAPE, "rs_resample_fwd: 0 <= n_utt <= 65535, max_out >= 0 and 0 <= samples_in, samples_out < 2^31 expected (got %d, %d, %lld, %lld)",
                a->n_utt, a->max_out, (long long)a->samples_in, (long long)a->samples_out);
    if (a->n_utt == 0 || a->max_out == 0) return FCL_OK;
    FCL_REQUIRE(a->x && a->smp_off_in && a->smp_off_out && a->table && a->y, FCL_ERR_INVALID, "rs_resample_fwd: null x / smp_off_in / smp_off_out / table / y");
    int inv = 1;
    FCL_REQUIRE(a->l == 1 || rs_gcd_inverse(a->m, a->l, &inv) == 1, FCL_ERR_SHAPE, "rs_resample_fwd: L / M must be in lowest terms (got %d / %d)", a->l, a->m);
    // the largest tile whose input span (tile - 1) M / L + 2 K + 2 fits the LDS buffer; whole periods of L outputs where one fits
    const long long room = (long long)RS_SPAN_CAP - 2LL * a->k - 2;
    FCL_REQUIRE(room >= 0 && room * a->l / a->m + 1 >= 64, FCL_ERR_SHAPE,
                "rs_resample_fwd: L / M = %d / %d with K = %d is outside the supported range (64 M / L + 2 K + 2 <= %d)", a->l, a->m, a->k, RS_SPAN_CAP);
    int tile = (int)std::min<long long>(RS_TILE_MAX, room * a->l / a->m + 1), period = 1, minv = 1;
    if (a->l >= 2 && a->l <= tile) {
        tile -= tile % a->l;
        period = a->l;
        minv = inv;
    }
    const unsigned tiles = (unsigned)(((long long)a->max_out + tile - 1) / tile);
    ProfScope ps("rs_resample_kernel", 2.0 * (2.0 * a->k + 1.0) * (double)a->samples_out, (double)a->samples_out, (hipStream_t)stream);
    hipLaunchKernelGGL(rs_resample_kernel, dim3(tiles, (unsigned)a->n_utt), dim3(256), 0, (hipStream_t)stream, a->x, a->smp_off_in, a->smp_off_out, a->table,
                       a->l, a->m, a->k, tile, period, minv, (int)a->samples_in, (int)a->samples_out, a->y);
    return check_hip(hipGetLastError(), "rs_resample_fwd");
}

}  // extern "C"
