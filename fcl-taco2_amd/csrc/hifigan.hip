// hifigan.hip — HiFi-GAN generator (kan-bayashi/ParallelWaveGAN `HiFiGANGenerator`, v1 / LJSpeech), the second generator family of the stage the
// reference shells out to (`parallel-wavegan-decode`, inference_student.sh:20-23).  gfx950 only.  Built from the published architecture; no upstream
// source, checkpoint or vector exists here: parity unpinned.
// Rows are SAMPLES at the stage's rate (time-major, utterances concatenated), channels are the contiguous dimension, so every convolution is a K-term
// GEMM over taps on v_mfma_f32_16x16x32_bf16 with the library's bf16x3 split (a.b ~= al.bh + ah.bl + ah.bh; FCL_GEMM_BF16: ah.bh alone).
// P32 convention throughout: a producer writes the fp32 value where a residual needs it and the planes of LeakyReLU(value), the next consumer's
// operand; no consumer applies an activation to its operand.
//   hfg_conv_kernel / hfg_tconv_kernel   one Conv1d (any width, K walked in chunks of 128 channels) / one ConvTranspose1d stage, polyphase: output
//                                        row n = s q + p takes the ku / s taps of phase p from the input rows around q (blockIdx.y = p)
//   hfg_unit_kernel<C>                   one residual unit LeakyReLU -> dilated Conv1d -> LeakyReLU -> Conv1d -> + x in ONE launch for C <= 128: the
//                                        intermediate with its (kr - 1) / 2-row halo never leaves LDS
//   hfg_out_kernel                       output_conv (a few output channels) + tanh, row-wise
//   hfg_maps_kernel, hfg_*_cap_kernel    the capacity form: the two tables and the live record from the device's frame starts; the kernels above with the
//                                        grid sized by a capacity and the rows read from that record (same bodies: a live row is the exact kernel's)
// The operand tile of a workgroup (128 rows + halo) is staged in LDS ONCE and every tap reads it at its row offset; lines are stored [chunk][row] with
// the 16-byte piece p of row r at slot p ^ ((r >> 1) & 7) (gemm_planes.hip's permutation).  Weight fragments come straight from L2 into registers: every
// workgroup walks the same few hundred KB.  Zero padding at UTTERANCE edges: an A fragment whose source row lies outside the utterance of its output
// row is replaced by zeros (utterance of a row from frame_utt / utt_off at the rate of the operand).
#include <algorithm>

#include "fcl_common.h"

namespace fcl {

typedef unsigned char u8;

__device__ __forceinline__ float hfg_lrelu(float v, float s) { return v >= 0.f ? v : v * s; }

// row range [lo, hi) of the utterance that owns row g (rate rows per frame); a row outside [0, M) belongs to no utterance (empty range)
__device__ __forceinline__ void hfg_bounds(const int* __restrict__ frame_utt, const int* __restrict__ utt_off, int rate, int M, int g, int& lo, int& hi) {
    lo = hi = 0;
    if (g >= 0 && g < M) {
        const int u = frame_utt[g / rate];
        lo = utt_off[u] * rate;
        hi = utt_off[u + 1] * rate;
    }
}

// rows [r0, r0 + nrows) x lines [l0, l0 + nl) of row-major planes (ld lines per row, rows valid in [0, M)) -> LDS tile [nl][nrows] lines, zeros outside
__device__ __forceinline__ void hfg_load_tile(const u16* __restrict__ xp, int ld, int M, int r0, int nrows, int l0, int nl, u8* tile, int tid) {
    const int per_row = nl * 8;
    for (int i = tid; i < nrows * per_row; i += 256) {
        const int r = i / per_row, rem = i - r * per_row, c = rem >> 3, p = rem & 7;
        const int g = r0 + r;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (g >= 0 && g < M) v = *reinterpret_cast<const uint4*>(xp + ((size_t)g * ld + l0 + c) * 64 + p * 8);
        *reinterpret_cast<uint4*>(tile + (size_t)(c * nrows + r) * 128 + ((p ^ ((r >> 1) & 7)) << 4)) = v;
    }
}

// one tap of a wave's TM x TN tiles over nl 32-channel chunks: A rows arow[tm] of the LDS tile (fragments of rows whose bit in okmask is clear are
// zeros), B rows n, n + 16, .. of the weight planes at wl (this lane's row and k-quarter).  Row tiles at or beyond tm_end are skipped.
template <int TM, int TN, bool HI>
__device__ __forceinline__ void hfg_tap(const u8* tile, int nrows, int nl, const int (&arow)[TM], unsigned okmask, int tm_end, const u16* __restrict__ wl, int ldw,
                                        int kq, f32x4 (&acc)[TM][TN]) {
    const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < nl; ++c) {
        s16x8 bh[TN], bl[TN];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const u16* w = wl + ((size_t)tn * 16 * ldw + c) * 64;
            bh[tn] = *reinterpret_cast<const s16x8*>(w);
            if (!HI) bl[tn] = *reinterpret_cast<const s16x8*>(w + 32);
        }
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            if (tm >= tm_end) continue;
            const int row = arow[tm], sw = (row >> 1) & 7;
            const u8* p = tile + (size_t)(c * nrows + row) * 128;
            const bool ok = (okmask >> tm) & 1u;
            s16x8 ah = *reinterpret_cast<const s16x8*>(p + ((kq ^ sw) << 4));
            ah = ok ? ah : zero;
            if (!HI) {
                s16x8 al = *reinterpret_cast<const s16x8*>(p + (((4 + kq) ^ sw) << 4));
                al = ok ? al : zero;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[tn], acc[tm][tn], 0, 0, 0);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[tn], acc[tm][tn], 0, 0, 0);
            }
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[tn], acc[tm][tn], 0, 0, 0);
        }
    }
}

// what a finished row (4 consecutive columns) is written as
struct HfgEpi {
    const float* resid;  // optional [rows, C]: added to the value
    float* y;            // optional fp32 value
    u16* yp;             // optional planes of LeakyReLU(value, slope)
    float slope;
    float* cs;           // optional stage sum: cs = first ? value * cs_scale : cs + value * cs_scale
    float cs_scale;
    int first;
    u16* csp;            // optional planes of LeakyReLU(new cs, csp_slope)
    float csp_slope;
};

__device__ __forceinline__ void hfg_store4(const HfgEpi& e, long long n, int C, int col, f32x4 v) {
    const size_t o = (size_t)n * C + col;
    const size_t po = ((size_t)n * (C >> 5) + (col >> 5)) * 64 + (col & 31);
    if (e.resid) v += *reinterpret_cast<const f32x4*>(e.resid + o);
    if (e.y) *reinterpret_cast<f32x4*>(e.y + o) = v;
    if (e.yp) {
        f32x4 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = hfg_lrelu(v[i], e.slope);
        uint2 h, l;
        split4(a, h, l);
        *reinterpret_cast<uint2*>(e.yp + po) = h;
        *reinterpret_cast<uint2*>(e.yp + po + 32) = l;
    }
    if (e.cs) {
        f32x4 s = v * e.cs_scale;
        if (!e.first) s += *reinterpret_cast<const f32x4*>(e.cs + o);
        *reinterpret_cast<f32x4*>(e.cs + o) = s;
        if (e.csp) {
            f32x4 a;
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = hfg_lrelu(s[i], e.csp_slope);
            uint2 h, l;
            split4(a, h, l);
            *reinterpret_cast<uint2*>(e.csp + po) = h;
            *reinterpret_cast<uint2*>(e.csp + po + 32) = l;
        }
    }
}

// wave layout of a 128-row x (PWT x 16)-column pass over 4 waves
template <int PWT>
struct HfgGeo {
    static constexpr int WN = PWT >= 4 ? 4 : 2, WM = 4 / WN, TN = PWT / WN, TM = 8 / WM, PW = PWT * 16, LDT = PW + 4;
};

struct HfgConvArgs {
    const u16* xp;  // operand planes [m_in, ldx lines]
    int ldx, m_in, cout;
    const u16* wp;  // [taps][cout][ldw lines]
    int ldw;
    const float* bias;
    int ntaps, dilation;  // Conv1d: tap j reads row q + (j - (ntaps - 1) / 2) * dilation with weight j
    int stride, pad;      // ConvTranspose1d: phase p = blockIdx.y, t = p + pad: tap j reads row q + t / stride - j with weight stride * j + t % stride
    int hl, hr;           // halo rows below / above the tile
    const int *frame_utt, *utt_off;
    int rate;  // operand rows per frame
    HfgEpi e;
};

template <int PWT, bool HI, bool TC>
__device__ __forceinline__ void hfg_conv_body(const HfgConvArgs& a, u8* smem) {
    using G = HfgGeo<PWT>;
    constexpr int TM = G::TM, TN = G::TN, WN = G::WN, PW = G::PW, LDT = G::LDT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN, r16 = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * 128, ROWS = 128 + a.hl + a.hr;
    int shift0 = -((a.ntaps - 1) / 2) * a.dilation, shift_step = a.dilation, w0 = 0, w_step = 1, phase = 0;
    if (TC) {
        phase = blockIdx.y;
        const int t = phase + a.pad;
        shift0 = t / a.stride;
        shift_step = -1;
        w0 = t % a.stride;
        w_step = a.stride;
    }
    int lo[TM], hi[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) hfg_bounds(a.frame_utt, a.utt_off, a.rate, a.m_in, q0 + (wm * TM + tm) * 16 + r16, lo[tm], hi[tm]);
    float* zt = reinterpret_cast<float*>(smem);
    for (int n_pass = 0; n_pass < a.cout; n_pass += PW) {
        const int n0 = n_pass + wn * TN * 16;
        f32x4 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int l0 = 0; l0 < a.ldx; l0 += 4) {
            const int nl = min(4, a.ldx - l0);
            __syncthreads();
            hfg_load_tile(a.xp, a.ldx, a.m_in, q0 - a.hl, ROWS, l0, nl, smem, tid);
            __syncthreads();
            for (int j = 0; j < a.ntaps; ++j) {
                const int shift = shift0 + j * shift_step;
                int arow[TM];
                unsigned ok = 0u;
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    const int r = (wm * TM + tm) * 16 + r16, g = q0 + r + shift;
                    arow[tm] = a.hl + r + shift;
                    ok |= (g >= lo[tm] && g < hi[tm]) ? (1u << tm) : 0u;
                }
                const u16* wl = a.wp + ((size_t)(w0 + j * w_step) * a.cout + n0 + r16) * a.ldw * 64 + (size_t)l0 * 64 + kq * 8;
                hfg_tap<TM, TN, HI>(smem, ROWS, nl, arow, ok, TM, wl, a.ldw, kq, acc);
            }
        }
        __syncthreads();  // the operand tile is dead: stage the pass's values for row-contiguous stores
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int cn = (wn * TN + tn) * 16 + (lane & 15);
                const float b = a.bias[n_pass + cn];
#pragma unroll
                for (int r = 0; r < 4; ++r) zt[((wm * TM + tm) * 16 + (lane >> 4) * 4 + r) * LDT + cn] = acc[tm][tn][r] + b;
            }
        __syncthreads();
        for (int i = tid; i < 128 * (PW / 4); i += 256) {
            const int r = i / (PW / 4), c4 = (i - r * (PW / 4)) * 4;
            if (q0 + r >= a.m_in) continue;
            const long long n = TC ? (long long)(q0 + r) * a.stride + phase : (long long)(q0 + r);
            hfg_store4(a.e, n, a.cout, n_pass + c4, *reinterpret_cast<const f32x4*>(zt + r * LDT + c4));
        }
    }
}

template <int PWT, bool HI>
__global__ __launch_bounds__(256) void hfg_conv_kernel(const HfgConvArgs a) {
    extern __shared__ __attribute__((aligned(1024))) u8 hfg_smem[];
    hfg_conv_body<PWT, HI, false>(a, hfg_smem);
}

template <int PWT, bool HI>
__global__ __launch_bounds__(256) void hfg_tconv_kernel(const HfgConvArgs a) {
    extern __shared__ __attribute__((aligned(1024))) u8 hfg_smem[];
    hfg_conv_body<PWT, HI, true>(a, hfg_smem);
}

// ---- capacity forms (fcl_hip.h "capacity form of the HiFi-GAN generator"): grids and buffers are sized by a CAPACITY (a.m_in / a.m rows); the rows the
// body works on are live[0] frames x the operand's rows per frame, read with one scalar load per workgroup.  A workgroup whose tile starts at or beyond
// the live rows returns before it touches memory; the others run the exact body on the same tiles, so a live row is what the exact kernel writes.
__device__ __forceinline__ int hfg_live_rows(const int* live, int rate, int cap) { return (int)min((long long)uniform_word(live, 0) * rate, (long long)cap); }

template <int PWT, bool HI>
__global__ __launch_bounds__(256) void hfg_conv_cap_kernel(const HfgConvArgs a, const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(1024))) u8 hfg_smem[];
    HfgConvArgs b = a;
    b.m_in = hfg_live_rows(live, a.rate, a.m_in);
    if ((int)blockIdx.x * 128 >= b.m_in) return;
    hfg_conv_body<PWT, HI, false>(b, hfg_smem);
}

template <int PWT, bool HI>
__global__ __launch_bounds__(256) void hfg_tconv_cap_kernel(const HfgConvArgs a, const int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(1024))) u8 hfg_smem[];
    HfgConvArgs b = a;
    b.m_in = hfg_live_rows(live, a.rate, a.m_in);
    if ((int)blockIdx.x * 128 >= b.m_in) return;
    hfg_conv_body<PWT, HI, true>(b, hfg_smem);
}

// ---- one residual unit in one launch: 112 output rows per workgroup; rows t0 .. t0 + 127 (t0 = m0 - h2) of the intermediate are computed from rows
// t0 - h1 .. t0 + 127 + h1 of the operand (h2 = (kr - 1) / 2, h1 = h2 * dilation) and stay in LDS as the second convolution's pre-split operand.
struct HfgUnitArgs {
    const u16* xp;   // planes of LeakyReLU(x) [m, C]
    const float* x;  // fp32 x (the residual)
    int m, kr, dil;
    const u16 *w1p, *w2p;  // [kr][C][C / 32 lines]
    const float *b1, *b2;
    const int *frame_utt, *utt_off;
    int rate;
    float slope;
    HfgEpi e;  // resid = x
};

template <int C, bool HI>
__global__ __launch_bounds__(256) void hfg_unit_kernel(const HfgUnitArgs a) {
#include "hfg_unit_body.inc"
}

template <int C, bool HI>
__global__ __launch_bounds__(256) void hfg_unit_cap_kernel(const HfgUnitArgs a_cap, const int* __restrict__ live) {
    HfgUnitArgs a = a_cap;
    a.m = hfg_live_rows(live, a_cap.rate, a_cap.m);
    if ((int)blockIdx.x * 112 >= a.m) return;
#include "hfg_unit_body.inc"
}

// output_conv + tanh: wav[m, o] = tanh(b[o] + sum_j sum_ch a[m + j - (k-1)/2, ch] w[j][o][ch]), a = the operand planes (hi + lo; hi alone and bf16-rounded
// weights in FCL_GEMM_BF16).  8 lanes per row, lane = one 16-byte piece of each line: the hi piece p and the lo piece 4 + p meet the same 8 weights.
__device__ __forceinline__ void hfg_out_body(const u16* __restrict__ cp, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                             const int* __restrict__ frame_utt, const int* __restrict__ utt_off, int rate, float* __restrict__ wav, int M, int C,
                                             int cout, int k, int hi_only) {
    const int sub = threadIdx.x & 7, hk = (k - 1) / 2;
    const long long g0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 3, gs = ((long long)gridDim.x * blockDim.x) >> 3;
    for (long long m = g0; m < M; m += gs) {
        int lo, hi;
        hfg_bounds(frame_utt, utt_off, rate, M, (int)m, lo, hi);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (!(hi_only && sub >= 4)) {
            for (int j = 0; j < k; ++j) {
                const long long q = m + j - hk;
                if (q < lo || q >= hi) continue;
                for (int c = 0; c < ld; ++c) {
                    const uint4 v = *reinterpret_cast<const uint4*>(cp + ((size_t)q * ld + c) * 64 + sub * 8);
                    const unsigned wd[4] = {v.x, v.y, v.z, v.w};
                    float f[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        f[2 * e] = __builtin_bit_cast(float, wd[e] << 16);
                        f[2 * e + 1] = __builtin_bit_cast(float, wd[e] & 0xFFFF0000u);
                    }
                    const int ch0 = c * 32 + (sub & 3) * 8;
                    for (int o = 0; o < cout; ++o) {
                        const float* wr = w + ((size_t)j * cout + o) * C + ch0;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float wv = hi_only ? (float)(__bf16)wr[e] : wr[e];
                            acc[o] = fmaf(f[e], wv, acc[o]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            acc[o] += __shfl_xor(acc[o], 1);
            acc[o] += __shfl_xor(acc[o], 2);
            acc[o] += __shfl_xor(acc[o], 4);
        }
        if (sub == 0)
            for (int o = 0; o < cout; ++o) wav[m * cout + o] = tanhf(acc[o] + b[o]);
    }
}

__global__ __launch_bounds__(256) void hfg_out_kernel(const u16* __restrict__ cp, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                                      const int* __restrict__ frame_utt, const int* __restrict__ utt_off, int rate, float* __restrict__ wav,
                                                      int M, int C, int cout, int k, int hi_only) {
    hfg_out_body(cp, ld, w, b, frame_utt, utt_off, rate, wav, M, C, cout, k, hi_only);
}

// (M is the capacity; a workgroup covers 32 consecutive rows on its first trip and only rows beyond them later)
__global__ __launch_bounds__(256) void hfg_out_cap_kernel(const u16* __restrict__ cp, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                                          const int* __restrict__ frame_utt, const int* __restrict__ utt_off, int rate, float* __restrict__ wav,
                                                          int M, int C, int cout, int k, int hi_only, const int* __restrict__ live) {
    const int m_live = hfg_live_rows(live, rate, M);
    if ((long long)blockIdx.x * (blockDim.x >> 3) >= m_live) return;
    hfg_out_body(cp, ld, w, b, frame_utt, utt_off, rate, wav, m_live, C, cout, k, hi_only);
}

// ---- the two tables of a batch from the synthesis pass's frame starts, to capacity, in one launch (fcl_hfg_maps_build).  Every workgroup rebuilds the
// frame starts (B + 1 words) in LDS and fills its share of frame_utt; frames [live, frames_cap) form one pseudo-utterance (index B) that owns the rest
// of every buffer: dead rows only ever see dead rows, and every index lies inside its buffer.
constexpr int HFG_MAPS_MAX_UTT = 1024;

// largest u in [0, n) with a[u] <= v (a non-decreasing, a[0] <= v): with equal neighbours (slots without frames) the LAST one, the slot that owns v
__device__ __forceinline__ int hfg_owner(const int* a, int n, int v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void hfg_maps_kernel(const int* __restrict__ utt_frame0, unsigned int* status, int B, int frames_cap, int hop,
                                                       int* __restrict__ frame_utt, int* __restrict__ utt_off, int* __restrict__ live) {
    __shared__ int off[HFG_MAPS_MAX_UTT + 1];
    __shared__ int s_ok, s_flag;
    const int tid = threadIdx.x;
    for (int i = tid; i <= B; i += blockDim.x) off[i] = utt_frame0[i];
    __syncthreads();
    if (tid == 0) {
        // `fits` depends on utt_frame0 alone (read-only here).  Workgroup 0 ORs FCL_STATUS_VOCODER_CAP into *status at the end of the kernel only when the
        // word was zero and `fits` is false, and then every workgroup refuses on `fits` whatever it reads from *status; when `fits` holds nobody writes
        // the word.  So all workgroups agree without an order between this read and that write.
        bool fits = off[0] == 0 && off[B] <= frames_cap;
        for (int u = 0; u < B; ++u) fits = fits && off[u + 1] >= off[u];
        const bool zero = *status == 0u;
        s_flag = !fits && zero ? 1 : 0;  // an incoming status stays as it is
        s_ok = fits && zero ? 1 : 0;
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    if (!ok)
        for (int i = tid; i <= B; i += blockDim.x) off[i] = 0;  // nothing is live: the whole capacity is the dead pseudo-utterance
    __syncthreads();
    const int nlive = off[B];
    for (long long f = blockIdx.x * (long long)blockDim.x + tid; f < frames_cap; f += (long long)gridDim.x * blockDim.x)
        frame_utt[f] = f < nlive ? hfg_owner(off, B, (int)f) : B;
    if (blockIdx.x == 0) {
        for (int i = tid; i < B; i += blockDim.x) utt_off[i] = off[i];
        if (tid == 0) {
            utt_off[B] = nlive;
            utt_off[B + 1] = frames_cap;
            int nz = 0;
            for (int u = 0; u < B; ++u) nz += off[u + 1] > off[u];
            live[0] = nlive;
            live[1] = nlive * hop;
            live[2] = 0;
            live[3] = nz;
            if (s_flag) atomicOr(status, (unsigned int)FCL_STATUS_VOCODER_CAP);
        }
    }
}

static bool hfg_planes_on() { return tunable("PRECISION", 1) != 0 && tunable("PLANES", 1) != 0; }
static bool hfg_line_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 127u) == 0; }

// live != nullptr: the capacity form (a.m_in / a.m is the capacity: grid and buffer extent)
template <int PWT, bool TC>
static int hfg_launch_conv_cfg(const HfgConvArgs& a, int phases, const char* name, double flops, hipStream_t s, const int* live) {
    const bool hi = gemm_mode() == FCL_GEMM_BF16;
    const int lds = std::max((128 + a.hl + a.hr) * std::min(a.ldx, 4) * 128, 128 * HfgGeo<PWT>::LDT * 4);
    const void* k;
    if (live)
        k = TC ? (hi ? reinterpret_cast<const void*>(hfg_tconv_cap_kernel<PWT, true>) : reinterpret_cast<const void*>(hfg_tconv_cap_kernel<PWT, false>))
               : (hi ? reinterpret_cast<const void*>(hfg_conv_cap_kernel<PWT, true>) : reinterpret_cast<const void*>(hfg_conv_cap_kernel<PWT, false>));
    else
        k = TC ? (hi ? reinterpret_cast<const void*>(hfg_tconv_kernel<PWT, true>) : reinterpret_cast<const void*>(hfg_tconv_kernel<PWT, false>))
               : (hi ? reinterpret_cast<const void*>(hfg_conv_kernel<PWT, true>) : reinterpret_cast<const void*>(hfg_conv_kernel<PWT, false>));
    const int rc = ensure_dyn_lds(k, lds);
    if (rc) return rc;
    char full[48];
    snprintf(full, sizeof(full), "%s%s", name, hi ? "/bf16" : "");
    ProfScope ps(full, flops, (double)a.m_in * phases, s);
    const dim3 grid((unsigned)((a.m_in + 127) / 128), (unsigned)phases);
    if (live) {
        if (TC) {
            if (hi) hipLaunchKernelGGL((hfg_tconv_cap_kernel<PWT, true>), grid, dim3(256), lds, s, a, live);
            else hipLaunchKernelGGL((hfg_tconv_cap_kernel<PWT, false>), grid, dim3(256), lds, s, a, live);
        } else {
            if (hi) hipLaunchKernelGGL((hfg_conv_cap_kernel<PWT, true>), grid, dim3(256), lds, s, a, live);
            else hipLaunchKernelGGL((hfg_conv_cap_kernel<PWT, false>), grid, dim3(256), lds, s, a, live);
        }
    } else if (TC) {
        if (hi) hipLaunchKernelGGL((hfg_tconv_kernel<PWT, true>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((hfg_tconv_kernel<PWT, false>), grid, dim3(256), lds, s, a);
    } else {
        if (hi) hipLaunchKernelGGL((hfg_conv_kernel<PWT, true>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((hfg_conv_kernel<PWT, false>), grid, dim3(256), lds, s, a);
    }
    return check_hip(hipGetLastError(), name);
}

template <bool TC>
static int hfg_launch_conv(const HfgConvArgs& a, int phases, double flops, hipStream_t s, const int* live) {
    const char* name = TC ? (live ? "hfg_tconv_cap_kernel" : "hfg_tconv_kernel") : (live ? "hfg_conv_cap_kernel" : "hfg_conv_kernel");
    if (a.cout % 128 == 0) return hfg_launch_conv_cfg<8, TC>(a, phases, name, flops, s, live);
    if (a.cout % 64 == 0) return hfg_launch_conv_cfg<4, TC>(a, phases, name, flops, s, live);
    return hfg_launch_conv_cfg<2, TC>(a, phases, name, flops, s, live);
}

template <int C>
static int hfg_launch_unit(const HfgUnitArgs& a, double flops, hipStream_t s, const int* live) {
    const bool hi = gemm_mode() == FCL_GEMM_BF16;
    const int h1 = (a.kr - 1) / 2 * a.dil;
    const int lds = (128 + 2 * h1) * (C / 32) * 128 + 128 * (C / 32) * 128;
    const void* k = live ? (hi ? reinterpret_cast<const void*>(hfg_unit_cap_kernel<C, true>) : reinterpret_cast<const void*>(hfg_unit_cap_kernel<C, false>))
                         : (hi ? reinterpret_cast<const void*>(hfg_unit_kernel<C, true>) : reinterpret_cast<const void*>(hfg_unit_kernel<C, false>));
    const int rc = ensure_dyn_lds(k, lds);
    if (rc) return rc;
    char full[48];
    snprintf(full, sizeof(full), "hfg_unit%s_kernel<%d>%s", live ? "_cap" : "", C, hi ? "/bf16" : "");
    ProfScope ps(full, flops, (double)a.m, s);
    const dim3 grid((unsigned)((a.m + 111) / 112));
    if (live) {
        if (hi) hipLaunchKernelGGL((hfg_unit_cap_kernel<C, true>), grid, dim3(256), lds, s, a, live);
        else hipLaunchKernelGGL((hfg_unit_cap_kernel<C, false>), grid, dim3(256), lds, s, a, live);
    } else {
        if (hi) hipLaunchKernelGGL((hfg_unit_kernel<C, true>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((hfg_unit_kernel<C, false>), grid, dim3(256), lds, s, a);
    }
    return check_hip(hipGetLastError(), live ? "hfg_unit_cap_fwd" : "hfg_unit_fwd");
}

// The four entries in both forms: `who` names the entry in its messages; cap: `live` is required and m / m_in is the capacity.
static int hfg_conv_entry(const fcl_hfg_conv_t* a, bool cap, const int32_t* live, fcl_stream_t stream) {
    const char* who = cap ? "hfg_conv_cap_fwd" : "hfg_conv_fwd";
    FCL_REQUIRE(a && a->xp && a->wp && a->bias && a->frame_utt && a->utt_off && (a->y || a->yp) && a->m > 0 && a->rate >= 1 && (!cap || live), FCL_ERR_INVALID,
                "%s: null argument", who);
    FCL_REQUIRE(hfg_planes_on(), FCL_ERR_INVALID, "%s: the HiFi-GAN kernels run on pre-split operands only (FCL_PRECISION=0 / FCL_PLANES=0 is set)", who);
    FCL_REQUIRE(a->cin > 0 && a->cout > 0 && a->cout % 32 == 0 && a->m <= 0x7fffffffLL / 2, FCL_ERR_SHAPE,
                "%s: output channels must be a multiple of 32 (got %d) and rows stay below 2^30", who, a->cout);
    FCL_REQUIRE(a->ksize >= 1 && (a->ksize & 1) && a->ksize <= 11 && a->dilation >= 1 && a->dilation <= 5, FCL_ERR_SHAPE,
                "%s: odd kernel size <= 11 and dilation 1..5 expected (got %d, %d)", who, a->ksize, a->dilation);
    FCL_REQUIRE(hfg_line_aligned(a->xp) && hfg_line_aligned(a->wp) && hfg_line_aligned(a->yp) && aligned16(a->y) && aligned16(a->resid), FCL_ERR_ALIGN,
                "%s: planes must be 128-byte, y / resid 16-byte aligned", who);
    HfgConvArgs g = {};
    g.xp = a->xp; g.ldx = (a->cin + 31) / 32; g.m_in = (int)a->m; g.cout = a->cout;
    g.wp = a->wp; g.ldw = g.ldx; g.bias = a->bias;
    g.ntaps = a->ksize; g.dilation = a->dilation; g.stride = 1;
    g.hl = g.hr = (a->ksize - 1) / 2 * a->dilation;
    g.frame_utt = a->frame_utt; g.utt_off = a->utt_off; g.rate = a->rate;
    g.e.resid = a->resid; g.e.y = a->y; g.e.yp = a->yp; g.e.slope = a->slope;
    return hfg_launch_conv<false>(g, 1, 2.0 * a->m * a->cin * a->cout * a->ksize, (hipStream_t)stream, cap ? live : nullptr);
}

static int hfg_tconv_entry(const fcl_hfg_tconv_t* a, bool cap, const int32_t* live, fcl_stream_t stream) {
    const char* who = cap ? "hfg_tconv_cap_fwd" : "hfg_tconv_fwd";
    FCL_REQUIRE(a && a->xp && a->wp && a->bias && a->frame_utt && a->utt_off && (a->y || a->yp) && a->m_in > 0 && a->rate_in >= 1 && a->stride >= 1 && (!cap || live),
                FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(hfg_planes_on(), FCL_ERR_INVALID, "%s: the HiFi-GAN kernels run on pre-split operands only (FCL_PRECISION=0 / FCL_PLANES=0 is set)", who);
    FCL_REQUIRE(a->ksize >= a->stride && a->ksize % a->stride == 0 && a->ksize / a->stride <= 8, FCL_ERR_SHAPE,
                "%s: the polyphase form needs a kernel size that is a multiple of the stride (got %d, stride %d)", who, a->ksize, a->stride);
    FCL_REQUIRE(a->padding >= 0 && a->ksize - 2 * a->padding == a->stride - a->stride % 2, FCL_ERR_SHAPE,
                "%s: padding %d does not give stride x input rows (kernel %d, stride %d, output_padding stride %% 2)", who, a->padding, a->ksize, a->stride);
    FCL_REQUIRE(a->cin > 0 && a->cin % 32 == 0 && a->cout > 0 && a->cout % 32 == 0, FCL_ERR_SHAPE, "%s: channels must be multiples of 32 (got %d -> %d)", who,
                a->cin, a->cout);
    FCL_REQUIRE(a->m_in * (int64_t)a->stride <= 0x7fffffffLL / 2, FCL_ERR_SHAPE, "%s: more than 2^30 output rows", who);
    FCL_REQUIRE(hfg_line_aligned(a->xp) && hfg_line_aligned(a->wp) && hfg_line_aligned(a->yp) && aligned16(a->y), FCL_ERR_ALIGN,
                "%s: planes must be 128-byte, y 16-byte aligned", who);
    HfgConvArgs g = {};
    g.xp = a->xp; g.ldx = a->cin / 32; g.m_in = (int)a->m_in; g.cout = a->cout;
    g.wp = a->wp; g.ldw = g.ldx; g.bias = a->bias;
    g.ntaps = a->ksize / a->stride; g.dilation = 1; g.stride = a->stride; g.pad = a->padding;
    g.hl = g.ntaps - 1;                                     // lowest shift: 0 - (taps - 1)
    g.hr = (a->stride - 1 + a->padding) / a->stride;        // highest shift: t / stride at the last phase
    g.frame_utt = a->frame_utt; g.utt_off = a->utt_off; g.rate = a->rate_in;
    g.e.y = a->y; g.e.yp = a->yp; g.e.slope = a->slope;
    return hfg_launch_conv<true>(g, a->stride, 2.0 * a->m_in * a->cin * a->cout * a->ksize, (hipStream_t)stream, cap ? live : nullptr);
}

static int hfg_unit_entry(const fcl_hfg_unit_t* a, bool cap, const int32_t* live_in, fcl_stream_t stream) {
    const char* who = cap ? "hfg_unit_cap_fwd" : "hfg_unit_fwd";
    FCL_REQUIRE(a && a->xp && a->x && a->w1p && a->b1 && a->w2p && a->b2 && a->frame_utt && a->utt_off && a->m > 0 && a->rate >= 1 && (!cap || live_in),
                FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->x_out || a->xp_out || (a->last && a->cs), FCL_ERR_INVALID, "%s: nothing to write (x_out / xp_out / cs)", who);
    FCL_REQUIRE(!a->last || a->cs, FCL_ERR_INVALID, "%s: the last unit of a block needs the stage sum cs", who);
    FCL_REQUIRE(hfg_planes_on(), FCL_ERR_INVALID, "%s: the HiFi-GAN kernels run on pre-split operands only (FCL_PRECISION=0 / FCL_PLANES=0 is set)", who);
    FCL_REQUIRE(a->c > 0 && a->c % 32 == 0, FCL_ERR_SHAPE, "%s: channels must be a multiple of 32 (got %d)", who, a->c);
    FCL_REQUIRE((a->ksize == 3 || a->ksize == 5 || a->ksize == 7 || a->ksize == 11) && a->dilation >= 1 && a->dilation <= 5, FCL_ERR_SHAPE,
                "%s: kernel size 3 / 5 / 7 / 11 and dilation 1..5 expected (got %d, %d)", who, a->ksize, a->dilation);
    FCL_REQUIRE(a->m <= 0x7fffffffLL / 2, FCL_ERR_SHAPE, "%s: more than 2^30 rows in one call", who);
    FCL_REQUIRE(a->xp_out != a->xp, FCL_ERR_INVALID, "%s: xp_out must not be xp (neighbouring tiles still read xp for their taps)", who);
    FCL_REQUIRE(hfg_line_aligned(a->xp) && hfg_line_aligned(a->xp_out) && hfg_line_aligned(a->csp) && hfg_line_aligned(a->w1p) && hfg_line_aligned(a->w2p) &&
                    hfg_line_aligned(a->tp) && aligned16(a->x) && aligned16(a->x_out) && aligned16(a->cs),
                FCL_ERR_ALIGN, "%s: planes must be 128-byte, x / x_out / cs 16-byte aligned", who);
    const int* live = cap ? live_in : nullptr;
    HfgEpi e = {};
    e.resid = a->x; e.y = a->x_out; e.yp = a->xp_out; e.slope = a->slope;
    if (a->last) {
        e.cs = a->cs; e.cs_scale = a->cs_scale; e.first = a->first; e.csp = a->csp; e.csp_slope = a->csp_slope;
    }
    const double flops = 2.0 * a->m * a->c * a->c * a->ksize;
    hipStream_t s = (hipStream_t)stream;
    if (a->c == 32 || a->c == 64 || a->c == 128) {
        HfgUnitArgs u = {};
        u.xp = a->xp; u.x = a->x; u.m = (int)a->m; u.kr = a->ksize; u.dil = a->dilation;
        u.w1p = a->w1p; u.w2p = a->w2p; u.b1 = a->b1; u.b2 = a->b2;
        u.frame_utt = a->frame_utt; u.utt_off = a->utt_off; u.rate = a->rate; u.slope = a->slope; u.e = e;
        return a->c == 32 ? hfg_launch_unit<32>(u, 2 * flops, s, live) : a->c == 64 ? hfg_launch_unit<64>(u, 2 * flops, s, live) : hfg_launch_unit<128>(u, 2 * flops, s, live);
    }
    // wider stages: one launch per convolution, the intermediate's planes through the workspace tp
    FCL_REQUIRE(a->tp, FCL_ERR_WORKSPACE, "%s: %d channels run as one launch per convolution and need the workspace tp", who, a->c);
    HfgConvArgs g = {};
    g.xp = a->xp; g.ldx = a->c / 32; g.m_in = (int)a->m; g.cout = a->c;
    g.wp = a->w1p; g.ldw = g.ldx; g.bias = a->b1;
    g.ntaps = a->ksize; g.dilation = a->dilation; g.stride = 1;
    g.hl = g.hr = (a->ksize - 1) / 2 * a->dilation;
    g.frame_utt = a->frame_utt; g.utt_off = a->utt_off; g.rate = a->rate;
    g.e.yp = a->tp; g.e.slope = a->slope;
    int rc = hfg_launch_conv<false>(g, 1, flops, s, live);
    if (rc) return rc;
    g.xp = a->tp; g.wp = a->w2p; g.bias = a->b2; g.dilation = 1;
    g.hl = g.hr = (a->ksize - 1) / 2;
    g.e = e;
    return hfg_launch_conv<false>(g, 1, flops, s, live);
}

static int hfg_out_entry(const uint16_t* cp, const float* w, const float* b, const int32_t* frame_utt, const int32_t* utt_off, int rate, float* wav, int64_t m, int c,
                         int cout, int ksize, bool cap, const int32_t* live, fcl_stream_t stream) {
    const char* who = cap ? "hfg_out_cap_fwd" : "hfg_out_fwd";
    FCL_REQUIRE(cp && w && b && frame_utt && utt_off && wav && m > 0 && rate >= 1 && (!cap || live), FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(hfg_planes_on(), FCL_ERR_INVALID, "%s: the HiFi-GAN kernels run on pre-split operands only (FCL_PRECISION=0 / FCL_PLANES=0 is set)", who);
    FCL_REQUIRE(c > 0 && c % 32 == 0 && cout >= 1 && cout <= 4 && ksize >= 1 && (ksize & 1) && m <= 0x7fffffffLL / 2, FCL_ERR_SHAPE,
                "%s: channels must be a multiple of 32 (got %d), 1..4 output channels and an odd kernel size expected", who, c);
    FCL_REQUIRE(hfg_line_aligned(cp) && aligned16(w), FCL_ERR_ALIGN, "%s: cp must be 128-byte, w 16-byte aligned", who);
    const int hi = gemm_mode() == FCL_GEMM_BF16;
    const long long blocks = (m * 8 + 255) / 256;
    const dim3 grid((unsigned)std::min<long long>(std::max<long long>(blocks, 1), 1 << 20));
    if (cap) {
        ProfScope ps(hi ? "hfg_out_cap_kernel/bf16" : "hfg_out_cap_kernel", 2.0 * m * c * cout * ksize, (double)m, (hipStream_t)stream);
        hipLaunchKernelGGL(hfg_out_cap_kernel, grid, dim3(256), 0, (hipStream_t)stream, cp, c / 32, w, b, frame_utt, utt_off, rate, wav, (int)m, c, cout, ksize, hi,
                           live);
        return check_hip(hipGetLastError(), who);
    }
    ProfScope ps(hi ? "hfg_out_kernel/bf16" : "hfg_out_kernel", 2.0 * m * c * cout * ksize, (double)m, (hipStream_t)stream);
    hipLaunchKernelGGL(hfg_out_kernel, grid, dim3(256), 0, (hipStream_t)stream, cp, c / 32, w, b, frame_utt, utt_off, rate, wav, (int)m, c, cout, ksize, hi);
    return check_hip(hipGetLastError(), who);
}

}  // namespace fcl

using namespace fcl;

extern "C" {

int fcl_hfg_conv_fwd(const fcl_hfg_conv_t* a, fcl_stream_t stream) { return hfg_conv_entry(a, false, nullptr, stream); }
int fcl_hfg_tconv_fwd(const fcl_hfg_tconv_t* a, fcl_stream_t stream) { return hfg_tconv_entry(a, false, nullptr, stream); }
int fcl_hfg_unit_fwd(const fcl_hfg_unit_t* a, fcl_stream_t stream) { return hfg_unit_entry(a, false, nullptr, stream); }
int fcl_hfg_out_fwd(const uint16_t* cp, const float* w, const float* b, const int32_t* frame_utt, const int32_t* utt_off, int rate, float* wav, int64_t m, int c,
                    int cout, int ksize, fcl_stream_t stream) {
    return hfg_out_entry(cp, w, b, frame_utt, utt_off, rate, wav, m, c, cout, ksize, false, nullptr, stream);
}

int fcl_hfg_maps_build(const int32_t* utt_frame0, uint32_t* status, int batch, int64_t frames_cap, int hop, int32_t* frame_utt, int32_t* utt_off, int32_t* live,
                       fcl_stream_t stream) {
    FCL_REQUIRE(utt_frame0 && status && frame_utt && utt_off && live, FCL_ERR_INVALID, "hfg_maps_build: null argument");
    FCL_REQUIRE(batch >= 1 && batch <= HFG_MAPS_MAX_UTT && frames_cap >= 1 && hop >= 1, FCL_ERR_INVALID,
                "hfg_maps_build: 1 <= batch <= %d, frames_cap >= 1 and hop >= 1 expected", HFG_MAPS_MAX_UTT);
    FCL_REQUIRE(frames_cap * (int64_t)hop < 0x7fffffffLL, FCL_ERR_SHAPE, "hfg_maps_build: frames_cap * hop must stay below 2^31 samples");
    ProfScope ps("hfg_maps_kernel", 0.0, (double)frames_cap, (hipStream_t)stream);
    const unsigned grid = (unsigned)std::min<int64_t>((frames_cap + 255) / 256, 2048);
    hipLaunchKernelGGL(hfg_maps_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, utt_frame0, status, batch, (int)frames_cap, hop, frame_utt, utt_off, live);
    return check_hip(hipGetLastError(), "hfg_maps_build");
}

int fcl_hfg_conv_cap_fwd(const fcl_hfg_conv_t* a, const int32_t* live, fcl_stream_t stream) { return hfg_conv_entry(a, true, live, stream); }
int fcl_hfg_tconv_cap_fwd(const fcl_hfg_tconv_t* a, const int32_t* live, fcl_stream_t stream) { return hfg_tconv_entry(a, true, live, stream); }
int fcl_hfg_unit_cap_fwd(const fcl_hfg_unit_t* a, const int32_t* live, fcl_stream_t stream) { return hfg_unit_entry(a, true, live, stream); }
int fcl_hfg_out_cap_fwd(const uint16_t* cp, const float* w, const float* b, const int32_t* frame_utt, const int32_t* utt_off, int rate, float* wav, int64_t m, int c,
                        int cout, int ksize, const int32_t* live, fcl_stream_t stream) {
    return hfg_out_entry(cp, w, b, frame_utt, utt_off, rate, wav, m, c, cout, ksize, true, live, stream);
}

}  // extern "C"
