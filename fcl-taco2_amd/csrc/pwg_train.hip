// pwg_train.hip -- the Parallel WaveGAN generator's residual block in its training form: forward with the gate activations kept, and backward (input,
// conditioning and weight gradients) (include/fcl_hip.h "Parallel WaveGAN generator, training form"; fcl_taco2_amd/pwg_generator.py; restated
// in float64 numpy in tests/pwgt_ref.py).  The inference form is pwg.hip; nothing is shared with it.
//
// Layout and contractions are pwg_rows.h's (shared with pwg_disc.hip): float32, channel-last, packed [samples, C]; every contraction is one shape -- rows x
// (a few shifted or plain row sources) x a tap-major weight matrix -- in exact fp32 (pwr_contract; the weight gradients are pwr_dw_kernel).  This file holds
// the gate, the epilogues and the entries.
#include "pwg_rows.h"

namespace fcl {

constexpr float PWT_SQRT_HALF = 0.70710678118654752440f;

// The gate with accurate functions: tanhf, and the sigmoid with a true division.  The inference path's clamped pwg_gate and lstm_epilogue.h's rcpf forms
// are not used: the backward pass takes 1 - a^2 and b (1 - b), differences near saturation, where an absolute error of a few ulp of 1 in a or b is a
// large relative error of the derivative.
__device__ __forceinline__ float pwt_tanh(float z) { return tanhf(z); }
__device__ __forceinline__ float pwt_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// The epilogues below visit the wave's results in the C / D layout: column = lane & 15, row = 4 (lane >> 4) + register.
#define PWT_FOR_RESULTS(NTILES)                                         \
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;    \
    _Pragma("unroll") for (int nt = 0; nt < (NTILES); ++nt)             \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                    \
    _Pragma("unroll") for (int reg = 0; reg < 4; ++reg)

// ---- gate forward: z = b_gate + (x taps | c) w_gate, K = k R + A, N = 2 R.  The wave holds both halves of every column pair (tiles nt and nt + NT / 2), so
// a and b of a channel meet in one lane.  ab = (tanh | sigmoid); z_out (tests only) = z.
template <int NT>
__global__ __launch_bounds__(256) void pwt_gate_kernel(PwrA A, const float* __restrict__ w, const float* __restrict__ bias, const int32_t* __restrict__ seg_lo,
                                                       const int32_t* __restrict__ seg_hi, float* __restrict__ ab, float* __restrict__ z_out, long long n) {
    constexpr int NH = NT / 2, R = NH * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NH) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float za = acc[mt][nt][reg] + bias[col], zb = acc[mt][nt + NH][reg] + bias[R + col];
        if (z_out) {
            z_out[row * (2 * R) + col] = za;
            z_out[row * (2 * R) + R + col] = zb;
        }
        ab[row * (2 * R) + col] = pwt_tanh(za);
        ab[row * (2 * R) + R + col] = pwt_sigmoid(zb);
    }
}

// ---- out forward: (o | s) = g w_out + b_out with g = a * b formed on load, K = R, N = 2 R; x_out = (o + x) sqrt(.5), skips = s or skips + s
template <int NT>
__global__ __launch_bounds__(256) void pwt_out_kernel(PwrA A, const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ x,
                                                      const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, float* __restrict__ x_out,
                                                      float* __restrict__ skips, long long n, int first) {
    constexpr int NH = NT / 2, R = NH * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_GATED, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NH) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float o = acc[mt][nt][reg] + bias[col], sk = acc[mt][nt + NH][reg] + bias[R + col];
        x_out[row * R + col] = (o + x[row * R + col]) * PWT_SQRT_HALF;
        skips[row * R + col] = first ? sk : skips[row * R + col] + sk;
    }
}

// ---- out backward: dg = (sqrt(.5) dxo | ds) w_dz, K = 2 R (R without dxo), N = R; dz = (dg b (1 - a^2) | dg a b (1 - b)) from the stored ab
template <int NT>
__global__ __launch_bounds__(256) void pwt_dz_kernel(PwrA A, const float* __restrict__ w, const float* __restrict__ ab, const int32_t* __restrict__ seg_lo,
                                                     const int32_t* __restrict__ seg_hi, float* __restrict__ dz, long long n) {
    constexpr int R = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NT) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float a = ab[row * (2 * R) + col], b = ab[row * (2 * R) + R + col], dg = acc[mt][nt][reg];
        dz[row * (2 * R) + col] = dg * b * (1.f - a * a);
        dz[row * (2 * R) + R + col] = dg * a * b * (1.f - b);
    }
}

// ---- conv backward: dx = dz taps w_dx (taps reversed in the weights) + sqrt(.5) dxo, K = 2 k R, N = R
template <int NT>
__global__ __launch_bounds__(256) void pwt_dx_kernel(PwrA A, const float* __restrict__ w, const float* __restrict__ dxo, const int32_t* __restrict__ seg_lo,
                                                     const int32_t* __restrict__ seg_hi, float* __restrict__ dx, long long n) {
    constexpr int R = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NT) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        float v = acc[mt][nt][reg];
        if (dxo) v += dxo[row * R + col] * PWT_SQRT_HALF;
        dx[row * R + col] = v;
    }
}

// ---- aux backward: dc = dz w_dc or dc + that, K = 2 R, N = A
template <int NT>
__global__ __launch_bounds__(256) void pwt_dc_kernel(PwrA A, const float* __restrict__ w, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                     float* __restrict__ dc, long long n, int write) {
    constexpr int AUX = NT * 16;
    const long long t0 = (long long)blockIdx.x * PWR_ROWS + (threadIdx.x >> 6) * 32;
    f32x4 acc[2][NT];
    pwr_contract<PWR_PLAIN, NT>(A, w, seg_lo, seg_hi, n, t0, acc);
    PWT_FOR_RESULTS(NT) {
        const long long row = t0 + mt * 16 + 4 * q + reg;
        if (row >= n) continue;
        const int col = nt * 16 + r;
        const float v = acc[mt][nt][reg];
        dc[row * AUX + col] = write ? v : dc[row * AUX + col] + v;
    }
}

static dim3 pwt_grid(long long n) { return dim3((unsigned)((n + PWR_ROWS - 1) / PWR_ROWS)); }

// what every entry checks: the struct, the widths, the kernel size, the dilation, the sample count, the tables
static int pwt_check(const fcl_pwt_t* a, const char* who) {
    FCL_REQUIRE(a, FCL_ERR_INVALID, "%s: null argument", who);
    FCL_REQUIRE(a->residual >= 16 && a->residual <= 64 && a->residual % 16 == 0, FCL_ERR_SHAPE,
                "%s: residual (= skip) channels must be a multiple of 16 from 16 to 64 (got %d)", who, a->residual);
    FCL_REQUIRE(a->aux >= 16 && a->aux <= 128 && a->aux % 16 == 0, FCL_ERR_SHAPE, "%s: aux channels must be a multiple of 16 from 16 to 128 (got %d)", who,
                a->aux);
    FCL_REQUIRE(a->ksize == 3 || a->ksize == 5, FCL_ERR_SHAPE, "%s: kernel size must be 3 or 5 (got %d)", who, a->ksize);
    FCL_REQUIRE(a->dilation >= 1, FCL_ERR_SHAPE, "%s: dilation must be positive (got %d)", who, a->dilation);
    FCL_REQUIRE(a->samples >= 1 && a->samples < 0x7fffffffLL, FCL_ERR_SHAPE, "%s: 1 <= samples < 2^31 expected (got %lld)", who, (long long)a->samples);
    FCL_REQUIRE(a->seg_lo && a->seg_hi, FCL_ERR_INVALID, "%s: null seg_lo / seg_hi", who);
    return FCL_OK;
}

#define PWT_EVEN_TILES(CALL) \
    switch (R / 16) {        \
        case 1: CALL(2); break; \
        case 2: CALL(4); break; \
        case 3: CALL(6); break; \
        case 4: CALL(8); break; \
    }
#define PWT_R_TILES(CALL)    \
    switch (R / 16) {        \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
    }

}  // namespace fcl

using namespace fcl;

extern "C" {

size_t fcl_pwt_dw_workspace_bytes(int64_t samples, int residual, int aux, int ksize) {
    if (samples < 1 || residual < 1 || aux < 1 || ksize < 1) return 0;
    return (size_t)pwr_chunks(samples) * ((size_t)ksize * residual + aux + 1) * 2 * residual * sizeof(float);
}

int fcl_pwt_block_fwd(const fcl_pwt_t* a, fcl_stream_t stream) {
    const int rc = pwt_check(a, "pwt_block_fwd");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->c && a->w_gate && a->b_gate && a->w_out && a->b_out && a->ab && a->x_out && a->skips, FCL_ERR_INVALID,
                "pwt_block_fwd: null x / c / w_gate / b_gate / w_out / b_out / ab / x_out / skips");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->c) && aligned16(a->w_gate) && aligned16(a->w_out) && aligned16(a->ab) && aligned16(a->x_out) &&
                    aligned16(a->skips) && aligned16(a->z_out),
                FCL_ERR_ALIGN, "pwt_block_fwd: x, c, w_gate, w_out, ab, x_out, skips and z_out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual, A = a->aux, k = a->ksize;
    {
        const PwrA in = {a->x, R, R, k, a->dilation, 1.f, a->c, A, A};
        ProfScope ps("pwt_gate_kernel", 2.0 * (k * R + A) * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) hipLaunchKernelGGL(pwt_gate_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_gate, a->b_gate, a->seg_lo, a->seg_hi, a->ab, a->z_out, n)
        PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
    }
    {
        const PwrA in = {a->ab, 2 * R, R, 1, 1, 1.f, nullptr, 0, 0};
        ProfScope ps("pwt_out_kernel", 2.0 * R * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    hipLaunchKernelGGL(pwt_out_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_out, a->b_out, a->x, a->seg_lo, a->seg_hi, a->x_out, a->skips, n, a->first)
        PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
    }
    return check_hip(hipGetLastError(), "pwt_block_fwd");
}

int fcl_pwt_block_dx(const fcl_pwt_t* a, fcl_stream_t stream) {
    const int rc = pwt_check(a, "pwt_block_dx");
    if (rc) return rc;
    FCL_REQUIRE(a->ds && a->ab && a->w_dz && a->dz, FCL_ERR_INVALID, "pwt_block_dx: null ds / ab / w_dz / dz");
    FCL_REQUIRE(a->last ? a->dxo == nullptr : a->dxo != nullptr, FCL_ERR_INVALID,
                "pwt_block_dx: dxo (the gradient of x_out) is needed for every block but the last, which has none");
    FCL_REQUIRE(!a->dx || a->w_dx, FCL_ERR_INVALID, "pwt_block_dx: dx needs w_dx");
    FCL_REQUIRE(!a->dc || a->w_dc, FCL_ERR_INVALID, "pwt_block_dx: dc needs w_dc");
    FCL_REQUIRE(aligned16(a->ds) && aligned16(a->dxo) && aligned16(a->ab) && aligned16(a->w_dz) && aligned16(a->w_dx) && aligned16(a->w_dc) &&
                    aligned16(a->dz) && aligned16(a->dx) && aligned16(a->dc),
                FCL_ERR_ALIGN, "pwt_block_dx: ds, dxo, ab, w_dz, w_dx, w_dc, dz, dx and dc must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual, A = a->aux, k = a->ksize;
    {
        // without dxo the contraction is over ds alone, on the Wskip rows of w_dz
        const PwrA in = {a->dxo, R, R, a->dxo ? 1 : 0, 1, PWT_SQRT_HALF, a->ds, R, R};
        const float* w = a->dxo ? a->w_dz : a->w_dz + (size_t)R * R;
        ProfScope ps("pwt_dz_kernel", 2.0 * (a->dxo ? 2 : 1) * R * R * (double)n, (double)n, s);
#define PWT_CALL(NN) hipLaunchKernelGGL(pwt_dz_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, w, a->ab, a->seg_lo, a->seg_hi, a->dz, n)
        PWT_R_TILES(PWT_CALL)
#undef PWT_CALL
    }
    if (a->dx) {
        const PwrA in = {a->dz, 2 * R, 2 * R, k, a->dilation, 1.f, nullptr, 0, 0};
        ProfScope ps("pwt_dx_kernel", 2.0 * k * 2 * R * R * (double)n, (double)n, s);
#define PWT_CALL(NN) hipLaunchKernelGGL(pwt_dx_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_dx, a->dxo, a->seg_lo, a->seg_hi, a->dx, n)
        PWT_R_TILES(PWT_CALL)
#undef PWT_CALL
    }
    if (a->dc) {
        const PwrA in = {a->dz, 2 * R, 2 * R, 1, 1, 1.f, nullptr, 0, 0};
        ProfScope ps("pwt_dc_kernel", 2.0 * 2 * R * A * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    case NN:         \
        hipLaunchKernelGGL(pwt_dc_kernel<NN>, pwt_grid(n), dim3(256), 0, s, in, a->w_dc, a->seg_lo, a->seg_hi, a->dc, n, a->last); \
        break;
        switch (A / 16) { PWT_CALL(1) PWT_CALL(2) PWT_CALL(3) PWT_CALL(4) PWT_CALL(5) PWT_CALL(6) PWT_CALL(7) PWT_CALL(8) }
#undef PWT_CALL
    }
    return check_hip(hipGetLastError(), "pwt_block_dx");
}

int fcl_pwt_block_dw(const fcl_pwt_t* a, fcl_stream_t stream) {
    const int rc = pwt_check(a, "pwt_block_dw");
    if (rc) return rc;
    FCL_REQUIRE(a->x && a->c && a->ab && a->dz && a->ds && a->dw_gate && a->db_gate && a->dw_out && a->db_out && a->workspace, FCL_ERR_INVALID,
                "pwt_block_dw: null x / c / ab / dz / ds / dw_gate / db_gate / dw_out / db_out / workspace");
    FCL_REQUIRE(a->last ? a->dxo == nullptr : a->dxo != nullptr, FCL_ERR_INVALID,
                "pwt_block_dw: dxo (the gradient of x_out) is needed for every block but the last, which has none");
    FCL_REQUIRE(aligned16(a->x) && aligned16(a->c) && aligned16(a->ab) && aligned16(a->dz) && aligned16(a->ds) && aligned16(a->dxo), FCL_ERR_ALIGN,
                "pwt_block_dw: x, c, ab, dz, ds and dxo must be 16-byte aligned");
    FCL_REQUIRE(a->workspace_bytes >= fcl_pwt_dw_workspace_bytes(a->samples, a->residual, a->aux, a->ksize), FCL_ERR_WORKSPACE,
                "pwt_block_dw: the workspace holds %zu bytes, fcl_pwt_dw_workspace_bytes asks for %zu", a->workspace_bytes,
                fcl_pwt_dw_workspace_bytes(a->samples, a->residual, a->aux, a->ksize));
    hipStream_t s = (hipStream_t)stream;
    const long long n = a->samples;
    const int R = a->residual, A = a->aux, k = a->ksize;
    const unsigned chunks = (unsigned)pwr_chunks(n);
    {
        const int rows = k * R + A, combos = rows / 16 + 1;
        const PwrA in = {a->x, R, R, k, a->dilation, 1.f, a->c, A, A};
        const dim3 grid(chunks, (unsigned)((combos + 3) / 4));
        {
            ProfScope ps("pwt_dw_kernel<gate>", 2.0 * rows * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    hipLaunchKernelGGL((pwr_dw_kernel<PWR_PLAIN, NN, NN / 2>), grid, dim3(256), 0, s, in, a->dz, a->dz + R, 2 * R, 1.f, 1, a->seg_lo, a->seg_hi, a->workspace, n)
            PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
        }
        const int nw = rows * 2 * R, nb = 2 * R;
        ProfScope ps("pwt_dw_reduce_kernel", 0.0, (double)chunks, s);
        hipLaunchKernelGGL(pwr_dw_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, a->workspace, (int)chunks, nw, nb, a->dw_gate,
                           a->db_gate);
    }
    {
        const int combos = R / 16 + 1;
        const PwrA in = {a->ab, 2 * R, R, 1, 1, 1.f, nullptr, 0, 0};
        const dim3 grid(chunks, (unsigned)((combos + 3) / 4));
        const float* b1 = a->dxo ? a->dxo : a->ds;  // (without dxo: a valid address, masked to zero)
        {
            ProfScope ps("pwt_dw_kernel<out>", 2.0 * R * 2 * R * (double)n, (double)n, s);
#define PWT_CALL(NN) \
    hipLaunchKernelGGL((pwr_dw_kernel<PWR_GATED, NN, NN / 2>), grid, dim3(256), 0, s, in, b1, a->ds, R, PWT_SQRT_HALF, a->dxo ? 1 : 0, a->seg_lo, a->seg_hi, a->workspace, n)
            PWT_EVEN_TILES(PWT_CALL)
#undef PWT_CALL
        }
        const int nw = R * 2 * R, nb = 2 * R;
        ProfScope ps("pwt_dw_reduce_kernel", 0.0, (double)chunks, s);
        hipLaunchKernelGGL(pwr_dw_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, a->workspace, (int)chunks, nw, nb, a->dw_out,
                           a->db_out);
    }
    return check_hip(hipGetLastError(), "pwt_block_dw");
}

}  // extern "C"
