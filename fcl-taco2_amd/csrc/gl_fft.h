// gl_fft.h — the LDS-resident real FFT shared by csrc/griffinlim.hip (Griffin-Lim vocoder) and csrc/features.hip (log-mel / energy feature
// extraction): the geometry of a 256-thread workgroup (GlGeo), the padded LDS index (gl_pad) and the Stockham radix-4 complex FFT of
// M = n_fft / 2 points (gl_fft); griffinlim.hip's header comment describes the algorithm.  The split stage of the real FFT stays with each kernel.
#pragma once
#include "fcl_common.h"

namespace fcl {

__device__ __forceinline__ int gl_pad(int i) { return i + (i >> 5); }

template <int N>
struct GlGeo {
    static constexpr int M = N / 2, Q = M / 4, FPW = 1024 / M, SLOT = M + M / 32, PLANE = FPW * SLOT, BINS = M + 1;
};

__device__ __forceinline__ float2 gl_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// complex FFT of the FPW frames in buffer 0 of re / im ([2][PLANE] each); returns the buffer that holds the result.  The caller has synchronised after
// filling buffer 0; the result is synchronised on return.  INV: the unscaled inverse (conjugated twiddles).
template <int N, bool INV>
__device__ __forceinline__ int gl_fft(float* re, float* im, const float2* __restrict__ tw, int tid) {
    using G = GlGeo<N>;
    constexpr int M = G::M, Q = G::Q, SLOT = G::SLOT, PLANE = G::PLANE;
    const int base = (tid / Q) * SLOT, t = tid % Q;  // FPW * Q == 256: one butterfly per thread and pass
    int cur = 0;
#pragma unroll
    for (int s = 1; s * 4 <= M; s *= 4) {
        const float *xr = re + cur * PLANE + base, *xi = im + cur * PLANE + base;
        float *yr = re + (cur ^ 1) * PLANE + base, *yi = im + (cur ^ 1) * PLANE + base;
        const int p = t / s, q = t - p * s;
        float2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = make_float2(xr[gl_pad(t + k * Q)], xi[gl_pad(t + k * Q)]);
        float2 w1 = tw[2 * p * s], w2 = tw[4 * p * s], w3 = tw[6 * p * s];
        if (INV) {
            w1.y = -w1.y;
            w2.y = -w2.y;
            w3.y = -w3.y;
        }
        const float2 apc = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), amc = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
        const float2 bpd = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), bmd = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
        const float2 jb = INV ? make_float2(bmd.y, -bmd.x) : make_float2(-bmd.y, bmd.x);  // +-i (b - d)
        const float2 o0 = make_float2(apc.x + bpd.x, apc.y + bpd.y);
        const float2 o1 = gl_cmul(w1, make_float2(amc.x - jb.x, amc.y - jb.y));
        const float2 o2 = gl_cmul(w2, make_float2(apc.x - bpd.x, apc.y - bpd.y));
        const float2 o3 = gl_cmul(w3, make_float2(amc.x + jb.x, amc.y + jb.y));
        const int o = q + s * 4 * p;
        yr[gl_pad(o)] = o0.x; yi[gl_pad(o)] = o0.y;
        yr[gl_pad(o + s)] = o1.x; yi[gl_pad(o + s)] = o1.y;
        yr[gl_pad(o + 2 * s)] = o2.x; yi[gl_pad(o + 2 * s)] = o2.y;
        yr[gl_pad(o + 3 * s)] = o3.x; yi[gl_pad(o + 3 * s)] = o3.y;
        __syncthreads();
        cur ^= 1;
    }
    if (M == 512) {  // 512 = 2 x 4^4: what is left is one radix-2 pass at stride M / 2 without twiddles
        constexpr int H = M / 2;
        for (int i = tid; i < G::FPW * H; i += 256) {
            const int b2 = (i / H) * SLOT, q = i % H;
            const float *xr = re + cur * PLANE + b2, *xi = im + cur * PLANE + b2;
            float *yr = re + (cur ^ 1) * PLANE + b2, *yi = im + (cur ^ 1) * PLANE + b2;
            const float ar = xr[gl_pad(q)], ai = xi[gl_pad(q)], br = xr[gl_pad(q + H)], bi = xi[gl_pad(q + H)];
            yr[gl_pad(q)] = ar + br; yi[gl_pad(q)] = ai + bi;
            yr[gl_pad(q + H)] = ar - br; yi[gl_pad(q + H)] = ai - bi;
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

}  // namespace fcl
