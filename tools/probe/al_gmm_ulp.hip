// al_gmm_ulp.hip — the function error of the device's expf and logf over the arguments al_gmm_loglik_kernel / al_gmm_post_kernel pass them
// (DESIGN 6v): expf on [-87.3, 0] (every l_c - mx; below that the result is subnormal or 0 against a sum of at least 1), logf on [1, 8] (a sum of at
// most 8 terms of at most 1, the dominant one exactly 1).  4 M points each: a uniform grid plus the grid's points nudged by a hash.  The error is
// |float result - float64 function of the same float argument| in units of the ulp of the float64 result's binade.  One line of JSON.
//   hipcc --offload-arch=gfx950 -O3 tools/probe/al_gmm_ulp.hip -o tools/probe/al_gmm_ulp && tools/probe/al_gmm_ulp
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

__global__ void eval(const float* a, float* e, float* s, float* l, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        e[i] = expf(a[i]);
        s[i] = 1.f + (a[i] / -87.3f) * 7.f;  // kept: the host takes the float64 logarithm of the very float the device took it of
        l[i] = logf(s[i]);
    }
}

static double ulps(float got, double want) {
    int ex;
    frexp(want, &ex);  // want = m 2^ex, 0.5 <= m < 1: the ulp of its binade is 2^(ex - 24)
    return fabs((double)got - want) / ldexp(1.0, ex - 24);
}

int main() {
    const int n = 1 << 22;
    std::vector<float> a(n), e(n), s(n), l(n);
    unsigned h = 12345u;
    for (int i = 0; i < n; ++i) {
        h = h * 1664525u + 1013904223u;
        a[i] = (float)(-87.3 * ((double)i + (double)(h >> 8) / 16777216.0) / n);
    }
    a[0] = 0.f;  // expf(0) and logf(1) themselves: the contract needs them to be exactly 1 and 0
    float *da, *de, *ds, *dl;
    if (hipMalloc(&da, n * 4) != hipSuccess || hipMalloc(&de, n * 4) != hipSuccess || hipMalloc(&ds, n * 4) != hipSuccess || hipMalloc(&dl, n * 4) != hipSuccess) return 1;
    if (hipMemcpy(da, a.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
    hipLaunchKernelGGL(eval, dim3(n / 256), dim3(256), 0, 0, da, de, ds, dl, n);
    if (hipMemcpy(e.data(), de, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(l.data(), dl, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double we = 0.0, wl = 0.0;
    for (int i = 0; i < n; ++i) {
        we = fmax(we, ulps(e[i], exp((double)a[i])));
        if (s[i] > 1.f) wl = fmax(wl, ulps(l[i], log((double)s[i])));
    }
    printf("{\"points\": %d, \"expf_worst_ulp\": %.4f, \"logf_worst_ulp\": %.4f, \"expf_of_0\": %.9g, \"logf_of_1\": %.9g}\n", n, we, wl, (double)e[0], (double)l[0]);
    return 0;
}
