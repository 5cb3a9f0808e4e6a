// pyin_log_ulp.hip — the function error of the device's logf over the arguments pyin_obs_kernel passes it: [1e-30, 1], the probability
// floor up to a whole frame's mass.  4 M points, log-spaced with a hashed nudge, then every power of two of the range with its two float neighbours,
// then 1e-30f and 1 themselves.  Compiled with the library's contraction mode.  The error is |float result - float64 logarithm of the same float
// argument| in units of the ulp of the float64 result's binade (as tools/probe/al_gmm_ulp.hip).  One line of JSON.
//   hipcc --offload-arch=gfx950 -O3 tools/probe/pyin_log_ulp.hip -o tools/probe/pyin_log_ulp && tools/probe/pyin_log_ulp
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#pragma clang fp contract(off)

__global__ void eval(const float* a, float* l, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) l[i] = logf(a[i]);
}

static double ulps(float got, double want) {
    int ex;
    frexp(want, &ex);  // want = m 2^ex, 0.5 <= m < 1: the ulp of its binade is 2^(ex - 24)
    return fabs((double)got - want) / ldexp(1.0, ex - 24);
}

int main() {
    const int grid = 1 << 22;
    std::vector<float> a;
    a.reserve(grid + 512);
    unsigned h = 12345u;
    const double lo = log(1e-30);
    for (int i = 0; i < grid; ++i) {
        h = h * 1664525u + 1013904223u;
        const float v = (float)exp(lo * (1.0 - ((double)i + (double)(h >> 8) / 16777216.0) / grid));
        a.push_back(fminf(fmaxf(v, 1e-30f), 1.f));
    }
    for (int e = -99; e <= 0; ++e) {
        const float p = ldexpf(1.f, e);
        a.push_back(p);
        a.push_back(fminf(nextafterf(p, 2.f), 1.f));
        a.push_back(fmaxf(nextafterf(p, 0.f), 1e-30f));
    }
    a.push_back(1e-30f);
    a.push_back(1.f);
    while (a.size() % 256) a.push_back(1.f);
    const int n = (int)a.size();
    std::vector<float> l(n);
    float *da, *dl;
    if (hipMalloc(&da, n * 4) != hipSuccess || hipMalloc(&dl, n * 4) != hipSuccess) return 1;
    if (hipMemcpy(da, a.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
    hipLaunchKernelGGL(eval, dim3(n / 256), dim3(256), 0, 0, da, dl, n);
    if (hipMemcpy(l.data(), dl, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double worst = 0.0;
    float at = 1.f;
    for (int i = 0; i < n; ++i) {
        if (a[i] == 1.f) continue;  // log 1 = 0 has no binade: reported below
        const double u = ulps(l[i], log((double)a[i]));
        if (u > worst) worst = u, at = a[i];
    }
    printf("{\"points\": %d, \"logf_worst_ulp\": %.4f, \"at\": %.9g, \"logf_of_1\": %.9g, \"logf_of_floor\": %.9g}\n", n, worst, (double)at, (double)l[n - 1],
           (double)l[grid + 300]);
    return 0;
}
