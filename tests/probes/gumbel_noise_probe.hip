// Hardware probe: how far is the samplers' Gumbel noise from its float64 definition?
// The four sampling kernels draw argmax(l / T + g) with g = gumbel_noise(bits) of hydragen_amd/csrc/vocab_row.h (the one
// text all of them include), built on fast_log2 = the hardware's approximate log2.  tests/sampler_mirror.py evaluates the same noise in
// float64 on the host and compares drawn tokens; the margin below which it does not compare a row (its EPS) rests on the number
// this program prints.  It measures the log instruction, not the samplers: one kernel evaluates the expression for every one of
// the 2^23 values of k = bits >> 9, the host evaluates
//     u = (k + 1/2) 2^-23,  e = max(-ln u, 2^-25),  g64 = -ln e
// in double, and the program prints max |g - g64| with where it occurs, the same maximum outside the 2^12 largest k (where
// -ln u is small and its relative error is at its largest), the range of g, and whether g is non-decreasing in k.
// Build and run:  hipcc -O3 --offload-arch=gfx950 -I hydragen_amd/csrc tests/probes/gumbel_noise_probe.hip -o gumbel_noise_probe
//                 ./gumbel_noise_probe
// Record: profiles/sampler_noise_probe.md.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hyd_common.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static const uint32_t kN = 1u << 23;

// = vocab_row.h gumbel_noise, restated so that this program builds alone (tests/test_sampler_noise.py pins the text of the header's
// first two lines)
__device__ __forceinline__ float gumbel(uint32_t bits) {
    const float u = ((float)(bits >> 9) + 0.5f) * 0x1p-23f;
    const float e = fmaxf(-hyd::kLn2 * hyd::fast_log2(u), 0x1p-25f);
    return -hyd::kLn2 * hyd::fast_log2(e);
}

__global__ __launch_bounds__(256) void gumbel_all(float* g, uint32_t n) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) g[k] = gumbel(k << 9 | (k & 0x1ffu));  // the low 9 bits of a word do not matter: fill them with something
}

int main() {
    float* dg = nullptr;
    CK(hipMalloc(&dg, (size_t)kN * sizeof(float)));
    hipLaunchKernelGGL(gumbel_all, dim3(kN / 256), dim3(256), 0, 0, dg, kN);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<float> g(kN);
    CK(hipMemcpy(g.data(), dg, (size_t)kN * sizeof(float), hipMemcpyDeviceToHost));
    CK(hipFree(dg));

    double worst = 0.0, worst_body = 0.0, gmin = INFINITY, gmax = -INFINITY;
    uint32_t at = 0, at_body = 0, drops = 0, first_drop = 0, not_finite = 0;
    for (uint32_t k = 0; k < kN; ++k) {
        const double u = ((double)k + 0.5) * 0x1p-23;
        const double e = fmax(-log(u), 0x1p-25);
        const double g64 = -log(e);
        if (!std::isfinite(g[k])) { ++not_finite; continue; }
        const double err = fabs((double)g[k] - g64);
        if (err > worst) { worst = err; at = k; }
        if (k < kN - 4096 && err > worst_body) { worst_body = err; at_body = k; }
        gmin = fmin(gmin, (double)g[k]);
        gmax = fmax(gmax, (double)g[k]);
        if (k && g[k] < g[k - 1]) { if (!drops) first_drop = k; ++drops; }
    }
    printf("gumbel over k = 0 .. 2^23 - 1 (u = (k + 1/2) 2^-23)\n");
    printf("not finite            : %u\n", not_finite);
    printf("range of g            : [%.6f, %.6f]\n", gmin, gmax);
    printf("max |g - g64|         : %.6e at k = %u (g = %.9g)\n", worst, at, (double)g[at]);
    printf("max |g - g64|, k < 2^23 - 4096 : %.6e at k = %u (g = %.9g)\n", worst_body, at_body, (double)g[at_body]);
    printf("non-decreasing in k   : %s (%u drops, first at k = %u)\n", drops ? "no" : "yes", drops, first_drop);
    return 0;
}
