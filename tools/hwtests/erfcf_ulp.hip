// The error of the device library's erfcf (and expf) ALONE against float64, in ulp of float32 at the true value and as a relative
// error in units of u = 2^-24: the figure E_erfc that the exact-GELU bound of tests/clip_ref.py takes (twice the maximum relative
// error seen here, a grid is not exhaustive).
// Stand-alone: hipcc --offload-arch=gfx950 -O3 -o erfcf_ulp erfcf_ulp.hip ; ./erfcf_ulp
//   erfcf on x = -6 + i 2^-20 for i in [0, 12 * 2^20] (12.6 million points; beyond +-6 the GELU's result is 0 or x to the last bit
//   shown by the bound's own terms), expf on the same count of points over [-87, 88].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));        \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

__global__ void eval_kernel(float lo, float step, int n, int which, float* x_out, float* y_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = lo + step * (float)i;
    x_out[i] = x;
    y_out[i] = which == 0 ? erfcf(x) : expf(x);
}

static double ulp_at(double v) {
    int e;
    frexp(fabs(v), &e);                       // |v| = f 2^e, f in [0.5, 1): the float32 ulp is 2^(e - 24), not below the subnormal step
    return ldexp(1.0, (e - 24 < -149) ? -149 : e - 24);
}

int main() {
    const int n = 12 * (1 << 20) + 1;
    float *dx, *dy;
    CHECK(hipMalloc(&dx, sizeof(float) * n));
    CHECK(hipMalloc(&dy, sizeof(float) * n));
    std::vector<float> x(n), y(n);
    const char* names[2] = {"erfcf", "expf"};
    const float los[2] = {-6.0f, -87.0f};
    const float steps[2] = {1.0f / (1 << 20), 175.0f / (12 * (1 << 20))};
    for (int which = 0; which < 2; ++which) {
        hipLaunchKernelGGL(eval_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, los[which], steps[which], n, which, dx, dy);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(x.data(), dx, sizeof(float) * n, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(y.data(), dy, sizeof(float) * n, hipMemcpyDeviceToHost));
        double worst = 0.0, worst_neg = 0.0, worst_pos = 0.0, worst_rel = 0.0;
        float at = 0.f;
        for (int i = 0; i < n; ++i) {
            const double ref = which == 0 ? erfc((double)x[i]) : exp((double)x[i]);
            const double err = fabs((double)y[i] - ref) / ulp_at(ref);
            if (err > worst) worst = err, at = x[i];
            if (ref >= ldexp(1.0, -126) && fabs((double)y[i] - ref) / ref > worst_rel) worst_rel = fabs((double)y[i] - ref) / ref;
            if (x[i] < 0 && err > worst_neg) worst_neg = err;
            if (x[i] >= 0 && err > worst_pos) worst_pos = err;
        }
        printf("%s: %d points in [%g, %g]: max error %.4f ulp at x = %.9g (x < 0: %.4f, x >= 0: %.4f); max relative error %.4f u, u = 2^-24\n",
               names[which], n, (double)x[0], (double)x[n - 1], worst, (double)at, worst_neg, worst_pos, worst_rel * 16777216.0);
    }
    CHECK(hipFree(dx));
    CHECK(hipFree(dy));
    return 0;
}
