// Test helper (NOT part of the product library): sincos_small of lc_common.h on an array of angles, so that its full-range fallback
// (angles of 1e4 and beyond, which no quaternion start reaches) can be checked in both of its forms.  Built twice by
// tests/test_gpu_pnp_onebody.py: with -DLC_SINCOS_FALLBACK_CALL=1 (the out-of-line function of the latency translation units) and =0.
#include "lc_common.h"

namespace {
__global__ __launch_bounds__(64) void sincos_probe_kernel(const double* x, double* s, double* c, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double sv, cv;
    lc::sincos_small(x[i], sv, cv);
    s[i] = sv;
    c[i] = cv;
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int sincos_probe(const double* x, double* s, double* c, int n, void* stream) {
    if (n <= 0 || !x || !s || !c) return 1;
    hipLaunchKernelGGL(sincos_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), x, s, c, n);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
