// Integer butterflies across the 64 lanes of a wavefront (every lane gets the result), in ONE copy for the VSD score, the annotation
// record and the mask crops.  Kept out of lc_shared.h, whose hash belongs to other libraries.
#pragma once
#include <hip/hip_runtime.h>

namespace lc {

template <typename Op>
__device__ __forceinline__ int wave_fold(int v, Op op) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) { return wave_fold(v, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ int wave_min(int v) { return wave_fold(v, [](int a, int b) { return min(a, b); }); }
__device__ __forceinline__ int wave_max(int v) { return wave_fold(v, [](int a, int b) { return max(a, b); }); }

}  // namespace lc
