// The length of the ray through a frame pixel per unit of depth (steps 1 and 2 of include/lc_amd_vsd.h), and the 16-byte-phase access to
// a row of a depth map, in ONE copy for the VSD score (vsd/lc_vsd.hip) and the annotation record (gtinfo/lc_gtinfo.hip).
// Both contracts round every fp64 operation on its own, and the libraries are built with -ffp-contract=on, which fuses a product and a
// sum only inside one expression.  So every operation below is a statement of its own, in the contracts' order: joining two of them
// changes a ray length in its last bit and, through `<= delta`, a count.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lc {

// the row's share: Y = (y + pcy - k12) / k11 of frame row y, as yy = Y Y and kY = k01 Y
struct RayRow { double yy, kY; };
__device__ __forceinline__ RayRow ray_row(int y, double pcy, double k12, double k11, double k01) {
    double py = (double)y;
    py = py + pcy;
    py = py - k12;
    const double Y = py / k11;
    const double yy = Y * Y;
    const double kY = k01 * Y;
    return RayRow{yy, kY};
}

// n = sqrt(X X + Y Y + 1) of frame column x, X = (x + pcx - k02 - k01 Y) / k00, the sum taken as (X X + Y Y) + 1
__device__ __forceinline__ double ray_length(int x, double pcx, double k02, double k00, double kY, double yy) {
    double px = (double)x;
    px = px + pcx;
    px = px - k02;
    const double num = px - kY;
    const double X = num / k00;
    const double xx = X * X;
    double s = xx + yy;
    s = s + 1.0;
    return sqrt(s);
}

__device__ __forceinline__ int lead_of(const float* row) { return (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3); }  // elements behind the 16-byte boundary

// the four elements of a row of width w from x on, 0 outside the row; a whole group starts on a 16-byte boundary where x = 4 g - lead_of(row)
__device__ __forceinline__ void load_group(const float* row, int x, int w, float (&f)[4]) {
    if (x >= 0 && x + 4 <= w) {
        const float4 v = *reinterpret_cast<const float4*>(row + x);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = (x + j >= 0 && x + j < w) ? row[x + j] : 0.0f;
    }
}

}  // namespace lc
