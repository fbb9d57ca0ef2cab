// The fixed-point coordinates of an affine warp (include/lc_amd_crop.h) and its launch geometry, in ONE copy for the zoom-in crops
// (crop/lc_crop.hip) and the training mask crops (maskcrop/lc_maskcrop.hip); tests/crops_oracle.coordinates is the yardstick of both.
// Every fp64 product and sum is rounded on its own, written with __dmul_rn / __dadd_rn: the libraries are built with -ffp-contract=on,
// and m01 * y + b1 in one expression would be fused and can move a coordinate by one.  Pieces, not a kernel: crop adds its one delta to
// the row terms, maskcrop forms both coordinate sets from one pair of sums (integer addition is exact: the same X either way).
#pragma once
#include <hip/hip_runtime.h>

namespace lc {

constexpr double kAbScale = 1024.0, kFixLimit = 1073741824.0;  // 1 << AB_BITS, 2^30
constexpr long long kNearestDelta = 512, kLinearDelta = 16;  // what a coordinate sum gains before it is split

// rint (half to even), clamped to +-2^30, as an integer.  fmax / fmin also turn a NaN into a bound.
__device__ __forceinline__ int fix(double v) { return (int)fmin(fmax(rint(v), -kFixLimit), kFixLimit); }

// A row's set-up: the fp64 inverse (m00 m01 b1 m10 m11 b2) of the six fp32 entries of M; returns ok (the caller's judgement so far) && all six finite.
__device__ __forceinline__ bool inverse_of(const float* M32, bool ok, double* inv) {
    double M[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float m = M32[k];
        ok = ok && (__float_as_uint(m) & 0x7f800000u) != 0x7f800000u;
        M[k] = (double)m;
    }
    double D = __dadd_rn(__dmul_rn(M[0], M[4]), -__dmul_rn(M[1], M[3]));
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double m00 = __dmul_rn(M[4], D), m01 = __dmul_rn(-M[1], D), m10 = __dmul_rn(-M[3], D), m11 = __dmul_rn(M[0], D);
    inv[0] = m00; inv[1] = m01; inv[2] = __dadd_rn(__dmul_rn(-m00, M[2]), -__dmul_rn(m01, M[5]));
    inv[3] = m10; inv[4] = m11; inv[5] = __dadd_rn(__dmul_rn(-m10, M[2]), -__dmul_rn(m11, M[5]));
    return ok;
}

// the two x terms of the four pixels from x0 on
__device__ __forceinline__ void quad_terms(double m00, double m10, int x0, int (&ax)[4], int (&ay)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double x = (double)(x0 + j);
        ax[j] = fix(__dmul_rn(__dmul_rn(m00, x), kAbScale));
        ay[j] = fix(__dmul_rn(__dmul_rn(m10, x), kAbScale));
    }
}

// the row term of one coordinate (m01, b1 for X0; m11, b2 for Y0), without a delta
__device__ __forceinline__ long long row_term(double m, double b, int y) {
    return (long long)fix(__dmul_rn(__dadd_rn(__dmul_rn(m, (double)y), b), kAbScale));
}

// the integer splits of a coordinate sum that HOLDS its delta: the nearest tap of X + 512, the linear taps and weights of X + 16, Y + 16
__device__ __forceinline__ int nearest_tap(long long Xd) { return (int)(Xd >> 10); }
struct LinearTaps { int sx, sy, fx, fy; };
__device__ __forceinline__ LinearTaps linear_taps(long long Xd, long long Yd) {
    const int Xs = (int)(Xd >> 5), Ys = (int)(Yd >> 5);
    return LinearTaps{Xs >> 5, Ys >> 5, Xs & 31, Ys & 31};
}

// The launch geometry: crop rows per workgroup, workgroups per row of the batch, log2 of the threads along x (a thread owns four x).
struct WarpGrid { int band, nbands, lg_tx; };
inline WarpGrid warp_grid(int h, int w, int threads, int min_band) {
    WarpGrid g{};
    const int quads = (w + 3) / 4;
    while ((1 << g.lg_tx) < quads && (1 << g.lg_tx) < threads) ++g.lg_tx;
    const int rows_per_pass = threads >> g.lg_tx;
    g.band = rows_per_pass > min_band ? rows_per_pass : min_band;
    g.nbands = (h + g.band - 1) / g.band;
    return g;
}

}  // namespace lc
