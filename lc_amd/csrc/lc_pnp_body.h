// Device body of the batched weighted-PnP solve: one workgroup runs one pose's whole Levenberg-Marquardt solve -- one wavefront
// (N <= 64), a TEAM of two wavefronts that split the 28 sums of an evaluation between them (small grids of the plain solve), or four
// wavefronts (N > 64); see the forms in front of solve_pose.
// Included by lc_pnp.hip / lc_pnp_latency.hip (stand-alone kernels) and lc_fused*.hip (loss + PnP in one launch).
//
// Replaces lib/pnp/cxx/ceres.cpp:72-145 (pnp_ceres_f32 -> ceres::Solve, DENSE_QR, autodiff Jets) and its OpenMP
// batch driver (:147-177).  Residual model = ceres.cpp:15-65; optimiser = Ceres 2.1.0's default trust-region LM,
// restated in oracle/pnp_lm_oracle.c (see that header for the schedule and the "parity unpinned" note).
//
// MI355X mapping: thread = correspondence (workgroup-stride when N > 256); the pose x = (angle-axis, t), the 6x6 normal
// equations and the LM state are wave-uniform values every lane carries.  One evaluation per LM iteration:
//   residuals in fp64 from R(x) X + t;  Jacobian rows from the closed form  J_rot = Jr(w) (R X x J_t)
//   (d(R(w)X)/dw = -R [X]x Jr(w) = -[R X]x Jr(w)^T, Jr = right Jacobian of SO(3)) -- no per-point 3x3 derivative, no autodiff;
//   J^T J (21) | J^T r (6) | r^T r (1) summed over the workgroup by the block sum of the form (lc_common.h): one wave streams its
//   entries to LDS slots as it forms them, four waves reduce-scatter in registers and meet in 192 doubles of LDS;
//   damped, Jacobi-scaled 6x6 system solved in registers (LDL^T, fp64).
// Only the final 7-float state, the trust radius and the flag go back to HBM.
// Differences from the Ceres path that do not change the iterates beyond rounding: normal equations instead of QR
// (Jacobi-scaled, fp64, cond ~1e4..1e6); the accepted point's Jacobian comes from the candidate evaluation (same x)
// instead of a re-evaluation; model_cost_change from the normal-equation identity y.(g/2) + sum(d y^2)/2.
#pragma once
#include <cfloat>

#include "lc_common.h"
#include "lc_kernels.h"

// Diagnostic build only (-DLC_STAMPS, scripts/diag_stamps.py): per-phase s_memtime sums, written to p.result_tr's
// neighbour buffer p.iters (reinterpreted) which nothing else reads in that build.  Never defined in the shipped library.
#ifdef LC_STAMPS
#define LC_PSTAMP_DECL unsigned long long pst_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt0_ = 0, pt1_ = 0
#define LC_PSTAMP_BEGIN()                                                                 \
    do {                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pt0_)::"memory");      \
        __builtin_amdgcn_sched_barrier(0);                                                \
    } while (0)
#define LC_PSTAMP(i)                                                                      \
    do {                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pt1_)::"memory");      \
        __builtin_amdgcn_sched_barrier(0);                                                \
        pst_[i] += pt1_ - pt0_;                                                           \
        pt0_ = pt1_;                                                                      \
    } while (0)
#else
#define LC_PSTAMP_DECL
#define LC_PSTAMP_BEGIN() do {} while (0)
#define LC_PSTAMP(i) do {} while (0)
#endif

#ifndef LC_PNP_TEAM2
#define LC_PNP_TEAM2 1  // A/B switch: the latency builds of the one-correspondence-per-lane solve (plain instantiations: lc_pnp_latency.hip, lc_fused_kernel.h) run TWO wavefronts per pose that share the products and the block sum (TeamWave below); 0 = one wavefront per pose
#endif
#ifndef LC_PNP_TEAM_REGSUM
#define LC_PNP_TEAM_REGSUM 1  // A/B switch: the team sums each wave's 14 entries in registers (lc_common.h: block_sum_team2_reg); 0 = through their LDS slots (block_sum_team2)
#endif

namespace lc {
namespace pnp {

template <int NW>
constexpr int kPnpLdsDoubles = [] { static_assert(NW == 1, "the four-wave kernels: kPnpWideReservedLdsDoubles"); return block_sum_lds_doubles(28); }();  // block_sum_close<28>
#if LC_PNP_TEAM_REGSUM
constexpr int kPnpTeamLdsDoubles = sum_team2_reg_lds_doubles(28);  // block_sum_team2_reg<28>: the two rows of totals
#else
constexpr int kPnpTeamLdsDoubles = sum_team2_lds_doubles(28);  // block_sum_team2<28>: the one-wave slots in rows of kTeamRowDoubles and a second row of totals
#endif
// Static LDS of the four-wave kernels: 7 644 doubles (61 KB) are RESERVED -- the size of a slot per thread and entry -- where
// block_sum_waves4 touches 192 doubles (block_sum_split: 194, in the split kernels' own array).  The size is in the kernel descriptor
// and decides how many workgroups share a compute unit, so shrinking it changes the speed and wants a measurement: kept to the byte
// until someone takes one.
constexpr int kPnpWideReservedLdsDoubles = 28 * 68 * 4 + 28;
static_assert(kPnpWideReservedLdsDoubles == 7644 && kPnpWideReservedLdsDoubles >= 128 + 64, "reserved size kept; block_sum_waves4 fits");

struct Point {
    double X[3];
    double u, v;     // measurement minus principal point (ceres.cpp:23-24)
    double a, b, c;  // L00, L10, L11 (ceres.cpp:25-27)
};

struct Rot {
    double R[9];   // AngleAxisRotatePoint as a matrix (both branches of ceres/rotation.h)
    double Jr[9];  // right Jacobian of SO(3) (identity in the small-angle branch, whose derivative is -R[pt]x with
                   // R = I + [aa]x, |aa| < 1.5e-8: within 1e-8 of the -[pt]x the autodiff of that branch yields)
};

__device__ __forceinline__ void make_rot(const double aa[3], Rot& o) {
    // aa is WAVE-UNIFORM (the pose every lane carries), so the two cases of ceres/rotation.h are a scalar branch: uniform() is an any-lane
    // ballot, and a caller whose lanes hold different poses would send all of them down the small arm as soon as one is small.
    // Found: such a uniform branch keeps the rotation in registers -- no kernel of the library gains a byte of scratch (a per-lane branch
    // had put `o` there) -- as long as the coefficients leave both arms through the same four locals and R, Jr are formed once behind it.
    // Bits: each arm evaluates the expressions of the former branch-free form with its selected values, the small arm 0 * x * y - 1 * z
    // and so on with the products of zeros left in, so signed zeros and non-finite inputs come out as before.
    const double x = aa[0], y = aa[1], z = aa[2];
    const double th2 = x * x + y * y + z * z;
    const bool small = !(th2 > DBL_EPSILON);  // ceres/rotation.h AngleAxisRotatePoint: pt + aa x pt, derivative -[pt]x
    double A, B, C, cd;
    if (__builtin_expect(uniform(small), 0)) {
        A = 1.0; B = 0.0; C = 0.0; cd = 1.0;
    } else {
        double th, ith;
        fast_sqrt_rsqrt_pos(th2, th, ith);
        double s, c;
        sincos_small(th, s, c);
        const double ith2 = ith * ith;
        A = s * ith;
        B = (1.0 - c) * ith2;
        C = (th - s) * ith2 * ith;
        cd = c;
    }
    // R = c I + A [w]x + B w w^T
    o.R[0] = cd + B * x * x;    o.R[1] = B * x * y - A * z; o.R[2] = B * x * z + A * y;
    o.R[3] = B * x * y + A * z; o.R[4] = cd + B * y * y;    o.R[5] = B * y * z - A * x;
    o.R[6] = B * x * z - A * y; o.R[7] = B * y * z + A * x; o.R[8] = cd + B * z * z;
    // Jr = (1 - C th2) I - B [w]x + C w w^T   (identity in the small-angle branch)
    const double d = 1.0 - C * th2;
    o.Jr[0] = d + C * x * x;     o.Jr[1] = C * x * y + B * z; o.Jr[2] = C * x * z - B * y;
    o.Jr[3] = C * x * y - B * z; o.Jr[4] = d + C * y * y;     o.Jr[5] = C * y * z + B * x;
    o.Jr[6] = C * x * z + B * y; o.Jr[7] = C * y * z - B * x; o.Jr[8] = d + C * z * z;
}

// adds one correspondence's contribution to acc = [J^T J upper (21) | J^T r (6) | r^T r | pad]
// (columns of J pre-multiplied by the Jacobi scaling sc: acc holds Js^T Js and Js^T r directly)
// FIRST: acc is written (not added to) -- saves zero-filling 32 accumulators and one add per entry when a lane owns one point.
// STREAM: (FIRST only) every finished entry goes straight to its LDS slot of the block sum instead of into acc[]
// PAR (FIRST only): 0 / 1 = only the entries of that parity are formed (the two waves of a team: stored with STREAM, block_sum_team2; left
// in acc[] without, block_sum_team2_reg; the other parity's acc[] stays unwritten); -1 = all
template <bool FIRST, bool STREAM = false, int PAR = -1>
__device__ __forceinline__ void accumulate_point(const Point& pt, const Rot& rt, const double t[3], const double k[6],
                                                 const double (&sc)[6], double (&acc)[28], double* lds = nullptr, int pos = 0) {
    double rx[3], q[3];  // R X and R X + t
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        rx[d] = rt.R[3 * d] * pt.X[0] + rt.R[3 * d + 1] * pt.X[1] + rt.R[3 * d + 2] * pt.X[2];
        q[d] = rx[d] + t[d];
    }
    const double iz = fast_rcp(q[2]);
    const double up = (q[0] * k[0] + q[1] * k[1]) * iz, vp = (q[0] * k[3] + q[1] * k[4]) * iz;
    const double du = up - pt.u, dv = vp - pt.v;
    const double r[2] = {du * pt.a + dv * pt.b, dv * pt.c};
    const double dup[3] = {k[0] * iz, k[1] * iz, -up * iz};
    const double dvp[3] = {k[3] * iz, k[4] * iz, -vp * iz};
    double J[2][6];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        J[0][3 + m] = pt.a * dup[m] + pt.b * dvp[m];
        J[1][3 + m] = pt.c * dvp[m];
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        // d(R(w) X)/dw = -R [X]x Jr(w) = -[R X]x Jl(w) with the left Jacobian Jl = R Jr = Jr^T: the row a = J_t of the residual gives
        // J_rot = Jl^T (R X x a) = Jr (R X x a) -- R X is at hand from the projection, so no R^T a is formed (9 fma fewer per row)
        double cr[3];
        cr[0] = rx[1] * J[rr][5] - rx[2] * J[rr][4];
        cr[1] = rx[2] * J[rr][3] - rx[0] * J[rr][5];
        cr[2] = rx[0] * J[rr][4] - rx[1] * J[rr][3];
#pragma unroll
        for (int m = 0; m < 3; ++m) J[rr][m] = (rt.Jr[3 * m] * cr[0] + rt.Jr[3 * m + 1] * cr[1] + rt.Jr[3 * m + 2] * cr[2]) * sc[m];  // Jr (R X x a)
#pragma unroll
        for (int m = 0; m < 3; ++m) J[rr][3 + m] *= sc[3 + m];
    }
    static_assert(PAR < 0 || FIRST, "entries are dealt by parity where a lane owns one point");
    constexpr auto mine = [](int k) { return PAR < 0 || (k & 1) == PAR; };  // (folds once the loops are unrolled)
    constexpr int kRow = PAR < 0 ? 68 : kTeamRowDoubles;                    // the team's LDS rows have their own stride (block_sum_team2)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            if (mine(tri6(i, j))) {
                const double v = __builtin_fma(J[0][i], J[0][j], J[1][i] * J[1][j]);
                if constexpr (STREAM) block_sum_put<kRow>(lds, pos, tri6(i, j), v);
                else acc[tri6(i, j)] = FIRST ? v : acc[tri6(i, j)] + v;
            }
        }
        if (mine(21 + i)) {
            const double gi = __builtin_fma(J[0][i], r[0], J[1][i] * r[1]);
            if constexpr (STREAM) block_sum_put<kRow>(lds, pos, 21 + i, gi);
            else acc[21 + i] = FIRST ? gi : acc[21 + i] + gi;
        }
    }
    if (mine(27)) {
        const double ss = __builtin_fma(r[0], r[0], r[1] * r[1]);
        if constexpr (STREAM) block_sum_put<kRow>(lds, pos, 27, ss);
        else acc[27] = FIRST ? ss : acc[27] + ss;
    }
}

// v_min_f64 / v_max_f64 as the instructions they are (clamp_diag below has the reason: fmin / fmax put a canonicalising v_max_f64 x, x in
// front wherever the compiler cannot see that x is no signalling NaN).  IEEE mode, the kernels' default: a quiet NaN operand gives the other.
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// solve (A + diag(dg)) y = rhs for symmetric A (packed upper 21) by LDL^T; false if a pivot is not positive/finite -- or, with RUNNING,
// true with a NaN y (below), which the caller's test of the model cost change turns down
template <bool RUNNING>
__device__ __forceinline__ bool ldlt_solve6(const double (&A)[21], const double (&dg)[6], const double (&rhs)[6], double (&y)[6]) {
    double L[6][6], Ld[6][6], id[6];
    // RUNNING: the pivots are not tested one by one (two compares and two mask operations each, holding VCC between dependent arithmetic of
    // a phase that is bound by issue): their running minimum and maximum are kept beside the factorisation and tested once.  v_min_f64 /
    // v_max_f64 return the OTHER operand for a quiet NaN, so over the pivots that are not NaN the two are exact (the pivots are results
    // of additions and multiplications, never signalling NaNs), and `lo > 0 && hi < DBL_MAX` is `every such pivot is > 0 and < DBL_MAX`.
    // A NaN pivot is dropped by them -- lo and hi start from d0 itself, not from a constant, so a NaN d0 is replaced by the next pivot that
    // is not NaN, and six NaN pivots fail `lo > 0` -- and needs no test of its own: id[j] = fast_rcp(NaN) is NaN, so y[j] = z[j] * id[j] - ...
    // is NaN, so every y[i] with i <= j is (y[i] subtracts L[j][i] * y[j]), so the caller's model cost change is NaN and its `mcc > 0`
    // false: the step is invalid as it was when the pivot test said so.  The only reader of the result is that conjunction.
    // !RUNNING: each pivot as it appears, the result in a scalar mask: for the kernel whose registers are full (FormDefaults::PIVOTS_RUNNING).
    [[maybe_unused]] double lo = 0, hi = 0;
    [[maybe_unused]] bool each = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = A[tri6(j, j)] + dg[j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= L[j][k] * Ld[j][k];
        if constexpr (RUNNING) {
            lo = j == 0 ? dj : min_f64(lo, dj);
            hi = j == 0 ? dj : max_f64(hi, dj);
        } else {
            each = each && (dj > 0) && (dj < DBL_MAX);
        }
        id[j] = fast_rcp(dj);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[tri6(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * Ld[j][k];
            Ld[i][j] = v;            // L[i][j] * d[j]
            L[i][j] = v * id[j];
        }
    }
    const bool ok = RUNNING ? (lo > 0) && (hi < DBL_MAX) : each;
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
        z[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = z[i] * id[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * y[k];
        y[i] = v;
    }
    return ok;
}

// one correspondence as it sits in HBM (fp32): the loads are issued first thing in the kernel, the conversion to the fp64 working
// form waits until the pose-independent set-up (quaternion -> angle-axis, ~700 cycles) has run in their shadow
struct RawPoint {
    float X[3];
    float2 u;
    float a, b, c;
};

// OPTS: the instantiation that honours PnpParams::options / weight_mask (input filtering and weight forms of the callers, done at
// the load instead of by separate element-wise launches); the plain instantiation does not even test the fields
template <bool OPTS = false>
__device__ __forceinline__ RawPoint load_raw_point(const PnpParams& p, size_t base, int n) {
    RawPoint o;
    const float* X = p.pts3d + (base + n) * 3;
    o.u = *reinterpret_cast<const float2*>(p.pts2d + (base + n) * 2);
    o.X[0] = X[0]; o.X[1] = X[1]; o.X[2] = X[2];
    if (OPTS && p.weight_mask) {  // unit information on the flagged correspondences, none on the others
        const float m = p.weight_mask[base + n] ? 1.f : 0.f;
        o.a = m; o.b = 0.f; o.c = m;
    } else if (p.sqrtL) {
        const float4 L = *reinterpret_cast<const float4*>(p.sqrtL + (base + n) * 4);
        o.a = L.x; o.b = L.z; o.c = L.w;
    } else {
        const float2 L = *reinterpret_cast<const float2*>(p.sqrt_diag + (base + n) * 2);
        o.a = L.x; o.b = 0.f; o.c = L.y;
    }
    if constexpr (OPTS) {
        if (p.options & kPnpWeightsAreStd) { o.a = 1.f / (o.a * o.a); o.c = 1.f / (o.c * o.c); }  // the sparse head's predicted deviations -> inverse variances (test.py:52)
        if (p.options & kPnpNanToNum) {
            o.u.x = nan_to_num(o.u.x); o.u.y = nan_to_num(o.u.y);
            o.X[0] = nan_to_num(o.X[0]); o.X[1] = nan_to_num(o.X[1]); o.X[2] = nan_to_num(o.X[2]);
            o.a = nan_to_num(o.a); o.b = nan_to_num(o.b); o.c = nan_to_num(o.c);
        }
        if (p.options & kPnpWeightsAreIcov) { o.a = sqrtf(o.a); o.c = sqrtf(o.c); }  // diagonal inverse covariance -> its factor (cer_solver.py:33-36)
    }
    return o;
}
__device__ __forceinline__ Point to_point(const RawPoint& r, const double cam[6]) {
    Point o;
    o.X[0] = r.X[0]; o.X[1] = r.X[1]; o.X[2] = r.X[2];
    o.u = (double)r.u.x - cam[2];
    o.v = (double)r.u.y - cam[5];
    o.a = r.a; o.b = r.b; o.c = r.c;
    return o;
}
template <bool OPTS = false>
__device__ __forceinline__ Point load_point(const PnpParams& p, size_t base, int n, const double cam[6]) {
    return to_point(load_raw_point<OPTS>(p, base, n), cam);
}

// fmin(fmax(h, 1e-6), 1e32) of a diagonal entry of J^T J, as the two instructions it is.  fmax / fmin must return the other operand for a
// signalling NaN too, so the compiler puts a canonicalising v_max_f64 h, h in front of them wherever it cannot see where h came from
// (the totals come back from LDS): six extra issue slots per LM iteration.  h is always the result of an addition or a multiplication
// -- never a signalling NaN -- and for every other input v_max_f64 / v_min_f64 (IEEE mode, the kernels' default) ARE fmax / fmin:
// a quiet NaN, -inf, +-0 and anything below 1e-6 give 1e-6, +inf and anything above 1e32 give 1e32, every other value itself.
__device__ __forceinline__ double clamp_diag(double h) {
    double lo, r;
    asm("v_max_f64 %0, %1, %2" : "=v"(lo) : "v"(h), "s"(1e-6));
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(lo), "s"(1e32));
    return r;
}

__device__ __forceinline__ double max_abs6(const double (&v)[6]) {
    double m = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) m = fmax(m, fabs(v[j]));
    return m;
}
__device__ __forceinline__ double norm6(const double (&v)[6]) {
    double m = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) m += v[j] * v[j];
    return fast_sqrt(m);
}

// ---------------------------------------------------------------------------------------------------------------------
// The forms of solve_pose.  One pose per workgroup of NW wavefronts; the wave-uniform LM algebra is replicated in every wave, the
// forms differ in where a thread's correspondences live and in how the 28 sums of an evaluation are formed:
//   1. ONE wave (N <= 64, the metric's shape), one correspondence per lane, in registers across the whole solve (REG).  The 28 entries
//      are streamed to their LDS slots as they are formed, then block_sum_close<28>.  bc: kPnpLdsDoubles<1>.
//   2. The two-wave TEAM: form 1 played by the two wavefronts of a 128-thread workgroup (TeamWave below), each with its 14 entries in
//      registers, block_sum_team2_reg (-DLC_PNP_TEAM_REGSUM=0: streamed to LDS slots, block_sum_team2).
//   3. FOUR waves (N <= 256), one correspondence per thread in registers (REG): accumulate_point<true>, then block_sum_waves4.
//   4. FOUR waves over rows of any width (e.g. the dense heads' N = 1024..1849, where four waves cut the per-evaluation point loop by
//      four): each thread adds up its correspondences -- cached prefix, tail, rescue or plain loop, below -- then block_sum_waves4,
//      block_sum_split, or nothing (the rescue form sums inside its loop).  bc of forms 3 and 4: kPnpWideReservedLdsDoubles.
// A form is a struct of named constants; each one below states only what it changes from FormDefaults.
//   OPTS: honours PnpParams::options / weight_mask / pose_mod (input filtering and weight forms of the callers, done at the load instead
//   of by separate element-wise launches); the plain forms do not even test the fields.
//   TRACE: diagnostic (lc_pnp_lm_trace_f32): also writes one row per trust-region iteration to p.trace, in the column layout of
//   oracle/pnp_lm_oracle.c's PNP_TRACE_COLS.
//   PPT (form 4): a thread keeps its first PPT correspondences (thread, thread + 256, ...) in registers as they sit in HBM (8 floats
//   each) across the whole solve; the block-stride loop otherwise re-reads them from L2 in every evaluation, ~1 us of exposed latency
//   each time.  TAIL: correspondences behind the cached prefix (n > 256 PPT) are read from memory; forms whose rows always fit the
//   prefix leave it out (the never-taken loop cost the test-time chain 1 us).  Same accumulation order, same results.
//   SPLIT = 1 (SplitPart): workgroup sx->part of the sx->G that share pose b -- it owns the correspondences part * 256 + thread + k * 256 G,
//   the block sum runs across the G workgroups (lc_common.h: block_sum_split), everything else is replicated; part 0 stores -- status 2
//   when its wait for another part ran out.  SPLIT = 2 (SplitRescue): ONE workgroup plays the sx->G parts in turn (the rescue launch of a
//   pose of status 2: block_sum_parts_serial) -- per thread the same correspondences in the same order, every sum in the same order: the
//   same bits.
//   TEAM = 0 / 1 (TeamWave; -1 = off): wave TEAM of a 128-thread workgroup whose TWO wavefronts solve ONE pose (`lane` = lane of the
//   wave, bc: kPnpTeamLdsDoubles).  Both waves hold all correspondences and run the whole solve -- load, quaternion -> angle-axis,
//   make_rot, geometry and Jacobian rows, Jacobi scaling, LDL^T, the schedule: the same expressions on the same values, so they take
//   every branch together -- but each forms and sums only the 14 of the 28 entries J^T J | J^T r | r^T r of its parity
//   (lc_common.h: block_sum_team2_reg, one workgroup barrier per evaluation; every break / continue / return is taken by both waves, so
//   their barrier counts agree; the n < 3 exit comes before the first).  Every total is summed in the one-wave form's order: the same
//   bits.  Wave 0 stores (the caller passes store = false to wave 1).
struct FormDefaults {
    static constexpr int NW = 1, PPT = 0, SPLIT = 0, TEAM = -1;
    static constexpr bool REG = true, OPTS = false, TRACE = false, TAIL = false;
    // the LDL^T tests the running minimum and maximum of its pivots once (ldlt_solve6); false: each pivot as it appears -- the same
    // decision, for the one kernel that has no two register pairs to spare in the factorisation: lc_pnp_lm_kernel at two waves per SIMD
    // (256 registers, no AGPRs) sends 20-28 B per lane to scratch with the running form, reloaded in every evaluation
    static constexpr bool PIVOTS_RUNNING = true;
};
template <bool O = false, bool PR = true>
struct OneWave : FormDefaults { static constexpr bool OPTS = O, PIVOTS_RUNNING = PR; };   // form 1
template <int W>
struct TeamWave : FormDefaults { static constexpr int TEAM = W; };                        // form 2, wave W of the team
struct OneWaveTrace : FormDefaults { static constexpr bool TRACE = true; };               // form 1, diagnostic
struct FourWaves : FormDefaults { static constexpr int NW = 4; };
template <bool O = false>
struct WideReg : FourWaves { static constexpr bool OPTS = O; };                           // form 3
struct WideLoop : FourWaves { static constexpr bool REG = false; };                       // form 4, every correspondence from memory
struct WideTrace : WideLoop { static constexpr bool TRACE = true; };                      // form 4, diagnostic
template <bool O, int P, bool T = false>
struct WideCached : WideLoop { static constexpr bool OPTS = O, TAIL = T; static constexpr int PPT = P; };  // form 4, cached prefix
template <bool O>
struct SplitPart : WideCached<O, 8, true> { static constexpr int SPLIT = 1; };            // form 4, one of G workgroups of a pose
template <bool O>
struct SplitRescue : WideLoop { static constexpr bool OPTS = O; static constexpr int SPLIT = 2; };  // form 4, the G parts in turn
template <class F>
constexpr bool form_is_legal() {
    static_assert(F::NW == 1 || F::NW == 4, "one wave or four (the team is two one-wave solves side by side)");
    static_assert(!F::REG || (F::PPT == 0 && !F::TAIL && F::SPLIT == 0), "one correspondence per thread: nothing to cache or to walk");
    static_assert(!F::TAIL || F::PPT > 0, "the tail is what lies behind a cached prefix");
    static_assert(F::SPLIT != 1 || (F::NW == 4 && !F::REG && F::PPT > 0 && !F::TRACE), "the split form is the four-wave cached-prefix solve");
    static_assert(F::SPLIT != 2 || (F::NW == 4 && !F::REG && F::PPT == 0 && !F::TRACE), "the rescue form walks memory, part by part");
    static_assert(F::TEAM < 0 || (F::TEAM <= 1 && F::REG && F::NW == 1 && !F::TRACE && !F::OPTS && F::SPLIT == 0), "the team form is the plain one-correspondence-per-lane solve");
    return true;
}

// store / handoff / start_override (the chained launch, lc_pnp.hip): store = false keeps the job's outputs in registers (a workgroup that
// repeats a solve another workgroup owns must not write the owner's rows a second time); handoff (7 floats of LDS) receives the state the
// solve would leave in p.states[b]; start_override replaces the start pose (7 floats, e.g. a previous solve's handoff).
// `lane`: the thread index within the workgroup (TeamWave: within the wave); sx: SplitPart / SplitRescue only.
template <class F>
__device__ __forceinline__ void solve_pose(const PnpParams& p, int b, int lane, double* bc, bool store = true, float* handoff = nullptr,
                                           const float* start_override = nullptr, [[maybe_unused]] SplitSum* sx = nullptr) {
    constexpr int NW = F::NW, PPT = F::PPT, SPLIT = F::SPLIT, TEAM = F::TEAM;
    constexpr bool REG = F::REG, OPTS = F::OPTS, TRACE = F::TRACE, TAIL = F::TAIL;
    static_assert(form_is_legal<F>());
    static_assert(NW == 4 || REG, "one wave has one correspondence per lane");
    constexpr int kThreads = kWave * NW;
    const int slot = SPLIT == 1 ? lane + kThreads * sx->part : lane;  // first correspondence of this thread, and the distance to its next
    const int stride = SPLIT == 1 ? kThreads * sx->G : kThreads;
#ifdef LC_TRACE_CLOCK
    const unsigned long long t_start_ = __builtin_amdgcn_s_memtime();
#endif
    LC_PSTAMP_DECL;
    LC_PSTAMP_BEGIN();
    const int n = p.counts ? p.counts[b] : p.Nmax;
    // pose_mod (OPTS launches): K and start hold pose_mod rows shared by the poses b, b + pose_mod, ... (several solves of the same
    // objects -- different correspondence selections -- batched into one launch)
    const int bk = (OPTS && p.pose_mod > 0) ? b % p.pose_mod : b;
    const float* st_in = start_override ? start_override : (p.start ? p.start + 7 * (size_t)bk : p.states + 7 * (size_t)b);
    const bool filter = OPTS && (p.options & kPnpNanToNum);
    auto fin = [&](float f) { return filter ? nan_to_num(f) : f; };
    if (n < 3) {  // ceres.cpp:84-91
        if (lane == 0 && store) {
            p.rets[b] = 1;
            p.result_tr[b] = 1.f;
            if (p.iters) p.iters[b] = 0;
        }
        if (lane < 7) {
            const float v = fin(st_in[lane]);
            if (store && (p.start || start_override || filter)) p.states[7 * (size_t)b + lane] = v;
            if (handoff) handoff[lane] = v;
        }
        return;
    }
    const size_t base = (size_t)b * p.Nmax;
    const bool active = lane < n;
    RawPoint raw;
    if constexpr (REG) raw = load_raw_point<OPTS>(p, base, active ? lane : 0);  // n >= 3 here: correspondence 0 exists
    [[maybe_unused]] RawPoint rawc[PPT > 0 ? PPT : 1];
    if constexpr (!REG && PPT > 0) {
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (slot + k * stride < n) rawc[k] = load_raw_point<OPTS>(p, base, slot + k * stride);
    }
    double cam[6];
    {
        const float* Kp = p.K + 9 * (size_t)bk;
#pragma unroll
        for (int i = 0; i < 6; ++i) cam[i] = fin(Kp[i]);  // only the first 6 floats are read (ceres.cpp:99-101)
    }
    double x[6];
    {
        // QuaternionToAngleAxis (ceres.cpp:96)
        // q0 is only used inside `if (s2 > 0)`, and the compiler sinks its LOAD in there: a second memory round trip after the one that
        // brought q1..q3 of the same cache line (seen in the ISA of the pose unit: global_load of start[0] behind the first s_waitcnt).  The
        // empty asm is a use of the seven loaded values in the straight-line code: their loads are issued with the others (with q0 alone
        // pinned, the compiler moved q1..q3 behind the wait instead).
        float stf[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) stf[i] = st_in[i];
        asm volatile("" : "+v"(stf[0]), "+v"(stf[1]), "+v"(stf[2]), "+v"(stf[3]), "+v"(stf[4]), "+v"(stf[5]), "+v"(stf[6]));
        const double q0 = fin(stf[0]), q1 = fin(stf[1]), q2 = fin(stf[2]), q3 = fin(stf[3]);
        const double s2 = q1 * q1 + q2 * q2 + q3 * q3;
        double kk = 2.0;
        if (s2 > 0.0) {
            const double s = fast_sqrt(s2);
            // ceres/rotation.h: 2 atan2(s, c) with c >= 0, or 2 atan2(-s, -c) with c < 0: both are +-2 atan(s / |c|), s > 0
            const double half = atan_ratio_pos(s, fabs(q0));
            const double two_theta = 2.0 * ((q0 < 0.0) ? -half : half);
            kk = two_theta / s;
        }
        x[0] = q1 * kk; x[1] = q2 * kk; x[2] = q3 * kk;
        x[3] = fin(stf[4]); x[4] = fin(stf[5]); x[5] = fin(stf[6]);
    }
    LC_PSTAMP(0);
    // Lanes without a correspondence (lane >= n) carry a copy of correspondence 0 with a ZERO information factor: their residuals
    // and Jacobian rows are exact zeros, so they add nothing to the sums and need no masking in the evaluation (56 selects per
    // evaluation before); their projection is finite exactly when correspondence 0's is, and a non-finite correspondence fails the
    // job either way (ceres.cpp:126-138 -> invalid).
    Point rp;
    if constexpr (REG) {
        rp = to_point(raw, cam);
        if (!active) { rp.a = 0.0; rp.b = 0.0; rp.c = 0.0; }
    }

    [[maybe_unused]] int sum_phase = 0;  // block_sum_waves4 / block_sum_split / block_sum_team2: which of its two rows of totals the next sum writes
    // full evaluation at xe with column scaling sc: H = Js^T Js (21), g = Js^T r (6), cost; false when anything is non-finite
    auto evaluate = [&](const double (&xe)[6], const double (&sc)[6], double (&H)[21], double (&g)[6], double& cost) -> bool {
        LC_PSTAMP(1);
        Rot rt;
        make_rot(xe, rt);
        LC_PSTAMP(2);
        const double t[3] = {xe[3], xe[4], xe[5]};
        double acc[28];
        if constexpr (NW == 1 && TEAM < 0) {
            // form 1.  Lanes beyond n hold zero-weight copies (exact zeros); the 28 partial sums go to LDS as they are produced
            const int pos = block_sum_open(lane);
            accumulate_point<true, true>(rp, rt, t, cam, sc, acc, bc, pos);
            LC_PSTAMP(3);
            block_sum_close<28>(acc, bc, lane);
        } else if constexpr (NW == 1) {
#if LC_PNP_TEAM_REGSUM
            // form 2.  This wave's half of the 28 partial sums stays in registers and is summed there; the sibling wave forms the other half
            accumulate_point<true, false, TEAM>(rp, rt, t, cam, sc, acc);
            LC_PSTAMP(3);
            block_sum_team2_reg<28, TEAM>(acc, bc, lane, sum_phase);
#else
            // form 2.  This wave's half of the 28 partial sums goes to LDS as it is produced; the sibling wave forms the other half
            const int pos = block_sum_open(lane);
            accumulate_point<true, true, TEAM>(rp, rt, t, cam, sc, acc, bc, pos);
            LC_PSTAMP(3);
            block_sum_team2<28, TEAM>(acc, bc, lane, sum_phase);
#endif
        } else if constexpr (REG) {
            // form 3.  The register block sum here too: 12.4 -> 11.6 us at 64 x 256 against sums streamed through LDS
            accumulate_point<true>(rp, rt, t, cam, sc, acc);
            LC_PSTAMP(3);
            block_sum_waves4<28>(acc, bc, lane, sum_phase);
        } else {
            // form 4
#pragma unroll
            for (int i = 0; i < 28; ++i) acc[i] = 0;
            if constexpr (PPT > 0) {
#pragma unroll
                for (int k = 0; k < PPT; ++k)
                    if (slot + k * stride < n) accumulate_point<false>(to_point(rawc[k], cam), rt, t, cam, sc, acc);
                // rows wider than the cached prefix (Nmax > 256 PPT): the correspondences behind it from memory, in the same per-thread
                // order as the plain loop below -- same sums bit for bit; empty when the pose's count fits the prefix
                if constexpr (TAIL)
                    for (int i = slot + PPT * stride; i < n; i += stride) accumulate_point<false>(load_point<OPTS>(p, base, i, cam), rt, t, cam, sc, acc);
            } else if constexpr (SPLIT == 2) {
                for (int g = 0; g < sx->G; ++g) {  // part g's share and its totals; the last call adds the parts in order
                    if (g > 0) {
#pragma unroll
                        for (int i = 0; i < 28; ++i) acc[i] = 0;
                    }
                    for (int i = lane + kThreads * g; i < n; i += kThreads * sx->G) accumulate_point<false>(load_point<OPTS>(p, base, i, cam), rt, t, cam, sc, acc);
                    block_sum_parts_serial<28>(acc, bc, lane, g, sx->G);
                }
            } else {
                for (int i = lane; i < n; i += kThreads) accumulate_point<false>(load_point<OPTS>(p, base, i, cam), rt, t, cam, sc, acc);
            }
            LC_PSTAMP(3);
            if constexpr (SPLIT == 2) {}
            else if constexpr (SPLIT == 1) block_sum_split<28>(acc, bc, lane, sum_phase, *sx);
            else block_sum_waves4<28>(acc, bc, lane, sum_phase);
        }
        LC_PSTAMP(4);
#pragma unroll
        for (int i = 0; i < 21; ++i) H[i] = acc[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = acc[21 + i];
        const double ss = acc[27];
        cost = 0.5 * ss;
        double chk = ss;  // every term is >= 0: the sum is finite iff all residuals and Jacobian entries are
#pragma unroll
        for (int i = 0; i < 6; ++i) chk += H[tri6(i, i)];
        LC_PSTAMP(5);
        if constexpr (SPLIT == 1) {
            if (sx->timed_out) return false;  // a workgroup of this pose never arrived: this launch gives the pose up (lc_common.h: SplitSum)
        }
        return chk <= DBL_MAX;
    };

    const double ftol = p.ftol, ptol = 1e-8, gtol = 1e-10;
    double H[21], g[6], cost;  // of the Jacobi-scaled problem from here on
    double scale[6], iscale[6];
    bool failed;
    {
        const double one[6] = {1, 1, 1, 1, 1, 1};
        failed = !evaluate(x, one, H, g, cost);
#pragma unroll
        for (int j = 0; j < 6; ++j) {  // Jacobi scaling 1/(1+||J_j||), fixed at iteration 0
            iscale[j] = 1.0 + fast_sqrt(H[tri6(j, j)]);  // 4e-15 relative (lc_common.h); the libm sqrt costs ~100 cycles x 6 on the start-up path
            scale[j] = fast_rcp(iscale[j]);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) H[tri6(i, j)] *= scale[i] * scale[j];
            g[i] *= scale[i];
        }
    }
    auto grad_max = [&](const double (&gs)[6]) {  // max-norm of the UNSCALED gradient J^T r
        double m = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) m = fmax(m, fabs(gs[j]) * iscale[j]);
        return m;
    };
    double gmax = grad_max(g);
    auto sqnorm6 = [](const double (&v)[6]) {
        double m = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) m += v[j] * v[j];
        return m;
    };
    double xn2 = sqnorm6(x);  // ||x||^2; the norm itself is only formed when the parameter-tolerance test is in reach
    double radius = 1e4, dfac = 2.0;
    int iter = 0, n_invalid = 0;
    bool converged = false;
    // kind: 0 invalid step, 1 accepted, 2 rejected, 3 parameter tolerance, 4 function tolerance
    auto trace = [&](int kind, double cost_x, double cost_cand, double mcc, double rho, double step_norm) {
        if constexpr (TRACE) {
            if (lane == 0 && p.trace && iter <= p.trace_rows) {
                double* row = p.trace + ((size_t)b * p.trace_rows + (iter - 1)) * 8;
                row[0] = kind; row[1] = cost_x; row[2] = cost_cand; row[3] = mcc; row[4] = rho; row[5] = step_norm;
                row[6] = radius; row[7] = gmax;
#ifdef LC_TRACE_CLOCK  // timing diagnostics only (scripts/ubench/pnp_iter_clock.py): shader cycles since the wave started
                row[7] = (double)(__builtin_amdgcn_s_memtime() - t_start_);
#endif
            }
        }
    };

    // `failed` and `converged` are only ever set on the way out (each assignment below is followed by its break): the loop is entered once
    // the first evaluation is known to be finite and left by a break -- no ballot over two flags at the head of every iteration.  The
    // exits are marked unlikely so that an accepted step runs as straight-line code and the others leave it by a taken branch.
    if (!uniform(failed)) for (;;) {
        // FinalizeIterationAndCheckIfMinimizerCanContinue
        if (__builtin_expect(iter >= p.max_iter, 0)) break;
        if (__builtin_expect(uniform(gmax <= gtol || radius <= 1e-32), 0)) { converged = true; break; }
        ++iter;
        // LevenbergMarquardtStrategy::ComputeStep on the Jacobi-scaled system
        double dg[6], y[6];
        const double inv_radius = fast_rcp(radius);
#pragma unroll
        for (int i = 0; i < 6; ++i) dg[i] = clamp_diag(H[tri6(i, i)]) * inv_radius;
        LC_PSTAMP(1);
        bool step_ok = ldlt_solve6<F::PIVOTS_RUNNING>(H, dg, g, y);
        LC_PSTAMP(6);
        // model_cost_change = y.g - y^T H y / 2 with (H + D) y = g  =>  (y.g + sum d_i y_i^2) / 2   (step = -y)
        double mcc = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) mcc += y[i] * (g[i] + dg[i] * y[i]);
        mcc *= 0.5;
        step_ok = step_ok && (mcc > 0.0) && (mcc <= DBL_MAX);  // a non-finite y makes mcc non-finite
        if (__builtin_expect(uniform(!step_ok), 0)) {  // HandleInvalidStep
            if (++n_invalid >= 5) { failed = true; trace(0, cost, 0.0, mcc, 0.0, 0.0); break; }
            radius /= dfac; dfac *= 2.0;
            trace(0, cost, 0.0, mcc, 0.0, 0.0);
            continue;
        }
        n_invalid = 0;
        double xc[6], delta[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) { delta[j] = -y[j] * scale[j]; xc[j] = x[j] + delta[j]; }
        // ParameterToleranceReached is  ||delta|| <= ptol (||x|| + ptol).  Since (a + b)^2 <= 2 (a^2 + b^2), a step with
        // ||delta||^2 > 2 ptol^2 (||x||^2 + ptol^2) cannot pass: two square roots per iteration are only taken next to convergence
        // (and by the diagnostic twin, which records the step norm).
        const double sn2 = sqnorm6(delta);
        const bool ptol_in_reach = TRACE || uniform(!(sn2 > 2.0 * ptol * ptol * (xn2 + ptol * ptol)));
        double step_norm = 0.0;
        bool ptol_hit = false;
        if (__builtin_expect(ptol_in_reach, 0)) {  // scalar branch
            step_norm = fast_sqrt(sn2);
            ptol_hit = uniform(step_norm <= ptol * (fast_sqrt(xn2) + ptol));
        }
        // the candidate's H, g overwrite the current ones (an accepted step then needs no copy and no second Jacobian);
        // a rejected step -- rare -- restores them by re-evaluating at x
        double cost_c;
        const bool cand_ok = evaluate(xc, scale, H, g, cost_c);
        if constexpr (SPLIT == 1) {
            if (sx->timed_out) { failed = true; break; }
        }
        if (!cand_ok) cost_c = DBL_MAX;
        if (__builtin_expect(ptol_hit, 0)) {  // ParameterToleranceReached
            converged = true; trace(3, cost, cost_c, mcc, 0.0, step_norm); break;
        }
        const double cost_change = cost - cost_c;
        if (__builtin_expect(uniform(fabs(cost_change) <= ftol * cost), 0)) {    // FunctionToleranceReached
            converged = true; trace(4, cost, cost_c, mcc, cost_change * fast_rcp(mcc), step_norm); break;
        }
        const double rel = cost_change * fast_rcp(mcc);
        if (__builtin_expect(uniform(rel > 1e-3), 1)) {  // HandleSuccessfulStep
#pragma unroll
            for (int j = 0; j < 6; ++j) x[j] = xc[j];
            const double cost_prev = cost;
            cost = cost_c;
            xn2 = sqnorm6(x);
            gmax = grad_max(g);
            const double tq = 2.0 * rel - 1.0;
            radius = fmin(1e16, radius * fast_rcp(fmax(1.0 / 3.0, 1.0 - tq * tq * tq)));
            dfac = 2.0;
            trace(1, cost_prev, cost_c, mcc, rel, step_norm);
        } else {
            radius /= dfac; dfac *= 2.0;
            trace(2, cost, cost_c, mcc, rel, step_norm);
            double cost_again;
            if (uniform(!evaluate(x, scale, H, g, cost_again))) { failed = true; break; }  // (a ballot like every other exit: one per-lane exit makes the compiler route ALL of them through a flag at the loop's end)
        }
    }
    LC_PSTAMP(1);
#ifdef LC_STAMPS
    if (lane == 0 && store && p.iters) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(p.iters) + 8 * (size_t)b;
        for (int i = 0; i < 6; ++i) o[i] = pst_[i];
        o[6] = iter;
        o[7] = pst_[6];  // LDL^T solve alone (the rest of the LM algebra is in slot 1)
    }
#endif
    const bool invalid = failed || !converged;
    if (invalid && lane < 7) {
        const float v = fin(st_in[lane]);
        if (store && (p.start || start_override || filter)) p.states[7 * (size_t)b + lane] = v;
        if (handoff) handoff[lane] = v;
    }
    if (lane == 0) {
        if (store) {
            p.rets[b] = invalid ? 1 : 0;
            if constexpr (SPLIT == 1) {
                if (sx->timed_out) p.rets[b] = kPnpPartNeverArrived;  // never leaves the launch pair: the rescue launch re-solves the pose
            }
            p.result_tr[b] = (float)radius;
#ifndef LC_STAMPS
            if (p.iters) p.iters[b] = iter;
#endif
        }
        if (!invalid) {  // ceres.cpp:131-144: AngleAxisToQuaternion, write back in place
            float stq[7];
            float* st = stq;
            const double t2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
            double q0 = 1.0, kk = 0.5;
            if (t2 > 0.0) {
                const double th = fast_sqrt(t2), h = 0.5 * th;
                double sh, ch;
                sincos_small(h, sh, ch);  // < 1 ulp on the reduced interval, like the libm call it replaces
                q0 = ch;
                kk = sh / th;
            }
            st[0] = (float)q0; st[1] = (float)(x[0] * kk); st[2] = (float)(x[1] * kk); st[3] = (float)(x[2] * kk);
            st[4] = (float)x[3]; st[5] = (float)x[4]; st[6] = (float)x[5];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                if (store) p.states[7 * (size_t)b + k] = stq[k];
                if (handoff) handoff[k] = stq[k];
            }
        }
    }
}

}  // namespace pnp
}  // namespace lc
