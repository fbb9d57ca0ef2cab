// Test-time pose covariance and predicted error, one launch (liblc_amd_posecov.so, C ABI in include/lc_amd_posecov.h).
//
// What the reference computes with functorch jacfwd + vmap over every correspondence, a batched Cholesky and an autograd loop over
// the box corners (lib/nll/pnp_auto.py:86-108 diff_pnp_perturb(with_cov=True), lib/cov_mixed.py:52-97 jac_update2alter,
// transformed_cov_from_jac, loss_cov_3d / loss_cov_2d), in closed form (the same algebra as lc_loss_body.h's pass 3 and serial section,
// with a MEASURED u: r != 0, and no z-clamp on the correspondences because residual_with_jac6d has none):
//
//   one workgroup per row; wave w walks the tiles w, w + NW, ... of 64 consecutive points; a lane forms the 21 upper-triangle entries of
//   its point's  sum_c w_c (J_c^T J_c + r_c Hess r_c)  in fp64; a tile is reduced by one fixed cross-lane tree (permlane swaps + DPP, no
//   LDS) and its partial row goes to LDS; 21 lanes add the rows in tile order.  Dead lanes (at or beyond counts[b]) contribute exact
//   zeros and are never loaded.  Hence the same bits for every workgroup width, batch size, row position and padding content.
//   Wave 0 then holds the 6x6 matrix one entry per lane: Gauss-Jordan sweeps whose pivots are the squared Cholesky diagonal (the SPD
//   test of safe_cholesky), the inverse, 24 / 16 lanes with one box-corner Jacobian row each, the mean.
//
// The in-tile tree is lc::wave_reduce_scatter16<32> of ../shared/lc_shared.h, the one copy the hot-path library's sums use as well
// (with tri6, shfl_f64, nan_to_num and quat_matrix); nothing else of lc_amd/csrc is included.  The library's source hash covers this
// directory, its header and that shared header (lc_amd/build.py: POSECOV.shared).
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/lc_amd_posecov.h"
#include "../shared/lc_shared.h"

#ifndef LC_AMD_POSECOV_SRC_HASH
#define LC_AMD_POSECOV_SRC_HASH "unrecorded"
#endif

namespace {

using namespace lc;

const char kSrcHash[] = "LC_AMD_POSECOV_SRC_HASH:" LC_AMD_POSECOV_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kTile = 64;  // the canonical tile: 64 consecutive correspondences
constexpr int kRow = 22;   // doubles per tile partial in LDS (21 sums + 1 pad: the lanes store pairs)
constexpr int kFixed = 24 + 36 + 24 + 2;  // LDS behind the tile rows: H totals | cov | var | flags

struct Params {
    const float* K;
    const float* pose;
    const float* pts3d;
    const float* pts2d;
    const float* weights;
    const int* counts;
    const float* bbox;
    const float* diameter;
    float* cov;
    float* var;
    float* perr;
    int* info;
    int N, options, object_rows, pose_rows;
};

struct PoseConst {
    double K[9];
    double R[9];   // the matrix the reference uses (two_s = 2/|q|, rotation_conversions.py:52)
    double Rt[9];  // proper rotation of the normalised quaternion
    double rho;
    double t[3];
};

// One correspondence: acc[tri6(i, j)] = sum_c w_c (J_c[i] J_c[j] + r_c Hess(r_c)[i][j]), i <= j.
// residual_with_jac6d (pnp_auto.py:13-56) at delta = 0 and the jacfwd of r * dr (pnp_auto.py:59-83) in closed form: the truncated
// rotation expansion of pnp_utils.py:52-78 is second-order consistent at 0, so its second derivative is -X d_il + (e_i X_l + e_l X_i)/2.
__device__ __forceinline__ void point_hessian(const PoseConst& pc, const double X[3], const double u[2], const double w[2], double (&acc)[32]) {
    double Xc[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) Xc[d] = pc.R[3 * d] * X[0] + pc.R[3 * d + 1] * X[1] + pc.R[3 * d + 2] * X[2] + pc.t[d];
    const double iz = 1.0 / Xc[2], x0 = Xc[0] * iz, y0 = Xc[1] * iz;
    double M0[9];  // -R [X]x
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double r0 = pc.R[3 * d], r1 = pc.R[3 * d + 1], r2 = pc.R[3 * d + 2];
        M0[3 * d + 0] = -r1 * X[2] + r2 * X[1];
        M0[3 * d + 1] = r0 * X[2] - r2 * X[0];
        M0[3 * d + 2] = -r0 * X[1] + r1 * X[0];
    }
    double Ju[2][6];  // d uv0 / d delta = iz (T_a - uv0_a T_2), T = [M0 | I]
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        Ju[0][l] = iz * (M0[l] - x0 * M0[6 + l]);
        Ju[1][l] = iz * (M0[3 + l] - y0 * M0[6 + l]);
    }
    Ju[0][3] = iz; Ju[0][4] = 0; Ju[0][5] = -iz * x0;
    Ju[1][3] = 0; Ju[1][4] = iz; Ju[1][5] = -iz * y0;
    double J[2][6], r[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double k0 = pc.K[3 * c], k1 = pc.K[3 * c + 1];  // uv = uv0 K[:2,:2]^T + K[:2,2]
#pragma unroll
        for (int l = 0; l < 6; ++l) J[c][l] = k0 * Ju[0][l] + k1 * Ju[1][l];
        r[c] = k0 * x0 + k1 * y0 + pc.K[3 * c + 2] - u[c];
    }
    // second-order part  sum_c w_c r_c Hess(r_c)
    const double rho0 = pc.K[0] * w[0] * r[0] + pc.K[3] * w[1] * r[1];
    const double rho1 = pc.K[1] * w[0] * r[0] + pc.K[4] * w[1] * r[1];
    const double iz2 = iz * iz;
    const double qv[3] = {-rho0 * iz2, -rho1 * iz2, (rho0 * x0 + rho1 * y0) * iz2};
    double tq[6], t2[6];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        tq[l] = M0[l] * qv[0] + M0[3 + l] * qv[1] + M0[6 + l] * qv[2];
        tq[3 + l] = qv[l];
        t2[l] = M0[6 + l];
        t2[3 + l] = l == 2 ? 1.0 : 0.0;
    }
    const double pv[3] = {iz * rho0, iz * rho1, -iz * (rho0 * x0 + rho1 * y0)};
    double pi[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) pi[l] = pc.R[l] * pv[0] + pc.R[3 + l] * pv[1] + pc.R[6 + l] * pv[2];
    const double piX = pi[0] * X[0] + pi[1] * X[1] + pi[2] * X[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double wj0 = w[0] * J[0][i], wj1 = w[1] * J[1][i];
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double h = t2[i] * tq[j] + tq[i] * t2[j];  // compile-time zeros of t2 fold away
            if (i < 3 && j < 3) h += 0.5 * (pi[i] * X[j] + X[i] * pi[j]) - (i == j ? piX : 0.0);
            acc[tri6(i, j)] = __builtin_fma(wj1, J[1][j], __builtin_fma(wj0, J[0][j], h));
        }
    }
}

// NW wavefronts per row: 1 for rows of one tile (N <= 64), 4 otherwise.  Dynamic LDS: ceil(N/64) tile rows + kFixed doubles.
template <int NW>
__global__ __launch_bounds__(kWave* NW) void lc_pose_cov_kernel(const Params p) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N;
    const int Tmax = (N + kTile - 1) / kTile;
    double* part = lds;                 // [Tmax][kRow]
    double* Htot = lds + (size_t)Tmax * kRow;  // 24
    double* S = Htot + 24;              // 36
    double* varl = S + 36;              // 24
    int n = p.counts ? p.counts[b] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    const int T = (n + kTile - 1) / kTile;
    const bool filter = (p.options & LC_POSE_COV_NAN_TO_NUM) != 0;
    const bool as_std = (p.options & LC_POSE_COV_WEIGHTS_ARE_STD) != 0;
    const bool scalar_w = (p.options & LC_POSE_COV_SCALAR_WEIGHTS) != 0;
    const bool cov2d = (p.options & LC_POSE_COV_2D) != 0;
    const int bo = b % p.object_rows, bp = b % p.pose_rows;
    auto fin = [&](float f) { return filter ? nan_to_num(f) : f; };

    PoseConst pc;
    {
        const float* Kp = p.K + 9 * (size_t)bo;
        const float* ps = p.pose + 7 * (size_t)bp;
#pragma unroll
        for (int i = 0; i < 9; ++i) pc.K[i] = fin(Kp[i]);
        const double q[4] = {fin(ps[0]), fin(ps[1]), fin(ps[2]), fin(ps[3])};
        pc.rho = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double irho = 1.0 / pc.rho;
        quat_matrix(q, 2.0 * irho, pc.R);
        quat_matrix(q, 2.0 * irho * irho, pc.Rt);
#pragma unroll
        for (int d = 0; d < 3; ++d) pc.t[d] = fin(ps[4 + d]);
    }

    const size_t base = (size_t)b * N;
    for (int t = wave; t < T; t += NW) {
        const int i = t * kTile + lane;
        double acc[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) acc[k] = 0.0;
        if (i < n) {
            const float* Xp = p.pts3d + (base + i) * 3;
            const float2 uf = *reinterpret_cast<const float2*>(p.pts2d + (base + i) * 2);
            float w0, w1;
            if (scalar_w) {
                w0 = w1 = p.weights[base + i];
            } else {
                const float2 wf = *reinterpret_cast<const float2*>(p.weights + (base + i) * 2);
                w0 = wf.x; w1 = wf.y;
            }
            if (as_std) { w0 = 1.f / (w0 * w0); w1 = 1.f / (w1 * w1); }  // the sparse head's deviations -> inverse variances (test.py:52), fp32 like the solver's load
            const double X[3] = {fin(Xp[0]), fin(Xp[1]), fin(Xp[2])};
            const double u[2] = {fin(uf.x), fin(uf.y)};
            const double w[2] = {fin(w0), fin(w1)};
            point_hessian(pc, X, u, w, acc);
        }
        wave_reduce_scatter16<32>(acc, lane);  // the in-tile tree: every lane of a quad ends with the sums base, base + 1 in acc[0], acc[1]
        const int bs = scatter16_base(lane, 2);
        if ((lane & 3) == 0 && bs < kRow) {
            part[t * kRow + bs] = acc[0];
            part[t * kRow + bs + 1] = acc[1];
        }
    }
    __syncthreads();
    if (tid < 21) {  // tile partials in tile order
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += part[t * kRow + tid];
        Htot[tid] = s;
    }
    __syncthreads();

    // ---- 6x6 section on wave 0: one matrix entry per lane (lanes >= 36 shadow lanes 0..27) ----
    const int mi = (lane % 36) / 6, mj = lane % 6;
    bool ok = true;
    if (wave == 0) {
        double cur = Htot[mi <= mj ? tri6(mi, mj) : tri6(mj, mi)];
        ok = __all(isfinite(cur) ? 1 : 0) != 0;
#pragma unroll
        for (int pz = 0; pz < 6; ++pz) {
            const double piv = shfl_f64(cur, 7 * pz);
            const double rowv = shfl_f64(cur, 6 * pz + mj);
            const double colv = shfl_f64(cur, 6 * mi + pz);
            ok = ok && (piv > 0) && isfinite(piv);  // the pivots are the squared Cholesky diagonal: safe_cholesky's test (pnp_utils.py:140-167)
            const double ip = 1.0 / piv;
            const double tt = rowv * ip;
            double out = cur - colv * tt;
            if (mj == pz) out = -colv * ip;
            if (mi == pz) out = (mj == pz) ? ip : tt;
            cur = out;
        }
        if (!ok) cur = (mi == mj) ? 1.0 : 0.0;  // make_sure_SPD: H := I
        if (lane < 36) {
            S[lane] = cur;
            p.cov[36 * (size_t)b + lane] = (float)cur;
        }
        if (lane == 0) p.info[b] = ok ? 0 : 1;
    }
    __syncthreads();

    // ---- one lane per row of the box-corner Jacobian (jac_update2alter, cov_mixed.py:52-65): var = g^T cov g ----
    const int gdim = cov2d ? 2 : 3, rows = 8 * gdim;
    double v = 0.0;
    bool good = true;
    if (wave == 0) {
        if (lane < rows) {
            const int k = lane / gdim, d = lane - k * gdim;
            const float* bb = p.bbox + ((size_t)bo * 8 + k) * 3;
            const double bbx = bb[0], bby = bb[1], bbz = bb[2];
            double g[6];
            if (!cov2d) {  // xform_3d: g = [ -rho (Rt[d,:] x b) | e_d ]
                const double r0 = d == 0 ? pc.Rt[0] : (d == 1 ? pc.Rt[3] : pc.Rt[6]);
                const double r1 = d == 0 ? pc.Rt[1] : (d == 1 ? pc.Rt[4] : pc.Rt[7]);
                const double r2 = d == 0 ? pc.Rt[2] : (d == 1 ? pc.Rt[5] : pc.Rt[8]);
                g[0] = -pc.rho * (r1 * bbz - r2 * bby);
                g[1] = -pc.rho * (r2 * bbx - r0 * bbz);
                g[2] = -pc.rho * (r0 * bby - r1 * bbx);
                g[3] = d == 0 ? 1.0 : 0.0; g[4] = d == 1 ? 1.0 : 0.0; g[5] = d == 2 ? 1.0 : 0.0;
            } else {  // xform_2d: project_apply of the corner (full K, z clamped at 0.1: transforms.py:47-63), chained with the 3D rows
                double Xc[3], xf[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) Xc[e] = pc.R[3 * e] * bbx + pc.R[3 * e + 1] * bby + pc.R[3 * e + 2] * bbz + pc.t[e];
#pragma unroll
                for (int e = 0; e < 3; ++e) xf[e] = pc.K[3 * e] * Xc[0] + pc.K[3 * e + 1] * Xc[1] + pc.K[3 * e + 2] * Xc[2];
                const double zpass = xf[2] >= 0.1 ? 1.0 : 0.0;
                const double zc = xf[2] >= 0.1 ? xf[2] : 0.1;
                const double izc = 1.0 / zc;
                const double proj = (d == 0 ? xf[0] : xf[1]) * izc;
                double pa[3];  // d proj_d / d Xc = (K[d,:] - zpass proj_d K[2,:]) / zc
#pragma unroll
                for (int l = 0; l < 3; ++l) pa[l] = ((d == 0 ? pc.K[l] : pc.K[3 + l]) - zpass * proj * pc.K[6 + l]) * izc;
                const double v0 = pa[0] * pc.Rt[0] + pa[1] * pc.Rt[3] + pa[2] * pc.Rt[6];
                const double v1 = pa[0] * pc.Rt[1] + pa[1] * pc.Rt[4] + pa[2] * pc.Rt[7];
                const double v2 = pa[0] * pc.Rt[2] + pa[1] * pc.Rt[5] + pa[2] * pc.Rt[8];
                g[0] = -pc.rho * (v1 * bbz - v2 * bby);
                g[1] = -pc.rho * (v2 * bbx - v0 * bbz);
                g[2] = -pc.rho * (v0 * bby - v1 * bbx);
                g[3] = pa[0]; g[4] = pa[1]; g[5] = pa[2];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double a = S[6 * i] * g[0];
#pragma unroll
                for (int l = 1; l < 6; ++l) a = __builtin_fma(S[6 * i + l], g[l], a);
                v = __builtin_fma(g[i], a, v);
            }
            varl[lane] = v;
            p.var[(size_t)rows * b + lane] = (float)v;
        }
        // loss_cov_3d / loss_cov_2d (cov_mixed.py:83-97): 'good' = every variance positive, else 1 per corner
        good = __all((lane >= rows || v > 0) ? 1 : 0) != 0;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < 8; ++k) {
            double c = varl[gdim * k] + varl[gdim * k + 1];
            if (!cov2d) c += varl[gdim * k + 2];
            s += sqrt(good ? c : 1.0);
        }
        s *= 0.125;
        if (!cov2d && p.diameter) s = s / (double)p.diameter[bo];
        p.perr[b] = (float)s;
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_posecov_version(void) { return LC_AMD_POSECOV_VERSION; }
const char* lc_amd_posecov_source_hash(void) { return kSrcHash + sizeof("LC_AMD_POSECOV_SRC_HASH:") - 1; }
const char* lc_amd_posecov_last_error(void) { return g_err.c_str(); }

int lc_pose_cov_f32(const float* K, const float* pose, const float* pts3d, const float* pts2d, const float* weights, const int* counts,
                    const float* bbox_3d, const float* diameter, int B, int N, int options, int object_rows, int pose_rows, float* cov,
                    float* var, float* pred_err, int* info, void* stream) {
    if (B < 0) return fail(1, "lc_pose_cov_f32: B < 0");
    if (B == 0) return 0;
    if (N < 1 || N > LC_POSE_COV_MAX_POINTS) return fail(2, "lc_pose_cov_f32: N must be in [1, " + std::to_string(LC_POSE_COV_MAX_POINTS) + "], got " + std::to_string(N));
    if (!K || !pose || !pts3d || !pts2d || !weights || !bbox_3d) return fail(3, "lc_pose_cov_f32: K, pose, pts3d, pts2d, weights and bbox_3d must not be NULL");
    if (!cov || !var || !pred_err || !info) return fail(4, "lc_pose_cov_f32: cov, var, pred_err and info must not be NULL");
    if (object_rows < 1 || B % object_rows || pose_rows < 1 || B % pose_rows) return fail(5, "lc_pose_cov_f32: object_rows and pose_rows must be positive divisors of B");
    if (options & ~(LC_POSE_COV_NAN_TO_NUM | LC_POSE_COV_WEIGHTS_ARE_STD | LC_POSE_COV_SCALAR_WEIGHTS | LC_POSE_COV_2D)) return fail(6, "lc_pose_cov_f32: unknown option bits");
    const Params p{K, pose, pts3d, pts2d, weights, counts, bbox_3d, diameter, cov, var, pred_err, info, N, options, object_rows, pose_rows};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = (N + kTile - 1) / kTile;
    const size_t lds = ((size_t)T * kRow + kFixed) * sizeof(double);  // <= 45.7 KB
    if (N <= kTile) hipLaunchKernelGGL(lc_pose_cov_kernel<1>, dim3(B), dim3(kWave), lds, s, p);
    else hipLaunchKernelGGL(lc_pose_cov_kernel<4>, dim3(B), dim3(4 * kWave), lds, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(10, std::string("lc_pose_cov_f32: launch: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
