// Symmetry-aware pose errors on the GPU: MSSD, MSPD (lib/utils/error6d.py:36-84) and the projection error proj (:157-172) of a batch of
// (estimate, ground truth) pairs, with each object's symmetry transforms read from the device table of lc_amd.symmetry.SymmetrySet and its
// vertices from a packed buffer (lc_amd.render.MeshSet keeps one): an object index per pose is all a launch needs.
//
//   s = (R_s, t_s):  R_gs = R_gt R_s,  t_gs = R_gt t_s + t_gt
//   mssd = min_s max_p || (R_est - R_gs) p + (t_est - t_gs) ||
//   mspd = min_s max_p || pi_est(p) - pi_gs(p) ||,  pi = rows 0, 1 of K [R | t] [p; 1] over row 2 (project_pts: no z clamp, any last row of K)
//   proj = mean_p || pi_est(p) - pi_gt(p) ||
//
// Arithmetic is fp64 on the fp32 inputs (the convention of lc_metrics.hip's ADD), every operation written out (fma, mul, add, one division
// per projection), so a (vertex, symmetry) pair goes through ONE instruction sequence wherever it is evaluated.
//
// Launch shape.  K runs from 1 to several hundred and M from a handful to 10^5, and a batch mixes them, so the grid is (pose, chunk of
// kSymErrChunk = 8 symmetries): one workgroup per pose would leave most of the device idle at B = 64 and make a K = 1 pose wait for a K = 768
// one.  In a workgroup of four wavefronts each wavefront takes one symmetry at a time (k0 + wave, k0 + wave + 4): the per-symmetry
// matrices (R_est - R_gs, t_est - t_gs, K [R_gs | t_gs]) are formed once, the lanes stride the vertices two at a time (i, i + 64: two
// independent fp64 chains per lane) and carry the running maxima of the SQUARED distances -- the correctly rounded square root is
// monotone, so one square root per symmetry after one cross-lane maximum gives the bits of the maximum of the roots.  proj is summed by the
// last wavefront of a pose's chunk 0 (idle there whenever K <= 3): every lane adds its vertices in rising order, then one fixed butterfly
// (wave_allreduce), an order that depends on the pose's own M only.
//
// Chunks meet in a small finish pass (one thread per pose), not through atomics: a chunk leaves, per error, ONE 64-bit key
// (fp32 bits of the error << 32 | k).  The errors are non-negative, so keys order as (error, k): the minimum key is the least error
// ROUNDED TO FP32 and, among the symmetries that share it, the lowest k.  min and max do not round, so err and arg do not depend on B, on
// the order or mix of objects, on the chunking, or on what else is in the launch.  No state lives in the workspace between calls; there is
// no host synchronisation and no allocation: the two launches can sit in a hipGraph.
//
// Non-finite intermediate values (a vertex on the camera plane, non-finite inputs) are not specified: the hardware maximum drops a NaN.
//
// A library of its own (liblc_amd_symerr.so, C ABI in include/lc_amd_symerr.h): the argument rules are lc_sym_metrics_args.h next to this
// file and sym_table_error of ../lc_sym_args.h, the cross-lane moves are ../shared/lc_shared.h (both named in the target's `shared` list).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_symerr.h"
#include "../lc_sym_args.h"
#include "../shared/lc_shared.h"
#include "lc_sym_metrics_args.h"

#ifndef LC_AMD_SYMERR_SRC_HASH
#define LC_AMD_SYMERR_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_SYMERR_SRC_HASH:" LC_AMD_SYMERR_SRC_HASH;
thread_local std::string g_err;

int fail(int code, const char* msg) {
    g_err = msg;
    return code;
}

// Pose b takes the obj_k[o] transforms of its object o = obj_index[b] from the table and the vertices
// pts[pts_off[b] : pts_off[b] + pts_cnt[b]] (both null: pts[0:P]).
struct SymErrParams {
    const float* R_est;  // (B,3,3)
    const float* t_est;  // (B,3)
    const float* R_gt;   // (B,3,3)
    const float* t_gt;   // (B,3)
    const float* cam_K;  // (B,3,3), all nine entries are read
    const float* pts;    // (P,3)
    const int* pts_off;  // (B,) or null
    const int* pts_cnt;  // (B,) or null
    int P;
    const int* obj_index;    // (B,)
    const double* sym_tab;   // (sym_rows,12)
    const int* obj_off;      // (n_obj,)
    const int* obj_k;        // (n_obj,)
    int n_obj, sym_rows, max_k;
    int B;
    float* err;              // (B,3) mssd, mspd, proj
    int* arg;                // (B,2) the symmetry of mssd and of mspd, counted inside the object's own rows
    void* workspace;         // host::sym_errors_workspace_bytes(B, max_k) bytes, 8-byte aligned; no state is kept in it between calls
};

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kUnroll = 2;  // vertices per lane and loop trip: a trip covers kWave * kUnroll = 128 vertices
constexpr int kChunk = host::kSymErrChunk;
constexpr unsigned long long kNoKey = ~0ull;

// maximum over the 64 lanes, in every lane (max does not round: any order gives the same bits)
__device__ __forceinline__ double wave_max(double x) {
    x = fmax(x, dpp_mov_f64<kDppQuadXor1>(x, x));
    x = fmax(x, dpp_mov_f64<kDppQuadXor2>(x, x));
    x = fmax(x, dpp_mov_f64<kDppHalfMirror>(x, x));
    x = fmax(x, dpp_mov_f64<kDppRowMirror>(x, x));
    const int lane = threadIdx.x & (kWave - 1);
    x = fmax(x, shfl_f64(x, lane ^ 16));
    x = fmax(x, shfl_f64(x, lane ^ 32));
    return x;
}

// what pose b works on; false: refused (nothing else is read for it)
struct PoseRow {
    int K, sym_off, M, pts_off;
};
__device__ __forceinline__ bool pose_row(const SymErrParams& p, int b, PoseRow& r) {
    r.K = r.sym_off = r.M = r.pts_off = 0;
    const int o = p.obj_index[b];
    if (o < 0 || o >= p.n_obj) return false;
    const int k = p.obj_k[o], f = p.obj_off[o];
    if (k < 1 || k > p.max_k || f < 0 || (long long)f + k > p.sym_rows) return false;
    const int M = p.pts_cnt ? p.pts_cnt[b] : p.P, off = p.pts_off ? p.pts_off[b] : 0;
    if (M <= 0 || off < 0 || (long long)off + M > p.P) return false;
    r.K = k; r.sym_off = f; r.M = M; r.pts_off = off;
    return true;
}

// P = K [R | t], row-major 3 x 4
__device__ __forceinline__ void camera_rows(const double (&K)[9], const double (&R)[9], const double (&t)[3], double (&P)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P[4 * r + c] = fma(K[3 * r + 2], R[6 + c], fma(K[3 * r + 1], R[3 + c], K[3 * r] * R[c]));
        P[4 * r + 3] = fma(K[3 * r + 2], t[2], fma(K[3 * r + 1], t[1], K[3 * r] * t[0]));
    }
}

__device__ __forceinline__ void project(const double (&P)[12], double x, double y, double z, double& u, double& v) {
    const double a = fma(P[2], z, fma(P[1], y, fma(P[0], x, P[3])));
    const double b = fma(P[6], z, fma(P[5], y, fma(P[4], x, P[7])));
    const double w = fma(P[10], z, fma(P[9], y, fma(P[8], x, P[11])));
    const double iw = 1.0 / w;
    u = a * iw;
    v = b * iw;
}

// squared image distance of the two projections of a vertex
__device__ __forceinline__ double image_dist2(const double (&Pa)[12], const double (&Pb)[12], double x, double y, double z) {
    double ua, va, ub, vb;
    project(Pa, x, y, z, ua, va);
    project(Pb, x, y, z, ub, vb);
    const double du = ua - ub, dv = va - vb;
    return fma(dv, dv, du * du);
}

__device__ __forceinline__ unsigned long long error_key(double max_sq, int k) {
    return ((unsigned long long)__float_as_uint((float)sqrt(max_sq)) << 32) | (unsigned)k;
}

__device__ __forceinline__ unsigned long long* chunk_keys(const SymErrParams& p, int b, int nchunks) {
    return static_cast<unsigned long long*>(p.workspace) + (size_t)b * (2 * (size_t)nchunks + 1);
}

__global__ __launch_bounds__(kThreads) void lc_sym_pose_errors_kernel(const SymErrParams p, int nchunks) {
    __shared__ unsigned long long s_key[2][kWaves];
    const int b = blockIdx.x / nchunks, chunk = blockIdx.x - b * nchunks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    PoseRow row;
    const int k0 = chunk * kChunk;
    if (!pose_row(p, b, row) || k0 >= row.K) return;  // the whole workgroup: nothing below is reached by a part of it
    const int M = row.M;
    const float* pts = p.pts + 3 * (size_t)row.pts_off;

    double Re[9], Rg[9], Kc[9], te[3], tg[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Re[i] = p.R_est[9 * (size_t)b + i];
        Rg[i] = p.R_gt[9 * (size_t)b + i];
        Kc[i] = p.cam_K[9 * (size_t)b + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { te[i] = p.t_est[3 * (size_t)b + i]; tg[i] = p.t_gt[3 * (size_t)b + i]; }
    double Pe[12];
    camera_rows(Kc, Re, te, Pe);

    unsigned long long best3 = kNoKey, best2 = kNoKey;
    const int kend = min(row.K, k0 + kChunk);
    for (int k = k0 + wave; k < kend; k += kWaves) {
        const double* S = p.sym_tab + 12 * ((size_t)row.sym_off + k);
        double Rgs[9], tgs[3], D[9], dt[3], Pg[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Rgs[3 * i + j] = fma(Rg[3 * i + 2], S[8 + j], fma(Rg[3 * i + 1], S[4 + j], Rg[3 * i] * S[j]));
            tgs[i] = fma(Rg[3 * i + 2], S[11], fma(Rg[3 * i + 1], S[7], Rg[3 * i] * S[3])) + tg[i];
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) D[i] = Re[i] - Rgs[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) dt[i] = te[i] - tgs[i];
        camera_rows(Kc, Rgs, tgs, Pg);

        double m3 = 0.0, m2 = 0.0;  // the distances are non-negative and M >= 1
        for (int i0 = 0; i0 < M; i0 += kWave * kUnroll) {
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = i0 + u * kWave + lane;
                if (i < M) {
                    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
                    const double dx = fma(D[2], z, fma(D[1], y, fma(D[0], x, dt[0])));
                    const double dy = fma(D[5], z, fma(D[4], y, fma(D[3], x, dt[1])));
                    const double dz = fma(D[8], z, fma(D[7], y, fma(D[6], x, dt[2])));
                    m3 = fmax(m3, fma(dz, dz, fma(dy, dy, dx * dx)));
                    m2 = fmax(m2, image_dist2(Pe, Pg, x, y, z));
                }
            }
        }
        m3 = wave_max(m3);
        m2 = wave_max(m2);
        const unsigned long long key3 = error_key(m3, k), key2 = error_key(m2, k);
        best3 = key3 < best3 ? key3 : best3;
        best2 = key2 < best2 ? key2 : best2;
    }
    if (lane == 0) { s_key[0][wave] = best3; s_key[1][wave] = best2; }

    if (chunk == 0 && wave == kWaves - 1) {  // proj: no symmetry, the ground truth itself
        double Pgt[12];
        camera_rows(Kc, Rg, tg, Pgt);
        double sum[1] = {0.0};
        for (int i0 = 0; i0 < M; i0 += kWave * kUnroll) {
            double d[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = i0 + u * kWave + lane;
                d[u] = 0.0;
                if (i < M) d[u] = sqrt(image_dist2(Pe, Pgt, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]));
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) sum[0] += d[u];  // a lane's vertices in rising order (+0.0 past the end: exact)
        }
        wave_allreduce<1>(sum);
        if (lane == 0) reinterpret_cast<double*>(chunk_keys(p, b, nchunks))[2 * (size_t)nchunks] = sum[0] / M;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long best = s_key[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) best = s_key[threadIdx.x][w] < best ? s_key[threadIdx.x][w] : best;
        chunk_keys(p, b, nchunks)[2 * (size_t)chunk + threadIdx.x] = best;
    }
}

// one thread per pose: the least key over the pose's chunks, or the refusal
__global__ __launch_bounds__(kThreads) void lc_sym_pose_errors_finish_kernel(const SymErrParams p, int nchunks) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= p.B) return;
    float* err = p.err + 3 * (size_t)b;
    int* arg = p.arg + 2 * (size_t)b;
    PoseRow row;
    if (!pose_row(p, b, row)) {
        err[0] = err[1] = err[2] = __builtin_nanf("");
        arg[0] = arg[1] = -1;
        return;
    }
    const unsigned long long* keys = chunk_keys(p, b, nchunks);
    unsigned long long best3 = kNoKey, best2 = kNoKey;
    const int used = (row.K + kChunk - 1) / kChunk;
    for (int c = 0; c < used; ++c) {
        best3 = keys[2 * c] < best3 ? keys[2 * c] : best3;
        best2 = keys[2 * c + 1] < best2 ? keys[2 * c + 1] : best2;
    }
    err[0] = __uint_as_float((unsigned)(best3 >> 32));
    err[1] = __uint_as_float((unsigned)(best2 >> 32));
    err[2] = (float)reinterpret_cast<const double*>(keys)[2 * (size_t)nchunks];
    arg[0] = (int)(unsigned)best3;
    arg[1] = (int)(unsigned)best2;
}

int launch_sym_pose_errors(const SymErrParams& p, hipStream_t stream) {
    const int nchunks = (int)host::sym_errors_chunks(p.max_k);
    hipLaunchKernelGGL(lc_sym_pose_errors_kernel, dim3((unsigned)((long long)p.B * nchunks)), dim3(kThreads), 0, stream, p, nchunks);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(lc_sym_pose_errors_finish_kernel, dim3((p.B + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, p, nchunks);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_symerr_version(void) { return LC_AMD_SYMERR_VERSION; }
const char* lc_amd_symerr_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_SYMERR_SRC_HASH:") - 1; }
const char* lc_amd_symerr_last_error(void) { return lc::g_err.c_str(); }

size_t lc_sym_pose_errors_workspace_bytes(int B, int max_k) { return lc::host::sym_errors_workspace_bytes(B, max_k); }

int lc_sym_pose_errors_f32(const float* R_est, const float* t_est, const float* R_gt, const float* t_gt, const float* cam_K, const float* pts,
                           const int* pts_off, const int* pts_cnt, int P, const int* obj_index, const double* sym_tab, const int* obj_off,
                           const int* obj_k, int n_obj, int sym_rows, int max_k, int B, float* err, int* arg, void* workspace,
                           size_t workspace_bytes, void* stream) {
    using lc::fail;
    if (const char* e = lc::host::sym_errors_size_error(B, P, max_k)) return fail(1, e);
    if (B == 0) return 0;
    if (const char* e = lc::host::sym_errors_args_error(R_est, t_est, R_gt, t_gt, cam_K, pts, pts_off, pts_cnt, P, max_k, B, err, arg, workspace,
                                                        workspace_bytes))
        return fail(1, e);
    if (const char* e = lc::host::sym_table_error(R_gt, obj_index, sym_tab, obj_off, obj_k, n_obj, sym_rows)) return fail(1, e);
    lc::SymErrParams p{R_est, t_est, R_gt, t_gt, cam_K, pts, pts_off, pts_cnt, P, obj_index, sym_tab, obj_off, obj_k, n_obj, sym_rows, max_k, B,
                       err, arg, workspace};
    return lc::launch_sym_pose_errors(p, static_cast<hipStream_t>(stream)) ? fail(11, "symmetry-aware pose-error launch failed") : 0;
}

}  // extern "C"
#pragma GCC visibility pop
