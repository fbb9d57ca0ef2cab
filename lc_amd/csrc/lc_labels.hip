// On-device label preparation of a training step (losses.py:68-139 annots_on_the_fly, symmetry.py:8-56), two launches:
//
// (A) lc_sym_select_kernel: select_pose_2d / select_pose_3d for every chunk of a batch at once.  One workgroup per sample; every lane
//     keeps its check points in registers (fp32, PPL per lane) for all candidates, the waves stride over the candidates and each
//     keeps a running argmin; the waves' winners meet in LDS.  Per-point arithmetic and the error sums are fp64: the lane adds its
//     points in index order, the wave sums by a fixed butterfly (wave_allreduce), the mean is sum / N -- every candidate's error is
//     a deterministic value, so duplicated candidates tie exactly.  The argmin is torch.argmin's: the smallest mean error, the first
//     index among equal ones, and a NaN error wins at its first occurrence.  In 3D mode K^-1 h (independent of the candidate) is
//     computed once per point in fp64 and kept as fp32.  The candidates come from the caller's array (the chunk table), or -- table form
//     -- are formed from the row's base pose and its object's symmetry transforms (sym_candidate) while they are staged in LDS:
//     12 outputs x 5 fp64 operations per candidate spread over the workgroup, a few per cent of the walk that follows.  A row of more
//     than kSelLdsCands candidates forms each one in the walk instead (every lane of the wave the same 12 values): no second launch, no
//     host knowledge of the batch's objects and no limit on the batch, at ~60 redundant fp64 operations per candidate and wave next to
//     the ~35 per check point the walk spends anyway.  With p.cand_out set the workgroup writes the row's candidates to global memory
//     instead of LDS and stops (lc_sym_candidates_f32, Rt_candi): the same loop, consecutive threads storing consecutive floats.
// (B) lc_label_targets_kernel: one streaming pass over B x H x W -- xyz_gt = R^T (K^-1 h - t) * m (fp64, stored fp32), then
//     xyz_to_nn_target: the model transform (and the mask again), / noc_scale, and the continuous target or the Gray-coded bit
//     planes of floatbits.mod_noc2bits_bb (the quantiser argument (noc + 1) * (2^n - 1) / 2 in fp32 from the fp32 noc, as torch
//     does, rounded half to even).  A thread takes PIX consecutive pixels of one sample, so every plane is written with PIX-byte
//     (bits) or 4*PIX-byte (floats) stores.
#include "lc_common.h"
#include "lc_kernels.h"
#include "lc_map.h"

namespace lc {
namespace {

constexpr int kSelThreads = 512;  // eight waves: two per SIMD (256 threads for 16 points per lane: their registers need one wave per SIMD)
constexpr int kTgtThreads = 256;
constexpr int kSelLdsCands = 1024;  // rows of up to this many candidates read them from LDS (48 KB)

__device__ __forceinline__ void inv3(const float* K, double (&Ki)[9]) {
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double id = 1.0 / (a * A + b * B + c * C);
    Ki[0] = A * id; Ki[1] = -(b * i - c * h) * id; Ki[2] = (b * f - c * e) * id;
    Ki[3] = B * id; Ki[4] = (a * i - c * g) * id;  Ki[5] = -(a * f - c * d) * id;
    Ki[6] = C * id; Ki[7] = -(a * h - b * g) * id; Ki[8] = (a * e - b * d) * id;
}

// (e, k) before (be, bk) in torch.argmin's order: NaN first (earliest), then the smaller value, then the smaller index
__device__ __forceinline__ bool argmin_before(double e, int k, double be, int bk) {
    if (bk < 0) return true;
    const bool n = e != e, bn = be != be;
    if (n || bn) return n && (!bn || k < bk);
    return e < be || (e == be && k < bk);
}

// row b's chunk: number of candidates and the first one (static indices only: the table stays in the kernel arguments)
__device__ __forceinline__ void row_candidates(const SymSelectParams& p, int b, int& K, int& off) {
    K = 0; off = 0;
#pragma unroll
    for (int c = 0; c < kSymMaxChunks; ++c)
        if (c < p.nchunks && b >= p.chunk_row[c] && b < p.chunk_row[c + 1]) {
            K = p.chunk_k[c];
            off = p.chunk_off[c] + (b - p.chunk_row[c]) * p.chunk_k[c];
        }
}

// row b's object in the table: number of transforms and the first one; K = 0 for a row the table does not hold (nothing of it is read)
__device__ __forceinline__ void table_row(const int* obj_index, const int* obj_off, const int* obj_k, int n_obj, int sym_rows, int b, int& K,
                                          int& off) {
    K = 0; off = 0;
    const int o = obj_index[b];
    if (o < 0 || o >= n_obj) return;
    const int k = obj_k[o], f = obj_off[o];
    if (k < 1 || f < 0 || (long long)f + k > sym_rows) return;
    K = k; off = f;
}

// Element e (row i = e / 4, column j = e % 4) of candidate k of a row: [R_b R_s | R_b t_s + t_b] for the base pose `base` (fp32, widened)
// and transform k of the object (`sym`: its first transform; fp64), every product and sum rounded on its own (no fma), in this order:
//   ((R_b[i][0] S[0][j] + R_b[i][1] S[1][j]) + R_b[i][2] S[2][j]) (+ t_b[i] for j = 3), then one rounding to fp32.
// Transform 0 of every object is the identity: candidate 0 IS the base pose, copied (also its NaNs, infinities and signed zeros).
__device__ __forceinline__ float sym_candidate(const float* base, const double* sym, int k, int e) {
    if (k == 0) return base[e];
    const int i = e >> 2, j = e & 3;
    const double* S = sym + 12 * (size_t)k;
    double v = __dadd_rn(__dadd_rn(__dmul_rn((double)base[4 * i], S[j]), __dmul_rn((double)base[4 * i + 1], S[4 + j])),
                         __dmul_rn((double)base[4 * i + 2], S[8 + j]));
    if (j == 3) v = __dadd_rn(v, (double)base[4 * i + 3]);
    return (float)v;
}

template <int PPL, int THREADS>
__global__ __launch_bounds__(THREADS) void lc_sym_select_kernel(const SymSelectParams p) {
    constexpr int kSelWaves = THREADS / kWave;
    __shared__ double s_e[kSelWaves];
    __shared__ int s_k[kSelWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, N = p.N;
    __shared__ float s_cand[12 * kSelLdsCands];
    int K, off;
    const bool table = p.sym_tab != nullptr;
    if (table) table_row(p.obj_index, p.obj_off, p.obj_k, p.n_obj, p.sym_rows, b, K, off);
    else row_candidates(p, b, K, off);
    const float* cand = table ? nullptr : p.cand + (size_t)off * 12;
    const float* base = table ? p.Rt_base + 12 * (size_t)b : nullptr;
    const double* sym = table ? p.sym_tab + 12 * (size_t)off : nullptr;
    if (p.cand_out) {  // materialise only (the whole grid takes this branch)
        const int row = p.row_off[b];
        if (row >= 0 && (long long)row + K <= p.out_rows)
            for (int i = tid; i < 12 * K; i += THREADS) p.cand_out[12 * (size_t)row + i] = sym_candidate(base, sym, i / 12, i % 12);
        return;
    }
    // the row's candidates are staged in LDS by the whole workgroup: each wave walks its candidates one after the other, and a global
    // load per candidate in that loop would put the memory latency on the critical path of every iteration
    const bool staged = K > 1 && K <= kSelLdsCands;
    if (staged) {
        if (table)
            for (int i = tid; i < 12 * K; i += THREADS) s_cand[i] = sym_candidate(base, sym, i / 12, i % 12);
        else
            for (int i = tid; i < 12 * K; i += THREADS) s_cand[i] = cand[i];
    }
    __syncthreads();
    const float* walk = staged ? s_cand : cand;
    const float nanf = __builtin_nanf("");

    // the lane's points: P = predicted / model point, Q = K^-1 h (3D) or the observed uv (2D)
    float P[PPL][3], Q[PPL][3];
    double Ki[9];
    if (p.mode == 1) inv3(p.cam_K + 9 * (size_t)b, Ki);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int n = lane + kWave * j;
        P[j][0] = P[j][1] = P[j][2] = Q[j][0] = Q[j][1] = Q[j][2] = 0.f;
        if (n >= N || K <= 1) continue;
        const size_t bn = (size_t)b * N + n;
        if (p.mode == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) P[j][i] = p.pts_a[bn * 3 + i];
            Q[j][0] = p.pts_b[bn * 2];
            Q[j][1] = p.pts_b[bn * 2 + 1];
            continue;
        }
        int x = 0, y = 0;
        bool inside = true;
        if (!p.pts_a || !p.pts_b) {
            long long cx = p.ck[bn * 2], cy = p.ck[bn * 2 + 1];
            cx += cx < 0 ? p.W : 0;
            cy += cy < 0 ? p.H : 0;
            inside = cx >= 0 && cx < p.W && cy >= 0 && cy < p.H;  // outside the map: the point's error is NaN, nothing is read
            x = inside ? (int)cx : 0;
            y = inside ? (int)cy : 0;
        }
        const size_t pix = (size_t)y * p.W + x;
        double h[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            h[i] = p.pts_b ? p.pts_b[bn * 3 + i] : (inside ? p.homo_z[((size_t)b * p.H * p.W + pix) * 3 + i] : nanf);
            P[j][i] = p.pts_a ? p.pts_a[bn * 3 + i]
                              : (inside ? map_scalar_at(p.xyz_map, p.map_dtype, (size_t)b * p.map_bs + (size_t)i * p.H * p.W + pix) *
                                              p.noc_scale[3 * (size_t)b + i]
                                        : nanf);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) Q[j][i] = (float)(Ki[3 * i] * h[0] + Ki[3 * i + 1] * h[1] + Ki[3 * i + 2] * h[2]);
    }

    double best_e = 0.0;
    int best_k = -1;
    if (K > 1) {
        double Kc[9];
        if (p.mode == 0)
#pragma unroll
            for (int i = 0; i < 9; ++i) Kc[i] = p.cam_K[9 * (size_t)b + i];
        for (int k = wave; k < K; k += kSelWaves) {
            float c[12];
            if (table && !staged) {
#pragma unroll
                for (int e = 0; e < 12; ++e) c[e] = sym_candidate(base, sym, k, e);
            } else {
#pragma unroll
                for (int e = 0; e < 12; ++e) c[e] = walk[12 * k + e];
            }
            double R[9], t[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                R[3 * r] = c[4 * r]; R[3 * r + 1] = c[4 * r + 1]; R[3 * r + 2] = c[4 * r + 2];
                t[r] = c[4 * r + 3];
            }
            double s = 0.0;
            if (p.mode == 0) {  // uv = pi(K (R p + t))
                double M[9], m[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    m[r] = Kc[3 * r] * t[0] + Kc[3 * r + 1] * t[1] + Kc[3 * r + 2] * t[2];
#pragma unroll
                    for (int q = 0; q < 3; ++q) M[3 * r + q] = Kc[3 * r] * R[q] + Kc[3 * r + 1] * R[3 + q] + Kc[3 * r + 2] * R[6 + q];
                }
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    if (lane + kWave * j >= N) break;
                    const double X = P[j][0], Y = P[j][1], Z = P[j][2];
                    const double h0 = M[0] * X + M[1] * Y + M[2] * Z + m[0];
                    const double h1 = M[3] * X + M[4] * Y + M[5] * Z + m[1];
                    const double h2 = M[6] * X + M[7] * Y + M[8] * Z + m[2];
                    const double du = h0 / h2 - (double)Q[j][0], dv = h1 / h2 - (double)Q[j][1];
                    s += sqrt(du * du + dv * dv);
                }
            } else {  // || p - R^T (K^-1 h - t) ||
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    if (lane + kWave * j >= N) break;
                    const double w0 = (double)Q[j][0] - t[0], w1 = (double)Q[j][1] - t[1], w2 = (double)Q[j][2] - t[2];
                    const double d0 = (double)P[j][0] - (R[0] * w0 + R[3] * w1 + R[6] * w2);
                    const double d1 = (double)P[j][1] - (R[1] * w0 + R[4] * w1 + R[7] * w2);
                    const double d2 = (double)P[j][2] - (R[2] * w0 + R[5] * w1 + R[8] * w2);
                    s += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
                }
            }
            double v[1] = {s};
            wave_allreduce<1>(v);
            const double e = v[0] / N;
            if (argmin_before(e, k, best_e, best_k)) {
                best_e = e;
                best_k = k;
            }
        }
    }
    if (lane == 0) {
        s_e[wave] = best_e;
        s_k[wave] = best_k;
    }
    __syncthreads();
    if (tid < 12) {
        int bk = K > 1 ? -1 : 0;
        double be = 0.0;
        if (K > 1)
            for (int w = 0; w < kSelWaves; ++w)
                if (s_k[w] >= 0 && argmin_before(s_e[w], s_k[w], be, bk)) {
                    be = s_e[w];
                    bk = s_k[w];
                }
        if (table && K == 0) bk = -1;
        p.Rt_best[12 * (size_t)b + tid] = !table ? cand[12 * bk + tid] : (K == 0 ? nanf : sym_candidate(base, sym, bk, tid));
        if (tid == 0 && p.best_idx) p.best_idx[b] = bk;
    }
}

template <int PIX>
struct PlaneWord;  // PIX one-byte flags as one store
template <>
struct PlaneWord<1> { typedef unsigned char type; };
template <>
struct PlaneWord<4> { typedef unsigned type; };
template <>
struct PlaneWord<8> { typedef uint2 type; };
template <>
struct PlaneWord<16> { typedef uint4 type; };

template <int PIX>
__device__ __forceinline__ void store_plane(unsigned char* q, const unsigned (&flags)[PIX]) {
    if constexpr (PIX == 1) {
        *q = (unsigned char)flags[0];
    } else {
        unsigned w[PIX / 4];
#pragma unroll
        for (int i = 0; i < PIX / 4; ++i) w[i] = flags[4 * i] | flags[4 * i + 1] << 8 | flags[4 * i + 2] << 16 | flags[4 * i + 3] << 24;
        typename PlaneWord<PIX>::type v;
        __builtin_memcpy(&v, w, sizeof(v));
        *reinterpret_cast<typename PlaneWord<PIX>::type*>(q) = v;
    }
}

template <int PIX>
__device__ __forceinline__ void store_floats(float* q, const float* v) {  // PIX floats
    if constexpr (PIX % 4 == 0) {
#pragma unroll
        for (int i = 0; i < PIX / 4; ++i) reinterpret_cast<float4*>(q)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < PIX; ++i) q[i] = v[i];
    }
}

template <int PIX>
__global__ __launch_bounds__(kTgtThreads) void lc_label_targets_kernel(const LabelParams p) {
    const long long first = ((long long)blockIdx.x * kTgtThreads + threadIdx.x) * PIX;
    if (first >= (long long)p.B * p.HW) return;
    const int b = (int)(first / p.HW), pix0 = (int)(first - (long long)b * p.HW);

    // per sample: A = R^T K^-1, c = R^T t (xyz = A h - c), the transform and 1 / noc_scale
    double A[9], c[3];
    {
        double Ki[9];
        inv3(p.cam_K + 9 * (size_t)b, Ki);
        const float* Rt = p.Rt + 12 * (size_t)b;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double r0 = Rt[i], r1 = Rt[4 + i], r2 = Rt[8 + i];  // column i of R
            c[i] = r0 * Rt[3] + r1 * Rt[7] + r2 * Rt[11];
#pragma unroll
            for (int j = 0; j < 3; ++j) A[3 * i + j] = r0 * Ki[j] + r1 * Ki[3 + j] + r2 * Ki[6 + j];
        }
    }
    const bool targets = p.noc_tgt || p.bin_tgt || p.bin_raw;

    float hz[3 * PIX];
    const float* hp = p.homo_z + 3 * (size_t)first;
    if constexpr (PIX % 4 == 0) {
#pragma unroll
        for (int i = 0; i < 3 * PIX / 4; ++i) {
            const float4 v = reinterpret_cast<const float4*>(hp)[i];
            hz[4 * i] = v.x; hz[4 * i + 1] = v.y; hz[4 * i + 2] = v.z; hz[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * PIX; ++i) hz[i] = hp[i];
    }
    float m[PIX];
#pragma unroll
    for (int i = 0; i < PIX; ++i) m[i] = 1.f;
    if (p.msk_f32) {
        if constexpr (PIX % 4 == 0) {
#pragma unroll
            for (int i = 0; i < PIX / 4; ++i) {
                const float4 v = reinterpret_cast<const float4*>(p.msk_f32 + first)[i];
                m[4 * i] = v.x; m[4 * i + 1] = v.y; m[4 * i + 2] = v.z; m[4 * i + 3] = v.w;
            }
        } else {
            m[0] = p.msk_f32[first];
        }
    }
    if (p.msk_u8) {
        unsigned char mb[PIX];
        if constexpr (PIX == 1) {
            mb[0] = p.msk_u8[first];
        } else {
            typename PlaneWord<PIX>::type v = *reinterpret_cast<const typename PlaneWord<PIX>::type*>(p.msk_u8 + first);
            __builtin_memcpy(mb, &v, PIX);
        }
#pragma unroll
        for (int i = 0; i < PIX; ++i) m[i] = mb[i] ? 1.f : 0.f;
    }

    float xyz[3 * PIX], noc[3][PIX];
#pragma unroll
    for (int q = 0; q < PIX; ++q) {
        const double h0 = hz[3 * q], h1 = hz[3 * q + 1], h2 = hz[3 * q + 2], mm = m[q];
        double x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            x[i] = (A[3 * i] * h0 + A[3 * i + 1] * h1 + A[3 * i + 2] * h2 - c[i]);
            if (p.msk_u8 || p.msk_f32) x[i] *= mm;
            xyz[3 * q + i] = (float)x[i];
        }
        if (!targets) continue;
        double y[3] = {x[0], x[1], x[2]};
        if (p.xform) {
            const float* T = p.xform + 16 * (size_t)b;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                y[i] = (double)T[4 * i] * x[0] + (double)T[4 * i + 1] * x[1] + (double)T[4 * i + 2] * x[2] + (double)T[4 * i + 3];
                if (p.msk_u8 || p.msk_f32) y[i] *= mm;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) noc[i][q] = (float)(y[i] / (double)p.noc_scale[3 * (size_t)b + i]);
    }
    if (p.xyz_gt) {
        float* o = p.xyz_gt + 3 * (size_t)first;
        if constexpr (PIX % 4 == 0) {
#pragma unroll
            for (int i = 0; i < 3 * PIX / 4; ++i)
                reinterpret_cast<float4*>(o)[i] = make_float4(xyz[4 * i], xyz[4 * i + 1], xyz[4 * i + 2], xyz[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < 3 * PIX; ++i) o[i] = xyz[i];
        }
    }
    if (p.noc_tgt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) store_floats<PIX>(p.noc_tgt + ((size_t)b * 3 + a) * p.HW + pix0, noc[a]);
    }
    if (!p.bin_tgt && !p.bin_raw) return;
    const int C = p.bits[0] + p.bits[1] + p.bits[2];
    int ch = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int n = p.bits[a];
        const float mx = (float)((1u << n) - 1u);
        unsigned v[PIX];
#pragma unroll
        for (int q = 0; q < PIX; ++q) {
            const float arg = (noc[a][q] + 1.f) * (mx * 0.5f);
            v[q] = (unsigned)(int)rintf(fminf(fmaxf(arg, 0.f), mx));  // torch.clamp + torch.round (half to even) + .to(int32)
        }
        for (int i = 0; i < n; ++i, ++ch) {
            const int sh = n - 1 - i;  // plane i of the axis holds bit n-1-i (most significant first)
            const size_t o = ((size_t)b * C + ch) * p.HW + pix0;
            if (p.bin_raw) {
                unsigned f[PIX];
#pragma unroll
                for (int q = 0; q < PIX; ++q) f[q] = (v[q] >> sh) & 1u;
                store_plane<PIX>(p.bin_raw + o, f);
            }
            if (p.bin_tgt) {
                const unsigned inv = (p.black && i < 2) ? 1u : 0u;
                unsigned f[PIX];
#pragma unroll
                for (int q = 0; q < PIX; ++q) f[q] = (((v[q] ^ (v[q] >> 1)) >> sh) & 1u) ^ inv;  // Gray code
                store_plane<PIX>(p.bin_tgt + o, f);
            }
        }
    }
}

}  // namespace

int launch_sym_select(const SymSelectParams& p, hipStream_t stream) {
    if (p.B <= 0) return 0;
    const dim3 grid(p.B), block(kSelThreads);
    if (p.N <= kWave) hipLaunchKernelGGL((lc_sym_select_kernel<1, kSelThreads>), grid, block, 0, stream, p);
    else if (p.N <= 2 * kWave) hipLaunchKernelGGL((lc_sym_select_kernel<2, kSelThreads>), grid, block, 0, stream, p);
    else if (p.N <= 4 * kWave) hipLaunchKernelGGL((lc_sym_select_kernel<4, kSelThreads>), grid, block, 0, stream, p);
    else if (p.N <= 8 * kWave) hipLaunchKernelGGL((lc_sym_select_kernel<8, kSelThreads>), grid, block, 0, stream, p);
    else if (p.N <= 16 * kWave) hipLaunchKernelGGL((lc_sym_select_kernel<16, 256>), grid, dim3(256), 0, stream, p);
    else return 3;
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_sym_candidates(const SymSelectParams& p, hipStream_t stream) {
    if (p.B <= 0) return 0;
    hipLaunchKernelGGL((lc_sym_select_kernel<1, kSelThreads>), dim3(p.B), dim3(kSelThreads), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_label_targets(const LabelParams& p, hipStream_t stream) {
    if (p.B <= 0) return 0;
    const long long total = (long long)p.B * p.HW;
    auto aligned = [](const void* q, unsigned bytes) { return (reinterpret_cast<uintptr_t>(q) & (bytes - 1)) == 0; };
    // vector width: PIX pixels of one sample per thread, every pointer aligned for the PIX-wide accesses
    auto fits = [&](int pix) {
        return p.HW % pix == 0 && aligned(p.homo_z, 16) && aligned(p.xyz_gt, 16) && aligned(p.noc_tgt, 16) && aligned(p.msk_f32, 16) &&
               aligned(p.msk_u8, pix) && aligned(p.bin_tgt, pix) && aligned(p.bin_raw, pix);
    };
    auto go = [&](auto kern, int pix) {
        const long long threads = total / pix;
        hipLaunchKernelGGL(kern, dim3((unsigned)((threads + kTgtThreads - 1) / kTgtThreads)), dim3(kTgtThreads), 0, stream, p);
    };
    if (fits(8)) go(lc_label_targets_kernel<8>, 8);
    else if (fits(4)) go(lc_label_targets_kernel<4>, 4);
    else go(lc_label_targets_kernel<1>, 1);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace lc
