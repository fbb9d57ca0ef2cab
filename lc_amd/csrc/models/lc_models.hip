// Per-object model preparation on the device: what `models_info.json` (extents, diameter) and the sparse heads' `fps` asset
// (farthest-point keypoints, dataset.py:232-236) hold, computed from the vertices of a MeshSet.
//
// DEFINITIONS (the tests hold the kernels to them bit for bit; tests/models_cases.py restates them in numpy).  All arithmetic is
// IEEE fp32 on the fp32 vertices, every operation rounded on its own (nothing here may be contracted into an FMA):
//
//     d2(a, b) = ((ax-bx)*(ax-bx) + (ay-by)*(ay-by)) + (az-bz)*(az-bz)
//
// Per mesh with vertices v[0..V), V >= 1:
//   extents   lo, hi = component-wise min and max (exact, order-free).
//   diameter  over all pairs i < j the largest d2(v[i], v[j]); ties go to the smallest i, then the smallest j;
//             diameter = sqrt(d2) correctly rounded, pair = (i, j) local to the mesh.  V == 1: diameter 0, pair (0, 0).
//   farthest points, count <= V:  c = (lo + hi) * 0.5f,  mind[v] = d2(v, c);  count times: k = argmax mind (ties: smallest index),
//             record k and v[k], then mind[v] = min(mind[v], d2(v, v[k])) for every v.  The first n rows of a count-point result are
//             the n-point result.
// The same inputs give the same bits on every call: every choice below is a maximum over totally ordered integer keys.
//
// KERNELS
//   lc_model_points_kernel    one workgroup of 1024 threads per mesh (the selection is serial: each pick needs the previous one).
//       Up to kModelFpsResident vertices the coordinates and mind stay in registers (8 points per thread); larger meshes stream
//       the coordinates from memory (L2-resident) and keep mind in the workspace.  A pick is a local update plus one
//       workgroup-wide maximum of the key (mind bits << 32 | ~index) -- non-negative floats order as unsigned integers, the
//       complemented index makes the smallest index win a tie -- and the winner's coordinates go to all threads through LDS.
//       Its first pass is the extents pass; with fps_count = 0 it is that pass alone.
//   lc_model_diameter_kernel  one workgroup of 128 threads per tile (i-block, j-block >= i-block) of the upper triangle of the pair
//       matrix, tiles of kModelDiamTile^2 pairs.  The j-block is staged in LDS as float4; a lane keeps two i-vertices in registers
//       and walks the block with broadcast 16-byte reads.  Each i-vertex carries its best (d2, j) and replaces it only on a
//       strictly larger d2 while j ascends, so the smallest j survives a tie for free; the lane, wave and workgroup maxima are
//       taken over the key (d2 bits << 32 | valid | ~i_local | ~j_local).  One 16-byte partial per workgroup, no atomics, no
//       workgroup waits for another.  Tile t = jb (jb + 1) / 2 + ib whatever the mesh's size, so the tiles of a mesh are a prefix
//       of its slots.
//   lc_model_diameter_reduce_kernel  one workgroup per mesh: the partials under the full (d2, i, j) order, then the square root.
//
// A library of its own (liblc_amd_models.so, C ABI in include/lc_amd_models.h): an offline tool's kernels, outside the run-time libraries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_models.h"
#include "../shared/lc_shared.h"

#ifndef LC_AMD_MODELS_SRC_HASH
#define LC_AMD_MODELS_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

// sha256 of the sources this library was compiled from, behind a marker lc_amd/build.py finds in the file's bytes (is_stale)
const char kSrcHash[] = "LC_AMD_MODELS_SRC_HASH:" LC_AMD_MODELS_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

typedef unsigned long long u64;

constexpr int kModelDiamTile = LC_MODEL_DIAM_TILE;        // vertices along one edge of a tile of the pair matrix
constexpr int kModelFpsResident = LC_MODEL_FPS_RESIDENT;  // most vertices whose coordinates and distances stay in registers
struct ModelParams {
    const float* verts;           // (total,3) vertices of every mesh, back to back
    const int* table;             // (n_meshes,4) DEVICE: vert_off, n_vert, face_off, n_face (the faces are not read)
    int n_meshes, max_verts, fps_count;
    int diam_tiles;               // tiles of the upper triangle of a mesh of max_verts vertices = partial slots per mesh
    float* lo;                    // (n_meshes,3) or null
    float* hi;                    // (n_meshes,3) or null
    float* diameter;              // (n_meshes,) or null
    int* pair;                    // (n_meshes,2) or null
    float* fps;                   // (n_meshes,fps_count,3) or null
    int* fps_index;               // (n_meshes,fps_count) or null
    void* partials;               // workspace: (n_meshes,diam_tiles) 16-byte records (d2 bits, i, j, valid)
    float* mind;                  // workspace: (n_meshes,mind_stride) distances of the streaming FPS form, or null
    long long mind_stride;
};
constexpr long long model_diam_tiles(long long max_verts) {
    const long long nb = (max_verts + kModelDiamTile - 1) / kModelDiamTile;
    return nb * (nb + 1) / 2;
}

constexpr int kPointThreads = 1024;
constexpr int kPointWaves = kPointThreads / kWave;
constexpr int kPointsPerThread = kModelFpsResident / kPointThreads;
static_assert(kPointsPerThread * kPointThreads == kModelFpsResident, "the resident form deals its points evenly");
constexpr int kDiamThreads = 128;
constexpr int kDiamWaves = kDiamThreads / kWave;
constexpr int kDiamPerLane = kModelDiamTile / kDiamThreads;
static_assert(kDiamPerLane * kDiamThreads == kModelDiamTile && kModelDiamTile <= 256, "local indices are packed into 8 bits each");
constexpr int kReduceThreads = 256;

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    const float xx = __fmul_rn(dx, dx), yy = __fmul_rn(dy, dy), zz = __fmul_rn(dz, dz);
    const float xy = __fadd_rn(xx, yy);
    return __fadd_rn(xy, zz);
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)v, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(v >> 32), (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ u64 xor_u64(u64 v, int mask) {
    const int lo = __shfl_xor((int)(unsigned)v, mask, kWave), hi = __shfl_xor((int)(unsigned)(v >> 32), mask, kWave);
    return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ u64 umax(u64 a, u64 b) { return a > b ? a : b; }
// a[c] for c in 0..2 without indexing registers by a run-time value
__device__ __forceinline__ float sel3(const float (&a)[3], int c) { return c == 0 ? a[0] : c == 1 ? a[1] : a[2]; }

// maximum over the 64 lanes, in every lane: the exchange pattern of wave_allreduce (lc_shared.h) on integer keys
__device__ __forceinline__ u64 wave_max(u64 v) {
    v = umax(v, dpp_u64<kDppQuadXor1>(v));
    v = umax(v, dpp_u64<kDppQuadXor2>(v));
    v = umax(v, dpp_u64<kDppHalfMirror>(v));
    v = umax(v, dpp_u64<kDppRowMirror>(v));
    v = umax(v, xor_u64(v, 16));
    return umax(v, xor_u64(v, 32));
}

// maximum over the workgroup, in every thread.  `red` (WAVES words) may be written again only after a later barrier.
template <int WAVES>
__device__ __forceinline__ u64 block_max(u64 v, u64* red, int tid) {
    v = wave_max(v);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = umax(r, red[w]);
    return r;
}

__device__ __forceinline__ u64 point_key(float mind, int index) {
    return ((u64)__float_as_uint(mind) << 32) | (0xFFFFFFFFu - (unsigned)index);  // an index is below 2^31: never 0 in the low word
}

// component-wise min / max over the workgroup, in every thread (once per launch: plain shuffles)
__device__ __forceinline__ void block_extents(float (&mn)[3], float (&mx)[3], float* lds, int tid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int s = 1; s < kWave; s <<= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], s, kWave));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], s, kWave));
        }
    }
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lds[6 * (tid / kWave) + c] = mn[c];
            lds[6 * (tid / kWave) + 3 + c] = mx[c];
        }
    }
    __syncthreads();
#pragma unroll 2  // (unrolled whole, its 96 reads are all in flight at once and push the resident form's points out of their registers)
    for (int w = 0; w < kPointWaves; ++w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn[c] = fminf(mn[c], lds[6 * w + c]);
            mx[c] = fmaxf(mx[c], lds[6 * w + 3 + c]);
        }
    }
}

struct PointShared {
    u64 red[kPointWaves];
    float ext[6 * kPointWaves];
    float win[4];
};

// one pick: the workgroup's maximum key -> index k; its owner (thread k % kPointThreads) hands the coordinates to everyone
template <class Owner>
__device__ __forceinline__ int pick(u64 best, PointShared& sh, int tid, float (&w)[3], Owner owner_coords) {
    const u64 key = block_max<kPointWaves>(best, sh.red, tid);
    const int k = (int)(0xFFFFFFFFu - (unsigned)key);
    if (tid == k % kPointThreads) {
        float c[3];
        owner_coords(k, c);
        sh.win[0] = c[0];
        sh.win[1] = c[1];
        sh.win[2] = c[2];
    }
    __syncthreads();  // also: every thread has read red, the next pick may write it
    w[0] = sh.win[0];
    w[1] = sh.win[1];
    w[2] = sh.win[2];
    return k;
}

template <bool RESIDENT>
__global__ __launch_bounds__(kPointThreads) void lc_model_points_kernel(const ModelParams p) {
    __shared__ PointShared sh;
    const int m = blockIdx.x, tid = threadIdx.x;
    const int off = p.table[4 * m], V = p.table[4 * m + 1];
    if (V < 1 || V > p.max_verts || off < 0) return;  // (refused by the entry point from the host copy of the table)
    if (RESIDENT != (V <= kModelFpsResident)) return;  // the other form's mesh
    const float* v = p.verts + 3 * (size_t)off;
    const bool want_fps = p.fps_count > 0 && (p.fps || p.fps_index);
    const int count = p.fps_count < V ? p.fps_count : V;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    float w[3];

    if (RESIDENT) {
        float x[kPointsPerThread], y[kPointsPerThread], z[kPointsPerThread], md[kPointsPerThread];
#pragma unroll
        for (int q = 0; q < kPointsPerThread; ++q) {
            const int i = q * kPointThreads + tid, ic = i < V ? i : V - 1;  // slots past the end repeat the last vertex: the extents ignore a repeat
            x[q] = v[3 * ic]; y[q] = v[3 * ic + 1]; z[q] = v[3 * ic + 2];
            mn[0] = fminf(mn[0], x[q]); mn[1] = fminf(mn[1], y[q]); mn[2] = fminf(mn[2], z[q]);
            mx[0] = fmaxf(mx[0], x[q]); mx[1] = fmaxf(mx[1], y[q]); mx[2] = fmaxf(mx[2], z[q]);
        }
        block_extents(mn, mx, sh.ext, tid);
        if (tid < 3) {
            if (p.lo) p.lo[3 * (size_t)m + tid] = sel3(mn, tid);
            if (p.hi) p.hi[3 * (size_t)m + tid] = sel3(mx, tid);
        }
        if (!want_fps) return;
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = __fmul_rn(__fadd_rn(mn[c], mx[c]), 0.5f);
        for (int it = 0; it < count; ++it) {
            u64 best = 0;  // below every key of a vertex
#pragma unroll
            for (int q = 0; q < kPointsPerThread; ++q) {
                const int i = q * kPointThreads + tid;
                const float d = dist2(x[q], y[q], z[q], w[0], w[1], w[2]);
                md[q] = it == 0 ? d : fminf(md[q], d);
                if (i < V) best = umax(best, point_key(md[q], i));
            }
            const int k = pick(best, sh, tid, w, [&](int kk, float (&c)[3]) {
                const int qk = kk / kPointThreads;
                c[0] = c[1] = c[2] = 0.f;
#pragma unroll
                for (int q = 0; q < kPointsPerThread; ++q)
                    if (q == qk) { c[0] = x[q]; c[1] = y[q]; c[2] = z[q]; }
            });
            if (tid == 0 && p.fps_index) p.fps_index[(size_t)m * p.fps_count + it] = k;
            if (tid < 3 && p.fps) p.fps[((size_t)m * p.fps_count + it) * 3 + tid] = sel3(w, tid);
        }
        return;
    }

    // streaming form
    for (int i = tid; i < V; i += kPointThreads) {
        const float xi = v[3 * i], yi = v[3 * i + 1], zi = v[3 * i + 2];
        mn[0] = fminf(mn[0], xi); mn[1] = fminf(mn[1], yi); mn[2] = fminf(mn[2], zi);
        mx[0] = fmaxf(mx[0], xi); mx[1] = fmaxf(mx[1], yi); mx[2] = fmaxf(mx[2], zi);
    }
    block_extents(mn, mx, sh.ext, tid);
    if (tid < 3) {
        if (p.lo) p.lo[3 * (size_t)m + tid] = sel3(mn, tid);
        if (p.hi) p.hi[3 * (size_t)m + tid] = sel3(mx, tid);
    }
    if (!want_fps || !p.mind) return;
    float* md = p.mind + (size_t)m * (size_t)p.mind_stride;  // element i is read and written by thread i % kPointThreads alone
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = __fmul_rn(__fadd_rn(mn[c], mx[c]), 0.5f);
    for (int it = 0; it < count; ++it) {
        u64 best = 0;
#pragma unroll 4
        for (int i = tid; i < V; i += kPointThreads) {
            float d = dist2(v[3 * i], v[3 * i + 1], v[3 * i + 2], w[0], w[1], w[2]);
            if (it > 0) d = fminf(md[i], d);
            if (it + 1 < count) md[i] = d;
            best = umax(best, point_key(d, i));
        }
        const int k = pick(best, sh, tid, w, [&](int kk, float (&c)[3]) {
            c[0] = v[3 * kk]; c[1] = v[3 * kk + 1]; c[2] = v[3 * kk + 2];
        });
        if (tid == 0 && p.fps_index) p.fps_index[(size_t)m * p.fps_count + it] = k;
        if (tid < 3 && p.fps) p.fps[((size_t)m * p.fps_count + it) * 3 + tid] = sel3(w, tid);
    }
}

// tile t of the upper triangle -> (ib, jb), ib <= jb, t = jb (jb + 1) / 2 + ib
__device__ __forceinline__ void tile_of(int t, int& ib, int& jb) {
    long long j = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > t) --j;
    while ((j + 1) * (j + 2) / 2 <= t) ++j;
    jb = (int)j;
    ib = t - (int)(j * (j + 1) / 2);
}

template <bool DIAG>
__device__ __forceinline__ void walk_tile(const float4* tile, int nj, const float (&x)[kDiamPerLane], const float (&y)[kDiamPerLane],
                                          const float (&z)[kDiamPerLane], int tid, float (&best)[kDiamPerLane], int (&bj)[kDiamPerLane]) {
#pragma unroll 4
    for (int jl = 0; jl < nj; ++jl) {
        const float4 wj = tile[jl];  // the same address in every lane: a broadcast read
#pragma unroll
        for (int r = 0; r < kDiamPerLane; ++r) {
            const float d = dist2(x[r], y[r], z[r], wj.x, wj.y, wj.z);
            bool take = d > best[r];
            if (DIAG) take = take && jl > r * kDiamThreads + tid;
            if (take) {
                best[r] = d;
                bj[r] = jl;
            }
        }
    }
}

__global__ __launch_bounds__(kDiamThreads) void lc_model_diameter_kernel(const ModelParams p) {
    __shared__ float4 tile[kModelDiamTile];
    __shared__ u64 red[kDiamWaves];
    const int m = blockIdx.x / p.diam_tiles, t = blockIdx.x % p.diam_tiles, tid = threadIdx.x;
    const int off = p.table[4 * m], V = p.table[4 * m + 1];
    if (V < 1 || V > p.max_verts || off < 0) return;
    const long long nb = (V + kModelDiamTile - 1) / kModelDiamTile;
    if (t >= nb * (nb + 1) / 2) return;  // a tile of a larger mesh of the set
    int ib, jb;
    tile_of(t, ib, jb);
    const float* v = p.verts + 3 * (size_t)off;
    const int i0 = ib * kModelDiamTile, j0 = jb * kModelDiamTile;
    const int nj = V - j0 < kModelDiamTile ? V - j0 : kModelDiamTile;
    for (int j = tid; j < nj; j += kDiamThreads) tile[j] = make_float4(v[3 * (j0 + j)], v[3 * (j0 + j) + 1], v[3 * (j0 + j) + 2], 0.f);
    float x[kDiamPerLane], y[kDiamPerLane], z[kDiamPerLane], best[kDiamPerLane];
    int bj[kDiamPerLane];
#pragma unroll
    for (int r = 0; r < kDiamPerLane; ++r) {
        const int i = i0 + r * kDiamThreads + tid;
        x[r] = y[r] = z[r] = 0.f;
        if (i < V) { x[r] = v[3 * i]; y[r] = v[3 * i + 1]; z[r] = v[3 * i + 2]; }
        best[r] = -1.f;  // below every d2: the first pair met is taken
        bj[r] = 0;
    }
    __syncthreads();
    if (ib == jb) walk_tile<true>(tile, nj, x, y, z, tid, best, bj);
    else walk_tile<false>(tile, nj, x, y, z, tid, best, bj);
    u64 key = 0;  // "no pair": below every key of a pair (bit 16 of their low word is set)
#pragma unroll
    for (int r = 0; r < kDiamPerLane; ++r) {
        const int il = r * kDiamThreads + tid;
        if (i0 + il < V && best[r] >= 0.f)
            key = umax(key, ((u64)__float_as_uint(best[r]) << 32) | 0x10000u | (unsigned)((255 - il) << 8) | (unsigned)(255 - bj[r]));
    }
    key = block_max<kDiamWaves>(key, red, tid);
    if (tid == 0) {
        const unsigned low = (unsigned)key;
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (low & 0x10000u) rec = make_uint4((unsigned)(key >> 32), (unsigned)(i0 + 255 - (int)((low >> 8) & 255u)), (unsigned)(j0 + 255 - (int)(low & 255u)), 1u);
        static_cast<uint4*>(p.partials)[(size_t)m * p.diam_tiles + t] = rec;
    }
}

__global__ __launch_bounds__(kReduceThreads) void lc_model_diameter_reduce_kernel(const ModelParams p) {
    __shared__ u64 red[2][kReduceThreads / kWave];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int V = p.table[4 * m + 1];
    if (V < 1 || V > p.max_verts) return;
    const long long nb = (V + kModelDiamTile - 1) / kModelDiamTile;
    const int nt = (int)(nb * (nb + 1) / 2);
    const uint4* part = static_cast<const uint4*>(p.partials) + (size_t)m * p.diam_tiles;
    // (d2 descending, i ascending) as one key, j beside it: strictly better under the full order replaces
    u64 bk = 0;
    unsigned bjv = 0;
    for (int t = tid; t < nt; t += kReduceThreads) {
        const uint4 r = part[t];
        const u64 k = r.w ? ((u64)r.x << 32) | 0x80000000u | (0x7FFFFFFFu - r.y) : 0ull;
        if (k > bk || (k == bk && k != 0 && r.z < bjv)) {
            bk = k;
            bjv = r.z;
        }
    }
    const u64 top = block_max<kReduceThreads / kWave>(bk, red[0], tid);
    // among the threads that hold the best (d2, i): the smallest j
    const u64 jtop = block_max<kReduceThreads / kWave>(bk == top && top != 0 ? (u64)(0xFFFFFFFFu - bjv) : 0ull, red[1], tid);
    if (tid == 0) {
        float d = 0.f;
        int i = 0, j = 0;
        if (top != 0) {
            // through fp64, so that the result is the correctly rounded fp32 root whatever fp32 sqrt the build selects: a correctly
            // rounded fp64 root rounds to the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits: no double-rounding case)
            d = (float)__dsqrt_rn((double)__uint_as_float((unsigned)(top >> 32)));
            i = (int)(0x7FFFFFFFu - ((unsigned)top & 0x7FFFFFFFu));
            j = (int)(0xFFFFFFFFu - (unsigned)jtop);
        }
        if (p.diameter) p.diameter[m] = d;
        if (p.pair) {
            p.pair[2 * (size_t)m] = i;
            p.pair[2 * (size_t)m + 1] = j;
        }
    }
}

// both forms take the whole set; a workgroup whose mesh belongs to the other form returns at once
int launch_model_points(const ModelParams& p, bool resident, bool streaming, hipStream_t stream) {
    if (resident) hipLaunchKernelGGL(lc_model_points_kernel<true>, dim3(p.n_meshes), dim3(kPointThreads), 0, stream, p);
    if (streaming) hipLaunchKernelGGL(lc_model_points_kernel<false>, dim3(p.n_meshes), dim3(kPointThreads), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_model_diameter(const ModelParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(lc_model_diameter_kernel, dim3((unsigned)((long long)p.n_meshes * p.diam_tiles)), dim3(kDiamThreads), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(lc_model_diameter_reduce_kernel, dim3(p.n_meshes), dim3(kReduceThreads), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// the two sections of the workspace: the diameter partials, then the distances of the streaming FPS form
size_t partial_bytes(int n_meshes, int max_verts) { return (size_t)16 * (size_t)n_meshes * (size_t)model_diam_tiles(max_verts); }
size_t mind_stride_of(int max_verts, int fps_count) { return fps_count > 0 && max_verts > kModelFpsResident ? ((size_t)max_verts + 3) / 4 * 4 : 0; }

template <typename... P>
bool misaligned(size_t bytes, P... ptrs) {
    return (((reinterpret_cast<uintptr_t>(ptrs) % bytes) != 0) || ...);
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_models_version(void) { return LC_AMD_MODELS_VERSION; }
const char* lc_amd_models_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_MODELS_SRC_HASH:") - 1; }
const char* lc_amd_models_last_error(void) { return lc::g_err.c_str(); }

size_t lc_model_workspace_bytes(int n_meshes, int max_verts, int fps_count) {
    if (n_meshes <= 0 || max_verts <= 0) return 0;
    return lc::partial_bytes(n_meshes, max_verts) + (size_t)4 * (size_t)n_meshes * lc::mind_stride_of(max_verts, fps_count);
}

int lc_model_prepare_f32(const float* verts, const int* table, const int* table_host, int n_meshes, int max_verts, int fps_count, float* lo,
                         float* hi, float* diameter, int* pair, float* fps, int* fps_index, void* workspace, size_t workspace_bytes,
                         void* stream) {
    using lc::fail;
    if (n_meshes <= 0) return fail(1, "n_meshes must be positive");
    if (max_verts <= 0) return fail(1, "max_verts must be positive");
    if (max_verts >= (1 << 30) / 3 * 2) return fail(1, "max_verts: 3 * max_verts must stay below 2^31 (the kernels index a mesh's coordinates with 32-bit integers)");
    if (fps_count < 0) return fail(1, "fps_count must not be negative");
    if (!verts || !table || !table_host) return fail(1, "null pointer");
    const bool want_fps = fps_count > 0 && (fps || fps_index), want_diam = diameter || pair, want_points = want_fps || lo || hi;
    if (!want_points && !want_diam) return fail(1, "no output");
    bool resident = false, streaming = false;
    for (int m = 0; m < n_meshes; ++m) {
        const int off = table_host[4 * m], nv = table_host[4 * m + 1];
        (nv <= lc::kModelFpsResident ? resident : streaming) = true;
        if (off < 0 || nv < 1 || nv > max_verts)
            return fail(1, "mesh " + std::to_string(m) + ": vertex offset " + std::to_string(off) + " / count " + std::to_string(nv) +
                               " outside 1.." + std::to_string(max_verts) + " (max_verts)");
        if (want_fps && fps_count > nv)
            return fail(1, "fps_count " + std::to_string(fps_count) + " exceeds the " + std::to_string(nv) + " vertices of mesh " + std::to_string(m));
    }
    const long long tiles = lc::model_diam_tiles(max_verts);
    if (want_diam && tiles * n_meshes >= (1ll << 31)) return fail(1, "diameter: 2^31 tiles or more");
    if ((long long)n_meshes * (fps_count > 0 ? fps_count : 1) * 3 >= (1ll << 31)) return fail(1, "outputs of 2^31 elements or more");
    const size_t part_bytes = lc::partial_bytes(n_meshes, max_verts), stride = lc::mind_stride_of(max_verts, fps_count);
    const size_t need = (want_diam ? part_bytes : 0) + (want_fps ? (size_t)4 * n_meshes * stride : 0);
    if (need) {
        if (!workspace) return fail(1, "workspace is null");
        if (workspace_bytes < lc_model_workspace_bytes(n_meshes, max_verts, fps_count))
            return fail(1, "workspace too small: lc_model_workspace_bytes(n_meshes, max_verts, fps_count) bytes are needed");
        if (lc::misaligned(16, workspace)) return fail(1, "workspace not 16-byte aligned");
    }
    if (lc::misaligned(4, verts, table, lo, hi, diameter, pair, fps, fps_index)) return fail(1, "pointer not 4-byte aligned");
    lc::ModelParams p{};
    p.verts = verts; p.table = table; p.n_meshes = n_meshes; p.max_verts = max_verts; p.fps_count = want_fps ? fps_count : 0;
    p.diam_tiles = (int)tiles; p.lo = lo; p.hi = hi; p.diameter = diameter; p.pair = pair; p.fps = fps; p.fps_index = fps_index;
    p.partials = workspace;
    p.mind = stride ? reinterpret_cast<float*>(static_cast<char*>(workspace) + part_bytes) : nullptr;
    p.mind_stride = (long long)stride;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (want_points && lc::launch_model_points(p, resident, streaming, st)) return fail(11, "model points launch failed");
    if (want_diam && lc::launch_model_diameter(p, st)) return fail(11, "model diameter launch failed");
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
