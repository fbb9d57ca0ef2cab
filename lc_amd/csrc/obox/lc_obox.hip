// The oriented model box on the device: what `models_xform.json` holds per object (model_transform.py:21-42), searched over a stated
// hierarchical grid of rotations for the box of least volume.
//
// DEFINITIONS: include/lc_amd_obox.h states them in full and tests/obox_oracle.py restates them in numpy; the tests hold the kernels to
// them bit for bit.  In short: a level's candidate c is the mesh's base quaternion (c == 0) or normalise(deltas[c] (x) base), formed in fp64
// with every operation rounded on its own and turned into a matrix that is rounded once to fp32; its score is the volume of the extents of the
// rotated vertices in fp32, every operation rounded on its own; the lowest score wins, ties to the lowest index, and is the next level's base.
//
// KERNELS
//   lc_obox_init_kernel    the workspace of one call: identity bases, cleared flags, the extrema slots at their neutral keys.
//   lc_obox_score_kernel   one workgroup of kScoreThreads per (mesh, chunk of kSplit vertices, block of kScoreThreads candidates).  A lane keeps
//       ONE candidate: nine matrix entries and six running extrema in registers.  The chunk goes through LDS in tiles of kTile vertices as
//       float4 and is read back as broadcasts (the same address in every lane).  Per (candidate, vertex): 9 multiplies, 6 adds, 6 min / max.
//       The lane's extrema join the candidate's six slots by vector atomics on order-preserving integer keys: min and max are exact in any
//       order, so neither the split nor the arrival order changes a bit.  The final pass is the same kernel with the one candidate 0 (the
//       base as it is); it also raises the mesh's flag on a coordinate that is not finite.
//   lc_obox_pick_kernel    one wave per mesh: every candidate's score from its slots, the minimum of (score bits << 32 | index), the
//       winner's quaternion into the base, its index into `path`; the slots go back to their neutral keys for the next level.
//   lc_obox_finish_kernel  one wave per mesh: centre, translation and half-extents from the final pass's slots, the 4 x 4 matrix, info.
// Nothing is read back between the launches: level l + 1 reads the base level l wrote.
//
// A library of its own (liblc_amd_obox.so, C ABI in include/lc_amd_obox.h): an offline tool's kernels, outside the run-time libraries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_obox.h"

#ifndef LC_AMD_OBOX_SRC_HASH
#define LC_AMD_OBOX_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

// sha256 of the sources this library was compiled from, behind a marker lc_amd/build.py finds in the file's bytes (is_stale)
const char kSrcHash[] = "LC_AMD_OBOX_SRC_HASH:" LC_AMD_OBOX_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

typedef unsigned long long u64;

constexpr int kWave = 64;
constexpr int kTile = LC_OBOX_TILE;    // vertices of one LDS tile
constexpr int kSplit = LC_OBOX_SPLIT;  // vertices of one workgroup's chunk
constexpr int kScoreThreads = 128;     // = candidates of one workgroup
static_assert(kSplit % kTile == 0 && kTile % kScoreThreads == 0, "a chunk is whole tiles, a tile is loaded in whole rounds");

struct OboxParams {
    const float* verts;    // (total,3) vertices of every mesh, back to back
    const int* table;      // (n_meshes,4) DEVICE: vert_off, n_vert, face_off, n_face (the faces are not read)
    int n_meshes, max_verts, chunks;  // chunks = ceil(max_verts / kSplit)
    const double* deltas;  // (n_cand,4) this level's table; not read by a launch with n_cand == 1
    int n_cand, max_cand;
    int level, levels;
    double* base;          // workspace: (n_meshes,4)
    int* flags;            // workspace: (n_meshes,)
    unsigned* slots;       // workspace: (n_meshes,6,max_cand) keys of min x y z, max x y z
    int final_pass;        // the score kernel raises flags
    float* xform;          // (n_meshes,4,4)
    float* noc_scale;      // (n_meshes,3)
    float* volume;         // (n_meshes,)
    float* aabb_volume;    // (n_meshes,)
    int* path;             // (n_meshes,levels+1)
    int* info;             // (n_meshes,)
};

// floats as unsigned integers of the same order (-inf lowest, +inf highest; -0 below +0: the definition counts both as +0 afterwards)
__device__ __forceinline__ unsigned ordered_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
constexpr unsigned kMinNeutral = 0xFFFFFFFFu, kMaxNeutral = 0u;

// candidate c of a level: the base itself, or normalise(d (x) b); one call per rounding
__device__ __forceinline__ void candidate_quat(const double* b, const double* d, int c, double (&q)[4]) {
    const double bw = b[0], bx = b[1], by = b[2], bz = b[3];
    if (c == 0) {
        q[0] = bw; q[1] = bx; q[2] = by; q[3] = bz;
        return;
    }
    const double dw = d[0], dx = d[1], dy = d[2], dz = d[3];
    const double pw = __dsub_rn(__dsub_rn(__dsub_rn(__dmul_rn(dw, bw), __dmul_rn(dx, bx)), __dmul_rn(dy, by)), __dmul_rn(dz, bz));
    const double px = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(dw, bx), __dmul_rn(dx, bw)), __dmul_rn(dy, bz)), __dmul_rn(dz, by));
    const double py = __dadd_rn(__dadd_rn(__dsub_rn(__dmul_rn(dw, by), __dmul_rn(dx, bz)), __dmul_rn(dy, bw)), __dmul_rn(dz, bx));
    const double pz = __dadd_rn(__dsub_rn(__dadd_rn(__dmul_rn(dw, bz), __dmul_rn(dx, by)), __dmul_rn(dy, bx)), __dmul_rn(dz, bw));
    const double n2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(pw, pw), __dmul_rn(px, px)), __dmul_rn(py, py)), __dmul_rn(pz, pz));
    const double n = __dsqrt_rn(n2);
    q[0] = __ddiv_rn(pw, n); q[1] = __ddiv_rn(px, n); q[2] = __ddiv_rn(py, n); q[3] = __ddiv_rn(pz, n);
}

__device__ __forceinline__ void quat_matrix(const double (&q)[4], float (&R)[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = __dmul_rn(x, x), yy = __dmul_rn(y, y), zz = __dmul_rn(z, z);
    const double xy = __dmul_rn(x, y), xz = __dmul_rn(x, z), yz = __dmul_rn(y, z);
    const double wx = __dmul_rn(w, x), wy = __dmul_rn(w, y), wz = __dmul_rn(w, z);
    R[0] = (float)__dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(yy, zz)));
    R[1] = (float)__dmul_rn(2.0, __dsub_rn(xy, wz));
    R[2] = (float)__dmul_rn(2.0, __dadd_rn(xz, wy));
    R[3] = (float)__dmul_rn(2.0, __dadd_rn(xy, wz));
    R[4] = (float)__dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, zz)));
    R[5] = (float)__dmul_rn(2.0, __dsub_rn(yz, wx));
    R[6] = (float)__dmul_rn(2.0, __dsub_rn(xz, wy));
    R[7] = (float)__dmul_rn(2.0, __dadd_rn(yz, wx));
    R[8] = (float)__dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, yy)));
}

// ((r0*x + r1*y) + r2*z), nothing contracted
__device__ __forceinline__ float row_dot(float r0, float r1, float r2, float x, float y, float z) {
#pragma clang fp contract(off)
    const float a = __fmul_rn(r0, x), b = __fmul_rn(r1, y), c = __fmul_rn(r2, z);
    const float ab = __fadd_rn(a, b);
    return __fadd_rn(ab, c);
}

__global__ __launch_bounds__(256) void lc_obox_init_kernel(const OboxParams p) {
    const size_t n_slots = (size_t)p.n_meshes * 6 * (size_t)p.max_cand;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const int k = (int)((i / (size_t)p.max_cand) % 6);
        p.slots[i] = k < 3 ? kMinNeutral : kMaxNeutral;
        if (i < (size_t)p.n_meshes) {
            p.flags[i] = 0;
            p.base[4 * i] = 1.0;
            p.base[4 * i + 1] = 0.0;
            p.base[4 * i + 2] = 0.0;
            p.base[4 * i + 3] = 0.0;
        }
    }
}

__global__ __launch_bounds__(kScoreThreads) void lc_obox_score_kernel(const OboxParams p) {
    __shared__ float4 tile[kTile];
    const int m = blockIdx.y, tid = threadIdx.x;
    const int chunk = blockIdx.x % p.chunks, cb = blockIdx.x / p.chunks;
    const int off = p.table[4 * m], V = p.table[4 * m + 1];
    if (V < 1 || V > p.max_verts || off < 0) return;  // (refused by the entry point from the host copy of the table)
    const int v0 = chunk * kSplit;
    if (v0 >= V) return;  // a chunk of a larger mesh of the set (the whole workgroup leaves)
    const int v1 = V - v0 < kSplit ? V : v0 + kSplit;
    const float* v = p.verts + 3 * (size_t)off;
    const int c = cb * kScoreThreads + tid;
    const bool active = c < p.n_cand;
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};  // a lane past the last candidate walks along and posts nothing
    if (active) {
        double q[4];
        candidate_quat(p.base + 4 * (size_t)m, p.deltas + 4 * (size_t)c, c, q);
        quat_matrix(q, R);
    }
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int t0 = v0; t0 < v1; t0 += kTile) {
        const int n = v1 - t0 < kTile ? v1 - t0 : kTile;
        __syncthreads();  // the previous tile has been walked by every lane
        for (int j = tid; j < n; j += kScoreThreads) {
            const size_t i = 3 * (size_t)(t0 + j);
            const float x = v[i], y = v[i + 1], z = v[i + 2];
            bad = bad || !(isfinite(x) && isfinite(y) && isfinite(z));
            tile[j] = make_float4(x, y, z, 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const float4 w = tile[j];  // the same address in every lane: a broadcast read
            const float px = row_dot(R[0], R[1], R[2], w.x, w.y, w.z);
            const float py = row_dot(R[3], R[4], R[5], w.x, w.y, w.z);
            const float pz = row_dot(R[6], R[7], R[8], w.x, w.y, w.z);
            mn[0] = fminf(mn[0], px); mn[1] = fminf(mn[1], py); mn[2] = fminf(mn[2], pz);
            mx[0] = fmaxf(mx[0], px); mx[1] = fmaxf(mx[1], py); mx[2] = fmaxf(mx[2], pz);
        }
    }
    if (active) {
        unsigned* s = p.slots + (size_t)m * 6 * (size_t)p.max_cand + c;  // neighbouring lanes, neighbouring words
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(s + (size_t)k * p.max_cand, ordered_key(mn[k]));
            atomicMax(s + (size_t)(3 + k) * p.max_cand, ordered_key(mx[k]));
        }
    }
    if (bad && p.final_pass) p.flags[m] = 1;  // (every writer writes the same word)
}

// lo, hi of candidate c from its slots, a zero of either sign as +0
__device__ __forceinline__ void slot_extents(const unsigned* s, int max_cand, float (&lo)[3], float (&hi)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = __fadd_rn(ordered_value(s[(size_t)k * max_cand]), 0.f);
        hi[k] = __fadd_rn(ordered_value(s[(size_t)(3 + k) * max_cand]), 0.f);
    }
}

__device__ __forceinline__ u64 xor_u64(u64 v, int mask) {
    const int lo = __shfl_xor((int)(unsigned)v, mask, kWave), hi = __shfl_xor((int)(unsigned)(v >> 32), mask, kWave);
    return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}

__global__ __launch_bounds__(kWave) void lc_obox_pick_kernel(const OboxParams p) {
    const int m = blockIdx.x, lane = threadIdx.x;
    unsigned* slots = p.slots + (size_t)m * 6 * (size_t)p.max_cand;
    u64 best = ~0ull;  // above every key of a candidate (an index is below 2^31)
    float first = 0.f;
    for (int c = lane; c < p.max_cand; c += kWave) {
        if (c < p.n_cand) {
#pragma clang fp contract(off)
            float lo[3], hi[3];
            slot_extents(slots + c, p.max_cand, lo, hi);
            const float ex = __fsub_rn(hi[0], lo[0]), ey = __fsub_rn(hi[1], lo[1]), ez = __fsub_rn(hi[2], lo[2]);
            const float exy = __fmul_rn(ex, ey);
            const float score = __fmul_rn(exy, ez);
            const u64 key = ((u64)__float_as_uint(score) << 32) | (unsigned)c;
            best = key < best ? key : best;
            if (c == 0) first = score;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) slots[(size_t)k * p.max_cand + c] = k < 3 ? kMinNeutral : kMaxNeutral;  // ready for the next level
    }
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const u64 o = xor_u64(best, s);
        best = o < best ? o : best;
    }
    if (lane == 0) {
        const int win = (int)(unsigned)best;  // a candidate's index: below n_cand whatever the scores were
        double q[4];
        double* b = p.base + 4 * (size_t)m;
        candidate_quat(b, p.deltas + 4 * (size_t)win, win, q);
        b[0] = q[0]; b[1] = q[1]; b[2] = q[2]; b[3] = q[3];
        p.path[(size_t)m * (p.levels + 1) + p.level] = win;
        p.volume[m] = __uint_as_float((unsigned)(best >> 32));
        if (p.level == 0) p.aabb_volume[m] = first;
    }
}

__global__ __launch_bounds__(kWave) void lc_obox_finish_kernel(const OboxParams p) {
#pragma clang fp contract(off)
    const int m = blockIdx.x;
    if (threadIdx.x != 0) return;
    const double* b = p.base + 4 * (size_t)m;
    const double q[4] = {b[0], b[1], b[2], b[3]};
    float R[9], lo[3], hi[3];
    quat_matrix(q, R);
    slot_extents(p.slots + (size_t)m * 6 * (size_t)p.max_cand, p.max_cand, lo, hi);
    float* X = p.xform + 16 * (size_t)m;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c = __fmul_rn(__fadd_rn(lo[k], hi[k]), 0.5f);
        X[4 * k] = R[3 * k];
        X[4 * k + 1] = R[3 * k + 1];
        X[4 * k + 2] = R[3 * k + 2];
        X[4 * k + 3] = -c;
        p.noc_scale[3 * (size_t)m + k] = fmaxf(__fsub_rn(hi[k], c), __fsub_rn(c, lo[k]));
    }
    X[12] = 0.f; X[13] = 0.f; X[14] = 0.f; X[15] = 1.f;
    p.info[m] = p.flags[m] ? 1 : 0;
}

size_t base_bytes(int n_meshes) { return (size_t)32 * (size_t)n_meshes; }
size_t flag_bytes(int n_meshes) { return ((size_t)4 * (size_t)n_meshes + 15) / 16 * 16; }
size_t slot_bytes(int n_meshes, int max_cand) { return (size_t)24 * (size_t)n_meshes * (size_t)max_cand; }

bool launched() { return hipGetLastError() == hipSuccess; }

template <typename... P>
bool misaligned(size_t bytes, P... ptrs) {
    return (((reinterpret_cast<uintptr_t>(ptrs) % bytes) != 0) || ...);
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_obox_version(void) { return LC_AMD_OBOX_VERSION; }
const char* lc_amd_obox_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_OBOX_SRC_HASH:") - 1; }
const char* lc_amd_obox_last_error(void) { return lc::g_err.c_str(); }

size_t lc_obox_workspace_bytes(int n_meshes, int max_cand) {
    if (n_meshes <= 0 || max_cand <= 0) return 0;
    return lc::base_bytes(n_meshes) + lc::flag_bytes(n_meshes) + lc::slot_bytes(n_meshes, max_cand);
}

int lc_obox_search_f32(const float* verts, int total_verts, const int* table, const int* table_host, int n_meshes, int max_verts, const double* deltas,
                       int n_level0, int n_refine, int levels, float* xform, float* noc_scale, float* volume, float* aabb_volume, int* path,
                       int* info, void* workspace, size_t workspace_bytes, void* stream) {
    using lc::fail;
    if (n_meshes <= 0 || n_meshes > 65535) return fail(1, "n_meshes must be in 1..65535");
    if (total_verts <= 0) return fail(1, "total_verts must be positive");
    if (max_verts <= 0) return fail(1, "max_verts must be positive");
    if (max_verts >= (1 << 30) / 3 * 2) return fail(1, "max_verts: 3 * max_verts must stay below 2^31 (the kernels index a mesh's coordinates with 32-bit integers)");
    if (levels < 0 || levels > LC_OBOX_MAX_LEVELS) return fail(1, "levels must be in 0.." + std::to_string(LC_OBOX_MAX_LEVELS));
    if (n_level0 < 1 || n_level0 > LC_OBOX_MAX_CAND) return fail(1, "n_level0 must be in 1.." + std::to_string(LC_OBOX_MAX_CAND));
    if (levels > 0 && (n_refine < 1 || n_refine > LC_OBOX_MAX_CAND)) return fail(1, "n_refine must be in 1.." + std::to_string(LC_OBOX_MAX_CAND));
    if (!verts || !table || !table_host || !deltas) return fail(1, "null pointer");
    if (!xform || !noc_scale || !volume || !aabb_volume || !path || !info) return fail(1, "null output");
    for (int m = 0; m < n_meshes; ++m) {
        const int off = table_host[4 * m], nv = table_host[4 * m + 1];
        if (off < 0 || nv < 1 || nv > max_verts)
            return fail(1, "mesh " + std::to_string(m) + ": vertex offset " + std::to_string(off) + " / count " + std::to_string(nv) +
                               " outside 1.." + std::to_string(max_verts) + " (max_verts)");
        if ((long long)off + nv > total_verts)
            return fail(1, "mesh " + std::to_string(m) + ": vertices " + std::to_string(off) + " + " + std::to_string(nv) + " end behind total_verts " +
                               std::to_string(total_verts));
    }
    const int max_cand = levels > 0 && n_refine > n_level0 ? n_refine : n_level0;
    if ((long long)n_meshes * 6 * max_cand >= (1ll << 31)) return fail(1, "2^31 extrema slots or more");
    if ((long long)n_meshes * (levels + 1) >= (1ll << 31) / 16) return fail(1, "outputs of 2^31 elements or more");
    if (!workspace) return fail(1, "workspace is null");
    if (workspace_bytes < lc_obox_workspace_bytes(n_meshes, max_cand))
        return fail(1, "workspace too small: lc_obox_workspace_bytes(n_meshes, max(n_level0, n_refine)) bytes are needed");
    if (lc::misaligned(16, workspace)) return fail(1, "workspace not 16-byte aligned");
    if (lc::misaligned(8, deltas)) return fail(1, "deltas not 8-byte aligned");
    if (lc::misaligned(4, verts, table, xform, noc_scale, volume, aabb_volume, path, info)) return fail(1, "pointer not 4-byte aligned");
    const int chunks = (max_verts + lc::kSplit - 1) / lc::kSplit;
    const long long cand_blocks = (max_cand + lc::kScoreThreads - 1) / lc::kScoreThreads;
    if (cand_blocks * chunks >= (1ll << 31)) return fail(1, "a grid of 2^31 workgroups or more");

    lc::OboxParams p{};
    p.verts = verts; p.table = table; p.n_meshes = n_meshes; p.max_verts = max_verts; p.chunks = chunks;
    p.max_cand = max_cand; p.levels = levels;
    char* ws = static_cast<char*>(workspace);
    p.base = reinterpret_cast<double*>(ws);
    p.flags = reinterpret_cast<int*>(ws + lc::base_bytes(n_meshes));
    p.slots = reinterpret_cast<unsigned*>(ws + lc::base_bytes(n_meshes) + lc::flag_bytes(n_meshes));
    p.xform = xform; p.noc_scale = noc_scale; p.volume = volume; p.aabb_volume = aabb_volume; p.path = path; p.info = info;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n_slots = (size_t)n_meshes * 6 * (size_t)max_cand;
    const unsigned init_blocks = (unsigned)((n_slots + 255) / 256 < 2048 ? (n_slots + 255) / 256 : 2048);
    hipLaunchKernelGGL(lc::lc_obox_init_kernel, dim3(init_blocks), dim3(256), 0, st, p);
    if (!lc::launched()) return fail(11, "obox init launch failed");
    for (int level = 0; level <= levels; ++level) {
        p.level = level;
        p.n_cand = level == 0 ? n_level0 : n_refine;
        p.deltas = deltas + 4 * (level == 0 ? (size_t)0 : (size_t)n_level0 + (size_t)(level - 1) * (size_t)n_refine);
        const unsigned blocks = (unsigned)((p.n_cand + lc::kScoreThreads - 1) / lc::kScoreThreads);
        hipLaunchKernelGGL(lc::lc_obox_score_kernel, dim3(blocks * (unsigned)chunks, (unsigned)n_meshes), dim3(lc::kScoreThreads), 0, st, p);
        if (!lc::launched()) return fail(11, "obox score launch failed");
        hipLaunchKernelGGL(lc::lc_obox_pick_kernel, dim3((unsigned)n_meshes), dim3(lc::kWave), 0, st, p);
        if (!lc::launched()) return fail(11, "obox pick launch failed");
    }
    p.n_cand = 1;
    p.final_pass = 1;
    hipLaunchKernelGGL(lc::lc_obox_score_kernel, dim3((unsigned)chunks, (unsigned)n_meshes), dim3(lc::kScoreThreads), 0, st, p);
    if (!lc::launched()) return fail(11, "obox final pass launch failed");
    hipLaunchKernelGGL(lc::lc_obox_finish_kernel, dim3((unsigned)n_meshes), dim3(lc::kWave), 0, st, p);
    if (!lc::launched()) return fail(11, "obox finish launch failed");
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
