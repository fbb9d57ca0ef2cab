// The symmetry deviation of a model on the device: for many rigid transforms S of many meshes, max over the query vertices x_i of the
// distance from S x_i to its nearest vertex of the same mesh -- BOP's geometric rule for a potential symmetry, evaluated, not annotated.
//
// DEFINITIONS: include/lc_amd_symfind.h states them in full and tests/symfind_oracle.py restates them in numpy; the tests hold the kernels
// to them bit for bit.  In short: the transformed query is formed in fp64, every operation rounded on its own, and rounded once to fp32;
// d2 is fp32 without FMA; n_i = min_j d2 (lowest j at ties, a NaN never wins), score = max_i n_i (lowest query position at ties).
//
// KERNELS
//   lc_symfind_clear_kernel   outputs to -1, info to 0, the rows' slots to 0 ("no query yet").
//   lc_symfind_walk_kernel    one workgroup of kWalkThreads per (job, row, tile of kQueries queries).  A lane transforms its kPerLane queries
//       once and keeps them in registers with their running minima.  The mesh goes through LDS in tiles of kTile vertices as float4, read
//       back as broadcasts (the same address in every lane).  Per (query, target): 3 subtractions, 3 multiplies, 2 adds, 1 min -- the
//       witness target is NOT tracked here.  A query's min is complete when the walk ends; the workgroup's largest key
//       (n_i bits << 32 | ~position: non-negative floats order as unsigned integers, the complemented position makes the lowest win a tie)
//       joins the row's slot by one 64-bit vector atomic max, exact in any order.
//   lc_symfind_finish_kernel  one workgroup per (job, row): the slot's query against every vertex once more under the key
//       (d2 bits << 32 | j), whose minimum is (n_i, the lowest j that has it); writes the three outputs.
// Nothing is read back between the launches.
//
// A library of its own (liblc_amd_symfind.so, C ABI in include/lc_amd_symfind.h): an offline tool's kernels, outside the run-time libraries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_symfind.h"

#ifndef LC_AMD_SYMFIND_SRC_HASH
#define LC_AMD_SYMFIND_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

// sha256 of the sources this library was compiled from, behind a marker lc_amd/build.py finds in the file's bytes (is_stale)
const char kSrcHash[] = "LC_AMD_SYMFIND_SRC_HASH:" LC_AMD_SYMFIND_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

typedef unsigned long long u64;

constexpr int kWave = 64;
constexpr int kTile = LC_SYMFIND_TILE;        // target vertices of one LDS tile
constexpr int kQueries = LC_SYMFIND_QUERIES;  // queries of one workgroup
constexpr int kWalkThreads = 128;
constexpr int kPerLane = kQueries / kWalkThreads;
constexpr int kFinishThreads = 256;
static_assert(kPerLane * kWalkThreads == kQueries && kTile % kWalkThreads == 0, "queries are dealt evenly, a tile is loaded in whole rounds");

struct SymfindParams {
    const float* verts;      // (total_verts,3) vertices of every mesh, back to back
    const int* mesh_table;   // (n_meshes,4) DEVICE: vert_off, n_vert, face_off, n_face (the faces are not read)
    int total_verts, n_meshes, max_verts;
    const double* table;     // (total_rows,12) row-major 3 x 4 [R | t]
    int total_rows;
    const int* mesh_index;   // (n_jobs,)
    const int* row_off;      // (n_jobs,)
    const int* row_k;        // (n_jobs,)
    int n_jobs, max_k;
    const int* query_idx;    // (total_queries,) or null: every vertex, in order
    const int* query_off;    // (n_jobs,), read with query_idx
    const int* query_n;      // (n_jobs,), read with query_idx
    int total_queries, max_queries, q_tiles;  // q_tiles = ceil(max_queries / kQueries)
    float* dev2;             // (n_jobs,max_k)
    int* arg_query;          // (n_jobs,max_k)
    int* arg_target;         // (n_jobs,max_k)
    int* info;               // (n_jobs,)
    u64* slots;              // workspace: (n_jobs,max_k) keys, 0 = no query
};

struct Job {
    const float* v;    // the mesh's vertices
    int V;             // and their number
    const double* rows;
    int K;
    const int* q;      // the job's query list, or null
    int nq;
    bool ok;
};

// the job's entries, judged: of a job that is not ok nothing else may be read
__device__ __forceinline__ Job load_job(const SymfindParams& p, int g) {
    Job j{};
    const int mi = p.mesh_index[g], ro = p.row_off[g], rk = p.row_k[g];
    if (mi < 0 || mi >= p.n_meshes || ro < 0 || rk < 0 || rk > p.max_k || (long long)ro + rk > p.total_rows) return j;
    const int off = p.mesh_table[4 * mi], V = p.mesh_table[4 * mi + 1];
    if (off < 0 || V < 0 || V > p.max_verts || (long long)off + V > p.total_verts) return j;
    j.nq = V;
    if (p.query_idx) {
        const int qo = p.query_off[g], qn = p.query_n[g];
        if (qo < 0 || qn < 0 || qn > p.max_queries || (long long)qo + qn > p.total_queries) return j;
        j.q = p.query_idx + qo;
        j.nq = qn;
    }
    j.v = p.verts + 3 * (size_t)off;
    j.V = V;
    j.rows = p.table + 12 * (size_t)ro;
    j.K = rk;
    j.ok = true;
    return j;
}

// fp32( ((r0*x + r1*y) + r2*z) + t ), every fp64 operation rounded on its own
__device__ __forceinline__ float row_point(const double* r, double x, double y, double z) {
    const double a = __dmul_rn(r[0], x), b = __dmul_rn(r[1], y), c = __dmul_rn(r[2], z);
    return (float)__dadd_rn(__dadd_rn(__dadd_rn(a, b), c), r[3]);
}

__device__ __forceinline__ void transform(const double* row, const float* vert, float (&q)[3]) {
    const double x = (double)vert[0], y = (double)vert[1], z = (double)vert[2];
    q[0] = row_point(row, x, y, z);
    q[1] = row_point(row + 4, x, y, z);
    q[2] = row_point(row + 8, x, y, z);
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    const float xx = __fmul_rn(dx, dx), yy = __fmul_rn(dy, dy), zz = __fmul_rn(dz, dz);
    const float xy = __fadd_rn(xx, yy);
    return __fadd_rn(xy, zz);
}

__device__ __forceinline__ u64 xor_u64(u64 v, int mask) {
    const int lo = __shfl_xor((int)(unsigned)v, mask, kWave), hi = __shfl_xor((int)(unsigned)(v >> 32), mask, kWave);
    return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}

// maximum (MAX) or minimum over the workgroup, valid in thread 0; `red` holds one word per wave
template <bool MAX, int WAVES>
__device__ __forceinline__ u64 block_best(u64 v, u64* red, int tid) {
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const u64 o = xor_u64(v, s);
        v = MAX ? (o > v ? o : v) : (o < v ? o : v);
    }
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = MAX ? (red[w] > r ? red[w] : r) : (red[w] < r ? red[w] : r);
    return r;
}

__global__ __launch_bounds__(256) void lc_symfind_clear_kernel(const SymfindParams p) {
    const size_t n = (size_t)p.n_jobs * (size_t)p.max_k;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        p.dev2[i] = -1.f;
        p.arg_query[i] = -1;
        p.arg_target[i] = -1;
        p.slots[i] = 0ull;
        if (i < (size_t)p.n_jobs) p.info[i] = 0;
    }
}

__global__ __launch_bounds__(kWalkThreads) void lc_symfind_walk_kernel(const SymfindParams p) {
    __shared__ float4 tile[kTile];
    __shared__ u64 red[kWalkThreads / kWave];
    const int g = blockIdx.y, tid = threadIdx.x;
    const int k = blockIdx.x / p.q_tiles, qt = blockIdx.x % p.q_tiles;
    const Job job = load_job(p, g);  // (the same answer in every workgroup of the job)
    if (!job.ok) {
        if (blockIdx.x == 0 && tid == 0) p.info[g] = -1;
        return;
    }
    const int q0 = qt * kQueries;
    if (k >= job.K || q0 >= job.nq || job.V == 0) return;  // a row or a query tile of a larger job of the call (the whole workgroup leaves)
    const double* row = job.rows + 12 * (size_t)k;
    float px[kPerLane], py[kPerLane], pz[kPerLane], best[kPerLane];
    bool live[kPerLane];
    bool skipped = false;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int pos = q0 + r * kWalkThreads + tid;
        px[r] = py[r] = pz[r] = 0.f;  // a lane without a query walks along and posts nothing
        best[r] = INFINITY;
        live[r] = false;
        if (pos < job.nq) {
            const int i = job.q ? job.q[pos] : pos;
            if (i >= 0 && i < job.V) {
                float q[3];
                transform(row, job.v + 3 * (size_t)i, q);
                px[r] = q[0]; py[r] = q[1]; pz[r] = q[2];
                live[r] = true;
            } else {
                skipped = true;
            }
        }
    }
    if (skipped && k == 0) p.info[g] = 1;  // (every writer writes the same word; row 0 sees every query of the job)
    for (int t0 = 0; t0 < job.V; t0 += kTile) {
        const int n = job.V - t0 < kTile ? job.V - t0 : kTile;
        __syncthreads();  // the previous tile has been walked by every lane
        for (int j = tid; j < n; j += kWalkThreads) {
            const size_t i = 3 * (size_t)(t0 + j);
            tile[j] = make_float4(job.v[i], job.v[i + 1], job.v[i + 2], 0.f);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < n; ++j) {
            const float4 w = tile[j];  // the same address in every lane: a broadcast read
#pragma unroll
            for (int r = 0; r < kPerLane; ++r) best[r] = fminf(best[r], dist2(px[r], py[r], pz[r], w.x, w.y, w.z));  // a NaN never wins
        }
    }
    u64 key = 0;  // "no query": below every key of a query (a position is below 2^31, its complement never 0)
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const unsigned pos = (unsigned)(q0 + r * kWalkThreads + tid);
        const u64 mine = ((u64)__float_as_uint(best[r]) << 32) | (0xFFFFFFFFu - pos);
        if (live[r] && mine > key) key = mine;
    }
    key = block_best<true, kWalkThreads / kWave>(key, red, tid);
    if (tid == 0 && key != 0) atomicMax(p.slots + (size_t)g * p.max_k + k, key);
}

__global__ __launch_bounds__(kFinishThreads) void lc_symfind_finish_kernel(const SymfindParams p) {
    __shared__ u64 red[kFinishThreads / kWave];
    const int g = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const Job job = load_job(p, g);
    if (!job.ok || k >= job.K) return;
    const size_t out = (size_t)g * p.max_k + k;
    const u64 top = p.slots[out];
    if (top == 0) return;  // no query was counted: the outputs stay at -1
    const int pos = (int)(0xFFFFFFFFu - (unsigned)top);
    const int i = job.q ? job.q[pos] : pos;  // posted by the walk: inside the list and inside the mesh
    float q[3];
    transform(job.rows + 12 * (size_t)k, job.v + 3 * (size_t)i, q);
    u64 low = ~0ull;  // above every key of a target
    for (int j = tid; j < job.V; j += kFinishThreads) {
        const float d = dist2(q[0], q[1], q[2], job.v[3 * (size_t)j], job.v[3 * (size_t)j + 1], job.v[3 * (size_t)j + 2]);
        const u64 mine = ((u64)__float_as_uint(d) << 32) | (unsigned)j;
        if (d == d && mine < low) low = mine;  // a NaN never wins
    }
    low = block_best<false, kFinishThreads / kWave>(low, red, tid);
    if (tid == 0) {
        p.dev2[out] = __uint_as_float((unsigned)(top >> 32));
        p.arg_query[out] = i;
        p.arg_target[out] = low == ~0ull ? 0 : (int)(unsigned)low;  // every d2 a NaN: n_i is +inf and no d2 equals it
    }
}

size_t slot_bytes(int n_jobs, int max_k) { return ((size_t)8 * (size_t)n_jobs * (size_t)max_k + 15) / 16 * 16; }

bool launched() { return hipGetLastError() == hipSuccess; }

template <typename... P>
bool misaligned(size_t bytes, P... ptrs) {
    return (((reinterpret_cast<uintptr_t>(ptrs) % bytes) != 0) || ...);
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_symfind_version(void) { return LC_AMD_SYMFIND_VERSION; }
const char* lc_amd_symfind_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_SYMFIND_SRC_HASH:") - 1; }
const char* lc_amd_symfind_last_error(void) { return lc::g_err.c_str(); }

size_t lc_symfind_workspace_bytes(int n_jobs, int max_k) {
    if (n_jobs <= 0 || max_k <= 0) return 0;
    return lc::slot_bytes(n_jobs, max_k);
}

int lc_symfind_deviation_f32(const float* verts, int total_verts, const int* mesh_table, const int* mesh_table_host, int n_meshes, int max_verts,
                             const double* table, int total_rows, const int* mesh_index, const int* row_off, const int* row_k, int n_jobs,
                             int max_k, const int* query_idx, const int* query_off, const int* query_n, int total_queries, int max_queries,
                             float* dev2, int* arg_query, int* arg_target, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    using lc::fail;
    if (n_meshes <= 0) return fail(1, "n_meshes must be positive");
    if (n_jobs <= 0 || n_jobs > 65535) return fail(1, "n_jobs must be in 1..65535");
    if (total_verts <= 0) return fail(1, "total_verts must be positive");
    if (max_verts <= 0) return fail(1, "max_verts must be positive");
    if (max_verts >= (1 << 30) / 3 * 2) return fail(1, "max_verts: 3 * max_verts must stay below 2^31 (the kernels index a mesh's coordinates with 32-bit integers)");
    if (total_rows <= 0 || total_rows >= (1 << 30) / 6) return fail(1, "total_rows must be positive, a table of fewer than 2^31 elements");
    if (max_k <= 0 || max_k > total_rows) return fail(1, "max_k must be in 1..total_rows");
    if (!verts || !mesh_table || !mesh_table_host || !table) return fail(1, "null pointer");
    if (!mesh_index || !row_off || !row_k) return fail(1, "null job array");
    if (query_idx) {
        if (!query_off || !query_n) return fail(1, "query_idx without query_off and query_n");
        if (total_queries <= 0) return fail(1, "total_queries must be positive with a query list");
        if (max_queries <= 0 || max_queries > total_queries) return fail(1, "max_queries must be in 1..total_queries");
    }
    if (!dev2 || !arg_query || !arg_target || !info) return fail(1, "null output");
    for (int m = 0; m < n_meshes; ++m) {
        const int off = mesh_table_host[4 * m], nv = mesh_table_host[4 * m + 1];
        if (off < 0 || nv < 0 || nv > max_verts)
            return fail(1, "mesh " + std::to_string(m) + ": vertex offset " + std::to_string(off) + " / count " + std::to_string(nv) +
                               " outside 0.." + std::to_string(max_verts) + " (max_verts)");
        if ((long long)off + nv > total_verts)
            return fail(1, "mesh " + std::to_string(m) + ": vertices " + std::to_string(off) + " + " + std::to_string(nv) + " end behind total_verts " +
                               std::to_string(total_verts));
    }
    if ((long long)n_jobs * max_k >= (1ll << 31)) return fail(1, "outputs of 2^31 elements or more");
    if (!workspace) return fail(1, "workspace is null");
    if (workspace_bytes < lc_symfind_workspace_bytes(n_jobs, max_k)) return fail(1, "workspace too small: lc_symfind_workspace_bytes(n_jobs, max_k) bytes are needed");
    if (lc::misaligned(16, workspace)) return fail(1, "workspace not 16-byte aligned");
    if (lc::misaligned(8, table)) return fail(1, "table not 8-byte aligned");
    if (lc::misaligned(4, verts, mesh_table, mesh_index, row_off, row_k, query_idx, query_off, query_n, dev2, arg_query, arg_target, info))
        return fail(1, "pointer not 4-byte aligned");
    const int max_q = query_idx ? max_queries : max_verts;
    const long long q_tiles = (max_q + lc::kQueries - 1) / lc::kQueries;
    if (q_tiles * max_k >= (1ll << 31)) return fail(1, "a grid of 2^31 workgroups or more");

    lc::SymfindParams p{};
    p.verts = verts; p.mesh_table = mesh_table; p.total_verts = total_verts; p.n_meshes = n_meshes; p.max_verts = max_verts;
    p.table = table; p.total_rows = total_rows;
    p.mesh_index = mesh_index; p.row_off = row_off; p.row_k = row_k; p.n_jobs = n_jobs; p.max_k = max_k;
    p.query_idx = query_idx; p.query_off = query_off; p.query_n = query_n;
    p.total_queries = query_idx ? total_queries : 0; p.max_queries = max_q; p.q_tiles = (int)q_tiles;
    p.dev2 = dev2; p.arg_query = arg_query; p.arg_target = arg_target; p.info = info;
    p.slots = static_cast<lc::u64*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)n_jobs * (size_t)max_k;
    const unsigned clear_blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(lc::lc_symfind_clear_kernel, dim3(clear_blocks), dim3(256), 0, st, p);
    if (!lc::launched()) return fail(11, "symfind clear launch failed");
    hipLaunchKernelGGL(lc::lc_symfind_walk_kernel, dim3((unsigned)(q_tiles * max_k), (unsigned)n_jobs), dim3(lc::kWalkThreads), 0, st, p);
    if (!lc::launched()) return fail(11, "symfind walk launch failed");
    hipLaunchKernelGGL(lc::lc_symfind_finish_kernel, dim3((unsigned)max_k, (unsigned)n_jobs), dim3(lc::kFinishThreads), 0, st, p);
    if (!lc::launched()) return fail(11, "symfind finish launch failed");
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
