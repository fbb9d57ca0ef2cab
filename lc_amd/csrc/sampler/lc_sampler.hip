// The device-resident training set's row sampler (liblc_amd_sampler.so; C ABI and the exact definition of every output in
// include/lc_amd_sampler.h; lc_amd/sampler.py is its statement in host numpy: `permute_host`, `draw_rows_host`, `select_rows_host`).
// What the reference's loader does on the host around `_get_single_item`: the epoch's shuffle, the gather of a step's records, and the
// retry on `valid_cnt` (dataset.py:332-338).
//
// Three kernels, all integer arithmetic and copies:
//   lc_sampler_rows_kernel    one thread per row in workgroups of 64: a row is a few dozen dependent integer operations and 32 words of
//                             record, so there is nothing to share between lanes -- no LDS.
//   lc_sampler_select_kernel  ONE workgroup of 1024 threads.  Rows are judged 64 at a time (a chunk = one wavefront's ballot); LDS holds,
//                             per chunk, the mask and the count of the bad primaries and of the good spares (24 KB at 1024 chunks); the
//                             counts are scanned in order (shuffles within a wavefront, LDS across the sixteen); a bad primary of rank i
//                             finds the i-th good spare by bisecting the scanned counts and picking a bit of that chunk's mask.  No
//                             atomics, no workspace: the result depends on nothing but the inputs.
//   lc_sampler_take_kernel    blockIdx.y names the tensor, whose pointers and row size sit in the kernel's argument; a grid-stride loop
//                             over 16-byte units (or bytes) of the B destination rows.
//
// The hash is maskcrop's, augment's and geometry's: shared/lc_keyed_hash.h; the wavefront sums are shared/lc_wave_int.h's.
//
// Bounds: rows -- thread j >= rows returns before it reads; index < N by construction (a cycle-walked value, or (key N) >> 32 with
// key < 2^32), and it is the only value that forms an address.  select -- a row index r < rows reads valid_cnt[r] and info[r]; chunk
// indices are below ceil(rows / 64) <= 1024, the size of the LDS arrays; take[j] is written for j < B only.  take -- take[j] forms an
// address only when 0 <= take[j] < rows.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_sampler.h"
#include "../shared/lc_keyed_hash.h"
#include "../shared/lc_wave_int.h"

#ifndef LC_AMD_SAMPLER_SRC_HASH
#define LC_AMD_SAMPLER_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_SAMPLER_SRC_HASH:" LC_AMD_SAMPLER_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kRowThreads = 64;
constexpr int kSelectThreads = 1024;
constexpr int kSelectWaves = kSelectThreads / 64;
constexpr int kMaxChunks = LC_SAMPLER_MAX_ROWS / 64;
constexpr int kTakeThreads = 256;
constexpr unsigned kMaxTakeBlocks = 2048;
static_assert(kMaxChunks == kSelectThreads, "one thread scans one chunk's counts");

struct Table {
    const int* ints[6];      // frame_index, mask_index, mesh_index, obj_id, scene_id, im_id
    const float* bbox;
    const float* cam_K;
    const float* R;
    const float* t;
};

struct RowsOut {
    int* index;
    int* ints[6];
    float* bbox;
    float* cam_K;
    float* R;
    float* t;
    int* info;
};

// One pass of the balanced Feistel network on 2k bits
__device__ inline unsigned feistel_pass(unsigned x, int k, unsigned mask, const unsigned (&rk)[4]) {
    unsigned L = x >> k, H = x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned nH = L ^ (fmix32(rk[r] ^ H) & mask);
        L = H;
        H = nH;
    }
    return (L << k) | H;
}

// perm(seed0, e)(q) for q < N, 1 <= N < 2^31
__device__ inline unsigned permute(unsigned long long seed0, unsigned long long e, unsigned q, unsigned N) {
    const int bits = 32 - __clz((int)(N - 1u)) ;  // bitlength(N - 1): __clz(0) = 32
    const int k = max(1, (bits + 1) >> 1);
    const unsigned mask = (1u << k) - 1u;
    const unsigned es = fmix32(sample_state(sample_state(seed_state((unsigned)(seed0 & 0xffffffffull), (unsigned)(seed0 >> 32)), (unsigned)(e & 0xffffffffull)),
                                            (unsigned)(e >> 32)) ^ (unsigned)LC_SAMPLER_OP_PERM);
    const unsigned rk[4] = {fmix32(es ^ LC_SAMPLER_ROUND_0), fmix32(es ^ LC_SAMPLER_ROUND_1), fmix32(es ^ LC_SAMPLER_ROUND_2), fmix32(es ^ LC_SAMPLER_ROUND_3)};
    unsigned x = q;
    do {
        x = feistel_pass(x, k, mask, rk);
    } while (x >= N);
    return x;
}

__global__ __launch_bounds__(kRowThreads) void lc_sampler_rows_kernel(const unsigned long long* seed, unsigned long long seed0, int N, int B, int rows, const Table tb,
                                                                      const RowsOut o) {
    const int j = (int)(blockIdx.x * kRowThreads + threadIdx.x);
    if (j >= rows) return;
    const unsigned long long w = *seed;
    const unsigned long long step = w - seed0;
    bool bad = N < 1 || (step >> LC_SAMPLER_MAX_STEP_BITS) != 0;
    unsigned index = 0;
    int rec[6] = {-1, -1, -1, -1, -1, -1};
    if (!bad) {
        if (j < B) {
            const unsigned long long p = step * (unsigned long long)B + (unsigned long long)j;
            const unsigned long long e = p / (unsigned long long)N;
            index = permute(seed0, e, (unsigned)(p - e * (unsigned long long)N), (unsigned)N);
        } else {
            const unsigned key = fmix32(fmix32(sample_state(seed_state((unsigned)(w & 0xffffffffull), (unsigned)(w >> 32)), (unsigned)j) ^ (unsigned)LC_SAMPLER_OP_SPARE));
            index = (unsigned)(((unsigned long long)key * (unsigned long long)(unsigned)N) >> 32);
        }
#pragma unroll
        for (int f = 0; f < 6; ++f) rec[f] = tb.ints[f][index];
        bad = rec[0] < 0 || rec[1] < 0 || rec[2] < 0;
    }
    const float nan32 = __builtin_nanf("");
    o.index[j] = bad ? -1 : (int)index;
#pragma unroll
    for (int f = 0; f < 6; ++f) o.ints[f][j] = bad ? -1 : rec[f];
    o.info[j] = bad ? -1 : 0;
    float* bbox = o.bbox + 4 * (size_t)j;
    float* cam_K = o.cam_K + 9 * (size_t)j;
    float* R = o.R + 9 * (size_t)j;
    float* t = o.t + 3 * (size_t)j;
    if (bad) {
#pragma unroll
        for (int c = 0; c < 4; ++c) bbox[c] = nan32;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            cam_K[c] = nan32;
            R[c] = nan32;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = nan32;
        return;
    }
    const float* sb = tb.bbox + 4 * (size_t)index;
    const float* sK = tb.cam_K + 9 * (size_t)index;
    const float* sR = tb.R + 9 * (size_t)index;
    const float* st = tb.t + 3 * (size_t)index;
#pragma unroll
    for (int c = 0; c < 4; ++c) bbox[c] = sb[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        cam_K[c] = sK[c];
        R[c] = sR[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = st[c];
}

// The exclusive prefix of one value per thread over the 1024 threads of the workgroup, in thread order, and the total: shuffles within a
// wavefront, `waves` (16 ints of LDS) across them.  Every thread of the workgroup calls it.
__device__ inline int block_exclusive_scan(int v, int* waves, int& total) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    const int wave_total = wave_sum(v);
    __syncthreads();  // the previous use of `waves` is over
    if (lane == 0) waves[wave] = wave_total;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kSelectWaves; ++i) {
        const int s = waves[i];
        before += i < wave ? s : 0;
        all += s;
    }
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kSelectThreads) void lc_sampler_select_kernel(const int* __restrict__ valid_cnt, const int* __restrict__ info, int valid_th, int B, int rows,
                                                                           int* __restrict__ take, int* __restrict__ shortfall) {
    __shared__ unsigned long long bad_mask[kMaxChunks];    // the bad primaries of a chunk
    __shared__ unsigned long long spare_mask[kMaxChunks];  // the good spares of a chunk
    __shared__ int bad_before[kMaxChunks];                 // the bad primaries in the chunks before this one
    __shared__ int spare_before[kMaxChunks];               // the good spares in the chunks before this one
    __shared__ int waves[kSelectWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = (rows + 63) >> 6;

    for (int c = wave; c < kMaxChunks; c += kSelectWaves) {  // (uniform per wavefront: every lane reaches the ballot)
        unsigned long long bm = 0, sm = 0;
        if (c < chunks) {
            const int r = 64 * c + lane;
            const bool in = r < rows;
            const bool good = in && info[r] >= 0 && valid_cnt[r] >= valid_th;
            bm = __ballot(in && r < B && !good);
            sm = __ballot(r >= B && good);
        }
        if (lane == 0) {
            bad_mask[c] = bm;
            spare_mask[c] = sm;
        }
    }
    __syncthreads();
    int n_bad, n_spare;
    const int b_before = block_exclusive_scan(__popcll(bad_mask[tid]), waves, n_bad);
    const int s_before = block_exclusive_scan(__popcll(spare_mask[tid]), waves, n_spare);
    bad_before[tid] = b_before;
    spare_before[tid] = s_before;
    __syncthreads();

    for (int j = tid; j < B; j += kSelectThreads) {
        const int c = j >> 6;
        const unsigned long long bit = 1ull << (j & 63);
        int out = j;
        if (bad_mask[c] & bit) {
            const int i = bad_before[c] + __popcll(bad_mask[c] & (bit - 1ull));
            out = -1;
            if (i < n_spare) {
                int lo = 0, hi = chunks - 1;  // the last chunk with spare_before <= i: it holds the i-th good spare
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (spare_before[mid] <= i) lo = mid; else hi = mid - 1;
                }
                unsigned long long m = spare_mask[lo];
                for (int n = i - spare_before[lo]; n > 0; --n) m &= m - 1ull;
                out = 64 * lo + (__ffsll((long long)m) - 1);
            }
        }
        take[j] = out;
    }
    if (tid == 0) *shortfall = n_bad > n_spare ? n_bad - n_spare : 0;
}

struct TakeParams {
    const unsigned char* src[LC_SAMPLER_MAX_TENSORS];
    unsigned char* dst[LC_SAMPLER_MAX_TENSORS];
    unsigned long long row_bytes[LC_SAMPLER_MAX_TENSORS];
    const int* take;
    int B, rows;
};

__global__ __launch_bounds__(kTakeThreads) void lc_sampler_take_kernel(const TakeParams p) {
    const int k = (int)blockIdx.y;
    const unsigned char* src = p.src[k];
    unsigned char* dst = p.dst[k];
    const unsigned long long rb = p.row_bytes[k];
    const unsigned long long first = (unsigned long long)blockIdx.x * kTakeThreads + threadIdx.x, stride = (unsigned long long)gridDim.x * kTakeThreads;
    const bool wide = (((unsigned long long)reinterpret_cast<uintptr_t>(src) | (unsigned long long)reinterpret_cast<uintptr_t>(dst) | rb) & 15ull) == 0;
    if (wide) {
        const unsigned long long per_row = rb >> 4, units = per_row * (unsigned long long)p.B;
        for (unsigned long long u = first; u < units; u += stride) {
            const unsigned long long j = u / per_row, c = u - j * per_row;
            const int from = p.take[j];
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (from >= 0 && from < p.rows) v = reinterpret_cast<const uint4*>(src + (unsigned long long)from * rb)[c];
            reinterpret_cast<uint4*>(dst + j * rb)[c] = v;
        }
    } else {
        const unsigned long long units = rb * (unsigned long long)p.B;
        for (unsigned long long u = first; u < units; u += stride) {
            const unsigned long long j = u / rb, c = u - j * rb;
            const int from = p.take[j];
            unsigned char v = 0;
            if (from >= 0 && from < p.rows) v = src[(unsigned long long)from * rb + c];
            dst[u] = v;
        }
    }
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

int launched(const std::string& me) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(9, me + "launch: " + hipGetErrorString(e));
    return 0;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_sampler_version(void) { return LC_AMD_SAMPLER_VERSION; }
const char* lc_amd_sampler_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_SAMPLER_SRC_HASH:") - 1; }
const char* lc_amd_sampler_last_error(void) { return lc::g_err.c_str(); }

int lc_sampler_rows(const uint64_t* seed, uint64_t seed0, int N, int B, int S, const void* const* table, void* const* out, void* stream) {
    using lc::fail;
    const std::string me = "lc_sampler_rows: ";
    if (B < 1 || S < 0 || (long long)B + (long long)S > LC_SAMPLER_MAX_ROWS)
        return fail(1, me + "1 <= B, 0 <= S and B + S <= " + std::to_string(LC_SAMPLER_MAX_ROWS) + ", got B = " + std::to_string(B) + ", S = " + std::to_string(S));
    if (!seed) return fail(2, me + "seed must not be NULL: it points to one uint64 on the device");
    if (!out) return fail(2, me + "out must not be NULL: it holds " + std::to_string(LC_SAMPLER_ROWS_POINTERS) + " device pointers");
    if (N >= 1 && !table) return fail(2, me + "table must not be NULL: it holds " + std::to_string(LC_SAMPLER_TABLE_POINTERS) + " device pointers");
    if (lc::misaligned(seed, 8)) return fail(7, me + "seed must be aligned to 8 bytes");
    for (int i = 0; i < LC_SAMPLER_ROWS_POINTERS; ++i) {
        if (!out[i]) return fail(2, me + "out[" + std::to_string(i) + "] must not be NULL");
        if (lc::misaligned(out[i], 4)) return fail(7, me + "out[" + std::to_string(i) + "] must be aligned to 4 bytes");
    }
    for (int i = 0; N >= 1 && i < LC_SAMPLER_TABLE_POINTERS; ++i) {
        if (!table[i]) return fail(2, me + "table[" + std::to_string(i) + "] must not be NULL");
        if (lc::misaligned(table[i], 4)) return fail(7, me + "table[" + std::to_string(i) + "] must be aligned to 4 bytes");
    }
    lc::Table tb{};
    if (N >= 1) {
        for (int f = 0; f < 6; ++f) tb.ints[f] = static_cast<const int*>(table[f]);
        tb.bbox = static_cast<const float*>(table[6]);
        tb.cam_K = static_cast<const float*>(table[7]);
        tb.R = static_cast<const float*>(table[8]);
        tb.t = static_cast<const float*>(table[9]);
    }
    lc::RowsOut o{};
    o.index = static_cast<int*>(out[0]);
    for (int f = 0; f < 6; ++f) o.ints[f] = static_cast<int*>(out[1 + f]);
    o.bbox = static_cast<float*>(out[7]);
    o.cam_K = static_cast<float*>(out[8]);
    o.R = static_cast<float*>(out[9]);
    o.t = static_cast<float*>(out[10]);
    o.info = static_cast<int*>(out[11]);
    const int rows = B + S;
    const unsigned blocks = ((unsigned)rows + lc::kRowThreads - 1) / lc::kRowThreads;
    hipLaunchKernelGGL(lc::lc_sampler_rows_kernel, dim3(blocks), dim3(lc::kRowThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(seed), (unsigned long long)seed0, N, B, rows, tb, o);
    return lc::launched(me);
}

int lc_sampler_select_i32(const int* valid_cnt, const int* info, int valid_th, int B, int rows, int* take, int* shortfall, void* stream) {
    using lc::fail;
    const std::string me = "lc_sampler_select_i32: ";
    if (rows < 1 || rows > LC_SAMPLER_MAX_ROWS || B < 1 || B > rows)
        return fail(1, me + "1 <= B <= rows <= " + std::to_string(LC_SAMPLER_MAX_ROWS) + ", got B = " + std::to_string(B) + ", rows = " + std::to_string(rows));
    if (!valid_cnt || !info || !take || !shortfall) return fail(2, me + "valid_cnt, info, take and shortfall must not be NULL");
    if (lc::misaligned(valid_cnt, 4) || lc::misaligned(info, 4) || lc::misaligned(take, 4) || lc::misaligned(shortfall, 4))
        return fail(7, me + "valid_cnt, info, take and shortfall must be aligned to 4 bytes");
    hipLaunchKernelGGL(lc::lc_sampler_select_kernel, dim3(1), dim3(lc::kSelectThreads), 0, static_cast<hipStream_t>(stream), valid_cnt, info, valid_th, B, rows, take,
                       shortfall);
    return lc::launched(me);
}

int lc_sampler_take_rows(const int* take, int B, int rows, int n, const void* const* src, void* const* dst, const uint64_t* row_bytes, void* stream) {
    using lc::fail;
    const std::string me = "lc_sampler_take_rows: ";
    if (rows < 1 || rows > LC_SAMPLER_MAX_ROWS || B < 1 || B > LC_SAMPLER_MAX_ROWS)
        return fail(1, me + "1 <= B, rows <= " + std::to_string(LC_SAMPLER_MAX_ROWS) + ", got B = " + std::to_string(B) + ", rows = " + std::to_string(rows));
    if (n < 1 || n > LC_SAMPLER_MAX_TENSORS) return fail(3, me + "1 <= n <= " + std::to_string(LC_SAMPLER_MAX_TENSORS) + ", got " + std::to_string(n));
    if (!take || !src || !dst || !row_bytes) return fail(2, me + "take, src, dst and row_bytes must not be NULL");
    if (lc::misaligned(take, 4)) return fail(7, me + "take must be aligned to 4 bytes");
    lc::TakeParams p{};
    unsigned long long most = 0;
    for (int k = 0; k < n; ++k) {
        if (!src[k] || !dst[k]) return fail(2, me + "src[" + std::to_string(k) + "] and dst[" + std::to_string(k) + "] must not be NULL");
        if (row_bytes[k] < 1 || row_bytes[k] > LC_SAMPLER_MAX_ROW_BYTES)
            return fail(4, me + "1 <= row_bytes <= " + std::to_string(LC_SAMPLER_MAX_ROW_BYTES) + ", got " + std::to_string(row_bytes[k]) + " for tensor " + std::to_string(k));
        p.src[k] = static_cast<const unsigned char*>(src[k]);
        p.dst[k] = static_cast<unsigned char*>(dst[k]);
        p.row_bytes[k] = row_bytes[k];
        const bool wide = ((reinterpret_cast<uintptr_t>(src[k]) | reinterpret_cast<uintptr_t>(dst[k]) | row_bytes[k]) & 15) == 0;
        const unsigned long long units = (wide ? row_bytes[k] >> 4 : row_bytes[k]) * (unsigned long long)B;
        most = units > most ? units : most;
    }
    p.take = take; p.B = B; p.rows = rows;
    unsigned long long blocks = (most + lc::kTakeThreads - 1) / lc::kTakeThreads;
    blocks = blocks > lc::kMaxTakeBlocks ? lc::kMaxTakeBlocks : blocks;
    hipLaunchKernelGGL(lc::lc_sampler_take_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(lc::kTakeThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me);
}

}  // extern "C"
#pragma GCC visibility pop
