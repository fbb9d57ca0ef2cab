// Training mask crops on the GPU: the visible masks that lc_gtinfo_f32 leaves on the device as bytes, warped into the network's crop
// (msk_vis, msk_noc), the count of valid pixels and the symmetry check points drawn from them (liblc_amd_maskcrop.so; C ABI and the
// exact definition of every output in include/lc_amd_maskcrop.h; tests/maskcrop_oracle.py is its numpy restatement).  What the
// reference's loader does per instance on a host core (dataset.py:414,425-442).
//
// Warp launch, as in lc_crop.hip (shared/lc_warp_grid.h): four waves per (row, band of crop rows).  Thread 0 forms the row's inverse in fp64
// and judges the row; a thread owns four consecutive x (its two x terms are formed once) and walks the band's rows.  Per pixel the ONE
// pair of 64-bit sums gives both coordinate sets (+ 512 for the nearest tap, + 16 for the four linear ones); the taps are bytes of the
// window, each judged on its own against the window; the linear value is an integer k <= 1024 times 2^-10.  A thread stores four
// pixels of msk_vis with one 16-byte store and four of msk_noc with one 4-byte store where w and the pointers allow it.  The valid
// pixels are summed per lane, across the wavefront, across the four wavefronts in 16 bytes of LDS, and one thread adds a non-zero
// sum to valid_cnt[b] with an integer atomic: the count cannot depend on the order.  A launch of its own zeroes the counts in-stream.
//
// Check-point launch: one workgroup of sixteen waves per row.  A pixel's sort key is the 48-bit composite (key_r(p) << 16) | p, unique
// per pixel (p < 65 536).  valid_cnt >= n_check is one round: a radix select on the composite, eight bits per pass (an LDS histogram
// of the pixels that share the prefix found so far, a wave scan to find the bucket that holds the n_check-th smallest), which ends as
// soon as the bucket is taken whole -- for hashed keys after two or three passes; the n_check <= 256 survivors are gathered in LDS and
// ranked by counting.  valid_cnt < n_check is up to 256 rounds that each sort ALL valid pixels, fewer than 256: the list is gathered
// once and every (round, pixel) item counts its own rank among the round's keys, with no barrier between rounds.
//
// Bounds: every tap is range-checked against the window on its own (that IS the border rule), a bad row sees a window of size zero, the
// mask index is checked before it is used, and every LDS slot handed out by an atomic is checked against the array.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_maskcrop.h"
#include "../shared/lc_keyed_hash.h"
#include "../shared/lc_warp_grid.h"
#include "../shared/lc_wave_int.h"

#ifndef LC_AMD_MASKCROP_SRC_HASH
#define LC_AMD_MASKCROP_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_MASKCROP_SRC_HASH:" LC_AMD_MASKCROP_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kCkThreads = 1024;
constexpr int kMaxCheck = LC_MASKCROP_MAX_CHECK;
constexpr int kMinBand = 16;  // crop rows per workgroup (more where a pass of the workgroup covers more)

struct Params {
    const unsigned char* masks;  // (F,Hm,Wm)
    const int* mask_index;       // (B) or null
    const int* origin;           // (B,2) or null
    const float* M;              // (B,2,3)
    const int* sample_id;        // (B) or null
    float* vis;                  // (B,h,w) or null
    unsigned char* noc;          // (B,h,w) or null (an output, or the workspace's copy for the check points)
    int* cnt;                    // (B) or null (likewise)
    void* ck;                    // (B,n_check,2) int32 / int64
    int* info;                   // (B) or null
    int F, Hm, Wm, B, h, w;
    WarpGrid grid;
    int vec_vis, vec_noc;        // four-pixel stores are possible
    int valid_th, n_check, ck64;
    unsigned seed_lo, seed_hi;
};

__global__ __launch_bounds__(kThreads) void lc_mask_zero_kernel(int* cnt, int B) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b < B) cnt[b] = 0;
}

template <bool LINEAR>
__global__ __launch_bounds__(kThreads) void lc_mask_warp_kernel(const Params p) {
    __shared__ double s_inv[6];
    __shared__ int s_src[3];  // the mask (-1 = bad row), x0, y0
    __shared__ int s_cnt[kWaves];

    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.grid.nbands, band = blockIdx.x - b * p.grid.nbands;
    if (tid == 0) {
        const int f = p.mask_index ? p.mask_index[b] : b;
        const int ox = p.origin ? p.origin[2 * (size_t)b] : 0, oy = p.origin ? p.origin[2 * (size_t)b + 1] : 0;
        bool ok = f >= 0 && f < p.F;
        ok = ok && ox >= -LC_MASKCROP_MAX_ORIGIN && ox <= LC_MASKCROP_MAX_ORIGIN && oy >= -LC_MASKCROP_MAX_ORIGIN && oy <= LC_MASKCROP_MAX_ORIGIN;
        ok = inverse_of(p.M + 6 * (size_t)b, ok, s_inv);
        s_src[0] = ok ? f : -1;
        s_src[1] = ok ? ox : 0;
        s_src[2] = ok ? oy : 0;
        if (band == 0 && p.info) p.info[b] = ok ? 0 : -1;
    }
    __syncthreads();

    const int f = s_src[0], ox = s_src[1], oy = s_src[2];
    const int Hm = f >= 0 ? p.Hm : 0, Wm = f >= 0 ? p.Wm : 0;  // a bad row: every tap is outside
    const unsigned char* src = p.masks + (size_t)(f >= 0 ? f : 0) * p.Hm * p.Wm;
    const double m00 = s_inv[0], m01 = s_inv[1], b1 = s_inv[2], m10 = s_inv[3], m11 = s_inv[4], b2 = s_inv[5];
    const size_t row0 = (size_t)b * p.h * p.w;
    float* vis = p.vis ? p.vis + row0 : nullptr;
    unsigned char* noc = p.noc ? p.noc + row0 : nullptr;

    const int TX = 1 << p.grid.lg_tx, TY = kThreads >> p.grid.lg_tx;
    const int tx = tid & (TX - 1), ty = tid >> p.grid.lg_tx;
    const int quads = (p.w + 3) >> 2;
    const int y_end = min(p.h, (band + 1) * p.grid.band);

    // frame pixel (xx, yy) as 0 / 1: the window's byte, 0 outside the window
    auto tap = [&](int xx, int yy) -> int {
        const int u = xx - ox, v = yy - oy;
        int s = 0;
        if ((unsigned)u < (unsigned)Wm && (unsigned)v < (unsigned)Hm) s = src[(size_t)v * Wm + u] != 0 ? 1 : 0;
        return s;
    };

    int count = 0;
    for (int xq = tx; xq < quads; xq += TX) {
        const int x0 = xq << 2;
        int ax[4], ay[4];
        quad_terms(m00, m10, x0, ax, ay);
        for (int y = band * p.grid.band + ty; y < y_end; y += TY) {
            const long long X0 = row_term(m01, b1, y), Y0 = row_term(m11, b2, y);
            float rv[4];
            unsigned bits = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long X = X0 + ax[j], Y = Y0 + ay[j];
                const int n = tap(nearest_tap(X + kNearestDelta), nearest_tap(Y + kNearestDelta));
                if (x0 + j < p.w) count += n;
                bits |= (unsigned)n << (8 * j);
                if constexpr (LINEAR) {
                    const auto [sx, sy, fx, fy] = linear_taps(X + kLinearDelta, Y + kLinearDelta);
                    const int k = (32 - fx) * (32 - fy) * tap(sx, sy) + fx * (32 - fy) * tap(sx + 1, sy) + (32 - fx) * fy * tap(sx, sy + 1) +
                                  fx * fy * tap(sx + 1, sy + 1);
                    rv[j] = (float)k * 0.0009765625f;  // k 2^-10: exact
                } else {
                    rv[j] = (float)n;
                }
            }
            const size_t o = (size_t)y * p.w + x0;
            if (vis) {
                if (p.vec_vis) {
                    *reinterpret_cast<float4*>(vis + o) = make_float4(rv[0], rv[1], rv[2], rv[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < p.w) vis[o + j] = rv[j];
                }
            }
            if (noc) {
                if (p.vec_noc) {
                    *reinterpret_cast<unsigned*>(noc + o) = bits;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < p.w) noc[o + j] = (unsigned char)((bits >> (8 * j)) & 0xff);
                }
            }
        }
    }

    if (p.cnt) {  // uniform over the launch
        const int total = wave_sum(count);
        if ((tid & (kWave - 1)) == 0) s_cnt[tid >> 6] = total;
        __syncthreads();
        if (tid == 0) {
            int v = 0;
#pragma unroll
            for (int wv = 0; wv < kWaves; ++wv) v += s_cnt[wv];
            if (v != 0) atomicAdd(p.cnt + b, v);
        }
    }
}

// (key << 16) | p of pixel p under the round's state
__device__ __forceinline__ unsigned long long composite(unsigned round_state, unsigned q) {
    return ((unsigned long long)fmix32(round_state ^ q) << 16) | q;
}

__device__ __forceinline__ void put_point(const Params& p, int b, int pos, int x, int y) {
    const size_t o = ((size_t)b * p.n_check + pos) * 2;
    if (p.ck64) {
        long long* out = static_cast<long long*>(p.ck) + o;
        out[0] = x;
        out[1] = y;
    } else {
        int* out = static_cast<int*>(p.ck) + o;
        out[0] = x;
        out[1] = y;
    }
}

__global__ __launch_bounds__(kCkThreads) void lc_mask_check_kernel(const Params p) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned long long s_c[kMaxCheck];
    __shared__ unsigned s_sel[3];  // the bucket, the count below it, its own count
    __shared__ int s_n;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = p.n_check, hw = p.h * p.w, w = p.w;
    const int V = p.cnt[b];
    if (V <= 0 || V < p.valid_th) {  // the whole workgroup; a bad row has counted nothing
        for (int i = tid; i < N; i += kCkThreads) put_point(p, b, i, -1, -1);
        return;
    }
    const unsigned char* noc = p.noc + (size_t)b * hw;
    const unsigned k = sample_state(seed_state(p.seed_lo, p.seed_hi), (unsigned)(p.sample_id ? p.sample_id[b] : b));
    if (tid == 0) s_n = 0;
    __syncthreads();

    if (V < N) {
        // rounds that each list every valid pixel: gather them once (their order in LDS does not matter, a rank is a count)
        for (int q = tid; q < hw; q += kCkThreads)
            if (noc[q]) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < kMaxCheck) s_c[slot] = (unsigned long long)q;
            }
        __syncthreads();
        const int n = min(s_n, kMaxCheck);
        if (n <= 0) return;
        const int rounds = (N + n - 1) / n, items = rounds * n;
        for (int it = tid; it < items; it += kCkThreads) {
            const int r = it / n, i = it - r * n;
            const unsigned kr = fmix32(k ^ (unsigned)r);
            const unsigned q = (unsigned)s_c[i];
            const unsigned long long c = composite(kr, q);
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += composite(kr, (unsigned)s_c[j]) < c ? 1 : 0;
            const int pos = r * n + rank;
            if (pos < N) put_point(p, b, pos, (int)(q % (unsigned)w), (int)(q / (unsigned)w));
        }
        return;
    }

    // one round: the N smallest composites of V >= N, by a radix select from the top byte down
    const unsigned k0 = fmix32(k);  // round 0
    unsigned long long prefix = 0;
    unsigned remaining = (unsigned)N;
    int shift = 40;
    for (int pass = 0; pass < 6; ++pass) {
        shift = 40 - 8 * pass;
        for (int i = tid; i < 256; i += kCkThreads) s_hist[i] = 0;
        __syncthreads();
        if (tid == 0) {  // behind the barrier: every thread has read the pass before
            s_sel[0] = 255u;
            s_sel[1] = 0u;
            s_sel[2] = 0u;
        }
        for (int q = tid; q < hw; q += kCkThreads)
            if (noc[q]) {
                const unsigned long long c = composite(k0, (unsigned)q);
                if ((c >> (shift + 8)) == prefix) atomicAdd(&s_hist[(unsigned)(c >> shift) & 255u], 1u);
            }
        __syncthreads();
        if (tid < kWave) {  // the first wavefront, whole: four bins per lane, an inclusive scan across the lanes
            unsigned a[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = s_hist[4 * tid + j];
                s += a[j];
            }
            unsigned incl = s;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const unsigned t = __shfl_up(incl, d, kWave);
                if (tid >= d) incl += t;
            }
            unsigned below = incl - s;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (below < remaining && remaining <= below + a[j]) {  // true for exactly one bin
                    s_sel[0] = (unsigned)(4 * tid + j);
                    s_sel[1] = below;
                    s_sel[2] = a[j];
                }
                below += a[j];
            }
        }
        __syncthreads();
        const unsigned bucket = s_sel[0], below = s_sel[1], held = s_sel[2];
        prefix = (prefix << 8) | bucket;
        remaining -= below;
        if (held == remaining) break;  // the bucket is taken whole (uniform: read from LDS behind a barrier)
    }
    // everything whose leading bits are at most the prefix: exactly N pixels
    for (int q = tid; q < hw; q += kCkThreads)
        if (noc[q]) {
            const unsigned long long c = composite(k0, (unsigned)q);
            if ((c >> shift) <= prefix) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < kMaxCheck) s_c[slot] = c;
            }
        }
    __syncthreads();
    const int n = min(s_n, kMaxCheck);
    for (int i = tid; i < n; i += kCkThreads) {
        const unsigned long long c = s_c[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += s_c[j] < c ? 1 : 0;
        const unsigned q = (unsigned)(c & 0xffffull);
        if (rank < N) put_point(p, b, rank, (int)(q % (unsigned)w), (int)(q / (unsigned)w));
    }
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_maskcrop_version(void) { return LC_AMD_MASKCROP_VERSION; }
const char* lc_amd_maskcrop_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_MASKCROP_SRC_HASH:") - 1; }
const char* lc_amd_maskcrop_last_error(void) { return lc::g_err.c_str(); }

size_t lc_mask_crops_workspace_bytes(int B, int h, int w, int n_check, int has_msk_noc, int has_valid_cnt) {
    if (B < 1 || h < 1 || w < 1 || n_check < 1) return 0;
    size_t n = 0;
    if (!has_valid_cnt) n += (size_t)B * sizeof(int);
    if (!has_msk_noc) n += lc::round4((size_t)B * (size_t)h * (size_t)w);
    return n;
}

int lc_mask_crops_u8(const unsigned char* masks, int F, int Hm, int Wm, const int* mask_index, const int* origin_xy, const float* M, int B, int h,
                     int w, int vis_interp, int valid_th, int n_check, uint64_t seed, const int* sample_id, int ck_dtype, float* msk_vis,
                     unsigned char* msk_noc, int* valid_cnt, void* sym_ck, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    using lc::fail;
    const std::string me = "lc_mask_crops_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (F < 0) return fail(2, me + "F < 0");
    const int lim = LC_MASKCROP_MAX_SIZE;
    if (Hm < 1 || Wm < 1 || Hm > lim || Wm > lim || h < 1 || w < 1 || h > lim || w > lim)
        return fail(3, me + "mask and crop sizes must be in [1, " + std::to_string(lim) + "], got " + std::to_string(Hm) + " x " + std::to_string(Wm) + " -> " +
                           std::to_string(h) + " x " + std::to_string(w));
    if (vis_interp != LC_MASKCROP_NEAREST && vis_interp != LC_MASKCROP_LINEAR) return fail(4, me + "vis_interp must be LC_MASKCROP_NEAREST or LC_MASKCROP_LINEAR");
    if (n_check < 0 || n_check > LC_MASKCROP_MAX_CHECK) return fail(5, me + "n_check must be in [0, " + std::to_string(LC_MASKCROP_MAX_CHECK) + "], got " + std::to_string(n_check));
    if (ck_dtype != LC_MASKCROP_I32 && ck_dtype != LC_MASKCROP_I64) return fail(6, me + "ck_dtype must be LC_MASKCROP_I32 or LC_MASKCROP_I64");
    const bool checks = n_check > 0 && sym_ck != nullptr;
    if (checks && (long long)h * w > LC_MASKCROP_MAX_CHECK_PIXELS)
        return fail(7, me + "check points need a crop of at most " + std::to_string(LC_MASKCROP_MAX_CHECK_PIXELS) + " pixels, got " + std::to_string(h) + " x " + std::to_string(w));
    if (!M || (F > 0 && !masks)) return fail(8, me + "masks and M must not be NULL");
    if (lc::misaligned(M, 4) || lc::misaligned(mask_index, 4) || lc::misaligned(origin_xy, 4) || lc::misaligned(sample_id, 4) || lc::misaligned(msk_vis, 4) ||
        lc::misaligned(valid_cnt, 4) || lc::misaligned(info, 4) || lc::misaligned(sym_ck, ck_dtype == LC_MASKCROP_I64 ? 8 : 4) || lc::misaligned(workspace, 4))
        return fail(9, me + "M, the int32 arrays, msk_vis, sym_ck and the workspace must be aligned to their element");

    lc::Params p{};
    p.masks = masks; p.mask_index = mask_index; p.origin = origin_xy; p.M = M; p.sample_id = sample_id;
    p.vis = msk_vis; p.noc = msk_noc; p.cnt = valid_cnt; p.ck = sym_ck; p.info = info;
    p.F = F; p.Hm = Hm; p.Wm = Wm; p.B = B; p.h = h; p.w = w;
    p.valid_th = valid_th; p.n_check = n_check; p.ck64 = ck_dtype == LC_MASKCROP_I64;
    p.seed_lo = (unsigned)(seed & 0xffffffffull); p.seed_hi = (unsigned)(seed >> 32);
    if (checks) {
        const size_t need = lc_mask_crops_workspace_bytes(B, h, w, n_check, msk_noc != nullptr, valid_cnt != nullptr);
        if (need > 0 && (!workspace || workspace_bytes < need))
            return fail(10, me + "the workspace is smaller than lc_mask_crops_workspace_bytes (" + std::to_string(need) + " bytes)");
        unsigned char* ws = static_cast<unsigned char*>(workspace);
        if (!p.cnt) {
            p.cnt = reinterpret_cast<int*>(ws);
            ws += (size_t)B * sizeof(int);
        }
        if (!p.noc) p.noc = ws;
    }
    p.grid = lc::warp_grid(h, w, lc::kThreads, lc::kMinBand);
    p.vec_vis = (w % 4 == 0) && !lc::misaligned(p.vis, 16);
    p.vec_noc = (w % 4 == 0) && !lc::misaligned(p.noc, 4);
    const long long blocks = (long long)B * p.grid.nbands;
    if (blocks > 0x7fffffffLL) return fail(11, me + "too many rows and bands for one launch");

    hipStream_t s = static_cast<hipStream_t>(stream);
    auto launched = [&](const char* what) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail(12, me + what + " launch: " + hipGetErrorString(e));
    };
    if (p.cnt) {
        hipLaunchKernelGGL(lc::lc_mask_zero_kernel, dim3((unsigned)((B + lc::kThreads - 1) / lc::kThreads)), dim3(lc::kThreads), 0, s, p.cnt, B);
        if (int rc = launched("zero")) return rc;
    }
    if (vis_interp == LC_MASKCROP_LINEAR) hipLaunchKernelGGL(lc::lc_mask_warp_kernel<true>, dim3((unsigned)blocks), dim3(lc::kThreads), 0, s, p);
    else hipLaunchKernelGGL(lc::lc_mask_warp_kernel<false>, dim3((unsigned)blocks), dim3(lc::kThreads), 0, s, p);
    if (int rc = launched("warp")) return rc;
    if (checks) {
        hipLaunchKernelGGL(lc::lc_mask_check_kernel, dim3((unsigned)B), dim3(lc::kCkThreads), 0, s, p);
        if (int rc = launched("check point")) return rc;
    }
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
