// The device-resident store of COCO run-length masks (liblc_amd_rle.so; C ABI, the format and the exact definition of every output in
// include/lc_amd_rle.h; tests/rle_oracle.py is its numpy restatement).  What the reference's loader does per sample on a host core
// through pycocotools (dataset.py:174-182,379).
//
// Index launch: one workgroup of four waves per mask.  The counts are taken 256 at a time; a wave scans its 64 in 64 bits across the
// lanes, the four wave totals meet in LDS (two buffers, one barrier per chunk) and a running carry joins the chunks.  A thread knows
// the first and last position of its own run from its inclusive sum alone, so area and box are per-thread sums, minima and maxima that
// are reduced once at the end.
//
// Decode launch: the store is column-major, the output row-major.  One workgroup per (row, 256 window columns, band of 32 window rows):
// a lane owns one window column, finds the run of its first in-frame position by bisection in `ends` and walks down the band's rows
// advancing its run, so that a wave's byte stores of one row step lie side by side in one row of the output.  Thread 0 judges the row.
//
// Encode launch: one workgroup of sixteen waves per mask, a lane per frame column, 1024 columns at a time.  A boundary is a position
// whose value differs from the one before it (before position 0: 0).  Pass one counts a column's boundaries and keeps the last; a scan
// of (count, last position) over the columns -- across the lanes, across the waves through LDS, a carry across the chunks -- gives
// every column the rank and position of the boundary before its first; pass two walks the column again and writes each difference
// where its rank says.  No atomic takes part: the list cannot depend on an order.
//
// Bounds: offsets, sizes, indices and origins are judged before they are used, every index into `ends` lies in [base, base + n) of a
// judged mask, every byte of a window is addressed from in-window coordinates, and every write to counts_out is checked against cap.
// The few lines of wave arithmetic are written out here: the scans are 64-bit and paired, other types than shared/lc_wave_int.h folds.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_rle.h"

#ifndef LC_AMD_RLE_SRC_HASH
#define LC_AMD_RLE_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_RLE_SRC_HASH:" LC_AMD_RLE_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kWave = 64;
constexpr int kThreads = 256;  // index, decode
constexpr int kWaves = kThreads / kWave;
constexpr int kBand = 32;      // window rows per decode workgroup
constexpr int kEncThreads = 1024;
constexpr int kEncWaves = kEncThreads / kWave;
constexpr int kMaxSize = LC_RLE_MAX_SIZE;
constexpr int kMaxOrigin = LC_RLE_MAX_ORIGIN;

struct Mask {
    long long base, n;  // counts[base .. base + n)
    int H, W;
};

// Mask f as its offsets and size allow it: a mask that fails is empty and sized 1 x 1
__device__ __forceinline__ bool judged(const long long* offsets, const int* sizes, long long T, int f, Mask& m) {
    const long long a = offsets[f], b = offsets[(size_t)f + 1];
    const int H = sizes[2 * (size_t)f], W = sizes[2 * (size_t)f + 1];
    const bool ok = a >= 0 && a <= b && b <= T && H >= 1 && H <= kMaxSize && W >= 1 && W <= kMaxSize;
    m.base = ok ? a : 0;
    m.n = ok ? b - a : 0;
    m.H = ok ? H : 1;
    m.W = ok ? W : 1;
    return ok;
}

struct IndexParams {
    const unsigned* counts;
    const long long* offsets;
    const int* sizes;
    long long T;
    unsigned* ends;
    int *area, *box, *valid;
};

__global__ __launch_bounds__(kThreads) void lc_rle_index_kernel(const IndexParams p) {
    __shared__ unsigned long long s_tot[2][kWaves];
    __shared__ int s_red[kWaves][5];  // area, x_min, y_min, x_max, y_max

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    Mask m;
    const bool ok = judged(p.offsets, p.sizes, p.T, f, m);
    const unsigned long long HW = (unsigned long long)m.H * (unsigned long long)m.W;
    const unsigned H = (unsigned)m.H;

    unsigned long long carry = 0;
    int area = 0, x_min = 0x7fffffff, y_min = 0x7fffffff, x_max = -1, y_max = -1;
    int buf = 0;
    for (long long k0 = 0; k0 < m.n; k0 += kThreads, buf ^= 1) {  // uniform over the workgroup
        const long long k = k0 + tid;
        const unsigned c = k < m.n ? p.counts[m.base + k] : 0u;
        unsigned long long incl = c;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += t;
        }
        if (lane == kWave - 1) s_tot[buf][wv] = incl;
        __syncthreads();
        unsigned long long before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const unsigned long long t = s_tot[buf][w];
            if (w < wv) before += t;
            total += t;
        }
        const unsigned long long end = before + incl;
        if (k < m.n) {
            p.ends[m.base + k] = (unsigned)end;
            if ((k & 1) && c > 0 && end <= HW) {  // a run of ones that lies in the frame: positions end - c .. end - 1
                const unsigned s = (unsigned)end - c, e = (unsigned)end - 1u;
                const unsigned xs = s / H, xe = e / H;
                const int ys = (int)(s - xs * H), ye = (int)(e - xe * H);
                area += (int)c;
                x_min = min(x_min, (int)xs);
                x_max = max(x_max, (int)xe);
                y_min = min(y_min, xs == xe ? ys : 0);
                y_max = max(y_max, xs == xe ? ye : (int)H - 1);
            }
        }
        carry += total;
    }

#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        area += __shfl_xor(area, d, kWave);
        x_min = min(x_min, __shfl_xor(x_min, d, kWave));
        y_min = min(y_min, __shfl_xor(y_min, d, kWave));
        x_max = max(x_max, __shfl_xor(x_max, d, kWave));
        y_max = max(y_max, __shfl_xor(y_max, d, kWave));
    }
    if (lane == 0) {
        s_red[wv][0] = area;
        s_red[wv][1] = x_min;
        s_red[wv][2] = y_min;
        s_red[wv][3] = x_max;
        s_red[wv][4] = y_max;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            area += s_red[w][0];
            x_min = min(x_min, s_red[w][1]);
            y_min = min(y_min, s_red[w][2]);
            x_max = max(x_max, s_red[w][3]);
            y_max = max(y_max, s_red[w][4]);
        }
        const bool good = ok && carry == HW;
        const bool any = good && area > 0;
        p.valid[f] = good ? 0 : -1;
        p.area[f] = good ? area : 0;
        int* box = p.box + 4 * (size_t)f;
        box[0] = any ? x_min : -1;
        box[1] = any ? y_min : -1;
        box[2] = any ? x_max : -1;
        box[3] = any ? y_max : -1;
    }
}

struct DecodeParams {
    const unsigned* ends;
    const long long* offsets;
    const int* sizes;
    const int* valid;
    long long T;
    const int* mask_index;  // (B) or null
    const int* origin;      // (B,2) or null
    unsigned char* out;     // (B,Hm,Wm)
    int* info;              // (B) or null
    int F, Hm, Wm, tiles, bands;
};

__global__ __launch_bounds__(kThreads) void lc_rle_decode_kernel(const DecodeParams p) {
    __shared__ int s_f;  // the mask, -1 for a refused row
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % p.tiles, rest = blockIdx.x / p.tiles;
    const int band = rest % p.bands, b = rest / p.bands;
    int ox = p.origin ? p.origin[2 * (size_t)b] : 0, oy = p.origin ? p.origin[2 * (size_t)b + 1] : 0;
    if (tid == 0) {
        const int f = p.mask_index ? p.mask_index[b] : b;
        bool ok = f >= 0 && f < p.F;
        ok = ok && ox >= -kMaxOrigin && ox <= kMaxOrigin && oy >= -kMaxOrigin && oy <= kMaxOrigin;
        ok = ok && p.valid[f] == 0;
        s_f = ok ? f : -1;
        if (tile == 0 && band == 0 && p.info) p.info[b] = ok ? 0 : -1;
    }
    __syncthreads();
    const int f = s_f;
    if (f < 0) ox = oy = 0;  // a refused origin takes no part in any sum

    const int j = tile * kThreads + tid;
    if (j >= p.Wm) return;  // no barrier follows
    const int i0 = band * kBand, i1 = min(p.Hm, i0 + kBand);
    unsigned char* out = p.out + ((size_t)b * p.Hm + i0) * p.Wm + j;

    Mask m{0, 0, 1, 1};
    bool ok = f >= 0;
    if (ok) ok = judged(p.offsets, p.sizes, p.T, f, m) && m.n > 0;  // what the index judged, judged again: `valid` is the caller's memory
    const int x = ox + j;
    // the band's rows inside the frame, as window rows [ia, ib)
    const int ia = max(i0, -oy), ib = min(i1, m.H - oy);
    const bool live = ok && x >= 0 && x < m.W && ia < ib;

    unsigned pos = 0, end = 0;
    long long k = 0;
    const unsigned* ends = p.ends + m.base;
    if (live) {
        pos = (unsigned)x * (unsigned)m.H + (unsigned)(oy + ia);
        long long lo = 0, hi = m.n - 1;  // the first run that ends behind pos
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (ends[mid] > pos) hi = mid;
            else lo = mid + 1;
        }
        k = lo;
        end = ends[k];
    }
    for (int i = i0; i < i1; ++i, out += p.Wm) {
        unsigned char v = 0;
        if (live && i >= ia && i < ib) {
            while (pos >= end && k + 1 < m.n) end = ends[++k];
            v = (unsigned char)((k & 1) != 0 && pos < end ? 1 : 0);
            ++pos;
        }
        *out = v;
    }
}

struct EncodeParams {
    const unsigned char* masks;  // (F,Hm,Wm)
    const int* sizes;            // (F,2) or null
    const int* origin;           // (F,2) or null
    unsigned* counts_out;        // (F,cap)
    int* n_runs;
    int* info;                   // (F) or null
    int Hm, Wm, cap;
};

__global__ __launch_bounds__(kEncThreads) void lc_rle_encode_kernel(const EncodeParams p) {
    __shared__ int s_cnt[2][kEncWaves];
    __shared__ unsigned s_last[2][kEncWaves];  // 1 + the position of a wave's last boundary, 0 for none

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int H = p.sizes ? p.sizes[2 * (size_t)f] : p.Hm, W = p.sizes ? p.sizes[2 * (size_t)f + 1] : p.Wm;
    const int ox = p.origin ? p.origin[2 * (size_t)f] : 0, oy = p.origin ? p.origin[2 * (size_t)f + 1] : 0;
    unsigned* row = p.counts_out + (size_t)f * p.cap;
    const bool ok = H >= 1 && H <= kMaxSize && W >= 1 && W <= kMaxSize && ox >= -kMaxOrigin && ox <= kMaxOrigin && oy >= -kMaxOrigin && oy <= kMaxOrigin;
    if (!ok) {  // the whole workgroup
        for (int i = tid; i < p.cap; i += kEncThreads) row[i] = 0u;
        if (tid == 0) {
            p.n_runs[f] = 0;
            if (p.info) p.info[f] = -1;
        }
        return;
    }
    const unsigned char* src = p.masks + (size_t)f * p.Hm * p.Wm;
    // the window inside the frame: columns [xa, xb), rows [ya, yb) of the frame
    const int xa = max(ox, 0), xb = min(ox + p.Wm, W), ya = max(oy, 0), yb = min(oy + p.Hm, H);
    const bool empty = xa >= xb || ya >= yb;
    const int ncols = empty ? 0 : (xb - xa) + (xb < W ? 1 : 0);  // the column behind the window closes a run that ends with it

    // The boundaries of frame column x in the order of their positions.  Only positions of the window's rows, the one below them and
    // row 0 can differ from the position before; the column behind the window has row 0 alone.
    auto walk = [&](int x, auto&& boundary) {
        // the last pixel of the column before, where the window holds it
        const bool above = x - 1 >= xa && yb == H && src[(size_t)(H - 1 - oy) * p.Wm + (x - 1 - ox)] != 0;
        bool prev = above;
        if (x == xb || ya > 0) {  // row 0 lies outside the window
            if (above) boundary((unsigned)x * (unsigned)H);
            prev = false;
        }
        if (x < xb) {
            const unsigned char* q = src + (size_t)(ya - oy) * p.Wm + (x - ox);
            unsigned pos = (unsigned)x * (unsigned)H + (unsigned)ya;
            for (int y = ya; y < yb; ++y, ++pos, q += p.Wm) {
                const bool cur = *q != 0;
                if (cur != prev) boundary(pos);
                prev = cur;
            }
            if (yb < H && prev) boundary(pos);
        }
    };

    int carry_cnt = 0;
    unsigned carry_last = 0;
    int buf = 0;
    for (int c0 = 0; c0 < ncols; c0 += kEncThreads, buf ^= 1) {  // uniform over the workgroup
        const int x = xa + c0 + tid;
        const bool mine = c0 + tid < ncols;
        int cnt = 0;
        unsigned last = 0;
        if (mine) walk(x, [&](unsigned pos) {
            ++cnt;
            last = pos + 1u;
        });
        int icnt = cnt;
        unsigned ilast = last;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int tc = __shfl_up(icnt, d, kWave);
            const unsigned tl = __shfl_up(ilast, d, kWave);
            if (lane >= d) {
                icnt += tc;
                ilast = max(ilast, tl);
            }
        }
        if (lane == kWave - 1) {
            s_cnt[buf][wv] = icnt;
            s_last[buf][wv] = ilast;
        }
        __syncthreads();
        int rank = carry_cnt, total = 0;
        unsigned before = carry_last, all_last = carry_last;
#pragma unroll
        for (int w = 0; w < kEncWaves; ++w) {
            const int tc = s_cnt[buf][w];
            const unsigned tl = s_last[buf][w];
            if (w < wv) {
                rank += tc;
                before = max(before, tl);
            }
            total += tc;
            all_last = max(all_last, tl);
        }
        // exclusive over the lanes: what lies before this column
        const int ec = __shfl_up(icnt, 1, kWave);
        const unsigned el = __shfl_up(ilast, 1, kWave);
        if (lane > 0) {
            rank += ec;
            before = max(before, el);
        }
        if (mine && cnt > 0) {
            unsigned from = before > 0 ? before - 1u : 0u;
            walk(x, [&](unsigned pos) {
                if (rank < p.cap) row[rank] = pos - from;
                from = pos;
                ++rank;
            });
        }
        carry_cnt += total;
        carry_last = all_last;
    }
    // the run that ends with the frame
    const int n = carry_cnt + 1;
    const unsigned HW = (unsigned)H * (unsigned)W;
    if (tid == 0) {
        if (carry_cnt < p.cap) row[carry_cnt] = HW - (carry_last > 0 ? carry_last - 1u : 0u);
        p.n_runs[f] = n;
        if (p.info) p.info[f] = n > p.cap ? -2 : 0;
    }
    __syncthreads();  // the list is written: zero what lies behind it, or all of it where it did not fit
    for (int i = (n > p.cap ? 0 : n) + tid; i < p.cap; i += kEncThreads) row[i] = 0u;
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

int launched(const std::string& me, const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(20, me + what + " launch: " + hipGetErrorString(e));
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_rle_version(void) { return LC_AMD_RLE_VERSION; }
const char* lc_amd_rle_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_RLE_SRC_HASH:") - 1; }
const char* lc_amd_rle_last_error(void) { return lc::g_err.c_str(); }

int lc_rle_index_u32(const uint32_t* counts, const int64_t* offsets, const int* sizes, int64_t T, int F, uint32_t* ends, int* area, int* box, int* valid,
                     void* stream) {
    using lc::fail;
    const std::string me = "lc_rle_index_u32: ";
    if (F < 0) return fail(1, me + "F < 0");
    if (F == 0) return 0;
    if (T < 0 || T > (int64_t)LC_RLE_MAX_COUNTS) return fail(2, me + "T must be in [0, " + std::to_string((long long)LC_RLE_MAX_COUNTS) + "], got " + std::to_string((long long)T));
    if (!offsets || !sizes || !area || !box || !valid || (T > 0 && (!counts || !ends))) return fail(3, me + "the store and the outputs must not be NULL");
    if (lc::misaligned(counts, 4) || lc::misaligned(offsets, 8) || lc::misaligned(sizes, 4) || lc::misaligned(ends, 4) || lc::misaligned(area, 4) ||
        lc::misaligned(box, 4) || lc::misaligned(valid, 4))
        return fail(4, me + "every array must be aligned to its element");
    lc::IndexParams p{};
    p.counts = counts; p.offsets = reinterpret_cast<const long long*>(offsets); p.sizes = sizes; p.T = T;
    p.ends = ends; p.area = area; p.box = box; p.valid = valid;
    hipLaunchKernelGGL(lc::lc_rle_index_kernel, dim3((unsigned)F), dim3(lc::kThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me, "index");
}

int lc_rle_decode_u8(const uint32_t* ends, const int64_t* offsets, const int* sizes, const int* valid, int64_t T, int F, const int* mask_index,
                     const int* origin_xy, int B, int Hm, int Wm, unsigned char* out, int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_rle_decode_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (F < 0) return fail(2, me + "F < 0");
    if (T < 0 || T > (int64_t)LC_RLE_MAX_COUNTS) return fail(3, me + "T must be in [0, " + std::to_string((long long)LC_RLE_MAX_COUNTS) + "], got " + std::to_string((long long)T));
    const int lim = LC_RLE_MAX_SIZE;
    if (Hm < 1 || Wm < 1 || Hm > lim || Wm > lim)
        return fail(4, me + "window sizes must be in [1, " + std::to_string(lim) + "], got " + std::to_string(Hm) + " x " + std::to_string(Wm));
    if (!out || (F > 0 && (!offsets || !sizes || !valid)) || (F > 0 && T > 0 && !ends)) return fail(5, me + "the store and out must not be NULL");
    if (lc::misaligned(ends, 4) || lc::misaligned(offsets, 8) || lc::misaligned(sizes, 4) || lc::misaligned(valid, 4) || lc::misaligned(mask_index, 4) ||
        lc::misaligned(origin_xy, 4) || lc::misaligned(info, 4))
        return fail(6, me + "every array must be aligned to its element");
    lc::DecodeParams p{};
    p.ends = ends; p.offsets = reinterpret_cast<const long long*>(offsets); p.sizes = sizes; p.valid = valid; p.T = T;
    p.mask_index = mask_index; p.origin = origin_xy; p.out = out; p.info = info;
    p.F = F; p.Hm = Hm; p.Wm = Wm;
    p.tiles = (Wm + lc::kThreads - 1) / lc::kThreads;
    p.bands = (Hm + lc::kBand - 1) / lc::kBand;
    const long long blocks = (long long)B * p.tiles * p.bands;
    if (blocks > 0x7fffffffLL) return fail(7, me + "too many rows, tiles and bands for one launch");
    hipLaunchKernelGGL(lc::lc_rle_decode_kernel, dim3((unsigned)blocks), dim3(lc::kThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me, "decode");
}

int lc_rle_encode_u8(const unsigned char* masks, int F, int Hm, int Wm, const int* sizes, const int* origin_xy, int cap, uint32_t* counts_out, int* n_runs,
                     int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_rle_encode_u8: ";
    if (F < 0) return fail(1, me + "F < 0");
    if (F == 0) return 0;
    const int lim = LC_RLE_MAX_SIZE;
    if (Hm < 1 || Wm < 1 || Hm > lim || Wm > lim)
        return fail(2, me + "window sizes must be in [1, " + std::to_string(lim) + "], got " + std::to_string(Hm) + " x " + std::to_string(Wm));
    if (cap < 1) return fail(3, me + "cap must be at least 1, got " + std::to_string(cap));
    if (!masks || !counts_out || !n_runs) return fail(4, me + "masks, counts_out and n_runs must not be NULL");
    if (lc::misaligned(sizes, 4) || lc::misaligned(origin_xy, 4) || lc::misaligned(counts_out, 4) || lc::misaligned(n_runs, 4) || lc::misaligned(info, 4))
        return fail(5, me + "every array must be aligned to its element");
    lc::EncodeParams p{};
    p.masks = masks; p.sizes = sizes; p.origin = origin_xy; p.counts_out = counts_out; p.n_runs = n_runs; p.info = info;
    p.Hm = Hm; p.Wm = Wm; p.cap = cap;
    hipLaunchKernelGGL(lc::lc_rle_encode_kernel, dim3((unsigned)F), dim3(lc::kEncThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me, "encode");
}

}  // extern "C"
#pragma GCC visibility pop
