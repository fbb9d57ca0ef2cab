// Training-time background switch and colour augmentation of the network's crops, one launch (liblc_amd_augment.so; C ABI and the exact
// definition of every output in include/lc_amd_augment.h; tests/augment_oracle.py is its numpy restatement).  What the reference's
// loader does per instance on a host core (dataset.py:137-148,413-419, imgaug).
//
// One workgroup of four waves per (row, 32 x 32 tile).  The row's 64 parameter words go to LDS, thread 0 judges them (a refused row has
// every stage off and is written as its crop), and all threads fill a 768-entry table of the FINISHED output values of the row: the
// LUT of the point operations (or the identity) followed by v / 255 and the normalisation, so that the last stage is one look-up.
//
// A thread works on a quad: four consecutive x of one image row, the three channels as the bytes of three words.
//   head (point-wise): the blend with the background, salt and pepper, and for rows without filter A the dropout
//   filtered form: the head of the tile plus a 4-pixel halo (40 x 40 x 3 bytes) is staged in LDS; filter A is evaluated on the
//     36 x 36 region at in-image positions, the dropout applied, the result staged in a second buffer; filter B is evaluated on the
//     tile.  Both filters read LDS through indices reflected at the IMAGE border; a reflected position of an in-image pixel always
//     lies inside the staged region (h, w >= 8: one reflection), and every LDS index is clamped to the region besides.
//   point-wise form (the caller states that no row uses a filter): the head of the tile's quads goes straight to the output.
// Global loads and stores move four pixels (4 bytes of uint8, 16 of the mask and of an fp32 output) where w is a multiple of four and
// the pointers are aligned to it; element by element otherwise.
//
// The hash is maskcrop's (MurmurHash3's finaliser, include/lc_amd_maskcrop.h), restated here: the headers of csrc/shared/ are pinned to
// the libraries that include them.
//
// Bounds: every quad is judged against the image before it is loaded or stored, the background index and the NULL inputs are judged
// before they are used, and a refused row reads its crop only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_augment.h"

#ifndef LC_AMD_AUGMENT_SRC_HASH
#define LC_AMD_AUGMENT_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_AUGMENT_SRC_HASH:" LC_AMD_AUGMENT_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kHalo = 4;
constexpr int kFrame = kTile + 2 * kHalo;     // 40: the staged region's side
constexpr int kFrameQuads = kFrame / 4;       // 10 quads per staged row
constexpr int kPlaneWords = kFrame * kFrameQuads;  // 400 words = 1600 bytes per channel
constexpr int kWords = LC_AUGMENT_WORDS;

constexpr int kBlend = 1, kSnp = 2, kFilterA = 4, kDrop = 8, kFilterB = 16, kLut = 32;

struct Params {
    const unsigned char* crops;  // (B,3,h,w)
    const unsigned char* bg;     // (G,3,h,w) or null
    const float* msk;            // (B,h,w) or null
    const int* params;           // (B,64)
    const unsigned char* lut;    // (B,3,256)
    const int* sample_id;        // (B) or null
    void* out;                   // (B,3,h,w)
    int* info;                   // (B) or null
    int B, G, h, w, tiles_x, tiles_y;
    int vec;                     // four-pixel loads and stores are possible
    int normalize;
    unsigned seed_lo, seed_hi;
    float mean[3], std[3];
};

template <int DT> struct Store { using type = unsigned short; };
template <> struct Store<LC_AUGMENT_U8> { using type = unsigned char; };
template <> struct Store<LC_AUGMENT_F32> { using type = float; };

template <typename T> struct alignas(4 * sizeof(T)) Vec4 { T v[4]; };

// The finished output value of byte v in channel c (lc_amd_crop.h): v / 255, then (. - mean) / std, each an IEEE fp32 operation; a 16-bit
// type is rounded once (nearest even) from that fp32.
template <int DT>
__device__ inline typename Store<DT>::type finish(int v, int c, const Params& p) {
    if constexpr (DT == LC_AUGMENT_U8) {
        return (unsigned char)v;
    } else {
        float q = __fdiv_rn((float)v, 255.0f);
        if (p.normalize) {
            q = __fsub_rn(q, p.mean[c]);
            q = __fdiv_rn(q, p.std[c]);
        }
        if constexpr (DT == LC_AUGMENT_F32) {
            return q;
        } else if constexpr (DT == LC_AUGMENT_F16) {
            return __builtin_bit_cast(unsigned short, (_Float16)q);
        } else {
            const unsigned u = __float_as_uint(q);
            if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)0x7fc0;
            return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
    }
}

// MurmurHash3's 32-bit finaliser
__device__ __forceinline__ unsigned fmix32(unsigned v) {
    v ^= v >> 16;
    v *= 0x85ebca6bu;
    v ^= v >> 13;
    v *= 0xc2b2ae35u;
    v ^= v >> 16;
    return v;
}

// What a workgroup knows of its row once it is judged
struct Row {
    int flags;                 // P[0], or 0 for a refused row
    int g, gh, gw;
    unsigned snp_th, drop_th;
    unsigned k_snp, k_snpv, k_drop;  // the key states behind the three op codes
};

__device__ inline bool weights_ok(const int* wq) {
    long long sum = 0;
    bool ok = true;
    for (int i = 0; i < 25; ++i) {
        ok = ok && wq[i] >= 0;
        sum += wq[i];
    }
    return ok && sum == 65536;
}

// four bytes at q as one word; pixels at x >= w read 0
__device__ __forceinline__ unsigned load4(const unsigned char* q, int x0, int w, int vec) {
    if (vec) return *reinterpret_cast<const unsigned*>(q);
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < w) r |= (unsigned)q[j] << (8 * j);
    return r;
}

// coarse dropout of the quad (x0.., y)
__device__ __forceinline__ void drop_quad(const Params& p, const Row& r, int x0, int y, unsigned (&v)[3]) {
    const int cy = (int)((unsigned)(y * r.gh) / (unsigned)p.h) * r.gw;
    unsigned keep = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cell = cy + (int)((unsigned)((x0 + j) * r.gw) / (unsigned)p.w);
        if (fmix32(r.k_drop ^ (unsigned)cell) < r.drop_th) keep &= ~(0xffu << (8 * j));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] &= keep;
}

// The point-wise head of the in-image quad (x0.., y) of row b, 0 <= y < h, 0 <= x0 < w: blend, salt and pepper, and with `drop` the dropout
__device__ __forceinline__ void head_quad(const Params& p, const Row& r, int b, int x0, int y, bool drop, unsigned (&v)[3]) {
    const size_t plane = (size_t)p.h * p.w;
    const size_t o = (size_t)y * p.w + x0;
    const unsigned char* src = p.crops + (size_t)b * 3 * plane + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = load4(src + c * plane, x0, p.w, p.vec);
    if (r.flags & kBlend) {
        float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* mp = p.msk + (size_t)b * plane + o;
        if (p.vec) {
            const float4 t = *reinterpret_cast<const float4*>(mp);
            m[0] = t.x, m[1] = t.y, m[2] = t.z, m[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < p.w) m[j] = mp[j];
        }
        unsigned k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = __fmul_rn(m[j], 1024.0f);
            k[j] = t >= 1024.0f ? 1024u : t > 0.0f ? (unsigned)rintf(t) : 0u;  // NaN: 0
        }
        const unsigned char* bgp = p.bg + (size_t)r.g * 3 * plane + o;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned back = load4(bgp + c * plane, x0, p.w, p.vec);
            unsigned res = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned S = k[j] * ((v[c] >> (8 * j)) & 0xffu) + (1024u - k[j]) * ((back >> (8 * j)) & 0xffu);
                const unsigned q = S >> 10, rem = S & 1023u;
                res |= (q + ((rem > 512u || (rem == 512u && (q & 1u))) ? 1u : 0u)) << (8 * j);  // <= 255: S <= 1024 * 255
            }
            v[c] = res;
        }
    }
    if (r.flags & kSnp) {
        unsigned keep = 0xffffffffu, salt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = (unsigned)(y * p.w + x0 + j);
            if (fmix32(r.k_snp ^ q) < r.snp_th) {
                keep &= ~(0xffu << (8 * j));
                if (fmix32(r.k_snpv ^ q) >> 31) salt |= 0xffu << (8 * j);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (v[c] & keep) | salt;
    }
    if (drop) drop_quad(p, r, x0, y, v);
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }
__device__ __forceinline__ int in_frame(int i) { return min(max(i, 0), kFrame - 1); }

// The 5x5 filter of the quad (x0.., y) with the Q16 weights wq (LDS), read from the staged planes `src` whose corner is image pixel (fx0, fy0)
__device__ __forceinline__ void filter_quad(const unsigned char* src, const int* wq, int fx0, int fy0, int x0, int y, int h, int w, unsigned (&v)[3]) {
    int rr[5], cc[8];
#pragma unroll
    for (int d = 0; d < 5; ++d) rr[d] = in_frame(reflect101(y + d - 2, h) - fy0) * kFrame;
#pragma unroll
    for (int i = 0; i < 8; ++i) cc[i] = in_frame(reflect101(x0 + i - 2, w) - fx0);
    int wv[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) wv[i] = wq[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned acc[4] = {32768u, 32768u, 32768u, 32768u};
#pragma unroll
        for (int d = 0; d < 5; ++d)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned t = src[c * (kPlaneWords * 4) + rr[d] + cc[i]];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i - j >= 0 && i - j <= 4) acc[j] += (unsigned)wv[d * 5 + i - j] * t;
            }
        // non-negative weights that sum to 65536: at most 255 after the shift
        v[c] = (acc[0] >> 16) | ((acc[1] >> 16) << 8) | ((acc[2] >> 16) << 16) | ((acc[3] >> 16) << 24);
    }
}

template <int DT, bool FILTERED>
__global__ __launch_bounds__(kThreads) void lc_augment_kernel(const Params p) {
    using T = typename Store<DT>::type;
    __shared__ int s_P[kWords];
    __shared__ Row s_row;
    __shared__ T s_table[768];
    __shared__ unsigned s_buf[FILTERED ? 2 * 3 * kPlaneWords : 1];

    const int tid = threadIdx.x;
    const int tiles = p.tiles_x * p.tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int tyi = t / p.tiles_x, txi = t - tyi * p.tiles_x;
    const int ty0 = tyi * kTile, tx0 = txi * kTile;

    if (tid < kWords) s_P[tid] = p.params[(size_t)b * kWords + tid];
    __syncthreads();
    if (tid == 0) {
        const int f = s_P[0];
        bool ok = (f & ~63) == 0;
        for (int j = 56; j < kWords; ++j) ok = ok && s_P[j] == 0;
        if (f & kFilterA) ok = ok && weights_ok(s_P + 6);
        if (f & kFilterB) ok = ok && weights_ok(s_P + 31);
        if (f & kDrop) ok = ok && s_P[4] >= 1 && s_P[4] <= p.h && s_P[5] >= 1 && s_P[5] <= p.w;
        if (f & kBlend) ok = ok && p.msk != nullptr && p.bg != nullptr && s_P[1] >= 0 && s_P[1] < p.G;
        if (!FILTERED && (f & (kFilterA | kFilterB))) ok = false;
        Row r;
        r.flags = ok ? f : 0;
        r.g = s_P[1], r.gh = s_P[4], r.gw = s_P[5];
        r.snp_th = (unsigned)s_P[2], r.drop_th = (unsigned)s_P[3];
        unsigned k = fmix32(p.seed_lo);
        k = fmix32(k ^ p.seed_hi);
        k = fmix32(k ^ (unsigned)(p.sample_id ? p.sample_id[b] : b));
        r.k_snp = fmix32(k ^ (unsigned)LC_AUGMENT_OP_SNP);
        r.k_snpv = fmix32(k ^ (unsigned)LC_AUGMENT_OP_SNPV);
        r.k_drop = fmix32(k ^ (unsigned)LC_AUGMENT_OP_DROP);
        s_row = r;
        if (t == 0 && p.info) p.info[b] = ok ? 0 : -1;
    }
    __syncthreads();
    const Row r = s_row;

    if (tid < 192) {  // the row's LUT, four entries per lane, finished
        const unsigned word = (r.flags & kLut) ? reinterpret_cast<const unsigned*>(p.lut + (size_t)b * 768)[tid] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * tid + j;
            const int v = (r.flags & kLut) ? (int)((word >> (8 * j)) & 0xffu) : (i & 255);
            s_table[i] = finish<DT>(v, i >> 8, p);
        }
    }

    unsigned v[3] = {0u, 0u, 0u};
    int x0, y;
    if constexpr (FILTERED) {
        const int fx0 = tx0 - kHalo, fy0 = ty0 - kHalo;
        const bool filter_a = (r.flags & kFilterA) != 0, filter_b = (r.flags & kFilterB) != 0, drop = (r.flags & kDrop) != 0;
        unsigned* head = s_buf;
        unsigned* mid = s_buf + 3 * kPlaneWords;
        for (int q = tid; q < kPlaneWords; q += kThreads) {
            const int ry = q / kFrameQuads, qx = q - ry * kFrameQuads;
            const int yy = fy0 + ry, xx = fx0 + 4 * qx;
            unsigned u[3] = {0u, 0u, 0u};
            if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) head_quad(p, r, b, xx, yy, drop && !filter_a, u);
#pragma unroll
            for (int c = 0; c < 3; ++c) head[c * kPlaneWords + q] = u[c];
        }
        __syncthreads();
        if (filter_a) {  // uniform over the workgroup
            for (int q = tid; q < (kFrame - 4) * kFrameQuads; q += kThreads) {
                const int ry = 2 + q / kFrameQuads, qx = q % kFrameQuads;
                const int yy = fy0 + ry, xx = fx0 + 4 * qx;
                unsigned u[3] = {0u, 0u, 0u};
                if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) {
                    // (the quad's columns 0, 1, 38, 39 of the region are formed from clamped taps and never read)
                    filter_quad(reinterpret_cast<const unsigned char*>(head), s_P + 6, fx0, fy0, xx, yy, p.h, p.w, u);
                    if (drop) drop_quad(p, r, xx, yy, u);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) mid[c * kPlaneWords + ry * kFrameQuads + qx] = u[c];
            }
            __syncthreads();
        }
        const unsigned* src = filter_a ? mid : head;
        const int ry = kHalo + (tid >> 3), qx = 1 + (tid & 7);
        y = fy0 + ry, x0 = fx0 + 4 * qx;
        if (y >= p.h || x0 >= p.w) return;  // behind the last barrier
        if (filter_b) {
            filter_quad(reinterpret_cast<const unsigned char*>(src), s_P + 31, fx0, fy0, x0, y, p.h, p.w, v);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = src[c * kPlaneWords + ry * kFrameQuads + qx];
        }
    } else {
        __syncthreads();  // the table
        y = ty0 + (tid >> 3), x0 = tx0 + 4 * (tid & 7);
        if (y >= p.h || x0 >= p.w) return;
        head_quad(p, r, b, x0, y, (r.flags & kDrop) != 0, v);
    }

    const size_t plane = (size_t)p.h * p.w;
    T* out = static_cast<T*>(p.out) + (size_t)b * 3 * plane + (size_t)y * p.w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Vec4<T> res;
#pragma unroll
        for (int j = 0; j < 4; ++j) res.v[j] = s_table[c * 256 + ((v[c] >> (8 * j)) & 0xffu)];
        if (p.vec) {
            *reinterpret_cast<Vec4<T>*>(out + c * plane) = res;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < p.w) out[c * plane + j] = res.v[j];
        }
    }
}

template <int DT>
void launch(const Params& p, int form, unsigned blocks, hipStream_t s) {
    if (form == LC_AUGMENT_POINTWISE) hipLaunchKernelGGL((lc_augment_kernel<DT, false>), dim3(blocks), dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((lc_augment_kernel<DT, true>), dim3(blocks), dim3(kThreads), 0, s, p);
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_augment_version(void) { return LC_AMD_AUGMENT_VERSION; }
const char* lc_amd_augment_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_AUGMENT_SRC_HASH:") - 1; }
const char* lc_amd_augment_last_error(void) { return lc::g_err.c_str(); }

int lc_augment_u8(const unsigned char* crops, const unsigned char* backgrounds, int G, const float* msk_in, const int* params, const unsigned char* lut,
                  int B, int h, int w, uint64_t seed, const int* sample_id, int out_dtype, int form, const float* mean, const float* std, void* out,
                  int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_augment_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (G < 0) return fail(2, me + "G < 0");
    const int lo = LC_AUGMENT_MIN_SIZE, hi = LC_AUGMENT_MAX_SIZE;
    if (h < lo || w < lo || h > hi || w > hi)
        return fail(3, me + "crop sizes must be in [" + std::to_string(lo) + ", " + std::to_string(hi) + "], got " + std::to_string(h) + " x " + std::to_string(w));
    if (out_dtype < LC_AUGMENT_U8 || out_dtype > LC_AUGMENT_BF16) return fail(4, me + "unknown out_dtype " + std::to_string(out_dtype));
    if (form != LC_AUGMENT_FILTERED && form != LC_AUGMENT_POINTWISE) return fail(5, me + "form must be LC_AUGMENT_FILTERED or LC_AUGMENT_POINTWISE");
    if ((mean == nullptr) != (std == nullptr)) return fail(6, me + "mean and std come together");
    if (mean && out_dtype == LC_AUGMENT_U8) return fail(6, me + "mean and std need a float output");
    if (!crops || !params || !lut || !out) return fail(7, me + "crops, params, lut and out must not be NULL");
    if ((G > 0) != (backgrounds != nullptr)) return fail(8, me + "backgrounds is NULL exactly when G = 0");
    const size_t elem = out_dtype == LC_AUGMENT_U8 ? 1 : out_dtype == LC_AUGMENT_F32 ? 4 : 2;
    if (lc::misaligned(params, 4) || lc::misaligned(lut, 4) || lc::misaligned(msk_in, 4) || lc::misaligned(sample_id, 4) || lc::misaligned(info, 4) ||
        lc::misaligned(out, elem))
        return fail(9, me + "params, lut, msk_in, sample_id, info and out must be aligned to their element (lut to 4 bytes)");

    lc::Params p{};
    p.crops = crops; p.bg = backgrounds; p.msk = msk_in; p.params = params; p.lut = lut; p.sample_id = sample_id;
    p.out = out; p.info = info;
    p.B = B; p.G = G; p.h = h; p.w = w;
    p.tiles_x = (w + lc::kTile - 1) / lc::kTile;
    p.tiles_y = (h + lc::kTile - 1) / lc::kTile;
    p.vec = (w % 4 == 0) && !lc::misaligned(crops, 4) && !lc::misaligned(backgrounds, 4) && !lc::misaligned(msk_in, 16) && !lc::misaligned(out, 4 * elem);
    p.normalize = mean != nullptr;
    for (int c = 0; c < 3 && mean; ++c) p.mean[c] = mean[c], p.std[c] = std[c];
    p.seed_lo = (unsigned)(seed & 0xffffffffull); p.seed_hi = (unsigned)(seed >> 32);
    const long long blocks = (long long)B * p.tiles_x * p.tiles_y;
    if (blocks > 0x7fffffffLL) return fail(10, me + "too many rows and tiles for one launch");

    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (out_dtype) {
        case LC_AUGMENT_U8: lc::launch<LC_AUGMENT_U8>(p, form, (unsigned)blocks, s); break;
        case LC_AUGMENT_F32: lc::launch<LC_AUGMENT_F32>(p, form, (unsigned)blocks, s); break;
        case LC_AUGMENT_F16: lc::launch<LC_AUGMENT_F16>(p, form, (unsigned)blocks, s); break;
        default: lc::launch<LC_AUGMENT_BF16>(p, form, (unsigned)blocks, s); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(11, me + "launch: " + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
