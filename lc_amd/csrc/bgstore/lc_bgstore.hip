// The device-resident background store: each row's pick, and the cut and blend of its background in place in the uint8 crop
// (liblc_amd_bgstore.so; C ABI and the exact definition of every output in include/lc_amd_bgstore.h).
//
// What the reference's loader does per instance on a host core with `_switch_bg(rgb_in, msk_in, np.random.choice(self.bg_list))`
// (dataset.py:137-148,413-415).  Two kernels, and between them the region matrices of lc_geometry_background_f32:
//
//   lc_bgstore_pick_kernel    one thread per row in workgroups of 64: the gate and the background of `draw` (lc_amd/augment.py) from the
//                             seed word on the device, and the chosen image's size out of the store's table.
//   lc_bgstore_switch_kernel  the launch geometry of the zoom-in crops (shared/lc_warp_grid.h): one workgroup of four waves per (row, band
//                             of crop rows), a thread owns four consecutive x.  A workgroup of a closed row exits before anything else.
//                             Thread 0 forms the row's inverse matrix and judges the row.  Per quad a thread loads four mask values;
//                             where all four k are 1024 it goes on, else it samples the four taps of image g (HWC bytes, row stride
//                             3 Wb, from the store's byte offset), blends and stores four bytes per channel plane.
//
// The coordinates and the hash are the shared headers'; the tap combination (include/lc_amd_crop.h) and the blend (bit 0 of
// include/lc_amd_augment.h) are restated here, and tests/test_gpu_bgstore.py holds them EQUAL to crop's and augment's.
//
// Bounds: the pick reads hw[2 g], hw[2 g + 1] with 0 <= g < G by construction.  The switch checks 0 <= g < G before it reads a table,
// refuses sizes outside [1, LC_BGSTORE_MAX_SIZE] and negative offsets, and range-checks every tap against (Hb, Wb) on its own (that IS
// the border rule); a thread reads and writes only the bytes of its own quad, so working in place needs no ordering.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_bgstore.h"
#include "../shared/lc_keyed_hash.h"
#include "../shared/lc_warp_grid.h"

#ifndef LC_AMD_BGSTORE_SRC_HASH
#define LC_AMD_BGSTORE_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_BGSTORE_SRC_HASH:" LC_AMD_BGSTORE_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kPickThreads = 64;
constexpr int kThreads = 256;
constexpr int kMinBand = 16;  // crop rows per workgroup, as the zoom-in crops have it

struct PickParams {
    double switch_bg_prob;
    const unsigned long long* seed;
    const int* sample_id;
    const int* hw;
    int* gate;
    int* which;
    int* bg_hw;
    int G, B;
};

__global__ __launch_bounds__(kPickThreads) void lc_bgstore_pick_kernel(const PickParams p) {
    const int b = (int)(blockIdx.x * kPickThreads + threadIdx.x);
    if (b >= p.B) return;
    const unsigned long long seed = *p.seed;
    const unsigned state = fmix32(sample_state(seed_state((unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)), (unsigned)p.sample_id[b]) ^
                                  (unsigned)LC_BGSTORE_OP_SWITCH);
    const bool open = key_uniform(fmix32(state ^ 0u)) < p.switch_bg_prob && p.G > 0;
    const int g = min((int)__dmul_rn(key_uniform(fmix32(state ^ 1u)), (double)p.G), max(p.G - 1, 0));  // in [0, G) where G > 0
    p.gate[b] = open ? 1 : 0;
    p.which[b] = open ? g : -1;
    p.bg_hw[2 * (size_t)b] = open ? p.hw[2 * (size_t)g] : 1;
    p.bg_hw[2 * (size_t)b + 1] = open ? p.hw[2 * (size_t)g + 1] : 1;
}

struct SwitchParams {
    unsigned char* crops;
    const float* msk;
    const unsigned char* pixels;
    const long long* offsets;
    const int* hw;
    const int* which;
    const float* M;
    int* info;
    int G, B, h, w;
    WarpGrid grid;
    int vec;  // four-pixel loads and stores are possible (w % 4 == 0, crops aligned to 4 bytes and msk_in to 16)
};

__global__ __launch_bounds__(kThreads) void lc_bgstore_switch_kernel(const SwitchParams p) {
    __shared__ double s_inv[6];
    __shared__ int s_ok;

    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.grid.nbands, band = blockIdx.x - b * p.grid.nbands;
    const int g = p.which[b];
    if (g < 0) {  // a closed gate: the same for the whole workgroup
        if (tid == 0 && band == 0) p.info[b] = 0;
        return;
    }
    const bool listed = g < p.G;
    const int Hb = listed ? p.hw[2 * (size_t)g] : 0, Wb = listed ? p.hw[2 * (size_t)g + 1] : 0;
    const long long offset = listed ? p.offsets[g] : -1;
    if (tid == 0) {
        bool ok = listed && offset >= 0 && Hb >= 1 && Hb <= LC_BGSTORE_MAX_SIZE && Wb >= 1 && Wb <= LC_BGSTORE_MAX_SIZE;
        ok = inverse_of(p.M + 6 * (size_t)b, ok, s_inv);
        s_ok = ok ? 1 : 0;
        if (band == 0) p.info[b] = ok ? 1 : -1;
    }
    __syncthreads();
    if (!s_ok) return;  // a refused row is untouched

    const unsigned char* src = p.pixels + offset;
    const double m00 = s_inv[0], m01 = s_inv[1], b1 = s_inv[2], m10 = s_inv[3], m11 = s_inv[4], b2 = s_inv[5];
    const size_t plane = (size_t)p.h * p.w;
    unsigned char* crop = p.crops + (size_t)b * 3 * plane;
    const float* msk = p.msk + (size_t)b * plane;

    const int TX = 1 << p.grid.lg_tx, TY = kThreads >> p.grid.lg_tx;
    const int tx = tid & (TX - 1), ty = tid >> p.grid.lg_tx;
    const int quads = (p.w + 3) >> 2;
    const int y_end = min(p.h, (band + 1) * p.grid.band);

    auto tap = [&](int xx, int yy, int (&s)[3]) {
        const bool in = (unsigned)xx < (unsigned)Wb && (unsigned)yy < (unsigned)Hb;
        const unsigned char* q = src + ((size_t)(in ? yy : 0) * Wb + (in ? xx : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = in ? (int)q[c] : 0;
    };

    for (int xq = tx; xq < quads; xq += TX) {
        const int x0 = xq << 2;
        int ax[4], ay[4];
        quad_terms(m00, m10, x0, ax, ay);
        for (int y = band * p.grid.band + ty; y < y_end; y += TY) {
            const size_t o = (size_t)y * p.w + x0;
            float m[4] = {1.0f, 1.0f, 1.0f, 1.0f};  // beyond the row's end: k = 1024, nothing to do
            if (p.vec) {
                const float4 t = *reinterpret_cast<const float4*>(msk + o);
                m[0] = t.x, m[1] = t.y, m[2] = t.z, m[3] = t.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < p.w) m[j] = msk[o + j];
            }
            unsigned k[4];
            bool keep = true;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = __fmul_rn(m[j], 1024.0f);
                k[j] = t >= 1024.0f ? 1024u : t > 0.0f ? (unsigned)rintf(t) : 0u;  // NaN: 0
                keep = keep && k[j] == 1024u;
            }
            if (keep) continue;

            unsigned v[3];  // the crop's four bytes per plane, x0 in the low byte
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned char* q = crop + c * plane + o;
                if (p.vec) {
                    v[c] = *reinterpret_cast<const unsigned*>(q);
                } else {
                    v[c] = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < p.w) v[c] |= (unsigned)q[j] << (8 * j);
                }
            }
            const long long X0 = row_term(m01, b1, y) + kLinearDelta, Y0 = row_term(m11, b2, y) + kLinearDelta;
            unsigned res[3] = {0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int back[3] = {0, 0, 0};
                if (k[j] != 1024u) {  // (a pixel with k = 1024 keeps its byte whatever lies behind it)
                    const auto [sx, sy, fx, fy] = linear_taps(X0 + ax[j], Y0 + ay[j]);
                    int s00[3], s01[3], s10[3], s11[3];
                    tap(sx, sy, s00);
                    tap(sx + 1, sy, s01);
                    tap(sx, sy + 1, s10);
                    tap(sx + 1, sy + 1, s11);
                    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
                    for (int c = 0; c < 3; ++c) back[c] = (w00 * s00[c] + w01 * s01[c] + w10 * s10[c] + w11 * s11[c] + 512) >> 10;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned S = k[j] * ((v[c] >> (8 * j)) & 0xffu) + (1024u - k[j]) * (unsigned)back[c];
                    const unsigned q = S >> 10, rem = S & 1023u;
                    res[c] |= (q + ((rem > 512u || (rem == 512u && (q & 1u))) ? 1u : 0u)) << (8 * j);  // <= 255: S <= 1024 * 255
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned char* q = crop + c * plane + o;
                if (p.vec) {
                    *reinterpret_cast<unsigned*>(q) = res[c];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < p.w) q[j] = (unsigned char)(res[c] >> (8 * j));
                }
            }
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

int lc_amd_bgstore_version(void) { return LC_AMD_BGSTORE_VERSION; }
const char* lc_amd_bgstore_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_BGSTORE_SRC_HASH:") - 1; }
const char* lc_amd_bgstore_last_error(void) { return lc::g_err.c_str(); }

int lc_bgstore_pick(double switch_bg_prob, int G, const uint64_t* seed, const int* sample_id, const int* hw, int B, int* gate, int* which, int* bg_hw,
                    void* stream) {
    using lc::fail;
    const std::string me = "lc_bgstore_pick: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (G < 0) return fail(2, me + "G < 0");
    if (!seed) return fail(3, me + "seed must not be NULL: it points to one uint64 on the device");
    if (!sample_id || !gate || !which || !bg_hw) return fail(3, me + "sample_id, gate, which and bg_hw must not be NULL");
    if (G > 0 && !hw) return fail(3, me + "hw must not be NULL where G > 0");
    if (!(switch_bg_prob >= 0.0 && switch_bg_prob <= 1.0)) return fail(4, me + "switch_bg_prob must lie in [0, 1], got " + std::to_string(switch_bg_prob));
    if (lc::misaligned(seed, 8)) return fail(7, me + "seed must be aligned to 8 bytes");
    if (lc::misaligned(sample_id, 4) || lc::misaligned(hw, 4) || lc::misaligned(gate, 4) || lc::misaligned(which, 4) || lc::misaligned(bg_hw, 4))
        return fail(7, me + "sample_id, hw, gate, which and bg_hw must be aligned to 4 bytes");

    lc::PickParams p{};
    p.switch_bg_prob = switch_bg_prob;
    p.seed = reinterpret_cast<const unsigned long long*>(seed);
    p.sample_id = sample_id; p.hw = hw; p.gate = gate; p.which = which; p.bg_hw = bg_hw;
    p.G = G; p.B = B;
    const unsigned blocks = ((unsigned)B + lc::kPickThreads - 1) / lc::kPickThreads;
    hipLaunchKernelGGL(lc::lc_bgstore_pick_kernel, dim3(blocks), dim3(lc::kPickThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me);
}

int lc_bgstore_switch_u8(unsigned char* crops, const float* msk_in, const unsigned char* pixels, const int64_t* offsets, const int* hw, int G,
                         const int* which, const float* M, int h, int w, int B, int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_bgstore_switch_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (G < 0) return fail(2, me + "G < 0");
    if (!crops || !msk_in || !which || !M || !info) return fail(3, me + "crops, msk_in, which, M and info must not be NULL");
    if (G > 0 && (!pixels || !offsets || !hw)) return fail(3, me + "pixels, offsets and hw must not be NULL where G > 0");
    if (h < 1 || w < 1 || h > LC_BGSTORE_MAX_SIZE || w > LC_BGSTORE_MAX_SIZE)
        return fail(5, me + "h and w must be in [1, " + std::to_string(LC_BGSTORE_MAX_SIZE) + "], got " + std::to_string(h) + " x " + std::to_string(w));
    if (lc::misaligned(offsets, 8)) return fail(7, me + "offsets must be aligned to 8 bytes");
    if (lc::misaligned(msk_in, 4) || lc::misaligned(hw, 4) || lc::misaligned(which, 4) || lc::misaligned(M, 4) || lc::misaligned(info, 4))
        return fail(7, me + "msk_in, hw, which, M and info must be aligned to 4 bytes");

    lc::SwitchParams p{};
    p.crops = crops; p.msk = msk_in; p.pixels = pixels;
    p.offsets = reinterpret_cast<const long long*>(offsets);
    p.hw = hw; p.which = which; p.M = M; p.info = info;
    p.G = G; p.B = B; p.h = h; p.w = w;
    p.grid = lc::warp_grid(h, w, lc::kThreads, lc::kMinBand);
    p.vec = (w % 4 == 0) && !lc::misaligned(crops, 4) && !lc::misaligned(msk_in, 16);
    const long long blocks = (long long)B * p.grid.nbands;
    if (blocks > 0x7fffffffLL) return fail(8, me + "too many rows and bands for one launch");
    hipLaunchKernelGGL(lc::lc_bgstore_switch_kernel, dim3((unsigned)blocks), dim3(lc::kThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me);
}

}  // extern "C"
#pragma GCC visibility pop
