// Zoom-in crops: exact integer affine warps of uint8 frames, one launch (liblc_amd_crop.so, C ABI and the exact definition of the
// result in include/lc_amd_crop.h).
//
// What the reference's loader does per instance on the host with cv2.warpAffine (dataset.py:409-411, 425-426) followed by
// `.to(float32).div(255)` and transforms.Normalize (test.py:163): here every crop of a batch is cut from frames that were uploaded
// once, in OpenCV's published fixed-point scheme for 8-bit images (coordinates on a 1/1024 px grid, bilinear weights on a 1/32 px
// grid), which is pure integer arithmetic after the inverse matrix (shared/lc_warp_grid.h, with the training mask crops).
//
//   one workgroup of four waves per (row, band of crop rows).  Thread 0 forms the row's inverse matrix in fp64 and judges the row;
//   all threads fill a 256 C-entry table of the FINISHED output values in LDS (there are only 256 values per channel, so the
//   division by 255 and the normalisation leave the pixel loop).  A thread then owns four consecutive x (its two x terms are formed
//   once) and walks the band's rows: four taps per pixel read as bytes, a blend in 32-bit integers, a table look-up per channel,
//   and one store of four pixels per channel plane (16 bytes for fp32, 8 for the 16-bit types, 4 for uint8; element by element
//   where w is no multiple of four or the output is not aligned).
//
// Bounds: every tap is range-checked against the frame on its own (that IS the border rule), a bad row sees a frame of size zero, and
// the frame index is checked before it is used, so that no input value can make the launch read or write outside its arrays.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_crop.h"
#include "../shared/lc_byte_finish.h"
#include "../shared/lc_warp_grid.h"

#ifndef LC_AMD_CROP_SRC_HASH
#define LC_AMD_CROP_SRC_HASH "unrecorded"
#endif

namespace {

const char kSrcHash[] = "LC_AMD_CROP_SRC_HASH:" LC_AMD_CROP_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 256;
constexpr int kMinBand = 16;  // crop rows per workgroup (more where a pass of the workgroup covers more)

struct Params {
    const unsigned char* frames;
    const int* frame_index;
    const float* M;
    void* out;
    int* info;
    int F, H, W, B, h, w;
    lc::WarpGrid grid;
    int vec;           // four-pixel stores are possible (w % 4 == 0 and the output is aligned to them)
    int normalize;
    float mean[3], std[3];
};

using lc::Store;
using lc::Vec4;
using lc::finish;  // the finished output value of a byte: shared/lc_byte_finish.h, with the colour augmentation
static_assert(LC_CROP_U8 == lc::kByteU8 && LC_CROP_F32 == lc::kByteF32 && LC_CROP_F16 == lc::kByteF16 && LC_CROP_BF16 == lc::kByteBF16, "the dtype codes of lc_byte_finish.h");

template <int DT, int C, bool LINEAR>
__global__ __launch_bounds__(kThreads) void lc_crop_warp_kernel(const Params p) {
    using T = typename Store<DT>::type;
    constexpr bool kTable = DT != LC_CROP_U8;
    __shared__ T table[kTable ? 256 * C : 1];
    __shared__ double s_inv[6];
    __shared__ int s_frame;  // -1 = bad row

    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.grid.nbands, band = blockIdx.x - b * p.grid.nbands;
    if (tid == 0) {
        const int f = p.frame_index ? p.frame_index[b] : b;
        bool ok = f >= 0 && f < p.F;
        ok = lc::inverse_of(p.M + 6 * (size_t)b, ok, s_inv);
        s_frame = ok ? f : -1;
        if (band == 0 && p.info) p.info[b] = ok ? 0 : -1;
    }
    if constexpr (kTable) {
        for (int i = tid; i < 256 * C; i += kThreads) table[i] = finish<DT>(i & 255, i >> 8, p);
    }
    __syncthreads();

    const int frame = s_frame;
    const int H = frame >= 0 ? p.H : 0, W = frame >= 0 ? p.W : 0;  // a bad row: every tap is outside
    const unsigned char* src = p.frames + (size_t)(frame >= 0 ? frame : 0) * p.H * p.W * C;
    const double m00 = s_inv[0], m01 = s_inv[1], b1 = s_inv[2], m10 = s_inv[3], m11 = s_inv[4], b2 = s_inv[5];
    T* out = static_cast<T*>(p.out) + (size_t)b * C * p.h * p.w;
    const size_t plane = (size_t)p.h * p.w;

    const int TX = 1 << p.grid.lg_tx, TY = kThreads >> p.grid.lg_tx;
    const int tx = tid & (TX - 1), ty = tid >> p.grid.lg_tx;
    const int quads = (p.w + 3) >> 2;
    const int y_end = min(p.h, (band + 1) * p.grid.band);
    constexpr long long kDelta = LINEAR ? lc::kLinearDelta : lc::kNearestDelta;

    auto tap = [&](int xx, int yy, int (&s)[C]) {
        const bool in = (unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H;
        const unsigned char* q = src + ((size_t)(in ? yy : 0) * W + (in ? xx : 0)) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] = in ? (int)q[c] : 0;
    };

    for (int xq = tx; xq < quads; xq += TX) {
        const int x0 = xq << 2;
        int ax[4], ay[4];
        lc::quad_terms(m00, m10, x0, ax, ay);
        for (int y = band * p.grid.band + ty; y < y_end; y += TY) {
            const long long X0 = lc::row_term(m01, b1, y) + kDelta, Y0 = lc::row_term(m11, b2, y) + kDelta;
            Vec4<T> res[C];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long X = X0 + ax[j], Y = Y0 + ay[j];
                int v[C];
                if constexpr (LINEAR) {
                    const auto [sx, sy, fx, fy] = lc::linear_taps(X, Y);
                    int s00[C], s01[C], s10[C], s11[C];
                    tap(sx, sy, s00);
                    tap(sx + 1, sy, s01);
                    tap(sx, sy + 1, s10);
                    tap(sx + 1, sy + 1, s11);
                    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = (w00 * s00[c] + w01 * s01[c] + w10 * s10[c] + w11 * s11[c] + 512) >> 10;
                } else {
                    tap(lc::nearest_tap(X), lc::nearest_tap(Y), v);
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if constexpr (kTable) res[c].v[j] = table[c * 256 + v[c]];
                    else res[c].v[j] = (T)v[c];
                }
            }
            const size_t o = (size_t)y * p.w + x0;
            if (p.vec) {
#pragma unroll
                for (int c = 0; c < C; ++c) *reinterpret_cast<Vec4<T>*>(out + c * plane + o) = res[c];
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < p.w) out[c * plane + o + j] = res[c].v[j];
            }
        }
    }
}

template <int DT, int C>
void launch_interp(const Params& p, int interp, unsigned blocks, hipStream_t s) {
    if (interp == LC_CROP_LINEAR) hipLaunchKernelGGL((lc_crop_warp_kernel<DT, C, true>), dim3(blocks), dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((lc_crop_warp_kernel<DT, C, false>), dim3(blocks), dim3(kThreads), 0, s, p);
}

template <int DT>
void launch_channels(const Params& p, int C, int interp, unsigned blocks, hipStream_t s) {
    if (C == 3) launch_interp<DT, 3>(p, interp, blocks, s);
    else launch_interp<DT, 1>(p, interp, blocks, s);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_crop_version(void) { return LC_AMD_CROP_VERSION; }
const char* lc_amd_crop_source_hash(void) { return kSrcHash + sizeof("LC_AMD_CROP_SRC_HASH:") - 1; }
const char* lc_amd_crop_last_error(void) { return g_err.c_str(); }

int lc_crop_warp_u8(const unsigned char* frames, int F, int H, int W, int C, const int* frame_index, const float* M, int B, int h, int w,
                    int interp, int out_dtype, const float* mean, const float* std, void* out, int* info, void* stream) {
    if (B < 0) return fail(1, "lc_crop_warp_u8: B < 0");
    if (B == 0) return 0;
    if (C != 1 && C != 3) return fail(2, "lc_crop_warp_u8: C must be 1 or 3, got " + std::to_string(C));
    if (F < 0) return fail(3, "lc_crop_warp_u8: F < 0");
    if (H < 1 || W < 1 || H > LC_CROP_MAX_SIZE || W > LC_CROP_MAX_SIZE || h < 1 || w < 1 || h > LC_CROP_MAX_SIZE || w > LC_CROP_MAX_SIZE)
        return fail(4, "lc_crop_warp_u8: frame and crop sizes must be in [1, " + std::to_string(LC_CROP_MAX_SIZE) + "], got " + std::to_string(H) +
                           " x " + std::to_string(W) + " -> " + std::to_string(h) + " x " + std::to_string(w));
    if (interp != LC_CROP_NEAREST && interp != LC_CROP_LINEAR) return fail(5, "lc_crop_warp_u8: interp must be LC_CROP_NEAREST or LC_CROP_LINEAR");
    if (out_dtype < LC_CROP_U8 || out_dtype > LC_CROP_BF16) return fail(6, "lc_crop_warp_u8: unknown out_dtype " + std::to_string(out_dtype));
    if ((mean == nullptr) != (std == nullptr)) return fail(7, "lc_crop_warp_u8: mean and std come together");
    if (mean && out_dtype == LC_CROP_U8) return fail(7, "lc_crop_warp_u8: mean and std need a float output");
    if (!M || !out || (F > 0 && !frames)) return fail(8, "lc_crop_warp_u8: frames, M and out must not be NULL");
    Params p{};
    p.frames = frames;
    p.frame_index = frame_index;
    p.M = M;
    p.out = out;
    p.info = info;
    p.F = F, p.H = H, p.W = W, p.B = B, p.h = h, p.w = w;
    p.grid = lc::warp_grid(h, w, kThreads, kMinBand);
    const size_t elem = out_dtype == LC_CROP_U8 ? 1 : out_dtype == LC_CROP_F32 ? 4 : 2;
    p.vec = (w % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % (4 * elem) == 0);
    p.normalize = mean != nullptr;
    for (int c = 0; c < C && mean; ++c) p.mean[c] = mean[c], p.std[c] = std[c];
    const long long blocks = (long long)B * p.grid.nbands;
    if (blocks > 0x7fffffffLL) return fail(9, "lc_crop_warp_u8: too many rows and bands for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (out_dtype) {
        case LC_CROP_U8: launch_channels<LC_CROP_U8>(p, C, interp, (unsigned)blocks, s); break;
        case LC_CROP_F32: launch_channels<LC_CROP_F32>(p, C, interp, (unsigned)blocks, s); break;
        case LC_CROP_F16: launch_channels<LC_CROP_F16>(p, C, interp, (unsigned)blocks, s); break;
        default: launch_channels<LC_CROP_BF16>(p, C, interp, (unsigned)blocks, s); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(10, std::string("lc_crop_warp_u8: launch: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
