// The training crops' geometry drawn on the device (liblc_amd_geometry.so; C ABI and the exact definition of every output in
// include/lc_amd_geometry.h; lc_amd/geometry.py is its statement in host numpy: `zoom_geometry_host`, `augment.background_matrices`).
// What the reference's loader computes per instance on a host core before it touches a pixel (dataset.py:313-327,402-405,437,470).
//
// Two kernels, one thread per sample in workgroups of 64: a row is some three hundred dependent fp64 operations on four box and nine
// camera numbers, so there is nothing to share between lanes and nothing to stage -- no LDS, no workspace, no atomics.  The seed is one
// word on the device that every thread reads: a replayed graph draws anew once the word has changed.
//
// The bits: every fp64 operation of the definition is written as __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn, one call per rounding,
// in the definition's order.  The build's -ffp-contract=on fuses a product and a sum that stand in ONE expression, and the definition
// rounds each Horner step twice.  The cosine and the sine are the definition's polynomial on its exactly reduced argument, never a
// library call.  Outputs are plain stores.
//
// The hash is maskcrop's and augment's: shared/lc_keyed_hash.h.
//
// Bounds: thread b >= B returns before it reads; row b reads sample_id[b], bbox[4 b .. 4 b + 3], cam_K[b K_stride .. + 8] (K_stride 0 or
// 9, checked on the host) and bg_hw[2 b .. 2 b + 1], and writes its own rows of the outputs; no input VALUE forms an address.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_geometry.h"
#include "../shared/lc_keyed_hash.h"

#ifndef LC_AMD_GEOMETRY_SRC_HASH
#define LC_AMD_GEOMETRY_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_GEOMETRY_SRC_HASH:" LC_AMD_GEOMETRY_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 64;

// The key state of (seed, sample_id, op): key(op, i) = fmix32(state ^ i)
__device__ inline unsigned key_state(unsigned long long seed, int sample_id, unsigned op) {
    return fmix32(sample_state(seed_state((unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)), (unsigned)sample_id) ^ op);
}

__device__ inline double uniform(unsigned state, unsigned i) { return key_uniform(fmix32(state ^ i)); }

// fl(pi / 4) and (-1)^(k/2) / k! rounded to fp64, k = 3, 5, ..., 17 and k = 2, 4, ..., 16: PI_4, SIN_C and COS_C of lc_amd/geometry.py
constexpr double kPi4 = 0x1.921fb54442d18p-1;
__device__ const double kSin[8] = {-0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                                   -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49};
__device__ const double kCos[8] = {-0x1.0000000000000p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16,
                                   -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37, 0x1.ae7f3e733b81fp-45};

// `cos_sin_turns`: (cos, sin) of 4 pi u4
__device__ inline void cos_sin_turns(double u4, double& c, double& s) {
    const double tau = __dmul_rn(2.0, u4);
    const double f = __dsub_rn(tau, floor(tau));
    const double f8 = __dmul_rn(8.0, f);
    const double fo = floor(f8);
    const int o = (int)fo;
    double g = __dsub_rn(f8, fo);
    if (o & 1) g = __dsub_rn(1.0, g);
    const double a = __dmul_rn(g, kPi4);
    const double z = __dmul_rn(a, a);
    double p = kSin[7], q = kCos[7];
#pragma unroll
    for (int j = 6; j >= 0; --j) {
        p = __dadd_rn(__dmul_rn(p, z), kSin[j]);
        q = __dadd_rn(__dmul_rn(q, z), kCos[j]);
    }
    const double S = __dmul_rn(a, __dadd_rn(__dmul_rn(p, z), 1.0));
    const double C = __dadd_rn(__dmul_rn(q, z), 1.0);
    switch (o & 7) {  // OCTANTS
        case 0: c = C; s = S; break;
        case 1: c = S; s = C; break;
        case 2: c = -S; s = C; break;
        case 3: c = -C; s = S; break;
        case 4: c = -C; s = -S; break;
        case 5: c = -S; s = -C; break;
        case 6: c = S; s = -C; break;
        default: c = C; s = -S; break;
    }
}

// `_affine`: the forward matrix of a (dst_w, dst_h) target, term for term, rounded to fp32 once
__device__ inline void affine(double scale, double c, double s, double cx, double cy, double dst_w, double dst_h, float* M) {
    const double k = __ddiv_rn(dst_w, scale);
    const double dx = __dmul_rn(dst_w, 0.5), dy = __dmul_rn(dst_h, 0.5);
    const double kc = __dmul_rn(k, c), ks = __dmul_rn(k, s), nks = __dmul_rn(-k, s);
    M[0] = (float)kc;
    M[1] = (float)ks;
    M[2] = (float)__dsub_rn(dx, __dadd_rn(__dmul_rn(kc, cx), __dmul_rn(ks, cy)));
    M[3] = (float)nks;
    M[4] = (float)kc;
    M[5] = (float)__dsub_rn(dy, __dadd_rn(__dmul_rn(nks, cx), __dmul_rn(kc, cy)));
}

struct ZoomParams {
    double dzi_scale_ratio, dzi_shift_ratio, dzi_pad_scale, rotate_prob;
    double max_im, in_w, in_h, out_w, out_h;
    const unsigned long long* seed;
    const int* sample_id;
    const float* bbox;
    const float* cam_K;
    float* in_affine;
    float* out_affine;
    float* out_K;
    float* out_pix_scale;
    int* step_id;
    int* info;
    double* centre;
    double* scale;
    double* cs;
    int train, K_stride, B;
};

__global__ __launch_bounds__(kThreads) void lc_geometry_zoom_kernel(const ZoomParams p) {
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (b >= p.B) return;
    const unsigned state = key_state(*p.seed, p.sample_id[b], LC_GEOMETRY_OP_ZOOM);
    const float* bx = p.bbox + 4 * (size_t)b;
    const float* Kf = p.cam_K + (size_t)p.K_stride * (size_t)b;
    const double x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
    float K32[9];
    bool finite = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        K32[j] = Kf[j];
        finite = finite && isfinite(K32[j]);
    }
    const double bcx = __dmul_rn(0.5, __dadd_rn(x1, x2)), bcy = __dmul_rn(0.5, __dadd_rn(y1, y2));
    const double bw = __dsub_rn(x2, x1), bh = __dsub_rn(y2, y1);
    double cx, cy, scale, c = 1.0, s = 0.0;
    if (p.train) {
        const double r0 = __dsub_rn(__dmul_rn(2.0, uniform(state, 0)), 1.0);
        const double r1 = __dsub_rn(__dmul_rn(2.0, uniform(state, 1)), 1.0);
        const double r2 = __dsub_rn(__dmul_rn(2.0, uniform(state, 2)), 1.0);
        const double ratio = __dadd_rn(1.0, __dmul_rn(p.dzi_scale_ratio, r0));
        cx = __dadd_rn(bcx, __dmul_rn(bw, __dmul_rn(p.dzi_shift_ratio, r1)));
        cy = __dadd_rn(bcy, __dmul_rn(bh, __dmul_rn(p.dzi_shift_ratio, r2)));
        scale = __dmul_rn(__dmul_rn(bh > bw ? bh : bw, ratio), p.dzi_pad_scale);
        scale = scale > p.max_im ? p.max_im : scale;
        if (uniform(state, 3) < p.rotate_prob) cos_sin_turns(uniform(state, 4), c, s);
    } else {
        cx = bcx;
        cy = bcy;
        double m = bw > bh ? bw : bh;
        m = m > 1.0 ? m : 1.0;
        scale = __dmul_rn(m, p.dzi_pad_scale);
    }
    const bool bad = !(finite && isfinite(scale) && scale > 0.0);

    float Mi[6], Mo[6], oK[6];
    affine(scale, c, s, cx, cy, p.in_w, p.in_h, Mi);
    affine(scale, c, s, cx, cy, p.out_w, p.out_h, Mo);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double a0 = Mo[3 * i], a1 = Mo[3 * i + 1], a2 = Mo[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j)
            oK[3 * i + j] = (float)__dadd_rn(__dadd_rn(__dmul_rn(a0, (double)K32[j]), __dmul_rn(a1, (double)K32[3 + j])), __dmul_rn(a2, (double)K32[6 + j]));
    }
    float pix = (float)__ddiv_rn(scale, p.out_w);

    const float nan32 = __builtin_nanf("");
    const double nan64 = __builtin_nan("");
    float* in_affine = p.in_affine + 6 * (size_t)b;
    float* out_affine = p.out_affine + 6 * (size_t)b;
    float* out_K = p.out_K + 9 * (size_t)b;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        in_affine[j] = bad ? nan32 : Mi[j];
        out_affine[j] = bad ? nan32 : Mo[j];
        out_K[j] = bad ? nan32 : oK[j];
    }
#pragma unroll
    for (int j = 6; j < 9; ++j) out_K[j] = bad ? nan32 : K32[j];
    p.out_pix_scale[b] = bad ? nan32 : pix;
    p.step_id[b] = (int)(fmix32(state ^ (unsigned)LC_GEOMETRY_STEP_INDEX) & 0x7fffffffu);
    p.info[b] = bad ? -1 : 0;
    if (p.centre) {
        p.centre[2 * (size_t)b] = bad ? nan64 : cx;
        p.centre[2 * (size_t)b + 1] = bad ? nan64 : cy;
    }
    if (p.scale) p.scale[b] = bad ? nan64 : scale;
    if (p.cs) {
        p.cs[2 * (size_t)b] = c;
        p.cs[2 * (size_t)b + 1] = s;
    }
}

struct BackgroundParams {
    const unsigned long long* seed;
    const int* sample_id;
    const int* bg_hw;  // (B,2) or null: the pair below
    float* M;
    int bg_h, bg_w, out_h, out_w, B;
};

__global__ __launch_bounds__(kThreads) void lc_geometry_background_kernel(const BackgroundParams p) {
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (b >= p.B) return;
    const unsigned state = key_state(*p.seed, p.sample_id[b], LC_GEOMETRY_OP_BG_REGION);
    const long long hb = p.bg_hw ? p.bg_hw[2 * (size_t)b] : p.bg_h, wb = p.bg_hw ? p.bg_hw[2 * (size_t)b + 1] : p.bg_w;
    const long long H = p.out_h, W = p.out_w;
    const auto lmax = [](long long a, long long b2) { return a > b2 ? a : b2; };
    const auto lmin = [](long long a, long long b2) { return a < b2 ? a : b2; };
    // |every product| < 2^32: the conversions to a 64-bit integer truncate towards zero, as np.trunc and astype do
    const long long roi_w = lmax((long long)__dmul_rn(uniform(state, 0), (double)wb), W);
    const long long roi_h = lmax((long long)__dmul_rn(uniform(state, 1), (double)hb), H);
    long long left = lmax((long long)__dmul_rn(uniform(state, 2), (double)(wb - roi_w)), 0);
    long long top = lmax((long long)__dmul_rn(uniform(state, 3), (double)(hb - roi_h)), 0);
    left = lmin(left, wb);
    top = lmin(top, hb);
    const double rw = (double)lmax(lmin(left + left + roi_w, wb) - left, 1);
    const double rh = (double)lmax(lmin(top + roi_h, hb) - top, 1);
    const double sx = __ddiv_rn((double)W, rw), sy = __ddiv_rn((double)H, rh);
    float* M = p.M + 6 * (size_t)b;
    M[0] = (float)sx;
    M[1] = 0.0f;
    M[2] = (float)__dsub_rn(__dmul_rn(__dsub_rn(0.5, (double)left), sx), 0.5);
    M[3] = 0.0f;
    M[4] = (float)sy;
    M[5] = (float)__dsub_rn(__dmul_rn(__dsub_rn(0.5, (double)top), sy), 0.5);
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

bool size_ok(int v) { return v >= 1 && v <= LC_GEOMETRY_MAX_SIZE; }

int launched(const std::string& me) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(9, me + "launch: " + hipGetErrorString(e));
    return 0;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_geometry_version(void) { return LC_AMD_GEOMETRY_VERSION; }
const char* lc_amd_geometry_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_GEOMETRY_SRC_HASH:") - 1; }
const char* lc_amd_geometry_last_error(void) { return lc::g_err.c_str(); }

int lc_geometry_zoom_f32(double dzi_scale_ratio, double dzi_shift_ratio, double dzi_pad_scale, double rotate_prob, int train, int im_h, int im_w,
                         int in_w, int in_h, int out_w, int out_h, const uint64_t* seed, const int* sample_id, const float* bbox_xyxy,
                         const float* cam_K, int K_stride, int B, float* in_affine, float* out_affine, float* out_K, float* out_pix_scale,
                         int* step_id, int* info, double* centre, double* scale, double* cs, void* stream) {
    using lc::fail;
    const std::string me = "lc_geometry_zoom_f32: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (!seed) return fail(2, me + "seed must not be NULL: it points to one uint64 on the device");
    if (!sample_id || !bbox_xyxy || !cam_K) return fail(2, me + "sample_id, bbox_xyxy and cam_K must not be NULL");
    if (!in_affine || !out_affine || !out_K || !out_pix_scale || !step_id || !info)
        return fail(2, me + "in_affine, out_affine, out_K, out_pix_scale, step_id and info must not be NULL");
    const int sizes[6] = {im_h, im_w, in_w, in_h, out_w, out_h};
    for (int v : sizes)
        if (!lc::size_ok(v))
            return fail(3, me + "im_h, im_w, in_w, in_h, out_w and out_h must be in [1, " + std::to_string(LC_GEOMETRY_MAX_SIZE) + "], got " + std::to_string(im_h) +
                               ", " + std::to_string(im_w) + ", " + std::to_string(in_w) + ", " + std::to_string(in_h) + ", " + std::to_string(out_w) + ", " +
                               std::to_string(out_h));
    if (!std::isfinite(dzi_scale_ratio) || !std::isfinite(dzi_shift_ratio) || !std::isfinite(dzi_pad_scale))
        return fail(4, me + "dzi_scale_ratio, dzi_shift_ratio and dzi_pad_scale must be finite, got " + std::to_string(dzi_scale_ratio) + ", " +
                           std::to_string(dzi_shift_ratio) + ", " + std::to_string(dzi_pad_scale));
    if (!(rotate_prob >= 0.0 && rotate_prob <= 1.0)) return fail(5, me + "rotate_prob must lie in [0, 1], got " + std::to_string(rotate_prob));
    if (K_stride != 0 && K_stride != 9) return fail(6, me + "K_stride must be 0 (one camera for all rows) or 9, got " + std::to_string(K_stride));
    if (lc::misaligned(seed, 8) || lc::misaligned(centre, 8) || lc::misaligned(scale, 8) || lc::misaligned(cs, 8))
        return fail(7, me + "seed, centre, scale and cs must be aligned to 8 bytes");
    if (lc::misaligned(sample_id, 4) || lc::misaligned(bbox_xyxy, 4) || lc::misaligned(cam_K, 4) || lc::misaligned(in_affine, 4) || lc::misaligned(out_affine, 4) ||
        lc::misaligned(out_K, 4) || lc::misaligned(out_pix_scale, 4) || lc::misaligned(step_id, 4) || lc::misaligned(info, 4))
        return fail(7, me + "sample_id, bbox_xyxy, cam_K and the 32-bit outputs must be aligned to 4 bytes");

    lc::ZoomParams p{};
    p.dzi_scale_ratio = dzi_scale_ratio; p.dzi_shift_ratio = dzi_shift_ratio; p.dzi_pad_scale = dzi_pad_scale; p.rotate_prob = rotate_prob;
    p.max_im = (double)(im_h > im_w ? im_h : im_w);
    p.in_w = in_w; p.in_h = in_h; p.out_w = out_w; p.out_h = out_h;
    p.seed = reinterpret_cast<const unsigned long long*>(seed);
    p.sample_id = sample_id; p.bbox = bbox_xyxy; p.cam_K = cam_K;
    p.in_affine = in_affine; p.out_affine = out_affine; p.out_K = out_K; p.out_pix_scale = out_pix_scale; p.step_id = step_id; p.info = info;
    p.centre = centre; p.scale = scale; p.cs = cs;
    p.train = train != 0; p.K_stride = K_stride; p.B = B;
    const unsigned blocks = ((unsigned)B + lc::kThreads - 1) / lc::kThreads;
    hipLaunchKernelGGL(lc::lc_geometry_zoom_kernel, dim3(blocks), dim3(lc::kThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me);
}

int lc_geometry_background_f32(const uint64_t* seed, const int* sample_id, int bg_h, int bg_w, const int* bg_hw, int out_h, int out_w, int B, float* M,
                               void* stream) {
    using lc::fail;
    const std::string me = "lc_geometry_background_f32: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (!seed) return fail(2, me + "seed must not be NULL: it points to one uint64 on the device");
    if (!sample_id || !M) return fail(2, me + "sample_id and M must not be NULL");
    if (!lc::size_ok(out_h) || !lc::size_ok(out_w))
        return fail(3, me + "out_h and out_w must be in [1, " + std::to_string(LC_GEOMETRY_MAX_SIZE) + "], got " + std::to_string(out_h) + " x " + std::to_string(out_w));
    if (!bg_hw && (!lc::size_ok(bg_h) || !lc::size_ok(bg_w)))
        return fail(3, me + "bg_h and bg_w must be in [1, " + std::to_string(LC_GEOMETRY_MAX_SIZE) + "] where bg_hw is NULL, got " + std::to_string(bg_h) + " x " +
                           std::to_string(bg_w));
    if (lc::misaligned(seed, 8)) return fail(7, me + "seed must be aligned to 8 bytes");
    if (lc::misaligned(sample_id, 4) || lc::misaligned(bg_hw, 4) || lc::misaligned(M, 4)) return fail(7, me + "sample_id, bg_hw and M must be aligned to 4 bytes");

    lc::BackgroundParams p{};
    p.seed = reinterpret_cast<const unsigned long long*>(seed);
    p.sample_id = sample_id; p.bg_hw = bg_hw; p.M = M;
    p.bg_h = bg_h; p.bg_w = bg_w; p.out_h = out_h; p.out_w = out_w; p.B = B;
    const unsigned blocks = ((unsigned)B + lc::kThreads - 1) / lc::kThreads;
    hipLaunchKernelGGL(lc::lc_geometry_background_kernel, dim3(blocks), dim3(lc::kThreads), 0, static_cast<hipStream_t>(stream), p);
    return lc::launched(me);
}

}  // extern "C"
#pragma GCC visibility pop
