// The synthetic scenes' object poses drawn on the device (liblc_amd_posedraw.so; C ABI and the exact definition of every output in
// include/lc_amd_posedraw.h; lc_amd/posedraw.py is its statement in host numpy: `draw_scene_poses_host`).
//
// One kernel, one wavefront of 64 per scene.  Lane m is the home of slot m: it reads the slot's mesh and radius, decides the refusals,
// forms the slot's rotation before the loop and keeps the slot's placed position in its registers.  The slots are then placed in order,
// because each depends on the ones before: for slot m lane k forms the candidate position of try k (three hashes, a dozen fp64
// operations), the sphere of every earlier placed slot j is read out of lane j (v_readlane: j is the same in every lane, so the value
// travels through scalar registers, not through LDS), every lane tests its candidate against it, and the winner is the lowest set bit
// of the ballot.  The chain is M dependent slots of up to m sphere tests each: latency, not bandwidth -- no LDS, no workspace, no
// atomics; the outputs are plain stores of lane m's own rows.
//
// The bits: every fp64 operation of the definition is written as __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn, one call
// per rounding, in the definition's order (the build's -ffp-contract=on fuses a product and a sum that stand in ONE expression).  The
// cosine and the sine are the polynomial of include/lc_amd_geometry.h on its exactly reduced argument, never a library call.
//
// Bounds: block s < S (the grid); lane m >= M reads and writes nothing of its own but still serves as a try.  Lane m < M reads
// mesh_index[s M + m] and, only where 0 <= mi < n_meshes, radius[mi]; every lane reads scene_id[s] and cam_K[s K_stride .. + 8]
// (K_stride 0 or 9, checked on the host); lane m < M writes rows s M + m of the outputs.  No other input VALUE forms an address.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_posedraw.h"
#include "../shared/lc_keyed_hash.h"

#ifndef LC_AMD_POSEDRAW_SRC_HASH
#define LC_AMD_POSEDRAW_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_POSEDRAW_SRC_HASH:" LC_AMD_POSEDRAW_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kWave = 64;
static_assert(LC_POSEDRAW_MAX_INSTANCES == kWave && LC_POSEDRAW_TRIES == kWave, "lane m = slot m, lane k = try k");

__device__ inline double uniform(unsigned state, unsigned i) { return key_uniform(fmix32(state ^ i)); }

// fl(pi / 4) and the Taylor coefficients rounded to fp64: PI_4, SIN_C and COS_C of lc_amd/geometry.py
constexpr double kPi4 = 0x1.921fb54442d18p-1;
__device__ const double kSin[8] = {-0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                                   -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49};
__device__ const double kCos[8] = {-0x1.0000000000000p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16,
                                   -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37, 0x1.ae7f3e733b81fp-45};

// `geometry.cos_sin_turns`: (cos, sin) of 4 pi x
__device__ inline void cos_sin_turns(double x, double& c, double& s) {
    const double tau = __dmul_rn(2.0, x);
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

// The value `v` has in lane `lane`, the same lane for the whole wavefront: two v_readlane_b32
__device__ inline double lane_value(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

struct Params {
    double z_min, z_max, x0, y0, x1, y1, gap, near;
    const unsigned long long* seed;
    const int* scene_id;
    const int* mesh_index;
    const float* radius;
    const float* cam_K;
    float* R;
    float* t;
    int* tries;
    int* info;
    int* mesh_index_out;
    int n_meshes, K_stride, M;
};

__global__ __launch_bounds__(kWave) void lc_posedraw_scenes_kernel(const Params p) {
    const int s = (int)blockIdx.x, lane = (int)threadIdx.x, M = p.M;
    const unsigned long long seed = *p.seed;
    const unsigned state = fmix32(sample_state(seed_state((unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)), (unsigned)p.scene_id[s]) ^
                                  (unsigned)LC_POSEDRAW_OP_POSE);
    const float* Kf = p.cam_K + (size_t)p.K_stride * (size_t)s;
    bool K_ok = true;
    double K[6];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const float v = Kf[j];
        K_ok = K_ok && isfinite(v);
        if (j < 6) K[j] = (double)v;
    }
    K_ok = K_ok && K[0] != 0.0 && K[4] != 0.0;

    // lane m: the slot's mesh, radius, refusal and rotation
    const bool slot = lane < M;
    const size_t row = (size_t)s * (size_t)M + (size_t)lane;
    int mi = -1, status = -3;
    double r = 0.0;
    if (slot) mi = p.mesh_index[row];
    if (slot && mi != -1) {
        status = -2;
        if (mi >= 0 && mi < p.n_meshes && K_ok) {
            r = (double)p.radius[mi];
            if (r >= 0.0 && isfinite(r) && __dsub_rn(p.z_min, r) > p.near) status = 0;
        }
    }
    double Rm[9];
    {
        const unsigned i0 = (unsigned)lane * (unsigned)(LC_POSEDRAW_TRIES * 8);
        const double u0 = uniform(state, i0), u1 = uniform(state, i0 + 1), u2 = uniform(state, i0 + 2);
        const double a = __dsqrt_rn(__dsub_rn(1.0, u0)), b = __dsqrt_rn(u0);
        double c1, s1, c2, s2;
        cos_sin_turns(__dmul_rn(u1, 0.5), c1, s1);
        cos_sin_turns(__dmul_rn(u2, 0.5), c2, s2);
        const double x = __dmul_rn(a, s1), y = __dmul_rn(a, c1), z = __dmul_rn(b, s2), w = __dmul_rn(b, c2);
        const double xx = __dmul_rn(x, x), yy = __dmul_rn(y, y), zz = __dmul_rn(z, z), xy = __dmul_rn(x, y), xz = __dmul_rn(x, z), yz = __dmul_rn(y, z);
        const double wx = __dmul_rn(w, x), wy = __dmul_rn(w, y), wz = __dmul_rn(w, z);
        Rm[0] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(yy, zz)));
        Rm[1] = __dmul_rn(2.0, __dsub_rn(xy, wz));
        Rm[2] = __dmul_rn(2.0, __dadd_rn(xz, wy));
        Rm[3] = __dmul_rn(2.0, __dadd_rn(xy, wz));
        Rm[4] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, zz)));
        Rm[5] = __dmul_rn(2.0, __dsub_rn(yz, wx));
        Rm[6] = __dmul_rn(2.0, __dsub_rn(xz, wy));
        Rm[7] = __dmul_rn(2.0, __dadd_rn(yz, wx));
        Rm[8] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, yy)));
    }

    // the slots in order: lane k = try k of slot m; the placed position of slot j stays in lane j
    const double wx_box = __dsub_rn(p.x1, p.x0), wy_box = __dsub_rn(p.y1, p.y0), wz_box = __dsub_rn(p.z_max, p.z_min);
    double px = 0.0, py = 0.0, pz = 0.0;
    int taken = 0;
    unsigned long long placed = 0;  // the same in every lane
    for (int m = 0; m < M; ++m) {
        if (__builtin_amdgcn_readlane(status, m) != 0) continue;
        const double r_m = lane_value(r, m);
        const unsigned i0 = ((unsigned)m * (unsigned)LC_POSEDRAW_TRIES + (unsigned)lane) * 8u;
        const double cpx = __dadd_rn(p.x0, __dmul_rn(uniform(state, i0 + 3), wx_box));
        const double cpy = __dadd_rn(p.y0, __dmul_rn(uniform(state, i0 + 4), wy_box));
        const double cz = __dadd_rn(p.z_min, __dmul_rn(uniform(state, i0 + 5), wz_box));
        const double yn = __ddiv_rn(__dsub_rn(cpy, K[5]), K[4]);
        const double xn = __ddiv_rn(__dsub_rn(__dsub_rn(cpx, K[2]), __dmul_rn(K[1], yn)), K[0]);
        const double cx = __dmul_rn(xn, cz), cy = __dmul_rn(yn, cz);
        bool good = true;
        for (unsigned long long rest = placed; rest; rest &= rest - 1) {
            const int j = __builtin_ctzll(rest);
            const double sep = __dadd_rn(__dadd_rn(r_m, lane_value(r, j)), p.gap);
            const double dx = __dsub_rn(cx, lane_value(px, j)), dy = __dsub_rn(cy, lane_value(py, j)), dz = __dsub_rn(cz, lane_value(pz, j));
            const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            good = good && d2 >= __dmul_rn(sep, sep);
        }
        const unsigned long long won = __ballot(good);
        if (won) {
            const int k = __builtin_ctzll(won);
            const double tx = lane_value(cx, k), ty = lane_value(cy, k), tz = lane_value(cz, k);
            if (lane == m) {
                px = tx;
                py = ty;
                pz = tz;
                taken = k;
            }
            placed |= 1ull << m;
        } else if (lane == m) {
            status = -1;
            taken = LC_POSEDRAW_TRIES;
        }
    }

    if (!slot) return;
    const bool is_placed = status == 0;
    float* R = p.R + 9 * row;
    float* t = p.t + 3 * row;
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = is_placed ? (float)Rm[j] : 0.0f;
    t[0] = is_placed ? (float)px : 0.0f;
    t[1] = is_placed ? (float)py : 0.0f;
    t[2] = is_placed ? (float)pz : 0.0f;
    p.tries[row] = taken;
    p.info[row] = status;
    p.mesh_index_out[row] = is_placed ? mi : -1;
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_posedraw_version(void) { return LC_AMD_POSEDRAW_VERSION; }
const char* lc_amd_posedraw_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_POSEDRAW_SRC_HASH:") - 1; }
const char* lc_amd_posedraw_last_error(void) { return lc::g_err.c_str(); }

int lc_posedraw_scenes_f32(double z_min, double z_max, double x0, double y0, double x1, double y1, double gap, double near, const uint64_t* seed,
                           const int* scene_id, const int* mesh_index, const float* radius, int n_meshes, const float* cam_K, int K_stride, int S, int M,
                           float* R, float* t, int* tries, int* info, int* mesh_index_out, void* stream) {
    using lc::fail;
    const std::string me = "lc_posedraw_scenes_f32: ";
    if (S < 0 || S > LC_POSEDRAW_MAX_SCENES) return fail(1, me + "0 <= S <= " + std::to_string(LC_POSEDRAW_MAX_SCENES) + ", got " + std::to_string(S));
    if (M < 1 || M > LC_POSEDRAW_MAX_INSTANCES) return fail(1, me + "1 <= M <= " + std::to_string(LC_POSEDRAW_MAX_INSTANCES) + ", got " + std::to_string(M));
    if (S == 0) return 0;
    if (n_meshes < 1) return fail(1, me + "n_meshes >= 1, got " + std::to_string(n_meshes));
    if (!seed) return fail(2, me + "seed must not be NULL: it points to one uint64 on the device");
    if (!scene_id || !mesh_index || !radius || !cam_K) return fail(2, me + "scene_id, mesh_index, radius and cam_K must not be NULL");
    if (!R || !t || !tries || !info || !mesh_index_out) return fail(2, me + "R, t, tries, info and mesh_index_out must not be NULL");
    const double numbers[8] = {z_min, z_max, x0, y0, x1, y1, gap, near};
    for (double v : numbers)
        if (!std::isfinite(v)) return fail(3, me + "z_min, z_max, x0, y0, x1, y1, gap and near must be finite");
    if (z_min > z_max) return fail(4, me + "z_min <= z_max, got " + std::to_string(z_min) + " and " + std::to_string(z_max));
    if (x0 > x1 || y0 > y1)
        return fail(4, me + "x0 <= x1 and y0 <= y1, got (" + std::to_string(x0) + ", " + std::to_string(y0) + ", " + std::to_string(x1) + ", " + std::to_string(y1) + ")");
    if (gap < 0.0) return fail(5, me + "gap >= 0, got " + std::to_string(gap));
    if (K_stride != 0 && K_stride != 9) return fail(6, me + "K_stride must be 0 (one camera for all scenes) or 9, got " + std::to_string(K_stride));
    if (lc::misaligned(seed, 8)) return fail(7, me + "seed must be aligned to 8 bytes");
    if (lc::misaligned(scene_id, 4) || lc::misaligned(mesh_index, 4) || lc::misaligned(radius, 4) || lc::misaligned(cam_K, 4) || lc::misaligned(R, 4) ||
        lc::misaligned(t, 4) || lc::misaligned(tries, 4) || lc::misaligned(info, 4) || lc::misaligned(mesh_index_out, 4))
        return fail(7, me + "scene_id, mesh_index, radius, cam_K and the outputs must be aligned to 4 bytes");

    lc::Params p{};
    p.z_min = z_min; p.z_max = z_max; p.x0 = x0; p.y0 = y0; p.x1 = x1; p.y1 = y1; p.gap = gap; p.near = near;
    p.seed = reinterpret_cast<const unsigned long long*>(seed);
    p.scene_id = scene_id; p.mesh_index = mesh_index; p.radius = radius; p.cam_K = cam_K;
    p.R = R; p.t = t; p.tries = tries; p.info = info; p.mesh_index_out = mesh_index_out;
    p.n_meshes = n_meshes; p.K_stride = K_stride; p.M = M;
    hipLaunchKernelGGL(lc::lc_posedraw_scenes_kernel, dim3((unsigned)S), dim3(lc::kWave), 0, static_cast<hipStream_t>(stream), p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(9, me + "launch: " + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
