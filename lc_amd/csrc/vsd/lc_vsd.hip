// BOP's Visible Surface Discrepancy on the GPU, the comparison stage: three depth maps per pose (the object under the estimated pose, under
// the ground-truth pose, and the scene's measured depth) in, a handful of integer counts and T errors per pose out.  The exact definition
// -- visib_mode 'bop19', cost_type 'step', every fp64 operation rounded on its own -- is include/lc_amd_vsd.h; tests/vsd_oracle.py is its
// numpy restatement.  The depth maps come from lc_amd.render.render_depth (lc_amd/vsd.py chains the two) or from any other renderer.
//
// Launch shape.  A pose's (h,w) maps are cut into strips of whole rows of about kStripPixels pixels, one workgroup of four wavefronts per
// (pose, strip).  Inside a strip the work items are (row, group of four pixels), flattened, so a 192-pixel window row leaves no lane idle.
// A row's groups start at the 16-byte boundary at or before the row's first element of depth_est; where depth_gt and the scene's row share
// that phase the three loads of a full group are 16-byte loads, else -- a window origin or a width that breaks the phase, the partial
// groups at both ends of a row -- four guarded 4-byte loads each.  The choice is uniform over a row.
//
// Arithmetic.  Most pixels of a frame see neither rendering and are done after three loads and two compares.  The others take one fp64
// division and one square root for the ray length (shared/lc_ray_length.h; Y's division is shared by a group), three products, and the
// comparisons of steps 2 to 4.  -ffp-contract=on fuses only inside one expression, so every product and sum below is a statement of its own.
//
// Counting.  Each lane keeps 3 + T integer counters in registers; a wavefront that counted anything sums them with a butterfly, the four
// wavefronts meet in LDS, and a workgroup adds its non-zero sums to counts[b] with integer atomics.  Integer addition is associative: the counts are the same
// bits for any grid shape and arrival order.  counts is zeroed in-stream by a launch of its own and turned into errors (or the refusal
// marks) by a finishing launch, one thread per pose: three launches, no workspace, no allocation, no wait.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_vsd.h"
#include "../shared/lc_ray_length.h"
#include "../shared/lc_wave_int.h"

#ifndef LC_AMD_VSD_SRC_HASH
#define LC_AMD_VSD_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_VSD_SRC_HASH:" LC_AMD_VSD_SRC_HASH;
thread_local std::string g_err;

int fail(int code, const char* msg) {
    g_err = msg;
    return code;
}

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxT = LC_VSD_MAX_TAUS;
constexpr int kHead = 3;  // union, inter, edge in front of the T costs
constexpr int kStripPixels = 4096;

struct VsdParams {
    const float* est;    // (B,h,w)
    const float* gt;     // (B,h,w)
    const float* test;   // (S,H,W)
    const int* scene;    // (B,)
    const float* K;      // (B,3,3)
    const float* diam;   // (B,) or null
    const int* win;      // (B,2) x0, y0 or null
    int B, h, w, S, H, W, T;
    float delta, pcx, pcy;
    int* counts;         // (B, T+3)
    float* errors;       // (B, T)
    float taus[kMaxT];
};

// where pose b's maps lie; false: refused (none of its maps is read)
struct PoseRow {
    int scene, x0, y0;
};
__device__ __forceinline__ bool pose_row(const VsdParams& p, int b, PoseRow& r) {
    r.scene = p.scene[b];
    r.x0 = p.win ? p.win[2 * (size_t)b] : 0;
    r.y0 = p.win ? p.win[2 * (size_t)b + 1] : 0;
    if (r.scene < 0 || r.scene >= p.S) return false;
    return r.x0 >= 0 && r.y0 >= 0 && (long long)r.x0 + p.w <= p.W && (long long)r.y0 + p.h <= p.H;
}

struct Camera {
    double k00, k01, k02, k11, k12, pcx, pcy, delta;
};

struct Counters {
    int n_union, n_inter, n_edge, cost[kMaxT];
};

// steps 1 to 4 of the header for one pixel; xf: its column in the frame, yy = Y Y and kY = K01 Y of its row
__device__ __forceinline__ void pixel(float fe, float fg, float ft, int xf, double yy, double kY, bool border, const Camera& c,
                                      const double (&thr)[kMaxT], int T, Counters& a) {
    const bool he = fe > 0.0f, hg = fg > 0.0f;
    if (!(he || hg)) return;
    a.n_edge += border ? 1 : 0;
    const double n = ray_length(xf, c.pcx, c.k02, c.k00, kY, yy);
    const bool missing = !(ft > 0.0f);
    const double dist_e = (double)fe * n;
    const double dist_g = (double)fg * n;
    const double dist_t = (double)ft * n;
    const double over_g = dist_g - dist_t;
    const double over_e = dist_e - dist_t;
    const bool vis_g = hg && (missing || over_g <= c.delta);
    const bool vis_e = he && (missing || over_e <= c.delta || vis_g);
    a.n_union += (vis_g || vis_e) ? 1 : 0;
    if (vis_g && vis_e) {
        a.n_inter += 1;
        const double diff = fabs(dist_g - dist_e);
#pragma unroll
        for (int k = 0; k < kMaxT; ++k)
            if (k < T) a.cost[k] += diff >= thr[k] ? 1 : 0;
    }
}

__device__ __forceinline__ bool aligned16(const float* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

__global__ __launch_bounds__(kThreads) void lc_vsd_zero_kernel(int* counts, long long n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) counts[i] = 0;
}

__global__ __launch_bounds__(kThreads) void lc_vsd_count_kernel(const VsdParams p, int strips, int rows_per_strip) {
    __shared__ int s_part[kWaves][kHead + kMaxT];
    const int b = blockIdx.x / strips, strip = blockIdx.x - b * strips;
    PoseRow row;
    if (!pose_row(p, b, row)) return;  // the whole workgroup
    const int T = p.T, h = p.h, w = p.w;
    const int r0 = strip * rows_per_strip, r1 = min(h, r0 + rows_per_strip);

    const float* K = p.K + 9 * (size_t)b;
    Camera c;
    c.k00 = K[0]; c.k01 = K[1]; c.k02 = K[2]; c.k11 = K[4]; c.k12 = K[5];
    c.pcx = p.pcx; c.pcy = p.pcy; c.delta = p.delta;
    const double diam = p.diam ? (double)p.diam[b] : 1.0;
    double thr[kMaxT];
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) thr[k] = k < T ? (double)p.taus[k] * diam : 0.0;

    const float* est = p.est + (size_t)b * h * w;
    const float* gt = p.gt + (size_t)b * h * w;
    const float* test = p.test + ((size_t)row.scene * p.H + row.y0) * p.W + row.x0;
    // the sides of the window that are not the frame's own
    const bool cut_l = row.x0 > 0, cut_r = row.x0 + w < p.W, cut_t = row.y0 > 0, cut_b = row.y0 + h < p.H;

    Counters a;
    a.n_union = a.n_inter = a.n_edge = 0;
#pragma unroll
    for (int k = 0; k < kMaxT; ++k) a.cost[k] = 0;

    const int gpr = (w + 6) / 4;  // groups per row: enough for a row that starts three elements behind a 16-byte boundary
    const int items = (r1 - r0) * gpr;
    for (int i = threadIdx.x; i < items; i += kThreads) {
        const int ry = i / gpr, g = i - ry * gpr;
        const int y = r0 + ry;
        const float* e_row = est + (size_t)y * w;
        const float* g_row = gt + (size_t)y * w;
        const float* t_row = test + (size_t)y * p.W;
        const int lead = lead_of(e_row);
        const int x = 4 * g - lead;
        if (x >= w) continue;
        float fe[4], fg[4], ft[4];
        if (x >= 0 && x + 4 <= w && aligned16(g_row + x) && aligned16(t_row + x)) {
            const float4 ve = *reinterpret_cast<const float4*>(e_row + x);
            const float4 vg = *reinterpret_cast<const float4*>(g_row + x);
            const float4 vt = *reinterpret_cast<const float4*>(t_row + x);
            fe[0] = ve.x; fe[1] = ve.y; fe[2] = ve.z; fe[3] = ve.w;
            fg[0] = vg.x; fg[1] = vg.y; fg[2] = vg.z; fg[3] = vg.w;
            ft[0] = vt.x; ft[1] = vt.y; ft[2] = vt.z; ft[3] = vt.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = x + j >= 0 && x + j < w;
                fe[j] = in ? e_row[x + j] : 0.0f;
                fg[j] = in ? g_row[x + j] : 0.0f;
                ft[j] = in ? t_row[x + j] : 0.0f;
            }
        }
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) any = any || fe[j] > 0.0f || fg[j] > 0.0f;
        if (!any) continue;
        const RayRow r = ray_row(y + row.y0, c.pcy, c.k12, c.k11, c.k01);
        const bool row_cut = (y == 0 && cut_t) || (y == h - 1 && cut_b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xj = x + j;  // a pixel outside the row holds zeros and counts nothing
            const bool border = row_cut || (xj == 0 && cut_l) || (xj == w - 1 && cut_r);
            pixel(fe[j], fg[j], ft[j], xj + row.x0, r.yy, r.kY, border, c, thr, T, a);
        }
    }

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    // a wavefront that saw no hit (most of a mostly empty frame) hands in zeros without the 3 + T butterflies: inter and the costs are
    // parts of union, so union and edge say whether any counter is set.  The test is uniform over the wavefront; the barrier is not inside it.
    if (__any((a.n_union | a.n_edge) != 0)) {
        const int u = wave_sum(a.n_union), n = wave_sum(a.n_inter), e = wave_sum(a.n_edge);
        if (lane == 0) { s_part[wave][0] = u; s_part[wave][1] = n; s_part[wave][2] = e; }
#pragma unroll
        for (int k = 0; k < kMaxT; ++k) {
            if (k < T) {
                const int v = wave_sum(a.cost[k]);
                if (lane == 0) s_part[wave][kHead + k] = v;
            }
        }
    } else if (lane < kHead + T) {
        s_part[wave][lane] = 0;
    }
    __syncthreads();
    if (threadIdx.x < kHead + T) {
        int v = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) v += s_part[wv][threadIdx.x];
        if (v != 0) atomicAdd(p.counts + (size_t)b * (kHead + T) + threadIdx.x, v);
    }
}

// one thread per pose: the errors from the counts, or the refusal marks
__global__ __launch_bounds__(kThreads) void lc_vsd_finish_kernel(const VsdParams p) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= p.B) return;
    int* cnt = p.counts + (size_t)b * (kHead + p.T);
    float* err = p.errors + (size_t)b * p.T;
    PoseRow row;
    if (!pose_row(p, b, row)) {
        for (int j = 0; j < kHead + p.T; ++j) cnt[j] = -1;
        for (int k = 0; k < p.T; ++k) err[k] = __builtin_nanf("");
        return;
    }
    const int n_union = cnt[0], n_inter = cnt[1];
    for (int k = 0; k < p.T; ++k) {
        const int wrong = cnt[kHead + k] + n_union - n_inter;  // at most n_union: no overflow
        err[k] = n_union == 0 ? 1.0f : (float)((double)wrong / (double)n_union);
    }
}

int launch_vsd(const VsdParams& p, hipStream_t stream) {
    const long long n = (long long)p.B * (kHead + p.T);
    hipLaunchKernelGGL(lc_vsd_zero_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, p.counts, n);
    if (hipGetLastError() != hipSuccess) return 2;
    const int rows_per_strip = p.w >= kStripPixels ? 1 : kStripPixels / p.w;
    const int strips = (p.h + rows_per_strip - 1) / rows_per_strip;
    hipLaunchKernelGGL(lc_vsd_count_kernel, dim3((unsigned)((long long)p.B * strips)), dim3(kThreads), 0, stream, p, strips, rows_per_strip);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(lc_vsd_finish_kernel, dim3((p.B + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

bool misaligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) != 0; }

// the argument rules of lc_vsd_score_f32 that need no device; null: in order
const char* args_error(const VsdParams& p, const float* taus) {
    if (p.B < 0 || p.T < 0 || p.h < 0 || p.w < 0 || p.S < 0 || p.H < 0 || p.W < 0) return "lc_vsd_score_f32: a negative size";
    if (p.B == 0) return nullptr;
    if (p.T < 1 || p.T > kMaxT) return "lc_vsd_score_f32: 1 to 16 thresholds (T)";
    if (p.S < 1) return "lc_vsd_score_f32: at least one scene (S)";
    if (p.H < 1 || p.W < 1 || p.H > LC_VSD_MAX_SIZE || p.W > LC_VSD_MAX_SIZE) return "lc_vsd_score_f32: frame sizes of 1 to 16384";
    if (p.h < 1 || p.w < 1 || p.h > p.H || p.w > p.W) return "lc_vsd_score_f32: the maps must fit the frame: 1 <= h <= H and 1 <= w <= W";
    if (!p.win && (p.h != p.H || p.w != p.W)) return "lc_vsd_score_f32: without window_xy the maps have the frame's size";
    if (!p.est || !p.gt || !p.test || !p.scene || !p.K || !taus || !p.counts || !p.errors) return "lc_vsd_score_f32: a null argument";
    if (misaligned4(p.est) || misaligned4(p.gt) || misaligned4(p.test) || misaligned4(p.scene) || misaligned4(p.K) || misaligned4(p.diam) ||
        misaligned4(p.win) || misaligned4(p.counts) || misaligned4(p.errors))
        return "lc_vsd_score_f32: every pointer must be 4-byte aligned";
    const long long strips = p.w >= kStripPixels ? p.h : (p.h + kStripPixels / p.w - 1) / (kStripPixels / p.w);
    if ((long long)p.B * strips >= (1ll << 31) || (long long)p.B * (kHead + kMaxT) >= (1ll << 31)) return "lc_vsd_score_f32: more than 2^31 strips or counts";
    return nullptr;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_vsd_version(void) { return LC_AMD_VSD_VERSION; }
const char* lc_amd_vsd_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_VSD_SRC_HASH:") - 1; }
const char* lc_amd_vsd_last_error(void) { return lc::g_err.c_str(); }

int lc_vsd_score_f32(const float* depth_est, const float* depth_gt, const float* depth_test, const int* scene_index, const float* K,
                     const float* diameter, const float* taus, int T, float delta, const int* window_xy, int B, int h, int w, int S, int H,
                     int W, float pcx, float pcy, int* counts, float* errors, void* stream) {
    lc::VsdParams p{};
    p.est = depth_est; p.gt = depth_gt; p.test = depth_test; p.scene = scene_index; p.K = K; p.diam = diameter; p.win = window_xy;
    p.B = B; p.h = h; p.w = w; p.S = S; p.H = H; p.W = W; p.T = T;
    p.delta = delta; p.pcx = pcx; p.pcy = pcy; p.counts = counts; p.errors = errors;
    if (const char* e = lc::args_error(p, taus)) return lc::fail(1, e);
    if (B == 0) return 0;
    for (int k = 0; k < T; ++k) p.taus[k] = taus[k];
    return lc::launch_vsd(p, static_cast<hipStream_t>(stream)) ? lc::fail(11, "vsd launch failed") : 0;
}

}  // extern "C"
#pragma GCC visibility pop
