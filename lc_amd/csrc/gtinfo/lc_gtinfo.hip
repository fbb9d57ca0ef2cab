// BOP's ground-truth visibility annotations on the GPU: one render per instance and the scene's depth in, the twelve integers of the
// annotation record and the visible mask per instance out (lc_gtinfo_f32); and, for scenes without a measured depth, the scene's depth
// as the per-pixel minimum over its instances' renders (lc_scene_compose_f32).  The exact definition of every output is
// include/lc_amd_gtinfo.h; tests/gtinfo_oracle.py is its numpy restatement.  The renders come from lc_amd.render.render_depth
// (lc_amd/gtinfo.py chains them) or from any other renderer.  Ray length and group loads: shared/lc_ray_length.h, with the VSD score.
//
// Launch shape.  An instance's (h,w) window is cut into tiles of kTileH rows by kGroups groups of four pixels, one workgroup of four
// wavefronts per (instance, tile); inside a tile the items are (row, group), flattened, so a 192-pixel window row leaves no lane idle.
// A row's groups start at the 16-byte boundary at or before the row's first element of the render, so a full group is one 16-byte load;
// the scene's row is read only by the groups that hold a hit, with a 16-byte load where the group lies in the frame and the frame row
// shares the phase (x0 and W decide that per row), else by guarded 4-byte loads.  The mask goes out as one 4-byte store per group where
// its row allows it, else bytewise.
//
// Arithmetic.  Most pixels see no render and are done after one load, one compare and the mask's zero.  A hit inside the frame whose
// scene depth is measured takes one fp64 division and one square root for the ray length (Y's division is shared by a group), two
// products and a difference.  -ffp-contract=on fuses only inside one expression, so every product and sum below is a statement of its own.
//
// Reduction.  Each lane keeps the twelve values in registers (four counts, four minima and maxima of each box); a wavefront that saw a
// hit folds them across its lanes, the four wavefronts meet in LDS (192 bytes, the only LDS here), and twelve threads of the workgroup
// issue at most twelve integer atomics (add, min, max) into info[b], skipping identities.  All three are associative and commutative on
// integers: the record is the same bits for any grid shape and arrival order.  info itself is the accumulator: a launch of its own sets
// the identities in-stream, a finishing launch of one thread per instance turns untouched boxes and refused rows into -1.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_gtinfo.h"
#include "../shared/lc_ray_length.h"
#include "../shared/lc_wave_int.h"

#ifndef LC_AMD_GTINFO_SRC_HASH
#define LC_AMD_GTINFO_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_GTINFO_SRC_HASH:" LC_AMD_GTINFO_SRC_HASH;
thread_local std::string g_err;

int fail(int code, const char* msg) {
    g_err = msg;
    return code;
}

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kCols = LC_GTINFO_COLUMNS;
constexpr int kTileH = LC_GTINFO_TILE_H;
constexpr int kGroups = LC_GTINFO_TILE_W / 4;  // groups of four pixels across a tile
constexpr int kSums = 4;                       // all, valid, visib, edge in front of the two boxes

struct Window {
    const float* maps;   // (B,h,w): the instances' renders
    const int* origin;   // (B,2) x0, y0 or null
    const int* scene;    // (B,)
    int B, h, w, S, H, W;
};

struct InfoParams {
    Window win;
    const float* test;   // (S,H,W)
    const float* K;      // (B,3,3)
    float delta, pcx, pcy;
    int* info;           // (B,12)
    unsigned char* mask; // (B,h,w) or null
};

struct ComposeParams {
    Window win;
    unsigned long long* keys;  // (S,H,W): (fp32 bits of z) << 32 | row
    float* depth;              // (S,H,W)
    int* instance;             // (S,H,W) or null
    int* info;                 // (B,)
};

// where row b's window lies; false: refused (none of its maps is read)
struct Place {
    int scene, x0, y0;
};
__device__ __forceinline__ bool place(const Window& p, int b, Place& r) {
    r.scene = p.scene[b];
    r.x0 = p.origin ? p.origin[2 * (size_t)b] : 0;
    r.y0 = p.origin ? p.origin[2 * (size_t)b + 1] : 0;
    if (r.scene < 0 || r.scene >= p.S) return false;
    return r.x0 >= -LC_GTINFO_MAX_ORIGIN && r.x0 <= LC_GTINFO_MAX_ORIGIN && r.y0 >= -LC_GTINFO_MAX_ORIGIN && r.y0 <= LC_GTINFO_MAX_ORIGIN;
}

// the tile of a workgroup: rows [r0, r1) and the groups [g0, g0 + gw) of every row
struct Tile {
    int b, r0, r1, g0, gw;
};
__device__ __forceinline__ Tile tile_of(const Window& p, int tiles_x, int tiles_y) {
    Tile t;
    const int per = tiles_x * tiles_y;
    t.b = blockIdx.x / per;
    const int rest = blockIdx.x - t.b * per;
    const int ty = rest / tiles_x, tx = rest - ty * tiles_x;
    t.r0 = ty * kTileH;
    t.r1 = min(p.h, t.r0 + kTileH);
    const int gpr = (p.w + 6) / 4;  // groups per row: enough for a row that starts three elements behind a 16-byte boundary
    t.g0 = tx * kGroups;
    t.gw = min(kGroups, gpr - t.g0);
    return t;
}

__device__ __forceinline__ void store_mask(unsigned char* row, int x, int w, unsigned bits) {
    if (x >= 0 && x + 4 <= w && (reinterpret_cast<uintptr_t>(row + x) & 3) == 0) {
        *reinterpret_cast<unsigned*>(row + x) = bits;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j >= 0 && x + j < w) row[x + j] = (unsigned char)((bits >> (8 * j)) & 0xff);
    }
}

struct Record {
    int n_all, n_valid, n_visib, n_edge;
    int ox0, oy0, ox1, oy1;  // obj: minima, maxima
    int vx0, vy0, vx1, vy1;  // visib
};

// column j of the record: 0 a sum, 1 a minimum, 2 a maximum
__device__ __host__ __forceinline__ int kind_of(int j) { return j < kSums ? 0 : (((j - kSums) & 3) < 2 ? 1 : 2); }
__device__ __host__ __forceinline__ int identity_of(int j) { return kind_of(j) == 0 ? 0 : (kind_of(j) == 1 ? INT_MAX : INT_MIN); }

__global__ __launch_bounds__(kThreads) void lc_gtinfo_init_kernel(int* info, long long n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) info[i] = identity_of((int)(i % kCols));
}

__global__ __launch_bounds__(kThreads) void lc_gtinfo_reduce_kernel(const InfoParams p, int tiles_x, int tiles_y) {
    __shared__ int s_part[kWaves][kCols];
    const Window& win = p.win;
    const Tile t = tile_of(win, tiles_x, tiles_y);
    const int b = t.b, h = win.h, w = win.w, H = win.H, W = win.W;
    const int items = (t.r1 - t.r0) * t.gw;
    const float* gt = win.maps + (size_t)b * h * w;
    unsigned char* mask = p.mask ? p.mask + (size_t)b * h * w : nullptr;
    Place at;
    if (!place(win, b, at)) {  // the whole workgroup: its part of the mask row is 0, nothing is read
        if (mask)
            for (int i = threadIdx.x; i < items; i += kThreads) {
                const int ry = i / t.gw, y = t.r0 + ry;
                const int x = 4 * (t.g0 + (i - ry * t.gw)) - lead_of(gt + (size_t)y * w);
                if (x < w) store_mask(mask + (size_t)y * w, x, w, 0u);
            }
        return;
    }
    const float* K = p.K + 9 * (size_t)b;
    const double k00 = K[0], k01 = K[1], k02 = K[2], k11 = K[4], k12 = K[5];
    const double pcx = p.pcx, pcy = p.pcy, delta = p.delta;
    const float* test = p.test + (size_t)at.scene * H * W;
    const int test_lead = lead_of(test);

    Record a;
    a.n_all = a.n_valid = a.n_visib = a.n_edge = 0;
    a.ox0 = a.oy0 = a.vx0 = a.vy0 = INT_MAX;
    a.ox1 = a.oy1 = a.vx1 = a.vy1 = INT_MIN;

    for (int i = threadIdx.x; i < items; i += kThreads) {
        const int ry = i / t.gw, y = t.r0 + ry;
        const float* g_row = gt + (size_t)y * w;
        const int x = 4 * (t.g0 + (i - ry * t.gw)) - lead_of(g_row);
        if (x >= w) continue;
        float fg[4];
        load_group(g_row, x, w, fg);
        unsigned bits = 0;
        if (fg[0] > 0.0f || fg[1] > 0.0f || fg[2] > 0.0f || fg[3] > 0.0f) {
            const int Y = y + at.y0, X = x + at.x0;
            const bool row_in = Y >= 0 && Y < H;
            float ft[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            double yy = 0.0, kY = 0.0;
            if (row_in) {
                const long long off = (long long)Y * W + X;  // of the group's first pixel in the scene's map; used only where that lies inside
                if (x >= 0 && x + 4 <= w && X >= 0 && X + 4 <= W && ((test_lead + off) & 3) == 0) {
                    const float4 v = *reinterpret_cast<const float4*>(test + off);
                    ft[0] = v.x; ft[1] = v.y; ft[2] = v.z; ft[3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j >= 0 && x + j < w && X + j >= 0 && X + j < W) ft[j] = test[off + j];
                }
                const RayRow r = ray_row(Y, pcy, k12, k11, k01);
                yy = r.yy, kY = r.kY;
            }
            const bool row_edge = y == 0 || y == h - 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(fg[j] > 0.0f)) continue;  // a pixel outside the row holds 0
                const int xj = x + j, Xj = X + j;
                a.n_all += 1;
                a.n_edge += (row_edge || xj == 0 || xj == w - 1) ? 1 : 0;
                a.ox0 = min(a.ox0, Xj); a.ox1 = max(a.ox1, Xj);
                a.oy0 = min(a.oy0, Y); a.oy1 = max(a.oy1, Y);
                if (!(row_in && Xj >= 0 && Xj < W)) continue;
                const bool missing = !(ft[j] > 0.0f);
                bool vis = missing;
                if (!missing) {
                    a.n_valid += 1;
                    const double n = ray_length(Xj, pcx, k02, k00, kY, yy);
                    const double dist_g = (double)fg[j] * n;
                    const double dist_t = (double)ft[j] * n;
                    const double over = dist_g - dist_t;
                    vis = over <= delta;
                }
                if (vis) {
                    a.n_visib += 1;
                    a.vx0 = min(a.vx0, Xj); a.vx1 = max(a.vx1, Xj);
                    a.vy0 = min(a.vy0, Y); a.vy1 = max(a.vy1, Y);
                    bits |= 1u << (8 * j);
                }
            }
        }
        if (mask) store_mask(mask + (size_t)y * w, x, w, bits);
    }

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    // a wavefront that saw no hit (most of a mostly empty window) hands in identities without the twelve butterflies: every other value
    // is a part of n_all.  The test is uniform over the wavefront; the barrier is not inside it.
    if (__any(a.n_all != 0)) {
        const int v0 = wave_sum(a.n_all), v1 = wave_sum(a.n_valid), v2 = wave_sum(a.n_visib), v3 = wave_sum(a.n_edge);
        const int v4 = wave_min(a.ox0), v5 = wave_min(a.oy0), v6 = wave_max(a.ox1), v7 = wave_max(a.oy1);
        const int v8 = wave_min(a.vx0), v9 = wave_min(a.vy0), v10 = wave_max(a.vx1), v11 = wave_max(a.vy1);
        if (lane == 0) {
            int* s = s_part[wave];
            s[0] = v0; s[1] = v1; s[2] = v2; s[3] = v3; s[4] = v4; s[5] = v5; s[6] = v6; s[7] = v7; s[8] = v8; s[9] = v9; s[10] = v10; s[11] = v11;
        }
    } else if (lane < kCols) {
        s_part[wave][lane] = identity_of(lane);
    }
    __syncthreads();
    if (threadIdx.x < kCols) {
        const int j = threadIdx.x, kind = kind_of(j);
        int v = s_part[0][j];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) {
            const int o = s_part[wv][j];
            v = kind == 0 ? v + o : (kind == 1 ? min(v, o) : max(v, o));
        }
        int* out = p.info + (size_t)b * kCols + j;
        if (v != identity_of(j)) {
            if (kind == 0) atomicAdd(out, v);
            else if (kind == 1) atomicMin(out, v);
            else atomicMax(out, v);
        }
    }
}

// one thread per instance: untouched boxes and refused rows become -1
__global__ __launch_bounds__(kThreads) void lc_gtinfo_finish_kernel(const InfoParams p) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= p.win.B) return;
    int* rec = p.info + (size_t)b * kCols;
    Place at;
    if (!place(p.win, b, at)) {
        for (int j = 0; j < kCols; ++j) rec[j] = -1;
        return;
    }
    if (rec[0] == 0)
        for (int j = 4; j < 8; ++j) rec[j] = -1;
    if (rec[2] == 0)
        for (int j = 8; j < 12; ++j) rec[j] = -1;
}

// fills the key map with the largest key (nothing hit) and says which rows are skipped
__global__ __launch_bounds__(kThreads) void lc_compose_init_kernel(const ComposeParams p, long long n_pix) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_pix) p.keys[i] = ~0ull;
    if (i < p.win.B) {
        Place at;
        p.info[i] = place(p.win, (int)i, at) ? 0 : -1;
    }
}

__global__ __launch_bounds__(kThreads) void lc_compose_min_kernel(const ComposeParams p, int tiles_x, int tiles_y) {
    const Window& win = p.win;
    const Tile t = tile_of(win, tiles_x, tiles_y);
    const int b = t.b, h = win.h, w = win.w, H = win.H, W = win.W;
    Place at;
    if (!place(win, b, at)) return;  // the whole workgroup
    const float* maps = win.maps + (size_t)b * h * w;
    unsigned long long* keys = p.keys + (size_t)at.scene * H * W;
    const int items = (t.r1 - t.r0) * t.gw;
    for (int i = threadIdx.x; i < items; i += kThreads) {
        const int ry = i / t.gw, y = t.r0 + ry;
        const int Y = y + at.y0;
        if (Y < 0 || Y >= H) continue;  // a window row outside the frame is not read
        const float* row = maps + (size_t)y * w;
        const int x = 4 * (t.g0 + (i - ry * t.gw)) - lead_of(row);
        if (x >= w) continue;
        float f[4];
        load_group(row, x, w, f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int Xj = x + j + at.x0;
            if (f[j] > 0.0f && f[j] < __builtin_inff() && Xj >= 0 && Xj < W) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(f[j]) << 32) | (unsigned)b;
                atomicMin(keys + (size_t)Y * W + Xj, key);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void lc_compose_finish_kernel(const ComposeParams p, long long n_pix) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_pix) return;
    const unsigned long long key = p.keys[i];
    const bool hit = key != ~0ull;
    p.depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    if (p.instance) p.instance[i] = hit ? (int)(unsigned)(key & 0xffffffffull) : -1;
}

long long tiles_x_of(int w) { return (((long long)w + 6) / 4 + kGroups - 1) / kGroups; }
long long tiles_y_of(int h) { return ((long long)h + kTileH - 1) / kTileH; }
unsigned blocks_of(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

int launch_info(const InfoParams& p, hipStream_t stream) {
    const Window& win = p.win;
    const long long n = (long long)win.B * kCols;
    hipLaunchKernelGGL(lc_gtinfo_init_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, stream, p.info, n);
    if (hipGetLastError() != hipSuccess) return 2;
    const int tx = (int)tiles_x_of(win.w), ty = (int)tiles_y_of(win.h);
    hipLaunchKernelGGL(lc_gtinfo_reduce_kernel, dim3((unsigned)((long long)win.B * tx * ty)), dim3(kThreads), 0, stream, p, tx, ty);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(lc_gtinfo_finish_kernel, dim3(blocks_of(win.B)), dim3(kThreads), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_compose(const ComposeParams& p, hipStream_t stream) {
    const Window& win = p.win;
    const long long n_pix = (long long)win.S * win.H * win.W;
    const long long n_init = n_pix > win.B ? n_pix : win.B;
    hipLaunchKernelGGL(lc_compose_init_kernel, dim3(blocks_of(n_init)), dim3(kThreads), 0, stream, p, n_pix);
    if (hipGetLastError() != hipSuccess) return 2;
    if (win.B > 0) {
        const int tx = (int)tiles_x_of(win.w), ty = (int)tiles_y_of(win.h);
        hipLaunchKernelGGL(lc_compose_min_kernel, dim3((unsigned)((long long)win.B * tx * ty)), dim3(kThreads), 0, stream, p, tx, ty);
        if (hipGetLastError() != hipSuccess) return 2;
    }
    hipLaunchKernelGGL(lc_compose_finish_kernel, dim3(blocks_of(n_pix)), dim3(kThreads), 0, stream, p, n_pix);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

bool misaligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) != 0; }

// the size rules both entry points share; null: in order.  `what` names the entry point in front of every message
const char* window_error(const Window& p, bool batch_needed, std::string& buf, const char* what) {
    auto say = [&](const char* msg) {
        buf = std::string(what) + ": " + msg;
        return buf.c_str();
    };
    if (p.B < 0 || p.h < 0 || p.w < 0 || p.S < 0 || p.H < 0 || p.W < 0) return say("a negative size");
    if (p.B == 0 && batch_needed) return nullptr;
    if (p.S < 1) return say("at least one scene (S)");
    if (p.H < 1 || p.W < 1 || p.H > LC_GTINFO_MAX_FRAME || p.W > LC_GTINFO_MAX_FRAME) return say("frame sizes of 1 to 16384");
    if ((long long)p.S * p.H * p.W >= (1ll << 31) * kThreads) return say("more than 2^39 frame pixels");
    if (p.B == 0) return nullptr;
    if (p.h < 1 || p.w < 1 || p.h > LC_GTINFO_MAX_WINDOW || p.w > LC_GTINFO_MAX_WINDOW) return say("window sizes of 1 to 49152");
    if ((long long)p.h * p.w >= (1ll << 31)) return say("a window of 2^31 pixels or more (the counts are int32)");
    if (!p.origin && (p.h != p.H || p.w != p.W)) return say("without origin_xy the maps have the frame's size");
    if ((long long)p.B * tiles_x_of(p.w) * tiles_y_of(p.h) >= (1ll << 31) || (long long)p.B * kCols >= (1ll << 31)) return say("more than 2^31 tiles or record entries");
    return nullptr;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_gtinfo_version(void) { return LC_AMD_GTINFO_VERSION; }
const char* lc_amd_gtinfo_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_GTINFO_SRC_HASH:") - 1; }
const char* lc_amd_gtinfo_last_error(void) { return lc::g_err.c_str(); }

int lc_gtinfo_f32(const float* depth_gt, const int* origin_xy, const float* depth_test, const int* scene_index, const float* K, int B, int h,
                  int w, int S, int H, int W, float pcx, float pcy, float delta, int* info, unsigned char* mask_visib, void* stream) {
    lc::InfoParams p{};
    p.win = lc::Window{depth_gt, origin_xy, scene_index, B, h, w, S, H, W};
    p.test = depth_test; p.K = K; p.delta = delta; p.pcx = pcx; p.pcy = pcy; p.info = info; p.mask = mask_visib;
    std::string buf;
    if (const char* e = lc::window_error(p.win, true, buf, "lc_gtinfo_f32")) return lc::fail(1, e);
    if (B == 0) return 0;
    if (!depth_gt || !depth_test || !scene_index || !K || !info) return lc::fail(1, "lc_gtinfo_f32: a null argument");
    if (lc::misaligned4(depth_gt) || lc::misaligned4(origin_xy) || lc::misaligned4(depth_test) || lc::misaligned4(scene_index) || lc::misaligned4(K) ||
        lc::misaligned4(info))
        return lc::fail(1, "lc_gtinfo_f32: every pointer but mask_visib must be 4-byte aligned");
    return lc::launch_info(p, static_cast<hipStream_t>(stream)) ? lc::fail(11, "gtinfo launch failed") : 0;
}

size_t lc_scene_compose_workspace_bytes(int S, int H, int W) {
    if (S < 1 || H < 1 || W < 1) return 0;
    return (size_t)S * (size_t)H * (size_t)W * sizeof(unsigned long long);
}

int lc_scene_compose_f32(const float* depth_inst, const int* origin_xy, const int* scene_index, int B, int h, int w, int S, int H, int W,
                         float* depth, int* instance, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    lc::ComposeParams p{};
    p.win = lc::Window{depth_inst, origin_xy, scene_index, B, h, w, S, H, W};
    p.keys = static_cast<unsigned long long*>(workspace); p.depth = depth; p.instance = instance; p.info = info;
    std::string buf;
    if (const char* e = lc::window_error(p.win, false, buf, "lc_scene_compose_f32")) return lc::fail(1, e);
    if (!depth || !workspace || (B > 0 && (!depth_inst || !scene_index || !info))) return lc::fail(1, "lc_scene_compose_f32: a null argument");
    if (lc::misaligned4(depth_inst) || lc::misaligned4(origin_xy) || lc::misaligned4(scene_index) || lc::misaligned4(depth) || lc::misaligned4(instance) ||
        lc::misaligned4(info))
        return lc::fail(1, "lc_scene_compose_f32: every pointer must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return lc::fail(1, "lc_scene_compose_f32: the workspace must be 8-byte aligned");
    if (workspace_bytes < lc_scene_compose_workspace_bytes(S, H, W)) return lc::fail(1, "lc_scene_compose_f32: the workspace is smaller than lc_scene_compose_workspace_bytes(S,H,W)");
    return lc::launch_compose(p, static_cast<hipStream_t>(stream)) ? lc::fail(11, "scene compose launch failed") : 0;
}

}  // extern "C"
#pragma GCC visibility pop
