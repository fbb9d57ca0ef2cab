// Depth-only rasteriser, two launches (liblc_amd_render.so, C ABI and the exact definition of the result in include/lc_amd_render.h).
//
// What the reference renders offline with an EGL/OpenGL renderer (tools/gen_z.py:153) and reads back as z_crop / homo_z
// (dataset.py:287-311): the camera-space depth of a mesh under a pose, here with coverage that is exact on a 2^-8 px grid.
//
//   setup   one thread per (row, face): gathers the three vertices, transforms and projects them in fp64, snaps the screen
//           coordinates to 2^-8 px and writes a 64-byte record (1/z per vertex, snapped coordinates, the box of covered pixel
//           indices clamped to the map; an empty box for dropped and zero-area faces).
//   raster  one workgroup of four waves per (row, 32x32 tile): a 64-bit key per pixel in LDS (8 KiB), all ones at the start.  The
//           waves stride over the row's records, a lane per face; a lane whose box meets the tile in at most 64 samples walks them
//           itself, larger intersections are taken by the whole wave, one face at a time.  A covered sample is one LDS atomicMin of
//           (fp32 bits of z) << 32 | face.  One barrier, then the lanes resolve the keys to depth / face / mask / homo_z with
//           contiguous stores.  No global atomics and no waiting between workgroups: the minimum of the keys is the same for every
//           order of evaluation.
//
// Bounds: vertex indices are checked against the mesh's vertex count, table entries against the array sizes and mesh_index against
// the table, all on the device, so that no input value can make a launch read or write outside its arrays.
//
// Self-contained on purpose: the library's source hash covers this directory and its header only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_render.h"

#ifndef LC_AMD_RENDER_SRC_HASH
#define LC_AMD_RENDER_SRC_HASH "unrecorded"
#endif

namespace {

const char kSrcHash[] = "LC_AMD_RENDER_SRC_HASH:" LC_AMD_RENDER_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;
constexpr int kTile = 32;                 // pixels per tile edge
constexpr int kTilePix = kTile * kTile;
constexpr int kSub = 256;                 // grid units per pixel (2^-8 px)
constexpr double kMaxSnap = 33554432.0;   // 2^25 grid units: edge functions stay below 2^53
constexpr int kCoop = 64;                 // box-in-tile samples above which the whole wave takes the face
constexpr unsigned long long kEmpty = ~0ull;

constexpr int kDropped = 1;  // record flags

struct alignas(16) FaceRec {
    double iz[3];   // 1/z of the vertices
    int sx[3];      // snapped screen coordinates, grid units
    int sy[3];
    short x0, x1, y0, y1;  // pixel indices whose samples lie inside the vertices' bounding box, clamped to the map; x0 > x1 = empty
    int flags;
    int pad;
};
static_assert(sizeof(FaceRec) == LC_RENDER_RECORD_BYTES, "record layout");

struct Params {
    const float* verts;
    const int* faces;
    const int* table;
    const int* mesh_index;
    const float* R;
    const float* t;
    const float* K;
    const float* pix2k;
    FaceRec* rec;
    float* depth;
    int* face;
    unsigned char* mask;
    float* homo;
    int* info;
    int n_meshes, total_verts, total_faces, max_faces;
    int B, H, W, tiles_x, tiles_y;
    int cxi, cyi;  // the sample offset in grid units
    float near, far, cx, cy;
};

struct MeshRef {
    int vert_off, n_vert, face_off, n_face;
    bool ok;
};

// The mesh of row b, or an empty one (ok = false) for anything that would reach outside the arrays.
__device__ __forceinline__ MeshRef mesh_of_row(const Params& p, int b) {
    MeshRef m{0, 0, 0, 0, false};
    const int mi = p.mesh_index[b];
    if (mi < 0 || mi >= p.n_meshes) return m;
    const int* tp = p.table + 4 * (size_t)mi;
    const int4 e = make_int4(tp[0], tp[1], tp[2], tp[3]);
    if (e.x < 0 || e.y < 0 || e.z < 0 || e.w < 0 || e.w > p.max_faces) return m;
    if ((long long)e.x + e.y > p.total_verts || (long long)e.z + e.w > p.total_faces) return m;
    return MeshRef{e.x, e.y, e.z, e.w, true};
}

__device__ __forceinline__ int floor_div(int a, int b) {  // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void lc_render_setup_kernel(const Params p) {
    const int b = blockIdx.y;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    const MeshRef m = mesh_of_row(p, b);
    if (f >= m.n_face) return;
    FaceRec r;
    r.x0 = 1; r.x1 = 0; r.y0 = 1; r.y1 = 0;
    r.flags = 0;
    r.pad = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.iz[k] = 0.0; r.sx[k] = 0; r.sy[k] = 0; }
    const int* fp = p.faces + 3 * ((size_t)m.face_off + f);
    const int vi[3] = {fp[0], fp[1], fp[2]};
    bool valid = true, dropped = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) valid = valid && vi[k] >= 0 && vi[k] < m.n_vert;
    if (valid) {
        double Rm[9], tv[3], Km[6];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rm[i] = p.R[9 * (size_t)b + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tv[i] = p.t[3 * (size_t)b + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) Km[i] = p.K[9 * (size_t)b + i];
        const double near = p.near;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* vp = p.verts + 3 * ((size_t)m.vert_off + vi[k]);
            const double X = vp[0], Y = vp[1], Z = vp[2];
            const double xc = Rm[0] * X + Rm[1] * Y + Rm[2] * Z + tv[0];
            const double yc = Rm[3] * X + Rm[4] * Y + Rm[5] * Z + tv[1];
            const double zc = Rm[6] * X + Rm[7] * Y + Rm[8] * Z + tv[2];
            if (!(zc > near)) { dropped = true; continue; }
            const double u = (Km[0] * xc + Km[1] * yc + Km[2] * zc) / zc;
            const double v = (Km[3] * xc + Km[4] * yc + Km[5] * zc) / zc;
            const double su = rint(u * kSub), sv = rint(v * kSub);  // round-half-even
            if (!(fabs(su) <= kMaxSnap) || !(fabs(sv) <= kMaxSnap)) { dropped = true; continue; }
            r.sx[k] = (int)su;
            r.sy[k] = (int)sv;
            r.iz[k] = 1.0 / zc;
        }
        if (dropped) {
            r.flags = kDropped;
        } else {
            const long long area = (long long)(r.sx[1] - r.sx[0]) * (r.sy[2] - r.sy[0]) - (long long)(r.sy[1] - r.sy[0]) * (r.sx[2] - r.sx[0]);
            if (area != 0) {
                const int mnx = min(r.sx[0], min(r.sx[1], r.sx[2])), mxx = max(r.sx[0], max(r.sx[1], r.sx[2]));
                const int mny = min(r.sy[0], min(r.sy[1], r.sy[2])), mxy = max(r.sy[0], max(r.sy[1], r.sy[2]));
                // pixel x has its sample at kSub x + cxi: inside [mnx, mxx]
                const int x0 = max(-floor_div(-(mnx - p.cxi), kSub), 0), x1 = min(floor_div(mxx - p.cxi, kSub), p.W - 1);
                const int y0 = max(-floor_div(-(mny - p.cyi), kSub), 0), y1 = min(floor_div(mxy - p.cyi, kSub), p.H - 1);
                if (x0 <= x1 && y0 <= y1) {
                    r.x0 = (short)x0; r.x1 = (short)x1; r.y0 = (short)y0; r.y1 = (short)y1;
                }
            }
        }
    }
    p.rec[(size_t)b * p.max_faces + f] = r;
}

struct FaceRegs {  // what a sample test needs, in registers
    double iz0, iz1, iz2;
    int ax, ay, bx, by, cx, cy;
};

// One sample of one face: an LDS atomicMin of the key where the sample is covered and near < z < far.
__device__ __forceinline__ void sample(const FaceRegs& r, unsigned face, int x, int y, int tx0, int ty0, const Params& p, unsigned long long* keys) {
    const double px = (double)(x * kSub + p.cxi), py = (double)(y * kSub + p.cyi);
    const double ax = r.ax, ay = r.ay, bx = r.bx, by = r.by, cx = r.cx, cy = r.cy;
    // edge functions of integer-valued doubles: every product and difference is exact
    const double w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx);  // weight of vertex a
    const double w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);  // of b
    const double w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);  // of c
    const bool in = (w0 >= 0 && w1 >= 0 && w2 >= 0) || (w0 <= 0 && w1 <= 0 && w2 <= 0);
    if (!in) return;
    const double area = w0 + w1 + w2;
    const double z = area / (w0 * r.iz0 + w1 * r.iz1 + w2 * r.iz2);
    const float zf = (float)z;
    if (!(zf > p.near && zf < p.far)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | face;
    atomicMin(&keys[(y - ty0) * kTile + (x - tx0)], key);
}

__global__ __launch_bounds__(kThreads) void lc_render_raster_kernel(const Params p) {
    __shared__ unsigned long long keys[kTilePix];
    __shared__ int dropped_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = p.tiles_x * p.tiles_y;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tx0 = (tile % p.tiles_x) * kTile, ty0 = (tile / p.tiles_x) * kTile;
    const int tx1 = min(tx0 + kTile, p.W) - 1, ty1 = min(ty0 + kTile, p.H) - 1;
    for (int i = tid; i < kTilePix; i += kThreads) keys[i] = kEmpty;
    if (tid == 0) dropped_total = 0;
    __syncthreads();

    const MeshRef m = mesh_of_row(p, b);
    const FaceRec* recs = p.rec + (size_t)b * p.max_faces;
    int dropped = 0;
    for (int base = wave * kWave; base < m.n_face; base += kThreads) {  // wave-uniform trip count
        const int f = base + lane;
        FaceRegs r{};
        int ix0 = 1, ix1 = 0, iy0 = 1, iy1 = 0;
        if (f < m.n_face) {
            const int4* q = reinterpret_cast<const int4*>(recs + f);
            const int4 q3 = q[3];  // x0 x1 | y0 y1 | flags | pad
            const short bx0 = (short)(q3.x & 0xffff), bx1 = (short)((unsigned)q3.x >> 16);
            const short by0 = (short)(q3.y & 0xffff), by1 = (short)((unsigned)q3.y >> 16);
            if (tile == 0) dropped += q3.z & kDropped;
            ix0 = max((int)bx0, tx0); ix1 = min((int)bx1, tx1);
            iy0 = max((int)by0, ty0); iy1 = min((int)by1, ty1);
            if (ix0 <= ix1 && iy0 <= iy1) {
                const int4 q0 = q[0], q1 = q[1], q2 = q[2];
                r.iz0 = __hiloint2double(q0.y, q0.x);
                r.iz1 = __hiloint2double(q0.w, q0.z);
                r.iz2 = __hiloint2double(q1.y, q1.x);
                r.ax = q1.z; r.bx = q1.w; r.cx = q2.x;
                r.ay = q2.y; r.by = q2.z; r.cy = q2.w;
            }
        }
        const int bw = ix1 - ix0 + 1, bh = iy1 - iy0 + 1;
        const int n = (bw > 0 && bh > 0) ? bw * bh : 0;
        const bool big = n > kCoop;
        if (n > 0 && !big) {
            for (int y = iy0; y <= iy1; ++y)
                for (int x = ix0; x <= ix1; ++x) sample(r, (unsigned)f, x, y, tx0, ty0, p, keys);
        }
        unsigned long long todo = __ballot(big ? 1 : 0);
        while (todo) {  // the whole wave on one large face at a time
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            FaceRegs s;
            s.iz0 = __hiloint2double(__shfl(__double2hiint(r.iz0), src, kWave), __shfl(__double2loint(r.iz0), src, kWave));
            s.iz1 = __hiloint2double(__shfl(__double2hiint(r.iz1), src, kWave), __shfl(__double2loint(r.iz1), src, kWave));
            s.iz2 = __hiloint2double(__shfl(__double2hiint(r.iz2), src, kWave), __shfl(__double2loint(r.iz2), src, kWave));
            s.ax = __shfl(r.ax, src, kWave); s.ay = __shfl(r.ay, src, kWave);
            s.bx = __shfl(r.bx, src, kWave); s.by = __shfl(r.by, src, kWave);
            s.cx = __shfl(r.cx, src, kWave); s.cy = __shfl(r.cy, src, kWave);
            const int sx0 = __shfl(ix0, src, kWave), sy0 = __shfl(iy0, src, kWave), sw = __shfl(bw, src, kWave), sn = __shfl(n, src, kWave);
            const unsigned sf = (unsigned)(base + src);
            for (int i = lane; i < sn; i += kWave) {
                const int dy = i / sw, dx = i - dy * sw;
                sample(s, sf, sx0 + dx, sy0 + dy, tx0, ty0, p, keys);
            }
        }
    }
    if (tile == 0 && dropped) atomicAdd(&dropped_total, dropped);
    __syncthreads();

    if (tile == 0 && tid == 0) p.info[b] = m.ok ? dropped_total : -1;
    const int tw = tx1 - tx0 + 1, th = ty1 - ty0 + 1;
    const size_t row0 = (size_t)b * p.H;
    for (int i = tid; i < kTilePix; i += kThreads) {  // a wave stores two 32-pixel map rows
        const int ly = i / kTile, lx = i - ly * kTile;
        if (lx >= tw || ly >= th) continue;
        const unsigned long long key = keys[i];
        const bool hit = key != kEmpty;
        const size_t o = (row0 + ty0 + ly) * p.W + tx0 + lx;
        p.depth[o] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
        if (p.face) p.face[o] = hit ? (int)(unsigned)(key & 0xffffffffu) : -1;
        if (p.mask) p.mask[o] = hit ? 1 : 0;
    }
    if (p.homo) {
        double M[6] = {1.0, 0.0, (double)p.cx, 0.0, 1.0, (double)p.cy};
        if (p.pix2k) {
#pragma unroll
            for (int k = 0; k < 6; ++k) M[k] = p.pix2k[6 * (size_t)b + k];
        }
        const int row_floats = 3 * tw;  // contiguous floats of one map row inside the tile
        for (int i = tid; i < th * row_floats; i += kThreads) {
            const int ly = i / row_floats, j = i - ly * row_floats, lx = j / 3, c = j - 3 * lx;
            const unsigned long long key = keys[ly * kTile + lx];
            float v = 0.f;
            if (key != kEmpty) {
                const float zf = __uint_as_float((unsigned)(key >> 32));
                const double x = tx0 + lx, y = ty0 + ly;
                const double pc = c == 0 ? M[0] * x + M[1] * y + M[2] : M[3] * x + M[4] * y + M[5];
                v = c == 2 ? zf : (float)(pc * (double)zf);  // one fp32 rounding of the product
            }
            p.homo[((row0 + ty0 + ly) * p.W + tx0) * 3 + j] = v;
        }
    }
}

bool on_grid(float c, int* units) {
    const double s = (double)c * kSub;
    if (!(std::fabs(s) <= 64.0 * kSub) || s != std::nearbyint(s)) return false;
    *units = (int)s;
    return true;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_render_version(void) { return LC_AMD_RENDER_VERSION; }
const char* lc_amd_render_source_hash(void) { return kSrcHash + sizeof("LC_AMD_RENDER_SRC_HASH:") - 1; }
const char* lc_amd_render_last_error(void) { return g_err.c_str(); }

size_t lc_render_workspace_bytes(int B, int max_faces) {
    if (B <= 0 || max_faces <= 0) return 0;
    return (size_t)B * (size_t)max_faces * sizeof(FaceRec);
}

int lc_render_depth_f32(const float* verts, const int* faces, const int* mesh_table, const int* mesh_index, int n_meshes, int total_verts,
                        int total_faces, int max_faces, const float* R, const float* t, const float* K, const float* pix2k, int B, int H,
                        int W, float near, float far, float cx, float cy, float* depth, int* face, unsigned char* mask, float* homo_z,
                        int* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0) return fail(1, "lc_render_depth_f32: B < 0");
    if (B == 0) return 0;
    if (H < 1 || W < 1 || H > LC_RENDER_MAX_SIZE || W > LC_RENDER_MAX_SIZE)
        return fail(2, "lc_render_depth_f32: H and W must be in [1, " + std::to_string(LC_RENDER_MAX_SIZE) + "], got " + std::to_string(H) + " x " + std::to_string(W));
    if (!(near < far)) return fail(3, "lc_render_depth_f32: near < far is required");
    int cxi = 0, cyi = 0;
    if (!on_grid(cx, &cxi) || !on_grid(cy, &cyi)) return fail(4, "lc_render_depth_f32: the sample offsets must be multiples of 2^-8 in [-64, 64]");
    if (n_meshes < 0 || total_verts < 0 || total_faces < 0 || max_faces < 0) return fail(5, "lc_render_depth_f32: negative mesh sizes");
    if (!mesh_table || !mesh_index || !R || !t || !K) return fail(6, "lc_render_depth_f32: mesh_table, mesh_index, R, t and K must not be NULL");
    if (max_faces > 0 && (!verts || !faces)) return fail(6, "lc_render_depth_f32: verts and faces must not be NULL");
    if (!depth || !info) return fail(7, "lc_render_depth_f32: depth and info must not be NULL");
    const size_t need = lc_render_workspace_bytes(B, max_faces);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(8, "lc_render_depth_f32: workspace must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const long long blocks = (long long)tiles_x * tiles_y * B;
    if (blocks > 0x7fffffffLL || B > 65535) return fail(9, "lc_render_depth_f32: too many tiles or rows for one launch");
    const Params p{verts, faces, mesh_table, mesh_index, R, t, K, pix2k, static_cast<FaceRec*>(workspace), depth, face, mask, homo_z, info,
                   n_meshes, total_verts, total_faces, max_faces, B, H, W, tiles_x, tiles_y, cxi, cyi, near, far, cx, cy};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (max_faces > 0) hipLaunchKernelGGL(lc_render_setup_kernel, dim3((max_faces + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, p);
    hipLaunchKernelGGL(lc_render_raster_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(10, std::string("lc_render_depth_f32: launch: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
