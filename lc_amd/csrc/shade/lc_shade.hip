// The shading pass behind the depth rasteriser: a vertex-coloured mesh under a Phong model, written as uint8 bytes over whatever the frame
// held (liblc_amd_shade.so; C ABI and the exact definition of every byte in include/lc_amd_shade.h).
//
// What the reference draws with its vendored OpenGL renderer (tools/lib/meshrenderer/meshrenderer_phong.py:125-165,
// shader/depth_shader_phong.{vs,frag}).  Two kernels around one pixel function:
//
//   lc_shade_instances_kernel  one workgroup of 256 threads per (row, 32 x 8 tile of the row's map), one thread per pixel.  The row is the
//                              workgroup's, so its mesh entry, R, t, K, light and phong are uniform loads.  A thread loads its face index and
//                              leaves at once where it is -1: most pixels.
//   lc_shade_scene_kernel      the same tiles over the frames of S scenes.  A thread loads its pixel's instance, leaves where it is -1, and
//                              shades with THAT row's tables at the row's window pixel: the row differs between lanes, so its loads are
//                              per lane.
//   shade_pixel                the arithmetic of one hit pixel for both: three vertex gathers (27 bytes each), about 150 fp64 operations
//                              with three roots and a dozen quotients, three byte stores.
//
// The contract rounds every fp64 operation on its own and the library is built with -ffp-contract=on, which fuses a product and a sum only
// inside one expression.  So every operation below is a statement of its own (as shared/lc_ray_length.h has it): joining two of them changes
// a weight in its last bit and, through the final rint, a byte.  The snapped projection restates the rasteriser's few lines
// (render/lc_render.hip, face setup); tests/test_gpu_shade.py pins the two to each other end to end.
//
// Bounds: a row's mesh index is checked against n_meshes before the table is read, the table entry against the arrays' counts before a
// face is read, the face index against n_face and each vertex index against n_vert before a vertex is read; in the scene form the instance
// is checked against B before anything of the row is read and the window pixel against (h,w) before the face map is.  A thread writes the
// three bytes of its own pixel and nothing else but its row's info word, into which every writer stores the same value.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_shade.h"

#ifndef LC_AMD_SHADE_SRC_HASH
#define LC_AMD_SHADE_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_SHADE_SRC_HASH:" LC_AMD_SHADE_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;  // kTileW * kTileH == kThreads; a wave covers two rows of 32 pixels
constexpr double kSub = 256.0;          // grid units per pixel (2^-8 px), as the rasteriser has it

struct Params {
    const float* verts;
    const float* normals;
    const unsigned char* colors;
    const int* faces;
    const int* table;
    const int* mesh_index;
    const int* scene_index;
    const float* R;
    const float* t;
    const float* K;
    const float* light;
    const float* phong;
    const int* face;
    const int* origin;    // NULL: every window lies at (0, 0)
    const int* instance;
    unsigned char* out;   // (B,h,w,3) or the frames (S,H,W,3)
    int* info;
    int n_meshes, total_verts, total_faces, B, h, w, S, H, W;
    int cxi, cyi;         // the sample offset in grid units
    int tiles_x, tiles;   // tiles per map row, and per map
};

struct Mesh {
    int vert_off, n_vert, face_off, n_face;
    bool ok;
};

// the row's table entry, refused where the index or the entry reaches outside what the caller declared
__device__ __forceinline__ Mesh mesh_of(const Params& p, int b) {
    Mesh m{0, 0, 0, 0, false};
    const int mi = p.mesh_index[b];
    if (mi < 0 || mi >= p.n_meshes) return m;
    const int* e = p.table + 4 * (size_t)mi;
    m.vert_off = e[0]; m.n_vert = e[1]; m.face_off = e[2]; m.n_face = e[3];
    m.ok = m.vert_off >= 0 && m.n_vert >= 0 && m.face_off >= 0 && m.n_face >= 0 && (long long)m.vert_off + m.n_vert <= p.total_verts &&
           (long long)m.face_off + m.n_face <= p.total_faces;
    return m;
}

// (a0 b0 + a1 b1) + a2 b2, five operations
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    const double p0 = a0 * b0;
    const double p1 = a1 * b1;
    const double p2 = a2 * b2;
    double s = p0 + p1;
    s = s + p2;
    return s;
}

// x / |x| per component, zero where the length is zero
__device__ __forceinline__ void unit3(double x, double y, double z, double (&u)[3]) {
    const double len = sqrt(dot3(x, y, z, x, y, z));
    const bool zero = len == 0.0;
    const double ux = x / len;
    const double uy = y / len;
    const double uz = z / len;
    u[0] = zero ? 0.0 : ux;
    u[1] = zero ? 0.0 : uy;
    u[2] = zero ? 0.0 : uz;
}

// one edge function (c - b) x (p - b) of integer-valued doubles
__device__ __forceinline__ double edge(double bx, double by, double cx, double cy, double px, double py) {
    const double ex = cx - bx;
    const double ey = cy - by;
    const double dx = px - bx;
    const double dy = py - by;
    const double m0 = ex * dy;
    const double m1 = ey * dx;
    return m0 - m1;
}

__device__ __forceinline__ unsigned char finish(double I, double c) {
    const double v = I * c;
    return v >= 255.0 ? (unsigned char)255 : v > 0.0 ? (unsigned char)(int)rint(v) : (unsigned char)0;  // NaN: 0
}

// The hit pixel of row b with face f at window pixel (x, y): steps 1 to 8 of the header.  false: refused, nothing written.
__device__ __forceinline__ bool shade_pixel(const Params& p, int b, const Mesh& m, int f, int x, int y, unsigned char* dst) {
    if (f < 0 || f >= m.n_face) return false;
    const int* tri = p.faces + 3 * ((size_t)m.face_off + (size_t)f);
    const int idx[3] = {tri[0], tri[1], tri[2]};
    if ((unsigned)idx[0] >= (unsigned)m.n_vert || (unsigned)idx[1] >= (unsigned)m.n_vert || (unsigned)idx[2] >= (unsigned)m.n_vert) return false;

    const float* Rf = p.R + 9 * (size_t)b;
    const float* tf = p.t + 3 * (size_t)b;
    const float* Kf = p.K + 9 * (size_t)b;
    double Rm[9], tv[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rm[i] = (double)Rf[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tv[i] = (double)tf[i];
    const double k00 = (double)Kf[0], k01 = (double)Kf[1], k02 = (double)Kf[2], k10 = (double)Kf[3], k11 = (double)Kf[4], k12 = (double)Kf[5];

    double Xc[3][3], sx[3], sy[3], nrm[3][3], col[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t v = 3 * ((size_t)m.vert_off + (size_t)idx[k]);
        const double X = (double)p.verts[v], Y = (double)p.verts[v + 1], Z = (double)p.verts[v + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double s = dot3(Rm[3 * r], Rm[3 * r + 1], Rm[3 * r + 2], X, Y, Z);
            Xc[k][r] = s + tv[r];
        }
        const double zc = Xc[k][2];
        const double nu = dot3(k00, k01, k02, Xc[k][0], Xc[k][1], zc);
        const double nv = dot3(k10, k11, k12, Xc[k][0], Xc[k][1], zc);
        const double u = nu / zc;
        const double vv = nv / zc;
        const double us = u * kSub;
        const double vs = vv * kSub;
        sx[k] = rint(us);  // round-half-even
        sy[k] = rint(vs);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nrm[k][c] = (double)p.normals[v + c];
            col[k][c] = (double)p.colors[v + c];
        }
    }

    const double px = (double)(x * 256 + p.cxi), py = (double)(y * 256 + p.cyi);
    const double w0 = edge(sx[1], sy[1], sx[2], sy[2], px, py);
    const double w1 = edge(sx[2], sy[2], sx[0], sy[0], px, py);
    const double w2 = edge(sx[0], sy[0], sx[1], sy[1], px, py);
    const double q0 = w0 / Xc[0][2];
    const double q1 = w1 / Xc[1][2];
    const double q2 = w2 / Xc[2][2];
    double Q = q0 + q1;
    Q = Q + q2;
    const double l0 = q0 / Q;
    const double l1 = q1 / Q;
    const double l2 = q2 / Q;

    double c[3], n[3], P[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = dot3(l0, l1, l2, col[0][i], col[1][i], col[2][i]);
        n[i] = dot3(l0, l1, l2, nrm[0][i], nrm[1][i], nrm[2][i]);
        P[i] = dot3(l0, l1, l2, Xc[0][i], Xc[1][i], Xc[2][i]);
    }

    const float* lf = p.light + 3 * (size_t)b;
    const float* pf = p.phong + 3 * (size_t)b;
    double N[3], L[3], V[3];
    unit3(dot3(Rm[0], Rm[1], Rm[2], n[0], n[1], n[2]), dot3(Rm[3], Rm[4], Rm[5], n[0], n[1], n[2]), dot3(Rm[6], Rm[7], Rm[8], n[0], n[1], n[2]), N);
    const double dx = (double)lf[0] - P[0];
    const double dy = (double)lf[1] - P[1];
    const double dz = (double)lf[2] - P[2];
    unit3(dx, dy, dz, L);
    unit3(-P[0], -P[1], -P[2], V);

    const double nl = dot3(N[0], N[1], N[2], L[0], L[1], L[2]);
    const double d = nl > 0.0 ? nl : 0.0;
    const double two = 2.0 * nl;
    double Rv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double mN = two * N[i];
        Rv[i] = mN - L[i];
    }
    const double rv = dot3(Rv[0], Rv[1], Rv[2], V[0], V[1], V[2]);
    const double s = rv > 0.0 ? rv : 0.0;
    const double kdd = (double)pf[1] * d;
    const double kss = (double)pf[2] * s;
    double I = (double)pf[0] + kdd;
    I = I + kss;

    dst[0] = finish(I, c[0]);
    dst[1] = finish(I, c[1]);
    dst[2] = finish(I, c[2]);
    return true;
}

__global__ __launch_bounds__(kThreads) void lc_shade_instances_kernel(const Params p) {
    const int b = (int)(blockIdx.x / (unsigned)p.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)p.tiles);
    const Mesh m = mesh_of(p, b);
    if (!m.ok) {  // the same for the whole workgroup
        if (tile == 0 && threadIdx.x == 0) p.info[b] = -1;
        return;
    }
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int x = tx * kTileW + (int)(threadIdx.x % kTileW), y = ty * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= p.w || y >= p.h) return;
    const size_t pix = ((size_t)b * p.h + y) * p.w + x;
    const int f = p.face[pix];
    if (f == -1) return;  // a miss: most pixels
    if (!shade_pixel(p, b, m, f, x, y, p.out + 3 * pix)) p.info[b] = 1;
}

__global__ __launch_bounds__(kThreads) void lc_shade_scene_kernel(const Params p) {
    const int s = (int)(blockIdx.x / (unsigned)p.tiles), tile = (int)(blockIdx.x - (unsigned)s * (unsigned)p.tiles);
    if (s == 0) {  // the rows' own refusals, whether or not a pixel names the row: the threads of scene 0 share the rows out
        for (long long r = (long long)tile * kThreads + threadIdx.x; r < p.B; r += (long long)p.tiles * kThreads)
            if (!mesh_of(p, (int)r).ok) p.info[r] = -1;
    }
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int X = tx * kTileW + (int)(threadIdx.x % kTileW), Y = ty * kTileH + (int)(threadIdx.x / kTileW);
    if (X >= p.W || Y >= p.H) return;
    const size_t pix = ((size_t)s * p.H + Y) * p.W + X;
    const int b = p.instance[pix];
    if (b < 0 || b >= p.B) return;  // -1: a miss, most pixels; anything else outside [0, B) names no row
    const Mesh m = mesh_of(p, b);
    if (!m.ok) return;  // (the row's -1 is written above)
    bool ok = p.scene_index[b] == s;
    const long long x = (long long)X - (p.origin ? p.origin[2 * (size_t)b] : 0), y = (long long)Y - (p.origin ? p.origin[2 * (size_t)b + 1] : 0);
    ok = ok && x >= 0 && x < p.w && y >= 0 && y < p.h;
    if (ok) {
        const int f = p.face[((size_t)b * p.h + (size_t)y) * p.w + (size_t)x];
        ok = shade_pixel(p, b, m, f, (int)x, (int)y, p.out + 3 * pix);
    }
    if (!ok) p.info[b] = 1;
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

bool on_grid(float c, int* units) {
    const double s = (double)c * kSub;
    if (!(std::fabs(s) <= 64.0 * kSub) || s != std::nearbyint(s)) return false;
    *units = (int)s;
    return true;
}

struct MeshArgs {
    const float* verts;
    const float* normals;
    const unsigned char* colors;
    const int* faces;
    const int* table;
    int n_meshes, total_verts, total_faces;
};

struct RowArgs {
    const int* mesh_index;
    const float* R;
    const float* t;
    const float* K;
    const float* light;
    const float* phong;
    const int* face;
    int B, h, w;
    float cx, cy;
};

// the rules both entry points share, in the header's order; fills what of `p` they determine
int common(const std::string& me, const MeshArgs& a, const RowArgs& r, int* info, Params* p) {
    if (a.n_meshes < 1) return fail(2, me + "n_meshes < 1");
    if (a.total_verts < 0 || a.total_faces < 0) return fail(2, me + "total_verts < 0 or total_faces < 0");
    if (!a.table) return fail(3, me + "mesh_table must not be NULL");
    if (a.total_verts > 0 && (!a.verts || !a.normals || !a.colors)) return fail(3, me + "verts, normals and colors must not be NULL where total_verts > 0");
    if (a.total_faces > 0 && !a.faces) return fail(3, me + "faces must not be NULL where total_faces > 0");
    if (!r.mesh_index || !r.R || !r.t || !r.K || !r.light || !r.phong || !r.face) return fail(3, me + "mesh_index, R, t, K, light, phong and face must not be NULL");
    if (!info) return fail(3, me + "info must not be NULL");
    if (r.h < 1 || r.w < 1 || r.h > LC_SHADE_MAX_SIZE || r.w > LC_SHADE_MAX_SIZE)
        return fail(5, me + "h and w must be in [1, " + std::to_string(LC_SHADE_MAX_SIZE) + "], got " + std::to_string(r.h) + " x " + std::to_string(r.w));
    if (!on_grid(r.cx, &p->cxi) || !on_grid(r.cy, &p->cyi)) return fail(6, me + "cx and cy must be multiples of 2^-8 in [-64, 64]");
    if (misaligned(a.verts, 4) || misaligned(a.normals, 4) || misaligned(a.faces, 4) || misaligned(a.table, 4))
        return fail(7, me + "verts, normals, faces and mesh_table must be aligned to 4 bytes");
    if (misaligned(r.mesh_index, 4) || misaligned(r.R, 4) || misaligned(r.t, 4) || misaligned(r.K, 4) || misaligned(r.light, 4) || misaligned(r.phong, 4) ||
        misaligned(r.face, 4) || misaligned(info, 4))
        return fail(7, me + "mesh_index, R, t, K, light, phong, face and info must be aligned to 4 bytes");
    p->verts = a.verts; p->normals = a.normals; p->colors = a.colors; p->faces = a.faces; p->table = a.table;
    p->n_meshes = a.n_meshes; p->total_verts = a.total_verts; p->total_faces = a.total_faces;
    p->mesh_index = r.mesh_index; p->R = r.R; p->t = r.t; p->K = r.K; p->light = r.light; p->phong = r.phong; p->face = r.face;
    p->B = r.B; p->h = r.h; p->w = r.w; p->info = info;
    return 0;
}

// info cleared on the stream, then the one launch over `maps` maps of H x W pixels
template <typename Kernel>
int launch(const std::string& me, Kernel kernel, Params& p, long long maps, int H, int W, void* stream) {
    p.tiles_x = (W + kTileW - 1) / kTileW;
    const long long tiles = (long long)p.tiles_x * ((H + kTileH - 1) / kTileH);
    if (tiles * maps > 0x7fffffffLL) return fail(8, me + "too many rows and tiles for one launch");
    p.tiles = (int)tiles;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(p.info, 0, sizeof(int) * (size_t)p.B, st);
    if (e != hipSuccess) return fail(9, me + "memset: " + hipGetErrorString(e));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles * maps)), dim3(kThreads), 0, st, p);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(9, me + "launch: " + hipGetErrorString(e));
    return 0;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_shade_version(void) { return LC_AMD_SHADE_VERSION; }
const char* lc_amd_shade_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_SHADE_SRC_HASH:") - 1; }
const char* lc_amd_shade_last_error(void) { return lc::g_err.c_str(); }

int lc_shade_instances_u8(const float* verts, const float* normals, const unsigned char* colors, const int* faces, const int* mesh_table, int n_meshes,
                          int total_verts, int total_faces, const int* mesh_index, const float* R, const float* t, const float* K, const float* light,
                          const float* phong, const int* face, int B, int h, int w, float cx, float cy, unsigned char* out, int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_shade_instances_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    lc::Params p{};
    if (const int rc = lc::common(me, {verts, normals, colors, faces, mesh_table, n_meshes, total_verts, total_faces},
                                  {mesh_index, R, t, K, light, phong, face, B, h, w, cx, cy}, info, &p))
        return rc;
    if (!out) return fail(3, me + "out must not be NULL");
    p.out = out;
    return lc::launch(me, lc::lc_shade_instances_kernel, p, B, h, w, stream);
}

int lc_shade_scene_u8(const float* verts, const float* normals, const unsigned char* colors, const int* faces, const int* mesh_table, int n_meshes,
                      int total_verts, int total_faces, const int* mesh_index, const int* scene_index, const float* R, const float* t, const float* K,
                      const float* light, const float* phong, const int* face, const int* origin_xy, int B, int h, int w, float cx, float cy,
                      const int* instance, unsigned char* frames, int S, int H, int W, int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_shade_scene_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    lc::Params p{};
    if (const int rc = lc::common(me, {verts, normals, colors, faces, mesh_table, n_meshes, total_verts, total_faces},
                                  {mesh_index, R, t, K, light, phong, face, B, h, w, cx, cy}, info, &p))
        return rc;
    if (S < 1) return fail(2, me + "S < 1");
    if (!scene_index || !instance || !frames) return fail(3, me + "scene_index, instance and frames must not be NULL");
    if (H < 1 || W < 1 || H > LC_SHADE_MAX_SIZE || W > LC_SHADE_MAX_SIZE)
        return fail(5, me + "H and W must be in [1, " + std::to_string(LC_SHADE_MAX_SIZE) + "], got " + std::to_string(H) + " x " + std::to_string(W));
    if (!origin_xy && (h != H || w != W)) return fail(5, me + "without origin_xy the maps must have the frame's size");
    if (lc::misaligned(scene_index, 4) || lc::misaligned(instance, 4) || lc::misaligned(origin_xy, 4))
        return fail(7, me + "scene_index, instance and origin_xy must be aligned to 4 bytes");
    p.scene_index = scene_index; p.origin = origin_xy; p.instance = instance; p.out = frames;
    p.S = S; p.H = H; p.W = W;
    return lc::launch(me, lc::lc_shade_scene_kernel, p, S, H, W, stream);
}

}  // extern "C"
#pragma GCC visibility pop
