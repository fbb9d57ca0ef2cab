// The textured shading pass behind the depth rasteriser: lc_shade.hip's pixel with the albedo sampled from a resident store of mip-mapped
// textures at per-corner texture coordinates (liblc_amd_texture.so; C ABI and the exact definition of every byte in
// include/lc_amd_texture.h).
//
//   lc_texshade_instances_kernel  one workgroup of 256 threads per (row, 16 x 16 tile of the row's map), one thread per pixel.  The row is
//                                 the workgroup's: its mesh and texture entries, wrap, R, t, K, light and phong are uniform loads, and
//                                 "has this mesh a texture" and `lod` are uniform branches.
//   lc_texshade_scene_kernel      the same tiles over the frames of S scenes; the row is the pixel's instance and differs between lanes.
//   tex_pixel                     one hit pixel for both: lc_shade.hip's arithmetic, and for a textured mesh six more float loads (the
//                                 face's corner coordinates), with `lod` two more perspective-correct interpolations (three quotients
//                                 each and their normalisation), and four dependent 32-bit texel gathers.  A wave covers 16 x 4 pixels
//                                 (tile choice: DESIGN.md, section 4), so the texels its lanes of one face gather are neighbours in both
//                                 directions of the texture.
//   lc_tex_mip_kernel             one level of one texture from the level above it, one thread per texel written; runs once per store.
//
// The contract rounds every fp64 operation on its own and the library is built with -ffp-contract=on, which fuses a product and a sum only
// inside one expression.  So every operation below is a statement of its own, as in lc_shade.hip, whose steps 1 to 4 and 6 to 8 are restated
// here (tests/test_gpu_texshade.py pins the two to each other on meshes without a texture and on constant textures).
//
// Bounds: everything lc_shade.hip checks, in its order; a mesh's tex_index against n_tex before the table is read; the table entry
// (offset, sizes, level count, and the end of its last level against total_texels) before a texel is read; the face index, which the mesh
// entry has placed inside total_faces, indexes uv; a texel index is clamped or reduced into [0, WL) x [0, HL) of a level inside the checked
// chain.  A pixel whose texel coordinate is not finite or at least 2^30 in size is refused before it is converted to an integer.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/lc_amd_texture.h"

#ifndef LC_AMD_TEXTURE_SRC_HASH
#define LC_AMD_TEXTURE_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_TEXTURE_SRC_HASH:" LC_AMD_TEXTURE_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 256;
constexpr int kTileW = 16, kTileH = 16;  // kTileW * kTileH == kThreads; a wave covers four rows of 16 pixels
constexpr int kMaxSize = 16384;          // of a map or frame side, as lc_shade.hip has it
constexpr double kSub = 256.0;           // grid units per pixel (2^-8 px), as the rasteriser has it
constexpr double kCoordLimit = 1073741824.0;  // 2^30: a texel coordinate of this size or more is refused

struct Params {
    const float* verts;
    const float* normals;
    const unsigned char* colors;
    const int* faces;
    const float* uv;
    const int* table;
    const int* tex_index;
    const uint32_t* texels;
    const long long* tex_table;
    const int* mesh_index;
    const int* scene_index;
    const float* R;
    const float* t;
    const float* K;
    const float* light;
    const float* phong;
    const int* wrap;
    const int* face;
    const int* origin;    // NULL: every window lies at (0, 0)
    const int* instance;
    unsigned char* out;   // (B,h,w,3) or the frames (S,H,W,3)
    int* info;
    long long total_texels;
    int n_meshes, total_verts, total_faces, n_tex, B, h, w, S, H, W;
    int cxi, cyi;         // the sample offset in grid units
    int lod;
    int tiles_x, tiles;   // tiles per map row, and per map
};

// what a row's pixels share: its mesh entry, its texture entry (tex < 0: none) and wrap
struct Row {
    int vert_off, n_vert, face_off, n_face;
    int tex, Ht, Wt, n_levels, wrap;
    long long tex_off;
    bool ok;
};

// H W summed over the levels [0, n) of a chain that starts at (H, W)
__host__ __device__ __forceinline__ long long chain_texels(int H, int W, int n) {
    long long sum = 0;
    for (int l = 0; l < n; ++l) {
        sum += (long long)H * W;
        H = H > 1 ? H >> 1 : 1;
        W = W > 1 ? W >> 1 : 1;
    }
    return sum;
}

__host__ __device__ __forceinline__ bool entry_ok(long long off, long long Ht, long long Wt, long long n_levels, long long total_texels) {
    if (off < 0 || Ht < 1 || Wt < 1 || Ht > LC_TEX_MAX_SIZE || Wt > LC_TEX_MAX_SIZE || n_levels < 1 || n_levels > LC_TEX_MAX_LEVELS) return false;
    return off <= total_texels && chain_texels((int)Ht, (int)Wt, (int)n_levels) <= total_texels - off;
}

// the row's entries, refused where an index or an entry reaches outside what the caller declared
__device__ __forceinline__ Row row_of(const Params& p, int b) {
    Row r{0, 0, 0, 0, -1, 1, 1, 1, 0, 0, false};
    const int mi = p.mesh_index[b];
    if (mi < 0 || mi >= p.n_meshes) return r;
    const int* e = p.table + 4 * (size_t)mi;
    r.vert_off = e[0]; r.n_vert = e[1]; r.face_off = e[2]; r.n_face = e[3];
    if (!(r.vert_off >= 0 && r.n_vert >= 0 && r.face_off >= 0 && r.n_face >= 0 && (long long)r.vert_off + r.n_vert <= p.total_verts &&
          (long long)r.face_off + r.n_face <= p.total_faces))
        return r;
    r.wrap = p.wrap[b];
    if (r.wrap != 0 && r.wrap != 1) return r;
    r.tex = p.tex_index[mi];
    if (r.tex < -1 || r.tex >= p.n_tex) return r;
    if (r.tex >= 0) {
        const long long* te = p.tex_table + 4 * (size_t)r.tex;
        const long long off = te[0], Ht = te[1], Wt = te[2], nl = te[3];
        if (!entry_ok(off, Ht, Wt, nl, p.total_texels)) return r;
        r.tex_off = off; r.Ht = (int)Ht; r.Wt = (int)Wt; r.n_levels = (int)nl;
    }
    r.ok = true;
    return r;
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

// steps 3 and 4 at the sample (px, py): the perspective-correct weights of the face's three corners
__device__ __forceinline__ void weights(const double (&sx)[3], const double (&sy)[3], double z0, double z1, double z2, double px, double py, double (&l)[3]) {
    const double w0 = edge(sx[1], sy[1], sx[2], sy[2], px, py);
    const double w1 = edge(sx[2], sy[2], sx[0], sy[0], px, py);
    const double w2 = edge(sx[0], sy[0], sx[1], sy[1], px, py);
    const double q0 = w0 / z0;
    const double q1 = w1 / z1;
    const double q2 = w2 / z2;
    double Q = q0 + q1;
    Q = Q + q2;
    l[0] = q0 / Q;
    l[1] = q1 / Q;
    l[2] = q2 / Q;
}

// (dU Wt)^2 + (dV Ht)^2 of a neighbouring sample's coordinates against the pixel's
__device__ __forceinline__ double rho2_of(double Un, double Vn, double U, double V, double Wt, double Ht) {
    const double du = Un - U;
    const double dv = Vn - V;
    const double a = du * Wt;
    const double b = dv * Ht;
    const double aa = a * a;
    const double bb = b * b;
    return aa + bb;
}

// a texel coordinate: its lower index and its weight in 256ths (0 .. 256)
__device__ __forceinline__ void split(double tc, int* i0, int* f8) {
    const double fl = floor(tc);
    const double fr = tc - fl;
    const double s = 256.0 * fr;
    *i0 = (int)fl;
    *f8 = (int)floor(s);
}

__device__ __forceinline__ int into_level(int i, int n, int wrap) {
    if (wrap) {
        const int m = i % n;
        return m < 0 ? m + n : m;
    }
    return i < 0 ? 0 : i >= n ? n - 1 : i;
}

__device__ __forceinline__ unsigned char finish(double I, double c) {
    const double v = I * c;
    return v >= 255.0 ? (unsigned char)255 : v > 0.0 ? (unsigned char)(int)rint(v) : (unsigned char)0;  // NaN: 0
}

// The hit pixel of row b with face f at window pixel (x, y): steps 1 to 8 of the header.  false: refused, nothing written.
__device__ __forceinline__ bool tex_pixel(const Params& p, int b, const Row& m, int f, int x, int y, unsigned char* dst) {
    if (f < 0 || f >= m.n_face) return false;
    const size_t fg = (size_t)m.face_off + (size_t)f;
    const int* tri = p.faces + 3 * fg;
    const int idx[3] = {tri[0], tri[1], tri[2]};
    if ((unsigned)idx[0] >= (unsigned)m.n_vert || (unsigned)idx[1] >= (unsigned)m.n_vert || (unsigned)idx[2] >= (unsigned)m.n_vert) return false;
    const bool textured = m.tex >= 0;

    const float* Rf = p.R + 9 * (size_t)b;
    const float* tf = p.t + 3 * (size_t)b;
    const float* Kf = p.K + 9 * (size_t)b;
    double Rm[9], tv[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rm[i] = (double)Rf[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tv[i] = (double)tf[i];
    const double k00 = (double)Kf[0], k01 = (double)Kf[1], k02 = (double)Kf[2], k10 = (double)Kf[3], k11 = (double)Kf[4], k12 = (double)Kf[5];

    double Xc[3][3], sx[3], sy[3], nrm[3][3];
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
        for (int c = 0; c < 3; ++c) nrm[k][c] = (double)p.normals[v + c];
    }

    const double px = (double)(x * 256 + p.cxi), py = (double)(y * 256 + p.cyi);
    double l[3];
    weights(sx, sy, Xc[0][2], Xc[1][2], Xc[2][2], px, py, l);

    double c[3];
    if (!textured) {  // the vertex colours, as lc_shade.hip has them
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double c0 = (double)p.colors[3 * ((size_t)m.vert_off + (size_t)idx[0]) + i];
            const double c1 = (double)p.colors[3 * ((size_t)m.vert_off + (size_t)idx[1]) + i];
            const double c2 = (double)p.colors[3 * ((size_t)m.vert_off + (size_t)idx[2]) + i];
            c[i] = dot3(l[0], l[1], l[2], c0, c1, c2);
        }
    } else {
        const float* uvf = p.uv + 6 * fg;
        const double u0 = (double)uvf[0], v0 = (double)uvf[1], u1 = (double)uvf[2], v1 = (double)uvf[3], u2 = (double)uvf[4], v2 = (double)uvf[5];
        const double U = dot3(l[0], l[1], l[2], u0, u1, u2);
        const double V = dot3(l[0], l[1], l[2], v0, v1, v2);
        if (!(fabs(U) < INFINITY) || !(fabs(V) < INFINITY)) return false;
        int level = 0;
        if (p.lod) {
            double lx[3], ly[3];
            const double pxn = px + kSub;
            const double pyn = py + kSub;
            weights(sx, sy, Xc[0][2], Xc[1][2], Xc[2][2], pxn, py, lx);
            weights(sx, sy, Xc[0][2], Xc[1][2], Xc[2][2], px, pyn, ly);
            const double Wt = (double)m.Wt, Ht = (double)m.Ht;
            const double r2x = rho2_of(dot3(lx[0], lx[1], lx[2], u0, u1, u2), dot3(lx[0], lx[1], lx[2], v0, v1, v2), U, V, Wt, Ht);
            const double r2y = rho2_of(dot3(ly[0], ly[1], ly[2], u0, u1, u2), dot3(ly[0], ly[1], ly[2], v0, v1, v2), U, V, Wt, Ht);
            const double r2 = r2x > r2y ? r2x : r2y;
            double thr = 2.0;  // 2^(2L-1) at L = 1
            for (int L = 1; L < m.n_levels; ++L) {
                level += r2 > thr ? 1 : 0;
                thr = thr * 4.0;
            }
        }
        long long off = m.tex_off;
        int HL = m.Ht, WL = m.Wt;
        for (int L = 0; L < level; ++L) {
            off += (long long)HL * WL;
            HL = HL > 1 ? HL >> 1 : 1;
            WL = WL > 1 ? WL >> 1 : 1;
        }
        const double mu = U * (double)WL;
        const double tx = mu - 0.5;
        const double omv = 1.0 - V;
        const double mv = omv * (double)HL;
        const double ty = mv - 0.5;
        if (!(fabs(tx) < kCoordLimit) || !(fabs(ty) < kCoordLimit)) return false;
        int x0, y0, a8, b8;
        split(tx, &x0, &a8);
        split(ty, &y0, &b8);
        const int xa = into_level(x0, WL, m.wrap), xb = into_level(x0 + 1, WL, m.wrap);
        const int ya = into_level(y0, HL, m.wrap), yb = into_level(y0 + 1, HL, m.wrap);
        const uint32_t* lev = p.texels + off;
        const uint32_t t00 = lev[(size_t)ya * WL + xa], t10 = lev[(size_t)ya * WL + xb];
        const uint32_t t01 = lev[(size_t)yb * WL + xa], t11 = lev[(size_t)yb * WL + xb];
        const int w00 = (256 - a8) * (256 - b8), w10 = a8 * (256 - b8), w01 = (256 - a8) * b8, w11 = a8 * b8;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int sh = 8 * i;
            const int c16 = w00 * (int)((t00 >> sh) & 255u) + w10 * (int)((t10 >> sh) & 255u) + w01 * (int)((t01 >> sh) & 255u) + w11 * (int)((t11 >> sh) & 255u);
            c[i] = (double)c16 / 65536.0;  // exact
        }
    }

    double n[3], P[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        n[i] = dot3(l[0], l[1], l[2], nrm[0][i], nrm[1][i], nrm[2][i]);
        P[i] = dot3(l[0], l[1], l[2], Xc[0][i], Xc[1][i], Xc[2][i]);
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

__global__ __launch_bounds__(kThreads) void lc_texshade_instances_kernel(const Params p) {
    const int b = (int)(blockIdx.x / (unsigned)p.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)p.tiles);
    const Row m = row_of(p, b);
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
    if (!tex_pixel(p, b, m, f, x, y, p.out + 3 * pix)) p.info[b] = 1;
}

__global__ __launch_bounds__(kThreads) void lc_texshade_scene_kernel(const Params p) {
    const int s = (int)(blockIdx.x / (unsigned)p.tiles), tile = (int)(blockIdx.x - (unsigned)s * (unsigned)p.tiles);
    if (s == 0) {  // the rows' own refusals, whether or not a pixel names the row: the threads of scene 0 share the rows out
        for (long long r = (long long)tile * kThreads + threadIdx.x; r < p.B; r += (long long)p.tiles * kThreads)
            if (!row_of(p, (int)r).ok) p.info[r] = -1;
    }
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int X = tx * kTileW + (int)(threadIdx.x % kTileW), Y = ty * kTileH + (int)(threadIdx.x / kTileW);
    if (X >= p.W || Y >= p.H) return;
    const size_t pix = ((size_t)s * p.H + Y) * p.W + X;
    const int b = p.instance[pix];
    if (b < 0 || b >= p.B) return;  // -1: a miss, most pixels; anything else outside [0, B) names no row
    const Row m = row_of(p, b);
    if (!m.ok) return;  // (the row's -1 is written above)
    bool ok = p.scene_index[b] == s;
    const long long x = (long long)X - (p.origin ? p.origin[2 * (size_t)b] : 0), y = (long long)Y - (p.origin ? p.origin[2 * (size_t)b + 1] : 0);
    ok = ok && x >= 0 && x < p.w && y >= 0 && y < p.h;
    if (ok) {
        const int f = p.face[((size_t)b * p.h + (size_t)y) * p.w + (size_t)x];
        ok = tex_pixel(p, b, m, f, (int)x, (int)y, p.out + 3 * pix);
    }
    if (!ok) p.info[b] = 1;
}

// level L+1 (Hd x Wd, at dst) of a texture from its level L (Hs x Ws, at src): the rounded mean of the 2 x 2 block, clamped at the edge
__global__ __launch_bounds__(kThreads) void lc_tex_mip_kernel(uint32_t* texels, long long src, long long dst, int Hs, int Ws, int Hd, int Wd) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)Hd * Wd) return;
    const int y = (int)(i / Wd), x = (int)(i - (long long)y * Wd);
    const int x0 = min(2 * x, Ws - 1), x1 = min(2 * x + 1, Ws - 1), y0 = min(2 * y, Hs - 1), y1 = min(2 * y + 1, Hs - 1);
    const uint32_t* s = texels + src;
    const uint32_t t00 = s[(size_t)y0 * Ws + x0], t10 = s[(size_t)y0 * Ws + x1], t01 = s[(size_t)y1 * Ws + x0], t11 = s[(size_t)y1 * Ws + x1];
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const uint32_t sum = ((t00 >> sh) & 255u) + ((t10 >> sh) & 255u) + ((t01 >> sh) & 255u) + ((t11 >> sh) & 255u) + 2u;
        o |= (sum >> 2) << sh;
    }
    texels[dst + i] = o;
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
    const float* uv;
    const int* table;
    const int* tex_index;
    int n_meshes, total_verts, total_faces;
    const unsigned char* texels;
    const long long* tex_table;
    int n_tex;
    long long total_texels;
};

struct RowArgs {
    const int* mesh_index;
    const float* R;
    const float* t;
    const float* K;
    const float* light;
    const float* phong;
    const int* wrap;
    const int* face;
    int B, h, w;
    float cx, cy;
    int lod;
};

// the rules both entry points share, in the header's order; fills what of `p` they determine
int common(const std::string& me, const MeshArgs& a, const RowArgs& r, int* info, Params* p) {
    if (a.n_meshes < 1) return fail(2, me + "n_meshes < 1");
    if (a.total_verts < 0 || a.total_faces < 0) return fail(2, me + "total_verts < 0 or total_faces < 0");
    if (a.n_tex < 0 || a.total_texels < 0) return fail(2, me + "n_tex < 0 or total_texels < 0");
    if (!a.table || !a.tex_index) return fail(3, me + "mesh_table and tex_index must not be NULL");
    if (a.total_verts > 0 && (!a.verts || !a.normals || !a.colors)) return fail(3, me + "verts, normals and colors must not be NULL where total_verts > 0");
    if (a.total_faces > 0 && (!a.faces || !a.uv)) return fail(3, me + "faces and uv must not be NULL where total_faces > 0");
    if (a.n_tex > 0 && (!a.texels || !a.tex_table)) return fail(3, me + "texels and tex_table must not be NULL where n_tex > 0");
    if (!r.mesh_index || !r.R || !r.t || !r.K || !r.light || !r.phong || !r.wrap || !r.face)
        return fail(3, me + "mesh_index, R, t, K, light, phong, wrap and face must not be NULL");
    if (!info) return fail(3, me + "info must not be NULL");
    if (r.h < 1 || r.w < 1 || r.h > kMaxSize || r.w > kMaxSize)
        return fail(5, me + "h and w must be in [1, " + std::to_string(kMaxSize) + "], got " + std::to_string(r.h) + " x " + std::to_string(r.w));
    if (!on_grid(r.cx, &p->cxi) || !on_grid(r.cy, &p->cyi)) return fail(6, me + "cx and cy must be multiples of 2^-8 in [-64, 64]");
    if (r.lod != 0 && r.lod != 1) return fail(6, me + "lod must be 0 or 1, got " + std::to_string(r.lod));
    if (misaligned(a.verts, 4) || misaligned(a.normals, 4) || misaligned(a.faces, 4) || misaligned(a.uv, 4) || misaligned(a.table, 4) || misaligned(a.tex_index, 4))
        return fail(7, me + "verts, normals, faces, uv, mesh_table and tex_index must be aligned to 4 bytes");
    if (misaligned(a.texels, 4) || misaligned(a.tex_table, 8)) return fail(7, me + "texels must be aligned to 4 bytes and tex_table to 8");
    if (misaligned(r.mesh_index, 4) || misaligned(r.R, 4) || misaligned(r.t, 4) || misaligned(r.K, 4) || misaligned(r.light, 4) || misaligned(r.phong, 4) ||
        misaligned(r.wrap, 4) || misaligned(r.face, 4) || misaligned(info, 4))
        return fail(7, me + "mesh_index, R, t, K, light, phong, wrap, face and info must be aligned to 4 bytes");
    p->verts = a.verts; p->normals = a.normals; p->colors = a.colors; p->faces = a.faces; p->uv = a.uv; p->table = a.table; p->tex_index = a.tex_index;
    p->n_meshes = a.n_meshes; p->total_verts = a.total_verts; p->total_faces = a.total_faces;
    p->texels = reinterpret_cast<const uint32_t*>(a.texels); p->tex_table = a.tex_table; p->n_tex = a.n_tex; p->total_texels = a.total_texels;
    p->mesh_index = r.mesh_index; p->R = r.R; p->t = r.t; p->K = r.K; p->light = r.light; p->phong = r.phong; p->wrap = r.wrap; p->face = r.face;
    p->B = r.B; p->h = r.h; p->w = r.w; p->lod = r.lod; p->info = info;
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

int lc_amd_texture_version(void) { return LC_AMD_TEXTURE_VERSION; }
const char* lc_amd_texture_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_TEXTURE_SRC_HASH:") - 1; }
const char* lc_amd_texture_last_error(void) { return lc::g_err.c_str(); }

int lc_tex_build_mips_u8(unsigned char* texels, long long total_texels, const long long* tex_table_host, int n_tex, void* stream) {
    using lc::fail;
    const std::string me = "lc_tex_build_mips_u8: ";
    if (n_tex < 0 || total_texels < 0) return fail(2, me + "n_tex < 0 or total_texels < 0");
    if (n_tex == 0) return 0;
    if (!texels || !tex_table_host) return fail(3, me + "texels and tex_table_host must not be NULL");
    if (lc::misaligned(texels, 4) || lc::misaligned(tex_table_host, 8)) return fail(7, me + "texels must be aligned to 4 bytes and tex_table_host to 8");
    for (int k = 0; k < n_tex; ++k) {
        const long long* e = tex_table_host + 4 * (size_t)k;
        if (!lc::entry_ok(e[0], e[1], e[2], e[3], total_texels))
            return fail(4, me + "texture " + std::to_string(k) + ": the entry (" + std::to_string(e[0]) + ", " + std::to_string(e[1]) + ", " + std::to_string(e[2]) + ", " +
                               std::to_string(e[3]) + ") is invalid or reaches outside the " + std::to_string(total_texels) + " texels");
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    for (int k = 0; k < n_tex; ++k) {
        const long long* e = tex_table_host + 4 * (size_t)k;
        long long src = e[0];
        int Hs = (int)e[1], Ws = (int)e[2];
        for (int L = 1; L < (int)e[3]; ++L) {
            const int Hd = Hs > 1 ? Hs >> 1 : 1, Wd = Ws > 1 ? Ws >> 1 : 1;
            const long long dst = src + (long long)Hs * Ws, n = (long long)Hd * Wd;
            hipLaunchKernelGGL(lc::lc_tex_mip_kernel, dim3((unsigned)((n + lc::kThreads - 1) / lc::kThreads)), dim3(lc::kThreads), 0, st,
                               reinterpret_cast<uint32_t*>(texels), src, dst, Hs, Ws, Hd, Wd);
            const hipError_t err = hipGetLastError();
            if (err != hipSuccess) return fail(9, me + "launch: " + hipGetErrorString(err));
            src = dst; Hs = Hd; Ws = Wd;
        }
    }
    return 0;
}

int lc_texshade_instances_u8(const float* verts, const float* normals, const unsigned char* colors, const int* faces, const float* uv, const int* mesh_table,
                             const int* tex_index, int n_meshes, int total_verts, int total_faces, const unsigned char* texels, const long long* tex_table,
                             int n_tex, long long total_texels, const int* mesh_index, const float* R, const float* t, const float* K, const float* light,
                             const float* phong, const int* wrap, const int* face, int B, int h, int w, float cx, float cy, int lod, unsigned char* out,
                             int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_texshade_instances_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    lc::Params p{};
    if (const int rc = lc::common(me, {verts, normals, colors, faces, uv, mesh_table, tex_index, n_meshes, total_verts, total_faces, texels, tex_table, n_tex, total_texels},
                                  {mesh_index, R, t, K, light, phong, wrap, face, B, h, w, cx, cy, lod}, info, &p))
        return rc;
    if (!out) return fail(3, me + "out must not be NULL");
    p.out = out;
    return lc::launch(me, lc::lc_texshade_instances_kernel, p, B, h, w, stream);
}

int lc_texshade_scene_u8(const float* verts, const float* normals, const unsigned char* colors, const int* faces, const float* uv, const int* mesh_table,
                         const int* tex_index, int n_meshes, int total_verts, int total_faces, const unsigned char* texels, const long long* tex_table, int n_tex,
                         long long total_texels, const int* mesh_index, const int* scene_index, const float* R, const float* t, const float* K,
                         const float* light, const float* phong, const int* wrap, const int* face, const int* origin_xy, int B, int h, int w, float cx,
                         float cy, int lod, const int* instance, unsigned char* frames, int S, int H, int W, int* info, void* stream) {
    using lc::fail;
    const std::string me = "lc_texshade_scene_u8: ";
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    lc::Params p{};
    if (const int rc = lc::common(me, {verts, normals, colors, faces, uv, mesh_table, tex_index, n_meshes, total_verts, total_faces, texels, tex_table, n_tex, total_texels},
                                  {mesh_index, R, t, K, light, phong, wrap, face, B, h, w, cx, cy, lod}, info, &p))
        return rc;
    if (S < 1) return fail(2, me + "S < 1");
    if (!scene_index || !instance || !frames) return fail(3, me + "scene_index, instance and frames must not be NULL");
    if (H < 1 || W < 1 || H > lc::kMaxSize || W > lc::kMaxSize)
        return fail(5, me + "H and W must be in [1, " + std::to_string(lc::kMaxSize) + "], got " + std::to_string(H) + " x " + std::to_string(W));
    if (!origin_xy && (h != H || w != W)) return fail(5, me + "without origin_xy the maps must have the frame's size");
    if (lc::misaligned(scene_index, 4) || lc::misaligned(instance, 4) || lc::misaligned(origin_xy, 4))
        return fail(7, me + "scene_index, instance and origin_xy must be aligned to 4 bytes");
    p.scene_index = scene_index; p.origin = origin_xy; p.instance = instance; p.out = frames;
    p.S = S; p.H = H; p.W = W;
    return lc::launch(me, lc::lc_texshade_scene_kernel, p, S, H, W, stream);
}

}  // extern "C"
#pragma GCC visibility pop
