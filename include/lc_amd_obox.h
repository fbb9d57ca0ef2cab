/*
 * lc_amd obox -- C ABI of the oriented model box search (liblc_amd_obox.so, built from lc_amd/csrc/obox/).
 *
 * A library of its own, next to liblc_amd.so and its siblings: the kernels of an offline tool (python -m lc_amd.prep_models --xform); no
 * other ABI is changed by it.
 *
 * What models_xform.json holds per object (model_transform.py:21-42): a rigid `xform` after which the model's bounding box is centred on the
 * origin, and the half-extents `xformed_noc_scale` of that box.  The rotation is searched: the candidate whose box has the least volume, over
 * a STATED hierarchical grid of rotations.  It is not a proven global minimum.
 *
 * INPUTS.  verts (total_verts,3) fp32; table (n_meshes,4) int32 rows (vert_off, n_vert, face_off, n_face) on the DEVICE and the same rows in HOST
 * memory as table_host: the argument rules are checked from the host copy, the kernels read the device copy; max_verts >= every n_vert >= 1,
 * every vert_off + n_vert <= total_verts, 3 * max_verts < 2^31.  deltas (n_level0 + levels * n_refine, 4) fp64 on the DEVICE: unit quaternions (w, x, y, z), the table of level 0
 * and behind it the tables of levels 1 .. levels.  The library reads the table as it is; lc_amd.obox.delta_table makes the stated one (below).
 *
 * CANDIDATES.  Every mesh carries a base quaternion b (fp64), the identity (1, 0, 0, 0) before level 0.  Candidate c of a level, with
 * d = deltas[c] of that level's table:
 *     c == 0:  q = b, as it is (no product, no normalisation);
 *     c  > 0:  the Hamilton product p = d (x) b,
 *                  pw = ((dw*bw - dx*bx) - dy*by) - dz*bz        px = ((dw*bx + dx*bw) + dy*bz) - dz*by
 *                  py = ((dw*by - dx*bz) + dy*bw) + dz*bx        pz = ((dw*bz + dx*by) - dy*bx) + dz*bw
 *              n = sqrt(((pw*pw + px*px) + py*py) + pz*pz),  q = (pw / n, px / n, py / n, pz / n).
 * The matrix of q = (w, x, y, z), row-major:
 *     R00 = 1 - 2*(y*y + z*z)   R01 = 2*(x*y - w*z)       R02 = 2*(x*z + w*y)
 *     R10 = 2*(x*y + w*z)       R11 = 1 - 2*(x*x + z*z)   R12 = 2*(y*z - w*x)
 *     R20 = 2*(x*z - w*y)       R21 = 2*(y*z + w*x)       R22 = 1 - 2*(x*x + y*y)
 * Every operation above is IEEE fp64, rounded on its own (no FMA), the square root and the divisions correctly rounded; each entry is then
 * rounded ONCE to fp32.  No libm function is called on the device.
 *
 * SCORE of a candidate for a mesh with vertices v[0..V).  All in IEEE fp32, every operation rounded on its own (no FMA):
 *     p = R v, each component ((r0*x + r1*y) + r2*z);  lo, hi = component-wise min and max of p over the mesh, a zero of either sign counted
 *     as +0 (lo + 0.0f, hi + 0.0f);  e = hi - lo;  score = (e.x * e.y) * e.z.
 * Min and max are exact in any order: how the vertices are split over workgroups changes no bit.
 *
 * WINNER of a level: the lowest score, ties to the lowest candidate index; its q is the base of the next level, its index goes to
 * path[level].  Candidate 0 is the base itself, so the winning score never rises from level to level, and a mesh whose score under the
 * identity is 0, the lowest there is (one vertex; a mesh flat along a model axis), keeps the identity with path all zero.
 *
 * FINAL PASS, with R the fp32 matrix of the last winner: lo, hi as above; c = (lo + hi) * 0.5f; t = -c;
 *     noc_scale = max(hi - c, c - lo) component-wise.  |fl(R v - c)| <= noc_scale then holds for every vertex in fp32 exactly.
 *
 * THE STATED TABLES (lc_amd.obox.delta_table; tests/obox_oracle.py restates them).  step0 = LC_OBOX_STEP0_DEG degrees = pi / 20 in fp64.  A
 * rotation vector r = (i, j, k) * s with integers i, j, k and n2 = i*i + j*j + k*k > 0 becomes a = s * sqrt(n2), h = a * 0.5, f = sin(h) / sqrt(n2),
 * d = (cos(h), i*f, j*f, k*f); the zero vector becomes (1, 0, 0, 0).  The vectors of a table are listed by ascending (n2, i, j, k), so the zero
 * vector is candidate 0 and -r is listed whenever r is.
 *     all orientations: level 0 is every (i, j, k) with n2 <= LC_OBOX_GRID_RADIUS^2 at s = step0 (LC_OBOX_LEVEL0_COUNT = 1419 candidates: rotation
 *         angles up to 63 degrees, a ball that covers every orientation modulo the cube's 24 rotations, whose farthest member turns by 62.8);
 *         level l >= 1 is the 125 vectors with i, j, k in -2..2 at s = step0 / 2^l.
 *     about model axis `axis`: only that component is non-zero; level 0 is 0 .. LC_OBOX_AXIS_LEVEL0_COUNT - 1 steps of step0 (the angles of
 *         [0, 90) degrees), in ascending order; level l >= 1 is the 5 vectors with the component in -2..2 at s = step0 / 2^l.  The other two
 *         components of every quaternion are exactly zero, so the row and the column of that axis in R are the unit vector.
 *
 * OUTPUTS, per mesh: xform (n_meshes,4,4) fp32 = [R | t; 0 0 0 1]; noc_scale (n_meshes,3); volume (n_meshes,) the last winner's score;
 * aabb_volume (n_meshes,) the score of the identity; path (n_meshes,levels+1) int32; info (n_meshes,) int32: 0, or 1 if a coordinate of the
 * mesh is not finite (the mesh's other outputs are then unspecified but written; other meshes are unaffected).  None may be NULL.
 *
 * The same inputs give the same bits on every call.  workspace: lc_obox_workspace_bytes(n_meshes, max_cand) bytes with
 * max_cand = max(n_level0, n_refine), 16-byte aligned, = 32 * n_meshes (the bases) + 4 * n_meshes rounded up to 16 (the flags)
 * + 24 * n_meshes * max_cand (six ordered-integer extrema per candidate); it carries nothing from call to call.  A mesh's vertices are split
 * over workgroups in chunks of LC_OBOX_SPLIT, staged through LDS in tiles of LC_OBOX_TILE.  Every rule is checked before anything is
 * launched; 2 * levels + 5 launches on `stream` (a hipStream_t passed as void*, NULL = default stream), no allocation, no wait, no
 * read-back, graph-capturable.
 * Return value: 0 on success, non-zero on error (lc_amd_obox_last_error() gives the text).
 */
#ifndef LC_AMD_OBOX_H
#define LC_AMD_OBOX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_OBOX_VERSION 1
#define LC_OBOX_TILE 256
#define LC_OBOX_SPLIT 1024
#define LC_OBOX_MAX_LEVELS 16
#define LC_OBOX_MAX_CAND 65536
#define LC_OBOX_STEP0_DEG 9
#define LC_OBOX_GRID_RADIUS 7
#define LC_OBOX_LEVEL0_COUNT 1419
#define LC_OBOX_AXIS_LEVEL0_COUNT 10

int lc_amd_obox_version(void);
const char *lc_amd_obox_last_error(void);
const char *lc_amd_obox_source_hash(void);
size_t lc_obox_workspace_bytes(int n_meshes, int max_cand);
int lc_obox_search_f32(const float *verts, int total_verts, const int *table, const int *table_host, int n_meshes, int max_verts, const double *deltas,
                       int n_level0, int n_refine, int levels, float *xform, float *noc_scale, float *volume, float *aabb_volume, int *path,
                       int *info, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LC_AMD_OBOX_H */
