/*
 * lc_amd render -- C ABI of the depth-only rasteriser (liblc_amd_render.so, built from lc_amd/csrc/render/).
 *
 * A library of its own, next to liblc_amd.so, liblc_amd_optim.so and liblc_amd_posecov.so: no other ABI is changed by it.
 *
 * lc_render_depth_f32 renders, for every row b of a batch, the depth map of one triangle mesh under the pose (R_b, t_b) and the
 * camera matrix K_b (last row (0,0,1), upper 2x3 general):
 *     depth[b,y,x] = camera-space z of the nearest surface point on the ray through K-coordinates (x + cx, y + cy), near < z < far,
 *                    0 where nothing is hit.  No back-face culling: the nearest of all faces wins.
 * A face with any vertex at z <= near is dropped whole and counted in info[b] (there is no near-plane clipping); so is a face with a
 * vertex that projects further than 2^17 px from the origin (outside the range in which coverage is exact).
 *
 * Coverage is exact: vertices are transformed and projected in fp64, screen coordinates are snapped to multiples of 2^-8 px
 * (round-half-even), the sample points lie on that grid, and the three edge functions are integer-valued doubles below 2^53.  A
 * sample is covered when all three have the same sign or are zero; zero-area faces cover nothing.  1/z is interpolated with the
 * exact barycentric weights and z rounded once to fp32.  Per pixel the smallest (fp32 bits of z, face index) pair wins, so the
 * result does not depend on the order of evaluation.  near < z < far is tested per sample on that fp32 value: a face whose vertices
 * pass z > near in fp64 but whose z rounds onto near (or onto far) covers nothing there and is not counted.  A face with a vertex
 * index outside [0, n_vert) of its mesh covers nothing and is not counted either.
 *
 *   verts (total_verts,3) f32, faces (total_faces,3) int32: the meshes' arrays concatenated; face indices are relative to the mesh
 *   mesh_table (n_meshes,4) int32 on the device: vert_off, n_vert, face_off, n_face
 *   mesh_index (B) int32 on the device: the mesh of row b; a value outside [0, n_meshes), or a table entry that reaches outside the
 *                                       arrays or holds more than max_faces faces, renders nothing and sets info[b] = -1
 *   R (B,3,3)  t (B,3)  K (B,3,3)  f32
 *   pix2k (B,2,3) f32 or NULL: homo_z[b,y,x,:] = (p_x, p_y, 1) z with p = pix2k_b (x,y,1); NULL = [[1,0,cx],[0,1,cy]]
 *   depth (B,H,W) f32;  optional (NULL = not written): face (B,H,W) int32, -1 where nothing is hit; mask (B,H,W) bytes 0/1;
 *   homo_z (B,H,W,3) f32;  info (B) int32
 *   workspace: lc_render_workspace_bytes(B, max_faces) bytes, 16-byte aligned (one 64-byte record per row and face)
 * cx, cy must be multiples of 2^-8 in [-64, 64]; 1 <= H, W <= LC_RENDER_MAX_SIZE; near < far.  B == 0 launches nothing; max_faces == 0
 * fills the outputs with the miss values.  Two launches (face setup, tile raster), asynchronous on `stream` (hipStream_t as
 * void*), no allocation and no wait; 0 on success, else lc_amd_render_last_error().
 */
#ifndef LC_AMD_RENDER_H
#define LC_AMD_RENDER_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_RENDER_VERSION 1
#define LC_RENDER_MAX_SIZE 16384
#define LC_RENDER_RECORD_BYTES 64

int lc_amd_render_version(void);
const char *lc_amd_render_last_error(void);
const char *lc_amd_render_source_hash(void);

size_t lc_render_workspace_bytes(int B, int max_faces);

int lc_render_depth_f32(const float *verts, const int *faces, const int *mesh_table, const int *mesh_index, int n_meshes,
                        int total_verts, int total_faces, int max_faces, const float *R, const float *t, const float *K,
                        const float *pix2k, int B, int H, int W, float near, float far, float cx, float cy, float *depth,
                        int *face, unsigned char *mask, float *homo_z, int *info, void *workspace, size_t workspace_bytes,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif
