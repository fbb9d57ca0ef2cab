/*
 * lc_amd texture -- C ABI of the textured shading pass behind the depth rasteriser (liblc_amd_texture.so, built from lc_amd/csrc/texture/).
 *
 * A library of its own, next to liblc_amd_shade.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  It is include/lc_amd_shade.h's pass with one change: where a mesh has a texture, the albedo of a pixel
 * is sampled from that texture at the pixel's interpolated texture coordinates instead of being interpolated from the vertex colours.  What
 * the object sets that ship a PLY with texture coordinates and a texture image need (the reference reads such models with
 * tools/lib/pysixd/inout.py:505-617); images are decoded by the caller.
 *
 * THE TEXTURE STORE.  `texels`: one buffer of 4-byte texels (R, G, B, 0), aligned to 4 bytes, total_texels of them.  tex_table (n_tex,4)
 * int64: per texture the offset of level 0 in texels, Ht, Wt and n_levels.  Level L+1 lies directly behind level L, rows top to bottom as
 * the image was given, H_{L+1} = max(1, H_L >> 1) and W likewise.  An entry is valid when offset >= 0, 1 <= Ht, Wt <= LC_TEX_MAX_SIZE,
 * 1 <= n_levels <= LC_TEX_MAX_LEVELS and offset + sum over its levels of H_L W_L <= total_texels.
 *
 * lc_tex_build_mips_u8 writes the levels 1 .. n_levels-1 of every texture from its level 0, on the device: per channel, texel (x, y) of
 * level L+1 is (c(x0,y0) + c(x1,y0) + c(x0,y1) + c(x1,y1) + 2) >> 2 read from level L with x0 = min(2x, W_L-1), x1 = min(2x+1, W_L-1) and
 * the same for y; the fourth byte is 0.  Integers: no order of evaluation matters.  Here tex_table is a HOST array, read before anything
 * is launched: an invalid entry is refused with nothing launched.  One launch per level and texture on `stream`, no wait, no allocation.
 *
 * THE MESHES: verts, normals, colors, faces, mesh_table as lc_shade_instances_u8 takes them, and two more arrays: uv (total_faces,3,2)
 * f32, the texture coordinates of every face CORNER, aligned with `faces` (so that two faces may give a shared vertex different
 * coordinates: a seam); tex_index (n_meshes) int32, the mesh's texture, or -1: the mesh has none and its pixels are exactly
 * include/lc_amd_shade.h's.  The rows: mesh_index, R, t, K, light, phong, face as there, and wrap (B) int32: 0 clamps texel indices to
 * the level, 1 repeats the texture.  lod (0 or 1) is one value per call.
 *
 * ONE HIT PIXEL of row b whose mesh has texture T = (offset, Ht, Wt, n_levels).  Steps 1 to 4 and 6 to 8 are include/lc_amd_shade.h's,
 * word for word: everything is widened exactly to fp64, every operation is one fp64 operation rounded on its own (nothing is fused), a sum
 * of three is (a + b) + c.  In step 5 the normal n and the point P are interpolated as there; the albedo c is:
 *   5a. U = (l0 u_0 + l1 u_1) + l2 u_2 and V likewise from the face's three corner coordinates (u_k, v_k), with the weights l_k of step 4.
 *   5b. the level.  lod = 0: level 0.  lod = 1: steps 3 and 4 are repeated at the samples (px + 256, py) and (px, py + 256) -- the edge
 *       expressions are affine and stay exact integers -- giving (U_x, V_x) and (U_y, V_y).  dux = (U_x - U) Wt, dvx = (V_x - V) Ht (the
 *       level-0 sizes), rho2x = dux dux + dvx dvx, rho2y likewise from the y sample, rho2 = rho2x where rho2x > rho2y else rho2y.
 *       level = the number of L in 1 .. n_levels-1 with rho2 > 2^(2L-1): comparisons with exact powers of two, no logarithm.  A NaN
 *       compares false (level 0 where rho2 is NaN; a NaN rho2x leaves rho2y); +inf selects the last level.
 *   5c. the texel coordinates at that level's (HL, WL): tx = U WL - 0.5, ty = (1 - V) HL - 0.5 (one product, one difference; 1 - V is an
 *       operation of its own).  v = 0 is the LAST row of the stored image: OpenGL's convention for an image loaded top row first; a caller
 *       who wants the other one passes 1 - v.  x0 = floor(tx), a8 = floor(256 (tx - x0)), and y0, b8 likewise (a8, b8 in 0 .. 256).
 *       The indices x0, x0 + 1, y0, y0 + 1 are clamped to the level (wrap 0) or taken floor-modulo its size (wrap 1).
 *   5d. per channel, in integers: c16 = (256-a8)(256-b8) c00 + a8 (256-b8) c10 + (256-a8) b8 c01 + a8 b8 c11 with c_ij the texel at
 *       (x_i, y_j); c = c16 / 65536, exact in fp64, on the 0..255 scale.
 * ONE level is sampled, bilinearly (OpenGL's GL_LINEAR_MIPMAP_NEAREST): there is no trilinear blend between levels and no anisotropic
 * filter, and one sample per pixel.  Only hit pixels are written: a pixel that is not hit, or is refused, keeps the byte that was there.
 *
 * lc_texshade_instances_u8: out (B,h,w,3) uint8; the hit rule of lc_shade_instances_u8.
 * lc_texshade_scene_u8: frames (S,H,W,3) uint8 in place, with instance, origin_xy and scene_index exactly as lc_shade_scene_u8 takes them.
 *
 * Refused on the device, each writing nothing:
 *   a row whose mesh_index lies outside [0, n_meshes) or whose mesh entry is negative or reaches outside the arrays; whose mesh's tex_index
 *   lies outside [-1, n_tex); whose texture's table entry is invalid (above); whose wrap is neither 0 nor 1:               info[b] = -1
 *   every pixel lc_amd_shade.h refuses (a face or vertex index outside its mesh; in the scene form a window pixel outside (h,w) or a row
 *   of another scene), and a textured pixel whose U or V is not finite or whose |tx| or |ty| >= 2^30:                       info[b] = 1
 *   an instance outside [0, B) other than -1: it names no row, so no row records it
 * info[b] = 0 for a row without any of these; it says WHETHER, not how many (no atomics: every writer stores the same value).
 * Nothing out of bounds is ever read: every index is checked against the tables, the counts and the sizes before it is used, and a texel
 * index is clamped or reduced into its level, which the entry's check has placed inside the buffer.
 *
 * Argument rules, checked before anything is launched: those of lc_amd_shade.h (B = 0 launches nothing and returns 0), and: uv is required
 * where total_faces > 0, tex_index and wrap always; n_tex >= 0 and total_texels >= 0; texels and tex_table are required where n_tex > 0;
 * uv, tex_index, wrap and texels are aligned to 4 bytes, tex_table to 8; lod is 0 or 1.  One memset node (info) and one launch on
 * `stream` (hipStream_t as void*): no workspace, no allocation, no atomics, no wait, capturable in a hipGraph.  0 on success, else
 * lc_amd_texture_last_error().
 */
#ifndef LC_AMD_TEXTURE_H
#define LC_AMD_TEXTURE_H

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_TEXTURE_VERSION 1
#define LC_TEX_MAX_SIZE 16384
#define LC_TEX_MAX_LEVELS 15 /* 16384 = 2^14: levels 0 .. 14 */

int lc_amd_texture_version(void);
const char *lc_amd_texture_last_error(void);
const char *lc_amd_texture_source_hash(void);

int lc_tex_build_mips_u8(unsigned char *texels, long long total_texels, const long long *tex_table_host, int n_tex, void *stream);

int lc_texshade_instances_u8(const float *verts, const float *normals, const unsigned char *colors, const int *faces, const float *uv,
                             const int *mesh_table, const int *tex_index, int n_meshes, int total_verts, int total_faces,
                             const unsigned char *texels, const long long *tex_table, int n_tex, long long total_texels,
                             const int *mesh_index, const float *R, const float *t, const float *K, const float *light, const float *phong,
                             const int *wrap, const int *face, int B, int h, int w, float cx, float cy, int lod, unsigned char *out,
                             int *info, void *stream);

int lc_texshade_scene_u8(const float *verts, const float *normals, const unsigned char *colors, const int *faces, const float *uv,
                         const int *mesh_table, const int *tex_index, int n_meshes, int total_verts, int total_faces,
                         const unsigned char *texels, const long long *tex_table, int n_tex, long long total_texels, const int *mesh_index,
                         const int *scene_index, const float *R, const float *t, const float *K, const float *light, const float *phong,
                         const int *wrap, const int *face, const int *origin_xy, int B, int h, int w, float cx, float cy, int lod,
                         const int *instance, unsigned char *frames, int S, int H, int W, int *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif
