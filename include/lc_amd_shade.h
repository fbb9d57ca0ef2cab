/*
 * lc_amd shade -- C ABI of the shading pass behind the depth rasteriser (liblc_amd_shade.so, built from lc_amd/csrc/shade/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference draws with its vendored OpenGL renderer for the rendered, background-less
 * `imgn` split (tools/lib/meshrenderer/meshrenderer_phong.py:125-165, shader/depth_shader_phong.{vs,frag}; dataset.py:413): a
 * vertex-coloured mesh under a Phong model with exponent 1 and a one-sided normal, composited over whatever the frame held.  The
 * rasteriser (include/lc_amd_render.h) says which face a pixel sees, the scene composition (include/lc_amd_gtinfo.h) which instance; this
 * library turns that into uint8 bytes.  One sample per pixel: the silhouette is the rasteriser's.
 *
 * The meshes: `verts`, `faces` and `mesh_table` exactly as lc_render_depth_f32 takes them, and two per-vertex arrays aligned with
 * `verts`: normals (total_verts,3) f32 in model space and colors (total_verts,3) uint8.
 * Per row b: mesh_index (B) int32, R (B,3,3), t (B,3), K (B,3,3) f32 as the rasteriser takes them; light (B,3) f32, the light's position
 * in camera coordinates (x right, y down, z forward); phong (B,3) f32 = (ka, kd, ks); face (B,h,w) int32 as the rasteriser writes it.
 *
 * ONE HIT PIXEL (x, y) of row b with face f = (i0, i1, i2).  Every input is widened exactly to fp64, and EVERY product, sum, difference,
 * quotient and root below is one fp64 operation rounded on its own (nothing is fused); a sum of three is (a + b) + c.
 *   1. Xc_k[r] = ((R[r][0] V_k.x + R[r][1] V_k.y) + R[r][2] V_k.z) + t[r]             the camera-space vertices, z_k = Xc_k[2]
 *   2. u_k = ((K[0][0] Xc_k.x + K[0][1] Xc_k.y) + K[0][2] z_k) / z_k, v_k with K[1][.]; s_k = (rint(256 u_k), rint(256 v_k)), half to even:
 *      the rasteriser's snapped screen coordinates
 *   3. with a, b, c = s_0, s_1, s_2 and the sample (px, py) = (256 x + 256 cx, 256 y + 256 cy):
 *        w0 = (c.x - b.x)(py - b.y) - (c.y - b.y)(px - b.x)
 *        w1 = (a.x - c.x)(py - c.y) - (a.y - c.y)(px - c.x)
 *        w2 = (b.x - a.x)(py - a.y) - (b.y - a.y)(px - a.x)              integer-valued, exact wherever the rasteriser accepts the face
 *   4. q_k = w_k / z_k,  Q = (q0 + q1) + q2,  l_k = q_k / Q                             the perspective-correct weights
 *   5. (l0 a0 + l1 a1) + l2 a2 for every component of: the byte colour c (on the 0..255 scale), the model normal n, the point P = Xc
 *   6. m[r] = (R[r][0] n.x + R[r][1] n.y) + R[r][2] n.z,  N = m / |m|;  D = light - P,  L = D / |D|;  V = (-P) / |P|
 *      with |x| = sqrt((x.x x.x + x.y x.y) + x.z x.z); a length of zero makes that unit vector zero
 *   7. nl = (N.x L.x + N.y L.y) + N.z L.z,  d = nl where nl > 0 else 0;  Rv = (2 nl) N - L (per component: one product, one difference);
 *      rv = (Rv.x V.x + Rv.y V.y) + Rv.z V.z,  s = rv where rv > 0 else 0;  I = (ka + kd d) + ks s
 *   8. per channel v = I c: the byte is 255 where v >= 255, rint(v) (half to even) where v > 0, else 0 (a NaN gives 0)
 * Only hit pixels are written: a pixel that is not hit, or is refused, keeps the byte that was there.
 *
 * lc_shade_instances_u8: out (B,h,w,3) uint8.  Pixel (x, y) of row b is hit when 0 <= face[b,y,x] < n_face of the row's mesh; -1 is a
 * miss; any other value is refused.
 *
 * lc_shade_scene_u8: frames (S,H,W,3) uint8, in place; instance (S,H,W) int32 as lc_scene_compose_f32 writes it; origin_xy (B,2) int32 =
 * (x0, y0) of row b's (h,w) maps in the frame, anywhere, or NULL where (h,w) = (H,W); scene_index (B) int32.  Frame pixel (X, Y) of
 * scene s with b = instance[s,Y,X]: b = -1 is a miss; otherwise the pixel is that of row b at window pixel (X - x0_b, Y - y0_b), sampled at
 * (X - x0_b + cx, Y - y0_b + cy) in K_b's coordinates and shaded with row b's mesh, pose, K, light and phong.  One thread owns one frame
 * pixel: nothing is written twice.
 *
 * Refused on the device, each writing nothing:
 *   a row whose mesh_index lies outside [0, n_meshes) or whose table entry is negative or reaches outside the arrays: info[b] = -1
 *   a pixel whose face index lies outside [0, n_face) (but for the miss, -1, of the instance form), a face with a vertex index outside
 *   [0, n_vert), and in the scene form a window pixel outside (h,w) or a row b with scene_index[b] != s:     info[b] = 1
 *   an instance outside [0, B) other than -1: it names no row, so no row records it
 * info[b] = 0 for a row without any of these.  The kernels use no atomic operation and no workspace, so info says WHETHER a pixel of the
 * row was refused, not how many: the entry point clears info on the stream, and every thread that refuses a pixel stores the same 1.
 * Nothing out of bounds is ever read: every index is checked against the table, the counts and the sizes before it is used.
 *
 * Argument rules, checked before anything is launched: B >= 0 (B = 0 launches nothing and returns 0); n_meshes >= 1, total_verts >= 0,
 * total_faces >= 0; every pointer is required but origin_xy (and verts, normals, colors, faces where their count is 0);
 * 1 <= h, w, H, W <= LC_SHADE_MAX_SIZE and S >= 1; without origin_xy (h,w) = (H,W); cx, cy are multiples of 2^-8 in [-64, 64]; the f32
 * and int32 arrays are aligned to 4 bytes.  One memset node (info) and one launch on `stream` (hipStream_t as void*): no workspace, no
 * allocation, no atomics, no wait, capturable in a hipGraph.  0 on success, else lc_amd_shade_last_error().
 */
#ifndef LC_AMD_SHADE_H
#define LC_AMD_SHADE_H

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_SHADE_VERSION 1
#define LC_SHADE_MAX_SIZE 16384

int lc_amd_shade_version(void);
const char *lc_amd_shade_last_error(void);
const char *lc_amd_shade_source_hash(void);

int lc_shade_instances_u8(const float *verts, const float *normals, const unsigned char *colors, const int *faces, const int *mesh_table,
                          int n_meshes, int total_verts, int total_faces, const int *mesh_index, const float *R, const float *t,
                          const float *K, const float *light, const float *phong, const int *face, int B, int h, int w, float cx,
                          float cy, unsigned char *out, int *info, void *stream);

int lc_shade_scene_u8(const float *verts, const float *normals, const unsigned char *colors, const int *faces, const int *mesh_table,
                      int n_meshes, int total_verts, int total_faces, const int *mesh_index, const int *scene_index, const float *R,
                      const float *t, const float *K, const float *light, const float *phong, const int *face, const int *origin_xy,
                      int B, int h, int w, float cx, float cy, const int *instance, unsigned char *frames, int S, int H, int W,
                      int *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif
