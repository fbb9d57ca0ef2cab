/*
 * lc_amd posedraw -- C ABI of the synthetic scenes' object poses drawn on the device (liblc_amd_posedraw.so, built from
 * lc_amd/csrc/posedraw/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  Per scene it forms the rotation and translation of up to LC_POSEDRAW_MAX_INSTANCES instances from
 * (configuration, seed word, scene id): rotations uniform on SO(3), positions drawn in a pixel box and a depth range and accepted by
 * rejection so that no two bounding spheres of a scene come nearer than `gap`.  The definition is lc_amd/posedraw.py
 * (`draw_scene_poses_host`), in host numpy; the kernel equals it bit for bit, so a captured graph of a whole synthetic scene changes with
 * one 64-bit word on the device.
 *
 * The launch: one wavefront of 64 per scene, lane k = try k of the slot being placed and lane m = the home of slot m's pose; 0 bytes of
 * LDS, no workspace, no atomics, no allocation, no wait: capturable in a hipGraph.  Every fp64 product, sum, difference, quotient and
 * square root is one IEEE operation rounded on its own, in the order written below (nothing is fused), every conversion to fp32 rounds
 * to nearest even, once.
 *
 * Random numbers: key(op, i) of include/lc_amd_augment.h, restated --
 *       f(v):  v ^= v >> 16;  v *= 0x85ebca6b;  v ^= v >> 13;  v *= 0xc2b2ae35;  v ^= v >> 16          (uint32, wrapping)
 *   k = f(seed & 0xffffffff);  k = f(k ^ (seed >> 32));  k = f(k ^ scene_id);  k = f(k ^ op);  key(op, i) = f(k ^ i)
 *   u(i) = (key(LC_POSEDRAW_OP_POSE, i) >> 8) / 2^24, exact in fp64
 * with seed the uint64 the DEVICE pointer `seed` names (aligned to 8 bytes), read by the kernel at every launch and replay, and the
 * sample the scene's id: a scene is the same in any batch.  LC_POSEDRAW_OP_POSE is the op code behind the sampler's two.
 * Draw d of try k of slot m is u((m LC_POSEDRAW_TRIES + k) 8 + d), written u_d(m, k) below.
 *
 * lc_posedraw_scenes_f32, for scene s (scene_id[s]) and slot m < M, with mi = mesh_index[s M + m]:
 *   info (S,M) int32, decided before anything is drawn:
 *     -3  mi == -1: an empty slot
 *     -2  a refused row: mi < -1 or mi >= n_meshes (an unknown mesh); r = radius[mi] widened to fp64 is not finite or negative;
 *         not (z_min - r > near) (the rasteriser would drop faces at the near plane); an entry of the scene's K that is not finite, or
 *         K00 == 0 or K11 == 0.  cam_K f32, scene s at cam_K + s K_stride (K_stride = 9, or 0: one camera serves all scenes), widened.
 *   Rotation of slot m, from u_0, u_1, u_2 of (m, 0) (it does not depend on the try), Shoemake's uniform quaternion:
 *     a = sqrt(1 - u_0), b = sqrt(u_0);  (c1, s1) and (c2, s2) = (cos, sin) of 2 pi u_1 and 2 pi u_2 by the polynomial of
 *     include/lc_amd_geometry.h at u / 2 (that polynomial takes the angle 4 pi x; x = u / 2 = n / 2^25 with n < 2^24 is reduced as exactly
 *     as u itself: tau = u, 8 tau = n / 2^21 and its fractional part hold 24 bits at the most);
 *     x = a s1, y = a c1, z = b s2, w = b c2;  the nine products xx, yy, zz, xy, xz, yz, wx, wy, wz;
 *     R = [ 1 - 2 (yy + zz)   2 (xy - wz)       2 (xz + wy)     ]
 *         [ 2 (xy + wz)       1 - 2 (xx + zz)   2 (yz - wx)     ]
 *         [ 2 (xz - wy)       2 (yz + wx)       1 - 2 (xx + yy) ]
 *   Position of slot m at try k, from u_3, u_4, u_5 of (m, k):
 *     px = x0 + u_3 (x1 - x0), py = y0 + u_4 (y1 - y0), z = z_min + u_5 (z_max - z_min)
 *     yn = (py - K12) / K11, xn = ((px - K02) - K01 yn) / K00;  p = (xn z, yn z, z)
 *   Placement, slots in order m = 0, 1, ...: try k is good when for every EARLIER PLACED slot j of the scene
 *     (dx dx + dy dy) + dz dz >= s s,  d = p_m,k - p_j,  s = (r_m + r_j) + gap,
 *   on the fp64 positions.  The slot takes the good try of lowest k: info = 0, tries = k.  Without a good try among the
 *   LC_POSEDRAW_TRIES: info = -1, tries = LC_POSEDRAW_TRIES, and the slot is left out of the scene (it blocks no later slot).
 *   Outputs: R (S,M,3,3) f32 and t (S,M,3) f32, the fp64 values rounded once; tries (S,M) int32 (0 for info -2 and -3);
 *   mesh_index_out (S,M) int32 = mi where info == 0, else -1: what the renderer is given, which refuses a row of -1.
 *   R and t of a slot that is not placed are zeros.
 *
 * Argument rules, checked before anything is launched: 0 <= S <= LC_POSEDRAW_MAX_SCENES (S = 0 launches nothing and returns 0);
 * 1 <= M <= LC_POSEDRAW_MAX_INSTANCES; n_meshes >= 1; the pointers are not NULL and aligned to their element; z_min <= z_max,
 * x0 <= x1, y0 <= y1, gap >= 0, all of them and near finite; K_stride is 0 or 9.
 * 0 on success, else lc_amd_posedraw_last_error().  `stream` is a hipStream_t as void*.
 */
#ifndef LC_AMD_POSEDRAW_H
#define LC_AMD_POSEDRAW_H

#include <stdint.h>

#define LC_AMD_POSEDRAW_VERSION 1
#define LC_POSEDRAW_MAX_INSTANCES 64
#define LC_POSEDRAW_TRIES 64
#define LC_POSEDRAW_MAX_SCENES 1048576
#define LC_POSEDRAW_OP_POSE 131088

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_posedraw_version(void);
const char *lc_amd_posedraw_last_error(void);
const char *lc_amd_posedraw_source_hash(void);

int lc_posedraw_scenes_f32(double z_min, double z_max, double x0, double y0, double x1, double y1, double gap, double near,
                           const uint64_t *seed, const int *scene_id, const int *mesh_index, const float *radius, int n_meshes,
                           const float *cam_K, int K_stride, int S, int M, float *R, float *t, int *tries, int *info,
                           int *mesh_index_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
