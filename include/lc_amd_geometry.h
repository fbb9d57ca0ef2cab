/*
 * lc_amd geometry -- C ABI of the training crops' geometry drawn on the device (liblc_amd_geometry.so, built from
 * lc_amd/csrc/geometry/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference's loader computes per instance on a host core before it touches a pixel
 * (dataset.py:313-327,402-405,437,470: `_aug_bbox`, the rotation, the two `_get_affine_transform` matrices, `affine33 @ cam_K`,
 * `out_pix_scale`) and the stretch of `_switch_bg`'s region: the few numbers that every pixel stage of the loader consumes.  The
 * definition is lc_amd/geometry.py (`zoom_geometry_host`, `augment.background_matrices`), in host numpy; the kernels equal it bit for
 * bit, so a captured graph of the whole training input changes with one 64-bit word on the device.
 *
 * Both launches: one thread per sample in workgroups of 64, 0 bytes of LDS, no workspace, no atomics, no allocation, no wait: capturable
 * in a hipGraph.  Every fp64 product, sum, difference and quotient is one IEEE operation rounded on its own, in the order the definition
 * writes them (nothing is fused), every conversion to fp32 rounds to nearest even, once.
 *
 * Random numbers: key(op, i) of include/lc_amd_augment.h, restated --
 *       f(v):  v ^= v >> 16;  v *= 0x85ebca6b;  v ^= v >> 13;  v *= 0xc2b2ae35;  v ^= v >> 16          (uint32, wrapping)
 *   k = f(seed & 0xffffffff);  k = f(k ^ (seed >> 32));  k = f(k ^ sample_id);  k = f(k ^ op);  key(op, i) = f(k ^ i)
 *   u(op, i) = (key(op, i) >> 8) / 2^24, exact in fp64
 * with seed the uint64 the DEVICE pointer `seed` names (aligned to 8 bytes), read by the kernel at every launch and replay.
 *
 * lc_geometry_zoom_f32, for row b, with ZOOM = LC_GEOMETRY_OP_ZOOM and u_i = u(ZOOM, i):
 *   bbox_xyxy (B,4) f32 = (x1, y1, x2, y2) and cam_K f32, row b at cam_K + b K_stride (K_stride = 9, or 0: one camera serves all rows),
 *   widened to fp64.
 *   train != 0:  cx = 0.5 (x1 + x2), cy = 0.5 (y1 + y2), bw = x2 - x1, bh = y2 - y1
 *                ratio = 1 + dzi_scale_ratio (2 u_0 - 1)
 *                centre = (cx + bw (dzi_shift_ratio (2 u_1 - 1)),  cy + bh (dzi_shift_ratio (2 u_2 - 1)))
 *                scale = min((max(bh, bw) ratio) dzi_pad_scale, max(im_h, im_w))
 *                (c, s) = the polynomial below of u_4 where u_3 < rotate_prob, else (1, 0)
 *   train == 0:  centre = (cx, cy), scale = max(bw, bh, 1) dzi_pad_scale, (c, s) = (1, 0); nothing is drawn
 *   the matrix of a (dst_w, dst_h) target, k = dst_w / scale:
 *                [ k c      k s    dst_w / 2 - ((k c) centre_x + (k s) centre_y)    ]
 *                [ (-k) s   k c    dst_h / 2 - (((-k) s) centre_x + (k c) centre_y) ]
 *   in_affine (B,2,3) f32 with (in_w, in_h), out_affine (B,2,3) f32 with (out_w, out_h)
 *   out_K (B,3,3) f32: rows i = 0, 1 are (A[i][0] K[0][j] + A[i][1] K[1][j]) + A[i][2] K[2][j] with A the fp32 out_affine widened
 *                again; row 2 is K's
 *   out_pix_scale (B) f32 = scale / out_w
 *   step_id (B) int32 = key(ZOOM, 5) & 0x7fffffff: the sample id `lc_mask_crops_u8` takes for this step's check points
 *   info (B) int32: 0, or -1 for a REFUSED row: a non-finite entry of its box or K, or a scale that is not finite or <= 0.  Such a row
 *                holds quiet NaNs in every float output (centre and scale too; not cs); its step_id is written as ever.
 *   centre (B,2), scale (B), cs (B,2) f64, each or all NULL: for information.
 *
 * (c, s) of the angle 4 pi u_4:  tau = 2 u_4, f = tau - floor(tau), o = floor(8 f), g = 8 f - o, for odd o g <- 1 - g (all exact);
 *   a = g fl(pi / 4), z = a a;  S = a (1 + z (s3 + z (s5 + ... + z s17))), C = 1 + z (c2 + z (c4 + ... + z c16)) by Horner's rule from
 *   the highest coefficient down, one product and one sum per step, the coefficients (-1)^(k/2) / k! rounded to fp64;
 *   (c, s) = (C,S) (S,C) (-S,C) (-C,S) (-C,-S) (-S,-C) (S,-C) (C,-S) for o = 0 .. 7.  No library sine or cosine is called.
 *
 * lc_geometry_background_f32, for row b, with r_i = u(LC_GEOMETRY_OP_BG_REGION, i): the background of (hb, wb) pixels -- the pair
 *   (bg_h, bg_w) by value where bg_hw is NULL, else bg_hw (B,2) int32 on the device -- stretched over a crop of (out_h, out_w), in
 *   64-bit integers but for the products with r_i:
 *   roi_w = max(trunc(r_0 wb), out_w), roi_h = max(trunc(r_1 hb), out_h)
 *   left = min(max(trunc(r_2 (wb - roi_w)), 0), wb), top = min(max(trunc(r_3 (hb - roi_h)), 0), hb)
 *   rw = max(min(left + left + roi_w, wb) - left, 1), rh = max(min(top + roi_h, hb) - top, 1)
 *   M (B,2,3) f32 = [ out_w / rw, 0, (0.5 - left)(out_w / rw) - 0.5 ;  0, out_h / rh, (0.5 - top)(out_h / rh) - 0.5 ]
 *   (`augment.background_matrices`: the matrix `lc_crop_warp_u8` takes to cut the region).  No row is refused: no value of bg_hw can
 *   make a quotient's divisor less than 1.
 *
 * Argument rules, checked before anything is launched: B >= 0 (B = 0 launches nothing and returns 0); the required pointers are not
 * NULL and aligned to their element; 1 <= every size (im_h, im_w, in_w, in_h, out_w, out_h, and bg_h, bg_w where bg_hw is NULL) <=
 * LC_GEOMETRY_MAX_SIZE, the bound of lc_amd_crop.h; the three dzi ratios are finite; 0 <= rotate_prob <= 1; K_stride is 0 or 9.
 * 0 on success, else lc_amd_geometry_last_error().  `stream` is a hipStream_t as void*.
 */
#ifndef LC_AMD_GEOMETRY_H
#define LC_AMD_GEOMETRY_H

#include <stdint.h>

#define LC_AMD_GEOMETRY_VERSION 1
#define LC_GEOMETRY_MAX_SIZE 16384
#define LC_GEOMETRY_OP_BG_REGION 131084
#define LC_GEOMETRY_OP_ZOOM 131085
#define LC_GEOMETRY_STEP_INDEX 5

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_geometry_version(void);
const char *lc_amd_geometry_last_error(void);
const char *lc_amd_geometry_source_hash(void);

int lc_geometry_zoom_f32(double dzi_scale_ratio, double dzi_shift_ratio, double dzi_pad_scale, double rotate_prob, int train, int im_h,
                         int im_w, int in_w, int in_h, int out_w, int out_h, const uint64_t *seed, const int *sample_id,
                         const float *bbox_xyxy, const float *cam_K, int K_stride, int B, float *in_affine, float *out_affine,
                         float *out_K, float *out_pix_scale, int *step_id, int *info, double *centre, double *scale, double *cs,
                         void *stream);

int lc_geometry_background_f32(const uint64_t *seed, const int *sample_id, int bg_h, int bg_w, const int *bg_hw, int out_h, int out_w,
                               int B, float *M, void *stream);

#ifdef __cplusplus
}
#endif

#endif
