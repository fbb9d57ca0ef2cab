/*
 * lc_amd vsd -- C ABI of BOP's Visible Surface Discrepancy from depth maps (liblc_amd_vsd.so, built from lc_amd/csrc/vsd/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.
 *
 * lc_vsd_score_f32 restates BOP's pose_error.vsd with visib_mode = 'bop19' and cost_type = 'step' in fixed arithmetic.  For pose b:
 *   depth_est, depth_gt (B,h,w) f32: the object's depth under the estimated and the ground-truth pose, 0 (anything not > 0) = no hit
 *   depth_test (S,H,W) f32: the scenes' measured depth in the same unit, !(d > 0) = no measurement;  scene_index (B) int32: pose b's scene
 *   K (B,3,3) f32: the camera; K00, K01, K02, K11, K12 are read (skew allowed, K10 = 0 assumed, last row (0,0,1))
 *   (pcx, pcy): the pixel centre;  window_xy (B,2) int32 = (x0, y0): where the (h,w) maps lie in the frame; NULL: (0,0) and h,w = H,W
 *   diameter (B) f32 or NULL (= 1);  taus: T <= LC_VSD_MAX_TAUS f32 on the HOST, passed to the kernel by value;  delta f32
 * All arithmetic is fp64 on the exactly widened fp32 inputs, every product, sum, quotient and root rounded on its own (no fused
 * multiply-add):
 *   1. ray length at array pixel (x,y):  px = (x + x0) + pcx - K02,  py = (y + y0) + pcy - K12,  Y = py / K11,  X = (px - K01 Y) / K00,
 *      n = sqrt(X X + Y Y + 1) with the sum taken as (X X + Y Y) + 1.  The distance of a depth z is z n; one n serves the three maps.
 *   2. vis_gt  = d_gt > 0  and (test missing or dist_gt - dist_test <= delta)
 *   3. vis_est = d_est > 0 and (test missing or dist_est - dist_test <= delta or vis_gt)
 *   4. union = #(vis_gt or vis_est),  inter = #(vis_gt and vis_est),
 *      cost_k = #(inter pixels with |dist_gt - dist_est| >= tau_k diameter_b), the product formed in fp64 from the two fp32 values
 *   5. e_k = (cost_k + union - inter) / union, formed in fp64 from the integers and rounded to fp32 once;  e_k = 1 when union = 0
 *   edge = #(pixels of the window's border with d_est > 0 or d_gt > 0, on a side of the window that is not also the frame's border):
 *      non-zero means the window may have cut the object.  Always 0 without a window.
 * Two deliberate differences from BOP's Python: it rounds the distance images to fp32 before it subtracts, here the differences stay
 * fp64; and cost_type = 'tlinear' (a sum of floats, whose result depends on the order of summation) is not built.
 *
 *   -> counts (B, T+3) int32 = union, inter, edge, cost_0 .. cost_{T-1};  errors (B,T) f32.
 * Every count is an integer sum: the results are the same bits for any batch, order, grid shape and launch.
 * A pose whose scene_index lies outside [0,S), or whose window reaches outside the frame (x0 < 0, y0 < 0, x0 + w > W, y0 + h > H), is
 * refused on the device: counts = -1, errors = NaN, and none of its maps is read.  Nothing out of bounds is read.
 * 1 <= T <= LC_VSD_MAX_TAUS; 1 <= h <= H, 1 <= w <= W <= LC_VSD_MAX_SIZE; S >= 1; h,w = H,W without a window; pointers 4-byte aligned
 * (16-byte loads are used on the rows where all three maps allow them).  B = 0 launches nothing.  Three launches (zero the counts,
 * count, finish) on `stream` (hipStream_t as void*): no allocation, no workspace, no wait, capturable in a hipGraph.
 * Returns 0, or non-zero with the reason in lc_amd_vsd_last_error().
 */
#ifndef LC_AMD_VSD_H
#define LC_AMD_VSD_H

#include <stddef.h>

#define LC_AMD_VSD_VERSION 1
#define LC_VSD_MAX_TAUS 16
#define LC_VSD_MAX_SIZE 16384

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_vsd_version(void);
const char *lc_amd_vsd_last_error(void);
const char *lc_amd_vsd_source_hash(void);

int lc_vsd_score_f32(const float *depth_est, const float *depth_gt, const float *depth_test, const int *scene_index, const float *K,
                     const float *diameter, const float *taus, int T, float delta, const int *window_xy, int B, int h, int w, int S,
                     int H, int W, float pcx, float pcy, int *counts, float *errors, void *stream);

#ifdef __cplusplus
}
#endif

#endif
