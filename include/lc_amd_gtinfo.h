/*
 * lc_amd gtinfo -- C ABI of BOP's ground-truth visibility annotations from depth maps (liblc_amd_gtinfo.so, built from
 * lc_amd/csrc/gtinfo/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the BOP toolkit's calc_gt_masks.py and calc_gt_info.py write per instance (mask_visib,
 * px_count_all / _valid / _visib, bbox_obj, bbox_visib) from one render of the instance and the scene's depth, in fixed arithmetic.
 *
 * lc_gtinfo_f32, for instance b:
 *   depth_gt (B,h,w) f32: the instance's render, 0 (anything not > 0, NaN included) = no hit
 *   origin_xy (B,2) int32 = (x0, y0) or NULL: where the (h,w) window lies in the (H,W) frame.  It may be negative and the window may reach
 *      outside the frame or be larger than it (BOP's 3H x 3W render of a truncated object is origin (-W,-H) with h,w = 3H,3W).
 *      NULL: origin (0,0) and h,w = H,W
 *   depth_test (S,H,W) f32: the scenes' depth in the same unit, !(d > 0) = no measurement;  scene_index (B) int32: instance b's scene
 *   K (B,3,3) f32: the camera; K00, K01, K02, K11, K12 are read (skew allowed, K10 = 0 assumed, last row (0,0,1))
 *   (pcx, pcy): the pixel centre;  delta f32: the visibility tolerance
 * Window pixel (x,y) is frame pixel (X,Y) = (x + x0, y + y0).  obj = d_gt > 0.  Where (X,Y) lies in the frame (0 <= X < W, 0 <= Y < H):
 *   1. ray length, fp64 on the exactly widened fp32 inputs, every product, sum, quotient and root rounded on its own (no fused
 *      multiply-add):  px = X + pcx - K02,  py = Y + pcy - K12,  Yk = py / K11,  Xk = (px - K01 Yk) / K00,
 *      n = sqrt(Xk Xk + Yk Yk + 1) with the sum taken as (Xk Xk + Yk Yk) + 1  (steps 1 and 2 of lc_amd_vsd.h; one copy on the device, csrc/shared/lc_ray_length.h)
 *   2. valid = obj and d_test > 0
 *      visib = obj and (test missing or d_gt n - d_test n <= delta), the two products and the difference formed in fp64
 * Outside the frame a pixel is obj at most: neither valid nor visible, and nothing of depth_test is read for it.
 *
 *   -> info (B,12) int32:
 *        0  px_count_all    #obj over the whole window
 *        1  px_count_valid  #valid
 *        2  px_count_visib  #visib
 *        3  edge            #obj on the window's outermost rows and columns (y = 0, y = h-1, x = 0, x = w-1; a pixel counts once):
 *                           non-zero means the window may have cut the silhouette, and columns 0 and 4-7 are then lower bounds
 *        4-7   x_min, y_min, x_max, y_max of obj, inclusive, in FRAME coordinates (they may lie outside the frame)
 *        8-11  x_min, y_min, x_max, y_max of visib, inclusive, in frame coordinates
 *      An empty box is four times -1; the count beside it (column 0, column 2) tells an empty box from a real -1 coordinate.
 *      How the counts become BOP's records (both boxes are [-1,-1,-1,-1] when px_count_visib = 0; width = x_max - x_min as the BOP
 *      toolkit forms it, or + 1) is lc_amd.gtinfo.bop_records: a rule of this project's, on the host, not of this library.
 *   -> mask_visib (B,h,w) bytes 0 / 1 or NULL (not written): visib in WINDOW coordinates, 0 outside the frame
 * A row whose scene_index lies outside [0,S), or whose origin has |x0| or |y0| > LC_GTINFO_MAX_ORIGIN (frame coordinates stay far from
 * the int32 range), is refused on the device: its info is -1 throughout, its mask row 0, and neither of its maps is read.
 * Nothing out of bounds is read.  Every output is an integer sum, minimum or maximum: the same bits for any batch, order and grid shape.
 * S >= 1; 1 <= H, W <= LC_GTINFO_MAX_FRAME; 1 <= h, w <= LC_GTINFO_MAX_WINDOW; h,w = H,W without an origin; every pointer but mask_visib
 * 4-byte aligned (16-byte loads are used on the rows where both maps allow them, 4-byte stores of the mask where it allows them).
 * B = 0 launches nothing.  Three launches (set the identities, reduce, finish) on `stream` (hipStream_t as void*): no allocation, no
 * workspace, no wait, capturable in a hipGraph.  A workgroup reduces a tile of LC_GTINFO_TILE_H window rows by LC_GTINFO_TILE_W pixels.
 *
 * lc_scene_compose_f32: a scene's depth from its instances' renders, for scenes without a measured depth.
 *   depth_inst (B,h,w) f32, origin_xy (B,2) int32 or NULL, scene_index (B) int32: as above
 *   -> depth (S,H,W) f32: at every frame pixel the z of the smallest pair (fp32 bits of z, row b) over the rows of that scene whose
 *      window covers the pixel with 0 < z < inf, 0 where there is none (the renderer's own tie rule: the result depends on no order)
 *   -> instance (S,H,W) int32 or NULL: the winning row, -1 where nothing is hit
 *   -> info (B) int32: 0, or -1 for a row that is skipped (scene_index outside [0,S), an origin beyond LC_GTINFO_MAX_ORIGIN)
 * Window parts outside the frame are ignored.  workspace: lc_scene_compose_workspace_bytes(S,H,W) bytes, 8-byte aligned, the caller's;
 * three launches (fill it, one 64-bit unsigned atomic minimum per covered pixel, split it into the two maps).  The size limits and the
 * rules on allocation, waiting and capture are those of lc_gtinfo_f32.  B = 0 still writes the empty maps.
 * Both return 0, or non-zero with the reason in lc_amd_gtinfo_last_error().
 */
#ifndef LC_AMD_GTINFO_H
#define LC_AMD_GTINFO_H

#include <stddef.h>

#define LC_AMD_GTINFO_VERSION 1
#define LC_GTINFO_COLUMNS 12
#define LC_GTINFO_MAX_FRAME 16384
#define LC_GTINFO_MAX_WINDOW 49152
#define LC_GTINFO_MAX_ORIGIN 16777216
#define LC_GTINFO_TILE_W 256
#define LC_GTINFO_TILE_H 16

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_gtinfo_version(void);
const char *lc_amd_gtinfo_last_error(void);
const char *lc_amd_gtinfo_source_hash(void);

int lc_gtinfo_f32(const float *depth_gt, const int *origin_xy, const float *depth_test, const int *scene_index, const float *K, int B,
                  int h, int w, int S, int H, int W, float pcx, float pcy, float delta, int *info, unsigned char *mask_visib,
                  void *stream);

size_t lc_scene_compose_workspace_bytes(int S, int H, int W);
int lc_scene_compose_f32(const float *depth_inst, const int *origin_xy, const int *scene_index, int B, int h, int w, int S, int H, int W,
                         float *depth, int *instance, int *info, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
