/*
 * lc_amd maskcrop -- C ABI of the training mask crops (liblc_amd_maskcrop.so, built from lc_amd/csrc/maskcrop/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference's loader makes per instance from the visible mask on a host core
 * (dataset.py:414,425-442: three cv2.warpAffine calls of a float 0/1 mask, the count of valid pixels, 256 check points drawn with
 * np.random), from the byte masks lc_gtinfo_f32 leaves on the device, in integer arithmetic.
 *
 * lc_mask_crops_u8, for row b of the batch:
 *   masks (F,Hm,Wm) uint8: non-zero = set;  mask_index (B) int32 or NULL: row b reads mask b
 *   origin_xy (B,2) int32 = (x0, y0) or NULL (0,0): where the (Hm,Wm) window lies in the frame, lc_gtinfo_f32's convention; it may be
 *      negative.  Frame pixel (X,Y) reads window pixel (X - x0, Y - y0); anything outside the window reads 0, each tap judged on its own
 *   M (B,2,3) f32: the forward matrix frame -> crop (what cv2.warpAffine takes)
 *   h, w: the crop;  vis_interp: LC_MASKCROP_NEAREST or LC_MASKCROP_LINEAR;  valid_th, n_check (0: no check points; at most
 *      LC_MASKCROP_MAX_CHECK);  seed (uint64, by value);  sample_id (B) int32 or NULL (row b is sample b)
 *
 * Coordinates: exactly those of lc_amd_crop.h (one copy on the device, csrc/shared/lc_warp_grid.h).  M widened to fp64, every product and sum rounded on its own:
 *     D = M00 M11 - M01 M10;  D = D != 0 ? 1 / D : 0
 *     m00 = M11 D   m01 = -M01 D   m10 = -M10 D   m11 = M00 D      b1 = -m00 M02 - m01 M12      b2 = -m10 M02 - m11 M12
 *   crop pixel (x, y); rint is round-half-even, every rint result is clamped to +-2^30, the sums are 64-bit:
 *     X = rint((m01 y + b1) 1024) + rint(m00 x 1024) + d
 *     Y = rint((m11 y + b2) 1024) + rint(m10 x 1024) + d          d = 512 (nearest), 16 (linear)
 *   nearest: the tap is (X >> 10, Y >> 10)
 *   linear:  X >>= 5, Y >>= 5;  sx = X >> 5, fx = X & 31 (the same for y); the taps are (sx, sy), (sx+1, sy), (sx, sy+1), (sx+1, sy+1)
 *
 * Outputs (each may be NULL and is then not written):
 *   msk_vis (B,h,w) f32.  linear: k / 1024 with k = sum over the four taps of a b [S != 0], a in {32 - fx, fx}, b in {32 - fy, fy};
 *      there is no + 512 and no shift: k is an integer in 0..1024 and k / 1024 is exact in fp32.  It is what OpenCV's float path gives for
 *      a float 0/1 mask (float table weights (32-fx)(32-fy)/1024 and the like, summed in fp32: every step exact).  nearest: 0 or 1
 *   msk_noc (B,h,w) bytes 0 / 1: the nearest tap is set
 *   valid_cnt (B) int32: the number of set pixels of msk_noc
 *   sym_ck (B,n_check,2) of ck_dtype (LC_MASKCROP_I32, or LC_MASKCROP_I64 for readers that index with 64-bit integers): (x, y) in crop pixels
 *   info (B) int32: 0, or -1 for a row with a non-finite M, a mask_index outside [0,F), or an origin with |x0| or |y0| >
 *      LC_MASKCROP_MAX_ORIGIN (the bound of lc_gtinfo_f32).  Such a row is written as all zero with valid_cnt 0 and check points -1, and
 *      nothing of the masks is read for it.
 *
 * Check points: the semantics of dataset.py:432-442, made reproducible.
 *   If valid_cnt < valid_th, or valid_cnt is 0, every entry is -1.  Otherwise the output is the concatenation of rounds r = 0, 1, ...;
 *   round r lists the valid pixels sorted by the pair (key_r(p), p), p = y w + x, truncated to what is still missing from n_check.
 *   Each round is a uniform draw without replacement in random order, as np.random.choice(valid_cnt, m, replace=False) is.
 *   key_r(p), in uint32 arithmetic (wrapping products), with f = MurmurHash3's 32-bit finaliser
 *       f(v):  v ^= v >> 16;  v *= 0x85ebca6b;  v ^= v >> 13;  v *= 0xc2b2ae35;  v ^= v >> 16
 *   applied once per input word:
 *       k = f(seed & 0xffffffff);  k = f(k ^ (seed >> 32));  k = f(k ^ sample_id);  k = f(k ^ r);  key_r(p) = f(k ^ p)
 *   It depends on nothing else: not on B, the row's place in the batch, the grid shape or valid_cnt.  The same sample with the same seed
 *   gets the same points in any batch.  With n_check > 0, h w <= LC_MASKCROP_MAX_CHECK_PIXELS (p fits 16 bits); a larger crop is refused.
 *
 * Workspace: the check points read msk_noc and valid_cnt; where n_check > 0 and one of them is NULL, it lives in the caller's
 * workspace of lc_mask_crops_workspace_bytes(B, h, w, n_check, msk_noc != NULL, valid_cnt != NULL) bytes, 4-byte aligned (0 bytes: NULL will do).
 * 1 <= Hm, Wm, h, w <= LC_MASKCROP_MAX_SIZE; F >= 0.  M, the int32 arrays, msk_vis and sym_ck must be aligned to their element.  No
 * input value can make a launch read or write outside its arrays.  B = 0 launches nothing.  At most three launches (zero the counts,
 * warp, check points) on `stream` (hipStream_t as void*): no allocation, no wait, capturable in a hipGraph.  Every output is an integer,
 * or an integer over 1024: the same bits for any batch, order and grid shape.  0 on success, else lc_amd_maskcrop_last_error().
 */
#ifndef LC_AMD_MASKCROP_H
#define LC_AMD_MASKCROP_H

#include <stddef.h>
#include <stdint.h>

#define LC_AMD_MASKCROP_VERSION 1
#define LC_MASKCROP_MAX_SIZE 16384
#define LC_MASKCROP_MAX_ORIGIN 16777216
#define LC_MASKCROP_MAX_CHECK 256
#define LC_MASKCROP_MAX_CHECK_PIXELS 65536

#define LC_MASKCROP_NEAREST 0
#define LC_MASKCROP_LINEAR 1

#define LC_MASKCROP_I32 0
#define LC_MASKCROP_I64 1

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_maskcrop_version(void);
const char *lc_amd_maskcrop_last_error(void);
const char *lc_amd_maskcrop_source_hash(void);

size_t lc_mask_crops_workspace_bytes(int B, int h, int w, int n_check, int has_msk_noc, int has_valid_cnt);
int lc_mask_crops_u8(const unsigned char *masks, int F, int Hm, int Wm, const int *mask_index, const int *origin_xy, const float *M, int B,
                     int h, int w, int vis_interp, int valid_th, int n_check, uint64_t seed, const int *sample_id, int ck_dtype,
                     float *msk_vis, unsigned char *msk_noc, int *valid_cnt, void *sym_ck, int *info, void *workspace,
                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
