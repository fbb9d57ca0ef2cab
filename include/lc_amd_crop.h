/*
 * lc_amd crop -- C ABI of the zoom-in crops (liblc_amd_crop.so, built from lc_amd/csrc/crop/).
 *
 * A library of its own, next to liblc_amd.so, liblc_amd_optim.so, liblc_amd_posecov.so and liblc_amd_render.so: no other ABI is
 * changed by it.
 *
 * lc_crop_warp_u8 warps, for every row b of a batch, one uint8 frame with the forward matrix M_b (source -> crop, what
 * cv2.warpAffine takes) into an (h, w) crop, in OpenCV's published fixed-point scheme for 8-bit images (INTER_BITS = 5,
 * AB_BITS = 10, constant border 0).  All of it is integer arithmetic once the inverse matrix is formed:
 *
 *   inverse, M widened to fp64, every product and sum rounded on its own:
 *     D = M00 M11 - M01 M10;  D = D != 0 ? 1 / D : 0
 *     m00 = M11 D   m01 = -M01 D   m10 = -M10 D   m11 = M00 D
 *     b1 = -m00 M02 - m01 M12      b2 = -m10 M02 - m11 M12
 *   coordinates of crop pixel (x, y); rint is round-half-even, every rint result is clamped to +-2^30, the sums are 64-bit:
 *     X = rint((m01 y + b1) 1024) + rint(m00 x 1024) + d
 *     Y = rint((m11 y + b2) 1024) + rint(m10 x 1024) + d          d = 512 (nearest), 16 (linear)
 *   nearest: the tap is (X >> 10, Y >> 10)
 *   linear:  X >>= 5, Y >>= 5;  sx = X >> 5, fx = X & 31 (the same for y);
 *            v = (sum over the four taps of a b S + 512) >> 10 with a in {32 - fx, fx}, b in {32 - fy, fy}
 *   a tap outside the frame reads 0, each tap judged on its own.
 *
 *   frames (F,H,W,C) uint8, C in {1, 3}
 *   frame_index (B) int32 on the device, or NULL: row b reads frame b
 *   M (B,2,3) f32 on the device
 *   mean, std: HOST arrays of C floats, read during the call (they travel as kernel arguments), or both NULL
 *   out (B,C,h,w) of out_dtype: LC_CROP_U8 holds v; the float types hold v / 255 (IEEE fp32 division), with mean / std
 *       (v / 255 - mean_c) / std_c (two more fp32 operations); a 16-bit output is rounded once, from fp32.  mean / std need a float type.
 *   info (B) int32 or NULL: 0, or -1 for a row whose M has a non-finite entry or whose frame index lies outside [0, F); such a
 *       row is written as all border (v = 0 everywhere).
 * 1 <= H, W, h, w <= LC_CROP_MAX_SIZE.  No input value can make the launch read or write outside its arrays.  B == 0 launches
 * nothing.  One launch, asynchronous on `stream` (hipStream_t as void*), no workspace, no allocation and no wait; 0 on success,
 * else lc_amd_crop_last_error().
 */
#ifndef LC_AMD_CROP_H
#define LC_AMD_CROP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_CROP_VERSION 1
#define LC_CROP_MAX_SIZE 16384

#define LC_CROP_NEAREST 0
#define LC_CROP_LINEAR 1

#define LC_CROP_U8 0
#define LC_CROP_F32 1
#define LC_CROP_F16 2
#define LC_CROP_BF16 3

int lc_amd_crop_version(void);
const char *lc_amd_crop_last_error(void);
const char *lc_amd_crop_source_hash(void);

int lc_crop_warp_u8(const unsigned char *frames, int F, int H, int W, int C, const int *frame_index, const float *M, int B, int h,
                    int w, int interp, int out_dtype, const float *mean, const float *std, void *out, int *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif
