/*
 * lc_amd augment -- C ABI of the training-time background switch and colour augmentation (liblc_amd_augment.so, built from
 * lc_amd/csrc/augment/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference's loader does per instance on a host core with the warped crop
 * (dataset.py:137-148,413-419: `img*msk + bg*(1-msk)`, np.round, then imgaug's SaltAndPepper, MotionBlur, CoarseDropout, GaussianBlur
 * and five point operations), restated in integers.  The host draws the few numbers per sample (lc_amd/augment.py: `draw`); ONE launch
 * does everything that touches pixels: it reads the crop, the background and the mask once and writes the network's input once.
 *
 * lc_augment_u8, for row b of the batch:
 *   crops (B,3,h,w) uint8: what lc_crop_warp_u8 writes with LC_CROP_U8
 *   backgrounds (G,3,h,w) uint8, or NULL with G = 0
 *   msk_in (B,h,w) f32 holding k / 1024, as lc_mask_crops_u8 writes msk_vis, or NULL
 *   params (B,64) int32, word j of a row is P[j];  lut (B,3,256) uint8
 *   seed (uint64, by value);  sample_id (B) int32 or NULL (row b is sample b)
 *   out_dtype, mean, std: the codes and rules of lc_amd_crop.h (LC_AUGMENT_U8 holds v; the float types hold v / 255 in IEEE fp32, with
 *      mean / std -- HOST arrays of 3 floats that travel as kernel arguments, or both NULL -- (v / 255 - mean_c) / std_c, two more fp32
 *      operations; a 16-bit output is rounded once, from fp32; mean / std need a float type)
 *   form: LC_AUGMENT_FILTERED serves every row; LC_AUGMENT_POINTWISE is the caller's statement that no row of the launch uses a 5x5
 *      filter (it drew the params): that form streams without staging a halo, and REFUSES a row with bit 2 or bit 4 set
 *   out (B,3,h,w) of out_dtype;  info (B) int32 or NULL: 0, or -1 for a refused row
 *
 * The stages run in this order; each produces uint8; rint is round-half-even; a stage is on when its bit of P[0] is set:
 *   bit 0  background switch: g = P[1]; t = 1024 msk_in (fp32); k = 1024 where t >= 1024, rint(t) where t > 0, else 0 (so NaN is 0);
 *          S = k fg + (1024 - k) bg_g;  v = (S + 512) >> 10, except that an exact tie (S & 1023 == 512) goes to the even neighbour.
 *          It is the reference's img*msk + bg*(1-msk) followed by np.round: with msk = k / 1024 both products and their sum are exact in fp32.
 *   bit 1  salt and pepper: pixel p = y w + x is replaced iff key(SNP, p) < (uint32)P[2]; by 255 when the top bit of key(SNPV, p) is
 *          set, else by 0; the same for all three channels
 *   bit 2  5x5 filter A (motion blur): weights P[6..30], row-major from (dy, dx) = (-2, -2), Q16, each >= 0, their sum exactly 65536;
 *          v(y, x) = (sum over dy, dx of w[dy][dx] in(y + dy, x + dx) + 32768) >> 16;  indices beyond the image reflect without
 *          repeating the edge (-1 -> 1, h -> h - 2: OpenCV's BORDER_REFLECT_101)
 *   bit 3  coarse dropout: grid P[4] = gh by P[5] = gw, 1 <= gh <= h, 1 <= gw <= w; cell c = (y gh / h) gw + (x gw / w) in integer
 *          division; the pixel is 0 in all channels iff key(DROP, c) < (uint32)P[3]
 *   bit 4  5x5 filter B (Gaussian blur): weights P[31..55], the rule of filter A; it reads the result of the stages before it,
 *          reflected at the image border in the same way
 *   bit 5  point operations: v = lut[b, c, v]
 * P[56..63] are reserved and must be 0.
 *
 * key(op, q), in uint32 arithmetic (wrapping products), with f = MurmurHash3's 32-bit finaliser as include/lc_amd_maskcrop.h states it
 *       f(v):  v ^= v >> 16;  v *= 0x85ebca6b;  v ^= v >> 13;  v *= 0xc2b2ae35;  v ^= v >> 16
 *   k = f(seed & 0xffffffff);  k = f(k ^ (seed >> 32));  k = f(k ^ sample_id);  k = f(k ^ op);  key(op, q) = f(k ^ q)
 * -- maskcrop's key_r with `op` in the place of the round r.  The op codes lie above every round number maskcrop uses (r < 256), and the
 * key depends on nothing else: not on B, the row's place in the batch or the grid shape.  (The host's draws use op codes of their own,
 * LC_AUGMENT_OP_HOST and up, in lc_amd/augment.py.)
 *
 * A row is refused -- info = -1, written as the unchanged crop converted to out_dtype -- when bits of P[0] above bit 5 are set, a
 * reserved word is non-zero, a stage that is ON has a negative weight, a weight sum other than 65536 or a grid size out of range,
 * bit 0 is set while msk_in or backgrounds is NULL or g lies outside [0, G), or a filter bit is set in an LC_AUGMENT_POINTWISE launch.
 * Words of a stage that is off are not judged.
 *
 * LC_AUGMENT_MIN_SIZE <= h, w <= LC_AUGMENT_MAX_SIZE (a reflected index is reflected once).  params, lut, msk_in, sample_id, info and a
 * float `out` must be aligned to 4 bytes (a 16-bit `out` to 2).  No input value can make the launch read or write outside its arrays.
 * B = 0 launches nothing.  One launch on `stream` (hipStream_t as void*): no workspace, no allocation, no wait, capturable in a
 * hipGraph.  Every output is defined bit for bit: the same for any batch, order and grid shape.  0 on success, else
 * lc_amd_augment_last_error().
 *
 * lc_augment_drawn_u8 is the same launch with the rows DRAWN BY THE KERNEL: neither `params` nor `lut` exists on the host.  The first
 * wavefront of every workgroup forms its own sample's row from (cfg, seed, sample_id, h, w) before the pixel work and hands it on where
 * lc_augment_u8 stages what it read; the row is then judged and used exactly as above.  It is the row `draw` of lc_amd/augment.py makes:
 *   u(op, i) = (key(op, i) >> 8) / 2^24 in fp64, with the host op codes LC_AUGMENT_OP_SWITCH ... LC_AUGMENT_OP_CONTRAST below
 *   switch   = u(SWITCH, 0) < switch_bg_prob and n_backgrounds > 0;  P[1] = min(trunc(u(SWITCH, 1) n_backgrounds), n_backgrounds - 1)
 *   chain    = u(CHAIN, 0) < pixel_aug_prob: the gate in front of every stage below
 *   salt     = use_peper_salt and u(SALT, 0) < 0.3;  P[2] = floor(0.05 2^32)
 *   motion   = use_motion_blur and u(MOTION, 0) < 0.2;  angle = 360 u(MOTION, 1) degrees, direction d = 2 u(MOTION, 2) - 1;  P[6..30]: five
 *              taps at s = -2..2 along (sin t, -cos t) from the centre, weighted (1 - d) / 2 + (s + 2) d / 4, each splatted bilinearly
 *   dropout  = u(DROPOUT, 0) < 0.5;  P[3] = floor(0.1 2^32), P[4] = max(1, 5 h / 100), P[5] = max(1, 5 w / 100) in integer division
 *   gauss    = u(GAUSS, 0) < 0.5 and sigma >= 1e-3, sigma = 1.2 u(GAUSS, 1);  P[31..55]: g_i = exp(-i^2 / 2 sigma^2), i = -2..2, normalised,
 *              the outer product
 *   add, invert, multiply per channel, multiply, contrast: gates u(op, 0) < 0.5, 0.4 (and use_invert), 0.5, 0.5, 0.5; bit 5 is set when
 *              one of them is open.  A per-channel value is u(op, 2 + c) where u(op, 1) < 0.3 (ADD, CONTRAST) or 0.5 (MUL_PC), else
 *              u(op, 2) for all three; channel c is inverted where u(INVERT, 1 + c) < 0.2.  The table of channel c is the composition, in
 *              this order, of  v + min(-25 + floor(51 u), 25),  255 - v,  v (0.6 + 0.8 u),  v (0.6 + 0.8 u),  128 + (0.5 + 1.7 u)(v - 128),
 *              every step clip(rint(.), 0, 255) in fp64, every product and sum rounded on its own (nothing fused)
 *   words of a stage whose gate is shut are 0, and the table of a row without bit 5 is the identity.
 * Bits, the background, the grid and the tables are EQUAL to `draw`'s, bit for bit.  A filter's 25 fp64 weights pass through
 * floor(x 65536 + 1/2) with the remainder to 65536 added to the centre; exp, sin and cos are polynomials of this library on a reduced
 * argument (the quadrant of the angle is taken from the integer key), not the host's math library, so each Q16 weight is within 1 of
 * `draw`'s, each is >= 0 and each set sums to exactly 65536.
 *   cfg: by value; the probabilities must lie in [0, 1]; 0 <= n_backgrounds <= G (a row names backgrounds 0 .. n_backgrounds - 1)
 *   seed: a DEVICE pointer to one uint64, aligned to 8 bytes, read by the kernel: a replayed graph draws anew once the word has changed.
 *      The salt and the dropout of the pixels use the same word.
 *   sample_id (B) int32: required
 *   params_out (B,64) int32 and lut_out (B,3,256) uint8, each or both NULL: the rows as drawn (before they are judged: a row that
 *      switches the background without msk_in is drawn, written here, and refused with info = -1), written by the drawing wavefront
 *   form: there is no argument.  The launch takes LC_AUGMENT_FILTERED unless cfg rules every filter out, which is pixel_aug_prob = 0
 *      (both filters stand behind the chain's gate, and the Gaussian behind no switch of cfg); then it takes LC_AUGMENT_POINTWISE.
 *   everything else -- crops, backgrounds, msk_in, out_dtype, mean, std, out, info, the sizes, alignment, B = 0, stream -- as above.
 */
#ifndef LC_AMD_AUGMENT_H
#define LC_AMD_AUGMENT_H

#include <stdint.h>

#define LC_AMD_AUGMENT_VERSION 1
#define LC_AUGMENT_MIN_SIZE 8
#define LC_AUGMENT_MAX_SIZE 16384
#define LC_AUGMENT_WORDS 64

#define LC_AUGMENT_U8 0
#define LC_AUGMENT_F32 1
#define LC_AUGMENT_F16 2
#define LC_AUGMENT_BF16 3

#define LC_AUGMENT_FILTERED 0
#define LC_AUGMENT_POINTWISE 1

#define LC_AUGMENT_OP_SNP 65537
#define LC_AUGMENT_OP_SNPV 65538
#define LC_AUGMENT_OP_DROP 65539
#define LC_AUGMENT_OP_HOST 131072
/* the host's decisions, one op code each (lc_amd/augment.py: OP_*); the index i of u(op, i) tells the draws of one decision apart */
#define LC_AUGMENT_OP_SWITCH 131073
#define LC_AUGMENT_OP_CHAIN 131074
#define LC_AUGMENT_OP_SALT 131075
#define LC_AUGMENT_OP_MOTION 131076
#define LC_AUGMENT_OP_DROPOUT 131077
#define LC_AUGMENT_OP_GAUSS 131078
#define LC_AUGMENT_OP_ADD 131079
#define LC_AUGMENT_OP_INVERT 131080
#define LC_AUGMENT_OP_MUL_PC 131081
#define LC_AUGMENT_OP_MUL 131082
#define LC_AUGMENT_OP_CONTRAST 131083
#define LC_AUGMENT_OP_BG_REGION 131084
#define LC_AUGMENT_OP_ZOOM 131085

/* what `draw` reads of AugmentConfig, and the number of backgrounds it may name */
typedef struct lc_augment_draw_config {
    double pixel_aug_prob;
    double switch_bg_prob;
    int use_peper_salt;
    int use_motion_blur;
    int use_invert;
    int n_backgrounds;
} lc_augment_draw_config;

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_augment_version(void);
const char *lc_amd_augment_last_error(void);
const char *lc_amd_augment_source_hash(void);

int lc_augment_u8(const unsigned char *crops, const unsigned char *backgrounds, int G, const float *msk_in, const int *params,
                  const unsigned char *lut, int B, int h, int w, uint64_t seed, const int *sample_id, int out_dtype, int form,
                  const float *mean, const float *std, void *out, int *info, void *stream);

int lc_augment_drawn_u8(const unsigned char *crops, const unsigned char *backgrounds, int G, const float *msk_in,
                        lc_augment_draw_config cfg, const uint64_t *seed, const int *sample_id, int B, int h, int w, int out_dtype,
                        const float *mean, const float *std, void *out, int *info, int *params_out, unsigned char *lut_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
