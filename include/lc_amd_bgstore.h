/*
 * lc_amd bgstore -- C ABI of the device-resident background store's per-row pick, cut and blend (liblc_amd_bgstore.so, built from
 * lc_amd/csrc/bgstore/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference's loader does per instance on a host core with
 * `_switch_bg(rgb_in, msk_in, np.random.choice(self.bg_list))` (dataset.py:137-148,413-415): choose one of the dataset's background
 * images, cut a random region of it, stretch it over the crop and blend it in behind the object's mask.  No new arithmetic: every number
 * is one that another header of this project already defines, composed.
 *
 * The store (lc_amd/backgrounds.py: `BackgroundStore`): G images of different sizes in ONE byte buffer `pixels`, image g as (Hb, Wb, 3)
 * uint8 rows of 3 Wb bytes without padding from byte `offsets[g]` on (int64, >= 0, a multiple of 4), with `hw` (G,2) int32 = (Hb, Wb),
 * 1 <= Hb, Wb <= LC_BGSTORE_MAX_SIZE.  The tables are the store's: the kernels range-check every tap against hw[g] and trust that
 * `pixels` holds offsets[g] + 3 Hb Wb bytes.
 *
 * lc_bgstore_pick, one thread per row b, with u(op, i) of include/lc_amd_augment.h and SWITCH = LC_BGSTORE_OP_SWITCH:
 *   gate[b]  = u(SWITCH, 0) < switch_bg_prob and G > 0                          (int32 0 / 1: bit 0 of `draw`'s P[0])
 *   which[b] = min(trunc(u(SWITCH, 1) G), G - 1) where the gate is open (`draw`'s P[1]), else -1
 *   bg_hw[b] = hw[which[b]] where the gate is open, else (1, 1): what lc_geometry_background_f32 takes as its per-row bg_hw, defined
 *              for every row
 *   seed: a DEVICE pointer to one uint64, aligned to 8 bytes, read by the kernel at every launch and replay; sample_id (B) int32.
 *
 * lc_bgstore_switch_u8, for row b with g = which[b], IN PLACE in crops (B,3,h,w) uint8:
 *   g < 0: the gate is closed; info[b] = 0 and the row is untouched.
 *   the row is REFUSED -- info[b] = -1, untouched -- when M_b has a non-finite entry, g >= G, hw[g] lies outside
 *   [1, LC_BGSTORE_MAX_SIZE] or offsets[g] < 0.  Otherwise info[b] = 1 and, for every pixel (x, y) and channel c:
 *   k   = the k of bit 0 of include/lc_amd_augment.h from msk_in (B,h,w) f32: t = 1024 msk_in (fp32); 1024 where t >= 1024,
 *         rint(t) where t > 0, else 0 (so NaN is 0).  A pixel with k = 1024 keeps its byte.
 *   bg  = the linear crop of include/lc_amd_crop.h of image g with the forward matrix M_b (B,2,3) f32 -- its inverse, its coordinates
 *         (lc_amd/csrc/shared/lc_warp_grid.h), taps, weights, `+ 512 >> 10` and border 0 -- at (x, y), channel c
 *   S   = k fg + (1024 - k) bg;  v = (S + 512) >> 10, except that an exact tie (S & 1023 == 512) goes to the even neighbour
 *   M is what lc_geometry_background_f32 writes from the pick's bg_hw.
 *   Launch geometry: that of lc_crop_warp_u8 (a thread owns four x of a band of rows); a workgroup of a closed row exits at once, a
 *   thread whose four k are all 1024 touches neither the image nor the crop.
 *
 * Argument rules, checked before anything is launched: B >= 0 (B = 0 launches nothing and returns 0); G >= 0, and the store's tables
 * may be NULL only where G = 0; every other pointer is required; 0 <= switch_bg_prob <= 1; 1 <= h, w <= LC_BGSTORE_MAX_SIZE; seed is
 * aligned to 8 bytes, offsets to 8, the int32 and f32 arrays to 4.  No input VALUE can make a launch read outside the store's tables,
 * the image its tables describe, or its own rows.  One launch each on `stream` (hipStream_t as void*): no workspace, no allocation,
 * no atomics, no wait, capturable in a hipGraph.  0 on success, else lc_amd_bgstore_last_error().
 */
#ifndef LC_AMD_BGSTORE_H
#define LC_AMD_BGSTORE_H

#include <stdint.h>

#define LC_AMD_BGSTORE_VERSION 1
#define LC_BGSTORE_MAX_SIZE 16384
#define LC_BGSTORE_OP_SWITCH 131073

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_bgstore_version(void);
const char *lc_amd_bgstore_last_error(void);
const char *lc_amd_bgstore_source_hash(void);

int lc_bgstore_pick(double switch_bg_prob, int G, const uint64_t *seed, const int *sample_id, const int *hw, int B, int *gate,
                    int *which, int *bg_hw, void *stream);

int lc_bgstore_switch_u8(unsigned char *crops, const float *msk_in, const unsigned char *pixels, const int64_t *offsets,
                         const int *hw, int G, const int *which, const float *M, int h, int w, int B, int *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif
