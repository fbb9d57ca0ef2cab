/*
 * lc_amd rle -- C ABI of the device-resident store of COCO run-length masks (liblc_amd_rle.so, built from lc_amd/csrc/rle/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference's loader does per sample on a host core through pycocotools
 * (dataset.py:174-182 writes one run-length record per instance, dataset.py:379 decodes one per sample), for a whole dataset's masks
 * that stay on the device: decoded per step by index into exactly the byte masks lc_mask_crops_u8 reads, and the reverse for the byte
 * masks lc_gtinfo_f32 writes.  Integer work throughout: every output is defined bit for bit.
 *
 * THE FORMAT.  A mask of a frame with H rows and W columns is a list of uint32 counts.  Position p = x H + y is column-major, as COCO
 * has it.  Run k covers the next counts[k] positions and has value k & 1; the first run is zeros and may be empty.
 *   A VALID mask's counts sum to H W.  DECODING accepts a zero count anywhere.  ENCODING emits the canonical list: only counts[0] may
 *   be zero; an all-zero mask is [H W]; an all-one mask is [0, H W].  1 <= H, W <= LC_RLE_MAX_SIZE, so every position fits 32 bits.
 * The store on the device is three arrays: counts (T) uint32, all masks concatenated;  offsets (F+1) int64: mask f is
 * counts[offsets[f] .. offsets[f+1]);  sizes (F,2) int32 = (H, W) per mask (masks of different frame sizes may share a store).
 * Offsets and sizes are device data: every kernel judges them itself (0 <= offsets[f] <= offsets[f+1] <= T, the size in range) and
 * reads nothing of a mask that fails.  T <= LC_RLE_MAX_COUNTS, so that a mask's sum cannot leave 64 bits.
 *
 * lc_rle_index_u32, once per store (one launch, one workgroup per mask, 144 bytes of LDS).  For mask f:
 *   ends (T) uint32: the inclusive running sum of f's counts, restarting per mask (its low 32 bits where the mask is invalid and the
 *      sum passes them); entries that belong to no mask with good offsets are not written, and where the ranges of two masks overlap
 *      the shared entries hold the sums of one of them
 *   area (F) int32: the sum of the odd runs
 *   box (F,4) int32: inclusive (x_min, y_min, x_max, y_max) of the set pixels, -1 four times for an empty mask.  A 1-run that crosses a
 *      column boundary covers rows 0 and H - 1
 *   valid (F) int32: 0, or -1 if the offsets or the size fail the rules above or the counts do not sum to exactly H W, judged in 64
 *      bits (the counts are not negative, so then no partial sum exceeds H W either).  An invalid mask has area 0 and box -1.
 *
 * lc_rle_decode_u8, per step (one launch, 4 bytes of LDS).  Row b reads mask mask_index[b] (NULL: row b reads mask b) through `ends`
 * and `valid` as the index wrote them, with origin_xy (B,2) int32 = (x0, y0) or NULL (0,0): where the (Hm,Wm) window lies in the frame,
 * the convention and bound of lc_mask_crops_u8 and lc_gtinfo_f32 (it may be negative; |x0|, |y0| <= LC_RLE_MAX_ORIGIN).
 *   out (B,Hm,Wm) uint8, row-major, bytes 0 or 1: window pixel (i, j) is frame pixel (x0 + j, y0 + i); anything outside the frame is 0
 *   info (B) int32 or NULL: 0, or -1 for an index outside [0,F), an invalid mask, or an origin beyond the bound.  Such a row is all
 *      zero, and nothing of ends, offsets and sizes is read for it (of `valid` one entry where the index is in range).
 *
 * lc_rle_encode_u8 (one launch, one workgroup per mask, 256 bytes of LDS).  Reads byte masks (F,Hm,Wm), non-zero = set, in a window
 * with origin_xy (F,2) or NULL inside a frame of sizes[f] (NULL: the frame is the window, (Hm, Wm)).  Pixels of the frame outside the
 * window are 0; pixels of the window outside the frame are ignored.
 *   counts_out (F,cap) uint32: the canonical list in the first n_runs[f] entries, the rest 0
 *   n_runs (F) int32
 *   info (F) int32 or NULL: 0; -2 when the mask needs more than `cap` runs (n_runs still holds the needed number and the row of
 *      counts_out is all zero); -1 for a size or an origin out of range (n_runs 0, the row all zero).
 * The run boundaries are ranked by integer counts and scans alone: no atomic takes part.
 *
 * 1 <= Hm, Wm <= LC_RLE_MAX_SIZE; cap >= 1.  Every array must be aligned to its element.  No value in any device array can make a
 * launch read or write outside its arrays.  B = 0 or F = 0 launches nothing (decode with F = 0 and B > 0 writes its refused rows).
 * Every entry point launches on `stream` (hipStream_t as void*): no allocation, no wait, capturable in a hipGraph.  The kernels use no
 * scratch.  Every output is an integer: the same bits for any batch, order and grid shape.  0 on success, else lc_amd_rle_last_error().
 */
#ifndef LC_AMD_RLE_H
#define LC_AMD_RLE_H

#include <stddef.h>
#include <stdint.h>

#define LC_AMD_RLE_VERSION 1
#define LC_RLE_MAX_SIZE 16384
#define LC_RLE_MAX_ORIGIN 16777216
#define LC_RLE_MAX_COUNTS 4294967296

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_rle_version(void);
const char *lc_amd_rle_last_error(void);
const char *lc_amd_rle_source_hash(void);

int lc_rle_index_u32(const uint32_t *counts, const int64_t *offsets, const int *sizes, int64_t T, int F, uint32_t *ends, int *area, int *box,
                     int *valid, void *stream);
int lc_rle_decode_u8(const uint32_t *ends, const int64_t *offsets, const int *sizes, const int *valid, int64_t T, int F, const int *mask_index,
                     const int *origin_xy, int B, int Hm, int Wm, unsigned char *out, int *info, void *stream);
int lc_rle_encode_u8(const unsigned char *masks, int F, int Hm, int Wm, const int *sizes, const int *origin_xy, int cap, uint32_t *counts_out,
                     int *n_runs, int *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif
