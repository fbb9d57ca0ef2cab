/*
 * lc_amd sampler -- C ABI of the device-resident training set's row sampler (liblc_amd_sampler.so, built from lc_amd/csrc/sampler/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and every other library is
 * the same bytes with or without it.  What the reference's loader does on the host around `_get_single_item`: the epoch's shuffle and
 * the gather of a step's records (the DataLoader's sampler and collate), and the retry of `BOP_Dataset.__getitem__` (dataset.py:332-338),
 * which draws another random instance whenever `valid_cnt < valid_pix_cnt_th`.  The definition is lc_amd/sampler.py (`permute_host`,
 * `draw_rows_host`, `select_rows_host`), in host numpy; the kernels equal it bit for bit -- everything here is integer arithmetic and
 * copies -- so a captured graph of the whole training input moves on to the next step's batch with one 64-bit word on the device.
 *
 * All three launches: on `stream` (a hipStream_t as void*), no workspace, no atomics, no allocation, no wait: capturable in a hipGraph.
 * Every output is written with plain vector stores.
 *
 * Random numbers: key(op, i) of include/lc_amd_augment.h, restated --
 *       f(v):  v ^= v >> 16;  v *= 0x85ebca6b;  v ^= v >> 13;  v *= 0xc2b2ae35;  v ^= v >> 16          (uint32, wrapping)
 *   seed_state(lo, hi) = f(f(lo) ^ hi);  sample_state(s, id) = f(s ^ id)
 *   key(w, id, op, i) = f(f(sample_state(seed_state(w & 0xffffffff, w >> 32), id) ^ op) ^ i)
 *
 * lc_sampler_rows -- the rows of one step, one thread per row in workgroups of 64, rows = B + S, 1 <= B, 0 <= S, rows <= LC_SAMPLER_MAX_ROWS.
 *   w = the uint64 the DEVICE pointer `seed` names (aligned to 8 bytes), read by the kernel at every launch and replay; seed0 by value.
 *   step = w - seed0 (uint64, wrapping).
 *   A primary row j < B:   p = step B + j,  e = p / N,  q = p % N,  index = perm(seed0, e)(q)
 *   A spare row j >= B:    index = (key(w, j, LC_SAMPLER_OP_SPARE, 0) N) >> 32                          (a 64-bit product)
 *   perm(seed0, e), a bijection of [0, N):  k = max(1, ceil(bitlength(N - 1) / 2)), mask = 2^k - 1,
 *       es = f(sample_state(sample_state(seed_state(seed0 & 0xffffffff, seed0 >> 32), e & 0xffffffff), e >> 32) ^ LC_SAMPLER_OP_PERM)
 *       rk_r = f(es ^ C_r), r = 0 .. 3, with C = LC_SAMPLER_ROUND_0 .. LC_SAMPLER_ROUND_3
 *       one pass over x < 2^(2k):  (L, H) = (x >> k, x & mask);  four times, r = 0 .. 3:  (L, H) <- (H, L ^ (f(rk_r ^ H) & mask));
 *                                  x <- (L << k) | H                                                   (a balanced Feistel network)
 *       perm(q): x = q; do x <- pass(x) while x >= N                                                   (cycle walking: 2^(2k) < 4 N + 4)
 *   Every epoch of N consecutive primaries p holds every index exactly once; an epoch may end inside a batch.  Spares are drawn with
 *   replacement, as the reference's retry draws, and may repeat a primary.
 *   The thread copies record `index` of the resident table into row j of the outputs:
 *     table: 10 device pointers in a HOST array read during the call, in this order -- frame_index, mask_index, mesh_index, obj_id,
 *            scene_id, im_id (N) int32;  bbox_xyxy (N,4), cam_K (N,9), R (N,9), t (N,3) float32
 *     out:   12 device pointers in a HOST array -- index, frame_index, mask_index, mesh_index, obj_id, scene_id, im_id (rows) int32;
 *            bbox_xyxy (rows,4), cam_K (rows,9), R (rows,9), t (rows,3) float32;  info (rows) int32
 *   info = 0, or -1 for a REFUSED row: all seven int32 outputs are -1 and every float is a quiet NaN.  Every row is refused when
 *   step >= 2^40 or N < 1 (nothing of the table is read then); one row is refused when its record's frame_index, mask_index or mesh_index
 *   is negative.
 *
 * lc_sampler_select_i32 -- which rows make the batch, one workgroup of 1024, rows <= LC_SAMPLER_MAX_ROWS, 1 <= B <= rows.
 *   valid_cnt (rows), info (rows) int32.  Row r is GOOD when info[r] >= 0 and valid_cnt[r] >= valid_th.  Rows below B are primaries,
 *   the others spares.
 *   take (B) int32:  take[j] = j for a good primary;  the i-th bad primary, in row order, takes the i-th good spare, in row order;
 *                    -1 once the good spares have run out.
 *   shortfall (1) int32 = the number of rows with take = -1.
 *   Ordered scans: ballot and popcount within a wavefront, LDS across wavefronts; the result depends on nothing but the inputs.
 *
 * lc_sampler_take_rows -- dst_k[j] = src_k[take[j]] for n tensors, 1 <= n <= LC_SAMPLER_MAX_TENSORS, src_k (rows, row_bytes_k) and
 *   dst_k (B, row_bytes_k) bytes, 1 <= row_bytes_k <= LC_SAMPLER_MAX_ROW_BYTES.  src, dst and row_bytes are HOST arrays of n entries read
 *   during the call: they travel by value in the kernel's argument, nothing is uploaded.  A tensor whose src, dst and row_bytes are all
 *   multiples of 16 moves in 16-byte loads and stores, any other byte by byte.  A row with take[j] outside [0, rows) is zero-filled.
 *   No dst may overlap a src (not checked).
 *
 * Argument rules, checked before anything is launched: the required pointers are not NULL and aligned to their element (none for the
 * tensors of take_rows); the sizes are in the ranges above.  0 on success, else lc_amd_sampler_last_error().
 */
#ifndef LC_AMD_SAMPLER_H
#define LC_AMD_SAMPLER_H

#include <stdint.h>

#define LC_AMD_SAMPLER_VERSION 1
#define LC_SAMPLER_MAX_ROWS 65536
#define LC_SAMPLER_MAX_N 2147483647
#define LC_SAMPLER_MAX_STEP_BITS 40
#define LC_SAMPLER_MAX_TENSORS 16
#define LC_SAMPLER_MAX_ROW_BYTES 1073741824
#define LC_SAMPLER_TABLE_POINTERS 10
#define LC_SAMPLER_ROWS_POINTERS 12
#define LC_SAMPLER_OP_SPARE 131086
#define LC_SAMPLER_OP_PERM 131087
#define LC_SAMPLER_ROUND_0 0x9e3779b9u
#define LC_SAMPLER_ROUND_1 0x3c6ef372u
#define LC_SAMPLER_ROUND_2 0xdaa66d2bu
#define LC_SAMPLER_ROUND_3 0x78dde6e4u

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_sampler_version(void);
const char *lc_amd_sampler_last_error(void);
const char *lc_amd_sampler_source_hash(void);

int lc_sampler_rows(const uint64_t *seed, uint64_t seed0, int N, int B, int S, const void *const *table, void *const *out, void *stream);

int lc_sampler_select_i32(const int *valid_cnt, const int *info, int valid_th, int B, int rows, int *take, int *shortfall, void *stream);

int lc_sampler_take_rows(const int *take, int B, int rows, int n, const void *const *src, void *const *dst, const uint64_t *row_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif

#endif
