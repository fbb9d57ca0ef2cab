/*
 * lc_amd symerr -- C ABI of the symmetry-aware pose errors (liblc_amd_symerr.so, built from lc_amd/csrc/symerr/).
 *
 * A library of its own, next to liblc_amd.so and the other side libraries: no other ABI is changed by it, and liblc_amd.so is the
 * same bytes with or without it.
 *
 * lc_sym_pose_errors_f32: lib/utils/error6d.py:36-84 (mssd, mspd) and :157-172 (proj), batched, with each object's symmetry transforms
 *   read from the device table of lc_amd.symmetry.SymmetrySet: sym_tab (sym_rows,12) float64, one transform [R_s | t_s] per row as a
 *   row-major 3 x 4 (8-byte aligned); object o owns rows [obj_off[o], obj_off[o] + obj_k[o]) (obj_off, obj_k: n_obj int32 each) and its
 *   first row is the exact identity; obj_index (B) int32 names each pose's object.  n_obj >= 1, 1 <= sym_rows < 2^31 / 12.  These are
 *   the arguments and rules of lc_sym_select_table_f32 (include/lc_amd.h), checked by the same function.
 *   R_* (B,3,3), t_* (B,3), cam_K (B,3,3, all nine entries are read); pts (P,3) model vertices with pts_off / pts_cnt (B) int32 selecting
 *   each pose's range, both NULL: every pose uses pts[0:P].  1 <= P < 2^31 / 3.  Every pointer but sym_tab and workspace: 4-byte aligned.
 *   With s = (R_s, t_s) over the object's rows, R_gs = R_gt R_s, t_gs = R_gt t_s + t_gt and pi = rows 0, 1 of K [R | t] [p; 1] over
 *   row 2 (no z clamp, nothing assumed about K's last row):
 *       mssd = min_s max_p |(R_est - R_gs) p + (t_est - t_gs)|,   mspd = min_s max_p |pi_est(p) - pi_gs(p)|,
 *       proj = mean_p |pi_est(p) - pi_gt(p)|   (no symmetry).
 *   fp64 arithmetic on the fp32 inputs, the three results rounded to fp32.
 *   -> err (B,3) = mssd, mspd, proj;  arg (B,2) int32 = the symmetry that gave mssd and the one that gave mspd, counted inside the
 *   object's own rows: the lowest k among those whose error, rounded to fp32, is the least.  est = gt gives three exact zeros and
 *   arg = 0.  err and arg of a pose are the same bits in any batch, order and mix of objects, alone or not, launch after launch.
 *   max_k: an upper bound of obj_k over the batch's objects (SymmetrySet.max_k); it sizes the grid and the workspace.
 *   A pose whose obj_index lies outside [0, n_obj), whose rows leave the table, whose obj_k exceeds max_k, or whose vertex range is
 *   empty or leaves pts: err = NaN, arg = -1, and neither its table rows nor its vertices are read.  B = 0: no launch.
 *   workspace: lc_sym_pose_errors_workspace_bytes(B, max_k) bytes, 8-byte aligned, owned by the call while it runs; nothing is kept
 *   in it between calls and it needs no initialisation.  No host synchronisation, no allocation: capturable in a hipGraph.
 *   Returns 0, or non-zero with the reason in lc_amd_symerr_last_error().
 */
#ifndef LC_AMD_SYMERR_H
#define LC_AMD_SYMERR_H

#include <stddef.h>

#define LC_AMD_SYMERR_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int lc_amd_symerr_version(void);
const char *lc_amd_symerr_last_error(void);
const char *lc_amd_symerr_source_hash(void);

size_t lc_sym_pose_errors_workspace_bytes(int B, int max_k);
int lc_sym_pose_errors_f32(const float *R_est, const float *t_est, const float *R_gt, const float *t_gt, const float *cam_K,
                           const float *pts, const int *pts_off, const int *pts_cnt, int P, const int *obj_index, const double *sym_tab,
                           const int *obj_off, const int *obj_k, int n_obj, int sym_rows, int max_k, int B, float *err, int *arg,
                           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
