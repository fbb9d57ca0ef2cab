/*
 * lc_amd posecov -- C ABI of the test-time pose covariance (liblc_amd_posecov.so, built from lc_amd/csrc/posecov/).
 *
 * A library of its own, next to liblc_amd.so and liblc_amd_optim.so: the hot-path ABI (include/lc_amd.h, LC_AMD_VERSION) is unchanged by it.
 *
 * lc_pose_cov_f32 evaluates, for every row b of a padded batch, what the reference's
 *     pnp_auto.diff_pnp_perturb(pose, K, X, u, w, with_cov=True)  ->  cov_mixed.jac_update2alter / transformed_cov_from_jac
 *     ->  cov_mixed.loss_cov_3d(var, diameter) | loss_cov_2d(var)
 * computes (lib/nll/pnp_auto.py:86-108, lib/cov_mixed.py:52-97):
 *     H    = sum_n sum_c w_nc (J_nc^T J_nc + r_nc Hess r_nc)   right perturbation R exp(a), t + tau; symmetric by construction
 *     cov  = H^-1, or the identity with info != 0 when H is not positive definite (no points, zero weights, non-finite sums)
 *     var  = diag(G cov G^T), G the Jacobian of the 8 box corners (24 rows, 3D) or of their projections (16 rows, LC_POSE_COV_2D)
 *     pred_err = mean over the corners of sqrt(sum of the corner's var) (1 per corner if any var <= 0), divided by diameter if given (3D)
 * in ONE launch, one workgroup per row.  Sums are fp64 in a canonical order (tiles of 64 consecutive points, a fixed tree inside
 * the tile, tile partials in tile order), so a row's result depends on neither B, nor its position, nor the padding behind
 * counts[b]; every output is rounded to fp32 once.
 *
 *   K (R,3,3)  bbox_3d (R,8,3)  diameter (R) or NULL     R = object_rows: row b reads object b % R (B a multiple of R)
 *   pose (P,7) w,x,y,z,tx,ty,tz                          P = pose_rows:   row b reads pose   b % P (B a multiple of P)
 *   pts3d (B,N,3)  pts2d (B,N,2)  weights (B,N,2), or (B,N) with LC_POSE_COV_SCALAR_WEIGHTS
 *   counts (B) int32 or NULL: entries at or beyond counts[b] are never read (clamped into [0, N])
 *   cov (B,6,6)  var (B,24 | 16)  pred_err (B)  info (B) int32
 * 1 <= N <= LC_POSE_COV_MAX_POINTS.  Asynchronous on `stream` (hipStream_t as void*); 0 on success, else lc_amd_posecov_last_error().
 */
#ifndef LC_AMD_POSECOV_H
#define LC_AMD_POSECOV_H

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_POSECOV_VERSION 1
#define LC_POSE_COV_MAX_POINTS 16384

#define LC_POSE_COV_NAN_TO_NUM 1      /* torch.nan_to_num on K, pose, pts3d, pts2d and the inverse variances, at the load */
#define LC_POSE_COV_WEIGHTS_ARE_STD 2 /* weights hold standard deviations s: used as 1 / (s * s), formed in fp32 before the filter */
#define LC_POSE_COV_SCALAR_WEIGHTS 4  /* weights is (B,N): one value for both image coordinates */
#define LC_POSE_COV_2D 8              /* covariance of the projected box corners (16 rows) instead of the 3D ones (24 rows) */

int lc_amd_posecov_version(void);
const char *lc_amd_posecov_last_error(void);
const char *lc_amd_posecov_source_hash(void);

int lc_pose_cov_f32(const float *K, const float *pose, const float *pts3d, const float *pts2d, const float *weights, const int *counts,
                    const float *bbox_3d, const float *diameter, int B, int N, int options, int object_rows, int pose_rows,
                    float *cov, float *var, float *pred_err, int *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif
