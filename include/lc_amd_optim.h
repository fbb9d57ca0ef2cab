/*
 * lc_amd optim -- C ABI of the fused optimizer step (liblc_amd_optim.so, built from lc_amd/csrc/optim/).
 *
 * A library of its own, next to liblc_amd.so: the hot-path ABI (include/lc_amd.h, LC_AMD_VERSION) is unchanged by it.
 *
 * lc_ranger_step_f32 performs one Ranger step (RAdam + Lookahead + gradient centralisation, lib/optim/ranger.py:109-198 of the
 * reference) for every tensor of a device table in one launch, or two when a centralised tensor has rows longer than
 * LC_RANGER_ONE_PASS_ROW (a row-mean launch first).  The table is ONE device buffer:
 *
 *   lc_ranger_scalars[ntensors]   the per-step scalars and gradient pointers (the host rewrites only this part from one step to the next)
 *   lc_ranger_tensor[ntensors]    pointers to p and the state tensors, and the shape of each tensor
 *   lc_ranger_block[nrowsum]      one per row of a tensor whose rows are longer than LC_RANGER_ONE_PASS_ROW (e0 = row index)
 *   lc_ranger_block[nupdate]      the update launch's workgroups, each a range [e0, e0 + n) of one tensor in storage order, n <= LC_RANGER_BLOCK_ELEMS;
 *                                 for a tensor with 0 < row <= LC_RANGER_ONE_PASS_ROW a range of whole rows (at most LC_RANGER_BLOCK_ROWS)
 *
 * p, grad, exp_avg, exp_avg_sq and slow_buffer of one tensor have identical strides and are walked in storage order, where every
 * dim-0 row is one contiguous block of `row` elements.  row_means (float, one per long row, at each tensor's mean_off) is the
 * workspace of the two-launch form.  Asynchronous on `stream` (hipStream_t as void*); 0 on success, else lc_amd_optim_last_error().
 */
#ifndef LC_AMD_OPTIM_H
#define LC_AMD_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_OPTIM_VERSION 1
#define LC_RANGER_BLOCK_ELEMS 8192 /* elements per workgroup of the update launch */
#define LC_RANGER_ONE_PASS_ROW 8192 /* longest row whose mean the update launch computes on chip */
#define LC_RANGER_BLOCK_ROWS 1024   /* rows per workgroup at most */

#define LC_RANGER_WEIGHT_DECAY 1 /* p += (-wd*lr) * p */
#define LC_RANGER_ADAPTIVE 2     /* the RAdam branch (N_sma > threshold): p += (-step_size*lr) * m / (sqrt(v) + eps) */
#define LC_RANGER_LOOKAHEAD 4    /* this tensor's Lookahead step: slow += alpha * (p - slow); p = slow */
/* An array is "in phase" with p when its address differs from p's by a multiple of 16 bytes: it is then read and written with the
 * same 16-byte accesses as p.  An array out of phase (e.g. a gradient that is a view into a flat bucket at an odd offset) is
 * accessed four floats at a time with 4-byte accesses; p itself sets the phase, whatever its alignment. */
#define LC_RANGER_GRAD_IN_PHASE 8       /* in lc_ranger_scalars.flags */
#define LC_RANGER_EXP_AVG_IN_PHASE 1    /* in lc_ranger_tensor.phase */
#define LC_RANGER_EXP_AVG_SQ_IN_PHASE 2
#define LC_RANGER_SLOW_IN_PHASE 4

typedef struct {
    float beta1, one_minus_beta1, beta2, one_minus_beta2;
    float neg_wd_lr;   /* -weight_decay * lr */
    float neg_step_lr; /* -step_size * lr */
    float eps, alpha;
    int flags; /* LC_RANGER_* */
    int pad;
    float *grad; /* this step's gradient: same strides as p, in place (the centred gradient is written back) */
} lc_ranger_scalars; /* 48 bytes, rewritten every step */

typedef struct {
    float *p, *exp_avg, *exp_avg_sq, *slow;
    long long numel;
    int row;      /* elements per dim-0 row to centralise, 0 = no centralisation */
    int mean_off; /* index of the tensor's first row in row_means (rows longer than LC_RANGER_ONE_PASS_ROW), else -1 */
    int phase;    /* LC_RANGER_*_IN_PHASE of exp_avg, exp_avg_sq, slow */
    int pad;
} lc_ranger_tensor; /* 56 bytes */

typedef struct {
    int tensor;
    int n;
    long long e0;
} lc_ranger_block; /* 16 bytes */

int lc_amd_optim_version(void);
const char *lc_amd_optim_last_error(void);
const char *lc_amd_optim_source_hash(void);

int lc_ranger_step_f32(const void *table, int ntensors, int nrowsum, int nupdate, float *row_means, void *stream);

#ifdef __cplusplus
}
#endif

#endif
