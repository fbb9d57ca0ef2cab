"""numpy float64 restatement of the three symmetry-aware errors of lc_sym_metrics.hip, written from the definitions of the reference
(`lib/utils/error6d.py:36-84` mssd, mspd; `:157-172` proj; `:8-22` project_pts), with the symmetry that gave each minimum.

    per_symmetry(R_est, t_est, R_gt, t_gt, K, pts, R_s, t_s) -> (e3 (Ks,), e2 (Ks,))  the maximum 3D / image distance under each symmetry
    errors(...)                                              -> (mssd, mspd, proj, k_mssd, k_mspd)   np.argmin: the first index on ties

Everything is float64; callers widen the float32 inputs.  `t_*` (3,), `R_s` (Ks,3,3), `t_s` (Ks,3), `pts` (M,3), `K` (3,3)."""
import numpy as np


def project(pts, K, R, t):
    """project_pts: rows 0 and 1 of K [R | t] [p; 1] over row 2.  No z clamp, nothing assumed about K's last row."""
    P = K @ np.concatenate((R, t.reshape(3, 1)), 1)
    h = P @ np.concatenate((pts, np.ones((len(pts), 1))), 1).T
    return (h[:2] / h[2]).T


def per_symmetry(R_est, t_est, R_gt, t_gt, K, pts, R_s, t_s):
    est3 = pts @ R_est.T + t_est
    est2 = project(pts, K, R_est, t_est)
    e3, e2 = [], []
    for Rs, ts in zip(R_s, t_s):
        R_gs, t_gs = R_gt @ Rs, R_gt @ ts + t_gt
        e3.append(np.linalg.norm(est3 - (pts @ R_gs.T + t_gs), axis=1).max())
        e2.append(np.linalg.norm(est2 - project(pts, K, R_gs, t_gs), axis=1).max())
    return np.asarray(e3), np.asarray(e2)


def proj(R_est, t_est, R_gt, t_gt, K, pts):
    return np.linalg.norm(project(pts, K, R_est, t_est) - project(pts, K, R_gt, t_gt), axis=1).mean()


def errors(R_est, t_est, R_gt, t_gt, K, pts, R_s, t_s):
    e3, e2 = per_symmetry(R_est, t_est, R_gt, t_gt, K, pts, R_s, t_s)
    k3, k2 = int(np.argmin(e3)), int(np.argmin(e2))
    return float(e3[k3]), float(e2[k2]), float(proj(R_est, t_est, R_gt, t_gt, K, pts)), k3, k2


def batch(case):
    """`errors` of every pose of a case dict (tests/symerr_cases.py): -> err (B,3) float64, arg (B,2) int64."""
    from tests import symerr_cases as C

    out = [errors(*C.pose_args(case, b)) for b in range(len(case["obj_index"]))]
    return np.asarray([o[:3] for o in out], np.float64).reshape(-1, 3), np.asarray([o[3:] for o in out], np.int64).reshape(-1, 2)
