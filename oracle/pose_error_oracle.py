"""CPU oracle of the pose-error metrics (TEST INFRASTRUCTURE ONLY): numpy restatement of `lib/utils/error6d.py:87-154`
(add, adi, re, te) as bundled by `lib/utils/evaluate.py:333-339`.  Pinned by tests/golden/pose_err_*.npz generated from
the reference's error6d module (tests/test_oracle_metrics.py)."""
import math

import numpy as np
from scipy import spatial


def transform(pts, R, t):
    return pts @ R.T + t.reshape(1, 3)


def add(R_est, t_est, R_gt, t_gt, pts):
    return np.linalg.norm(transform(pts, R_est, t_est) - transform(pts, R_gt, t_gt), axis=1).mean()


def nearest(R_est, t_est, R_gt, t_gt, pts, k=1):
    """Distances and indices of the k nearest est-pose vertices of every gt-pose vertex: (M,) for k = 1, (M, k) otherwise."""
    est, gt = transform(pts, R_est, t_est), transform(pts, R_gt, t_gt)
    return spatial.cKDTree(est).query(gt, k=k)


def adi(R_est, t_est, R_gt, t_gt, pts):
    d, _ = nearest(R_est, t_est, R_gt, t_gt, pts)
    return d.mean()


def adi_without_target(R_est, t_est, R_gt, t_gt, pts, j):
    """ADI when est-pose vertex j is missing from the search (every gt-pose vertex is still a query)."""
    est, gt = transform(pts, R_est, t_est), transform(pts, R_gt, t_gt)
    d, _ = spatial.cKDTree(np.delete(est, j, axis=0)).query(gt, k=1)
    return d.mean()


def re(R_est, R_gt):
    c = 0.5 * (np.trace(R_est @ np.linalg.inv(R_gt)) - 1.0)
    return math.degrees(math.acos(min(1.0, max(-1.0, float(c)))))


def re_transposed(R_est, R_gt):
    """`re` with R_gt^T in place of inv(R_gt): the same number for an orthonormal R_gt, and what lc_metrics.hip computes (the trace of
    R_est R_gt^T is the sum of the nine products of equal entries)."""
    c = 0.5 * (float(np.sum(R_est * R_gt)) - 1.0)
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def te(t_est, t_gt):
    return float(np.linalg.norm(t_gt.reshape(3) - t_est.reshape(3)))


def compute_pose_errors(R_est, t_est, R_gt, t_gt, pts):
    return dict(adi=adi(R_est, t_est, R_gt, t_gt, pts), add=add(R_est, t_est, R_gt, t_gt, pts), re=re(R_est, R_gt), te=te(t_est, t_gt))
