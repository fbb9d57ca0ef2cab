"""Pose covariance and predicted error at test time, in one HIP launch (lc_amd/csrc/posecov/lc_pose_cov.hip,
lc_amd/_C/liblc_amd_posecov.so, C ABI in include/lc_amd_posecov.h).

    pose_covariance(K, pts3d, pts2d, weights, pose, counts=None, *, bbox_3d, diameter=None, cov_2d=False,
                    nan_to_num=False, weights_are_std=False, shared_poses=None) -> PoseCov(cov, var, pred_err, info)

What the reference's `pnp_auto.diff_pnp_perturb(pose, K, X, u, w, with_cov=True)` (lib/nll/pnp_auto.py:86-108) followed by
`cov_mixed.jac_update2alter`, `transformed_cov_from_jac` and `loss_cov_3d(var, diameter)` / `loss_cov_2d(var)` (lib/cov_mixed.py:52-97)
computes at a solved pose: the covariance of the 6-d pose update (rotation axis-angle first, translation last), the variances of the
eight 3D box corners' coordinates (or of their projections, `cov_2d`), and the mean predicted corner error.  A row whose Hessian is not
positive definite (no points, all-zero weights, non-finite sums) gets `cov = I` and `info != 0`, as `safe_cholesky` does.

The options mirror the solver's load-time options, so that the covariance describes the problem that was solved: `nan_to_num`
(torch.nan_to_num per element at the load), `weights_are_std` (weights are standard deviations s, used as 1/s**2; else inverse
variances), weights of shape (B,N) (one value per point), `counts` (device int32; entries at or beyond counts[b] are never read),
`shared_poses=P` (K, bbox_3d and diameter have P rows shared by the rows b, b + P, ... of a (kP,N,.) batch; pose has P or kP rows).

float32 HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device,
can be captured into a graph.
"""
from __future__ import annotations

from ctypes import c_int, c_void_p
from typing import NamedTuple

import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

NAN_TO_NUM, WEIGHTS_ARE_STD, SCALAR_WEIGHTS, COV_2D = 1, 2, 4, 8  # include/lc_amd_posecov.h: LC_POSE_COV_*
MAX_POINTS = 16384  # LC_POSE_COV_MAX_POINTS


class PoseCov(NamedTuple):
    cov: Tensor       # (B,6,6) covariance of the pose update, or I where info != 0
    var: Tensor       # (B,24) variances of the box corners' coordinates, or (B,16) of their projections (cov_2d)
    pred_err: Tensor  # (B,) mean over the corners of sqrt(sum of the corner's variances) [/ diameter]
    info: Tensor      # (B,) int32: 0 = the Hessian was positive definite


_SO = _lib.SideLibrary(_build.POSECOV, {"lc_pose_cov_f32": (c_int, [c_void_p] * 8 + [c_int] * 5 + [c_void_p] * 5)})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("posecov")


@torch.no_grad()
def pose_covariance(K, pts3d, pts2d, weights, pose, counts=None, *, bbox_3d, diameter=None, cov_2d=False, nan_to_num=False,
                    weights_are_std=False, shared_poses=None) -> PoseCov:
    K = _lib.require_hip_f32("K", K)
    X = _lib.require_hip_f32("pts3d", pts3d)
    U = _lib.require_hip_f32("pts2d", pts2d)
    Wt = _lib.require_hip_f32("weights", weights)
    pose = _lib.require_hip_f32("pose", pose)
    bbox = _lib.require_hip_f32("bbox_3d", bbox_3d)
    diam = None if diameter is None else _lib.require_hip_f32("diameter", diameter)
    if X.dim() != 3 or X.shape[-1] != 3:
        raise ValueError(f"lc_amd.posecov: pts3d must be (B,N,3), got {tuple(X.shape)}")
    B, N = X.shape[:2]
    if not 1 <= N <= MAX_POINTS:
        raise ValueError(f"lc_amd.posecov: rows of 1 to {MAX_POINTS} points, got N = {N}")
    dev = X.device
    _A.rows("pts2d", U, (B, N, 2))
    if Wt.dim() == 2:
        _A.rows("weights", Wt, (B, N))
    else:
        _A.rows("weights", Wt, (B, N, 2))
    P = int(shared_poses) if shared_poses else B
    if P < 1 or B % P:
        raise ValueError(f"lc_amd.posecov: shared_poses = {shared_poses} does not divide the batch of {B} rows")
    _A.rows("K", K, (P, 3, 3))
    _A.rows("bbox_3d", bbox, (P, 8, 3))
    if pose.dim() != 2 or pose.shape[1] != 7 or pose.shape[0] not in (P, B):
        raise ValueError(f"lc_amd.posecov: pose must be ({P},7)" + (f" or ({B},7)" if P != B else "") + f", got {tuple(pose.shape)}")
    if diam is not None:
        if cov_2d:
            raise ValueError("lc_amd.posecov: diameter divides the 3D corner error only (loss_cov_2d takes none)")
        _A.rows("diameter", diam, (P,))
    if counts is not None:
        if not isinstance(counts, Tensor) or not counts.is_cuda or counts.dtype != torch.int32:
            raise TypeError("lc_amd.posecov: counts must be an int32 tensor on the GPU")
        _A.rows("counts", counts, (B,))
        counts = counts.contiguous()
    _A.same_device(dev, "pts3d on {}", K=K, pts2d=U, weights=Wt, pose=pose, bbox_3d=bbox, diameter=diam, counts=counts)
    lib = load()
    rows = 16 if cov_2d else 24
    cov = torch.empty(B, 6, 6, device=dev, dtype=torch.float32)
    var = torch.empty(B, rows, device=dev, dtype=torch.float32)
    perr = torch.empty(B, device=dev, dtype=torch.float32)
    info = torch.empty(B, device=dev, dtype=torch.int32)
    opts = (NAN_TO_NUM if nan_to_num else 0) | (WEIGHTS_ARE_STD if weights_are_std else 0) | (SCALAR_WEIGHTS if Wt.dim() == 2 else 0) | (COV_2D if cov_2d else 0)
    with _lib.on_device(dev):
        rc = lib.lc_pose_cov_f32(_lib.ptr(K), _lib.ptr(pose), _lib.ptr(X), _lib.ptr(U), _lib.ptr(Wt), _lib.ptr(counts), _lib.ptr(bbox), _lib.ptr(diam),
                                 B, N, opts, P, int(pose.shape[0]), _lib.ptr(cov), _lib.ptr(var), _lib.ptr(perr), _lib.ptr(info), _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("posecov.pose_covariance", rc)
    return PoseCov(cov, var, perr, info)
