"""BOP's Visible Surface Discrepancy on the device (lc_amd/csrc/vsd/lc_vsd.hip, lc_amd/_C/liblc_amd_vsd.so; C ABI and the exact
definition of every output in include/lc_amd_vsd.h): `pose_error.vsd` with visib_mode='bop19' and cost_type='step'.

    vsd_from_depth(depth_est, depth_gt, depth_test, K, *, delta, taus, ...) -> VsdResult(errors, counts)
        the scoring stage alone, for depth maps from any renderer
    compute_vsd(meshes, mesh_index, R_est, t_est, R_gt, t_gt, K, depth_test, *, delta, taus, near, far, ...) -> VsdRendered(errors, counts, info)
        one `render.render_depth` call over the 2B rows (estimates, then ground truths), then the score
    vsd_from_states(meshes, mesh_index, states_est, states_gt, K, depth_test, **kw)   the same from (B,7) quaternion states
    window_origins(t_est, t_gt, K, diameter, window_hw, frame_hw) -> (B,2) int32      where to put a (h,w) window for each pose

`errors` (B,T) float32: e_k = (cost_k + union - inter) / union, 1 where union = 0.  `counts` (B,T+3) int32: union, inter, edge, cost_0 ..
cost_{T-1}; `edge` > 0 says that a window may have cut the object.  A refused row (scene_index outside the scenes, a window that reaches
outside the frame, an unknown mesh) has counts of -1 and NaN errors.  Everything is an integer count or one fp32 rounding of a ratio of
integers: the same bits for any batch, order and launch.

`pixel_center` = (0, 0), the default, gives pixel (x,y) the K-coordinates (x,y): the convention of BOP's depth-to-distance conversion.
`render.render_depth` alone defaults to (0.5, 0.5); `compute_vsd` hands it the value given here.

float32 HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device,
allocates its outputs only and can be captured into a graph.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_float, c_int, c_void_p
from typing import NamedTuple

import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

MAX_TAUS = 16     # LC_VSD_MAX_TAUS
MAX_SIZE = 16384  # LC_VSD_MAX_SIZE
BOP_TAUS = tuple(0.05 * k for k in range(1, 11))  # BOP's vsd_taus: 0.05 .. 0.5 of the object's diameter


class VsdResult(NamedTuple):
    errors: Tensor  # (B,T) float32
    counts: Tensor  # (B,T+3) int32: union, inter, edge, cost_0 .. cost_{T-1}


class VsdRendered(NamedTuple):
    errors: Tensor
    counts: Tensor
    info: Tensor    # (B,2) int32: the renderer's info of the estimate's and of the ground truth's render (-1: unknown mesh)


_SO = _lib.SideLibrary(_build.VSD, {
    "lc_vsd_score_f32": (c_int, [c_void_p] * 6 + [ctypes.POINTER(c_float), c_int, c_float, c_void_p] + [c_int] * 6 + [c_float] * 2 + [c_void_p] * 3),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("vsd")


def _scalars(delta, taus):
    """(delta, taus) as Python floats; every rule that needs no tensor."""
    delta = _A.delta(delta)
    if isinstance(taus, (Tensor, str)) or not hasattr(taus, "__iter__"):
        raise TypeError(f"lc_amd.vsd: taus must be a sequence of numbers on the host, got {type(taus)}")
    taus = list(taus)
    if any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in taus):
        raise TypeError("lc_amd.vsd: taus must be a sequence of numbers on the host")
    if not 1 <= len(taus) <= MAX_TAUS:
        raise ValueError(f"lc_amd.vsd: 1 to {MAX_TAUS} taus, got {len(taus)}")
    if not all(math.isfinite(x) for x in taus):
        raise ValueError("lc_amd.vsd: taus must be finite")
    return delta, [float(x) for x in taus]


@torch.no_grad()
def vsd_from_depth(depth_est, depth_gt, depth_test, K, *, delta, taus, diameter=None, scene_index=None, window_xy=None,
                   pixel_center=(0.0, 0.0)) -> VsdResult:
    """depth_est, depth_gt (B,h,w); depth_test (H,W) or (S,H,W) with scene_index (B,) int32 / int64 (default: the one scene, or scene b
    for pose b when S = B); K (3,3) or (B,3,3); diameter (B,) or None (the taus are then absolute); window_xy (B,2) int32 / int64 = (x0,y0)
    of the (h,w) maps in the (H,W) frame, or None for full-frame maps."""
    delta, taus = _scalars(delta, taus)
    pcx, pcy = _A.center(pixel_center, cx_cy=True)
    De = _A.f32("depth_est", depth_est, (None, None, None))
    B, h, w = (int(n) for n in De.shape)
    Dg = _A.f32("depth_gt", depth_gt, (B, h, w))
    Dt, S = _A.scenes(depth_test, scene_index, B, "poses")
    H, W = int(Dt.shape[1]), int(Dt.shape[2])
    Kc = _A.cam_K("K", K, B)
    if diameter is not None:
        _A.f32("diameter", diameter, (B,))
    if window_xy is not None:
        _A.i32("window_xy", window_xy, (B, 2))
        if not (h <= H and w <= W):
            raise ValueError(f"lc_amd.vsd: a {h} x {w} window does not fit the {H} x {W} frame")
    elif (h, w) != (H, W):
        raise ValueError(f"lc_amd.vsd: without window_xy the rendered maps ({h} x {w}) must have the frame's size ({H} x {W})")
    if not (1 <= h and 1 <= w and H <= MAX_SIZE and W <= MAX_SIZE):
        raise ValueError(f"lc_amd.vsd: map sizes of 1 to {MAX_SIZE}, got {h} x {w} in {H} x {W}")
    De = _lib.require_hip_f32("depth_est", De)
    dev = De.device
    _A.same_device(dev, "depth_est is on {}", depth_gt=Dg, depth_test=Dt, K=Kc, diameter=diameter, scene_index=scene_index, window_xy=window_xy)
    Dg, Dt, Kc = Dg.contiguous(), Dt.contiguous(), Kc.contiguous()
    diam = None if diameter is None else diameter.contiguous()
    win = None if window_xy is None else window_xy.to(torch.int32).contiguous()
    T = len(taus)
    counts = torch.empty(B, T + 3, device=dev, dtype=torch.int32)
    errors = torch.empty(B, T, device=dev, dtype=torch.float32)
    if B:
        idx = _A.scene_index(scene_index, S, B, dev)
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_vsd_score_f32(_lib.ptr(De), _lib.ptr(Dg), _lib.ptr(Dt), _lib.ptr(idx), _lib.ptr(Kc), _lib.ptr(diam), (c_float * T)(*taus), T,
                                      delta, _lib.ptr(win), B, h, w, S, H, W, pcx, pcy, _lib.ptr(counts), _lib.ptr(errors), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("lc_vsd_score_f32", rc)
    return VsdResult(errors, counts)


def _project_centre(t: Tensor, K: Tensor):
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    return (K[:, 0, 0] * x + K[:, 0, 1] * y) / z + K[:, 0, 2], (K[:, 1, 0] * x + K[:, 1, 1] * y) / z + K[:, 1, 2]


@torch.no_grad()
def window_origins(t_est, t_gt, K, diameter, window_hw, frame_hw) -> Tensor:
    """(B,2) int32 (x0,y0): the (h,w) window centred on the midpoint of the two projected object centres, rounded to whole pixels and
    clamped into the (H,W) frame.  Elementwise torch on the tensors' own device, nothing read back.  `diameter` (B,) or None places nothing
    (whether a window of this size holds the object depends on the pose as well, and is what `counts[:, 2]`, edge, reports afterwards): it
    is checked against the batch so that a call passes the same rows here and to `compute_vsd`."""
    h, w = int(window_hw[0]), int(window_hw[1])
    H, W = int(frame_hw[0]), int(frame_hw[1])
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"lc_amd.vsd: a {h} x {w} window does not fit the {H} x {W} frame")
    te = _A.f32("t_est", t_est.reshape(-1, 3) if isinstance(t_est, Tensor) else t_est, (None, 3))
    B = int(te.shape[0])
    tg = _A.f32("t_gt", t_gt.reshape(-1, 3) if isinstance(t_gt, Tensor) else t_gt, (B, 3))
    Kc = _A.cam_K("K", K, B)
    if diameter is not None:
        _A.f32("diameter", diameter, (B,))
    _A.same_device(te.device, "depth_est is on {}", t_gt=tg, K=Kc, diameter=diameter)
    ue, ve = _project_centre(te, Kc)
    ug, vg = _project_centre(tg, Kc)
    x0 = torch.floor((ue + ug) * 0.5 - 0.5 * w + 0.5).clamp(0, W - w)
    y0 = torch.floor((ve + vg) * 0.5 - 0.5 * h + 0.5).clamp(0, H - h)
    return torch.stack((x0, y0), -1).to(torch.int32)


@torch.no_grad()
def compute_vsd(meshes, mesh_index, R_est, t_est, R_gt, t_gt, K, depth_test, *, scene_index=None, delta, taus, diameter=None, near, far,
                window_hw=None, window_xy=None, pixel_center=(0.0, 0.0)) -> VsdRendered:
    """Render and score.  meshes: a `render.MeshSet`; mesh_index (B,) int32 on the device (`meshes.index_of(obj_ids)`; an unknown mesh
    refuses the row); R_* (B,3,3), t_* (B,3) or (B,3,1), K (3,3) or (B,3,3); depth_test, scene_index, delta, taus, diameter as in
    `vsd_from_depth`.  window_hw = (h,w) with window_xy (B,2) int32 (`window_origins`) renders and scores that window of the frame only:
    the render uses K with K02 - x0 and K12 - y0 (formed in fp32: exact for an integer-valued principal point), the score the given K and
    the origin.  Returns the errors, the counts and the renderer's `info` of both renders as (B,2)."""
    from . import render as _render

    if not isinstance(meshes, _render.MeshSet):
        raise TypeError(f"lc_amd.vsd: meshes must be a lc_amd.render.MeshSet, got {type(meshes)}")
    _scalars(delta, taus)
    _A.center(pixel_center, cx_cy=True)
    B, (Re, Rg), (te, tg), Kc = _A.pose_batch(mesh_index, dict(R_est=R_est, R_gt=R_gt), dict(t_est=t_est, t_gt=t_gt), K)
    Dt, S = _A.scenes(depth_test, scene_index, B, "poses")
    H, W = int(Dt.shape[1]), int(Dt.shape[2])
    if (window_hw is None) != (window_xy is None):
        raise ValueError("lc_amd.vsd: window_hw and window_xy go together")
    if window_xy is not None:
        h, w = int(window_hw[0]), int(window_hw[1])
        _A.i32("window_xy", window_xy, (B, 2))
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"lc_amd.vsd: a {h} x {w} window does not fit the {H} x {W} frame")
    else:
        h, w = H, W
    if diameter is not None:
        _A.f32("diameter", diameter, (B,))
    dev = meshes.device
    _A.same_device(dev, _args.MESHES_ON, mesh_index=mesh_index, R_est=Re, R_gt=Rg, t_est=te, t_gt=tg, K=Kc, depth_test=Dt, scene_index=scene_index,
                   diameter=diameter, window_xy=window_xy)
    Kr = Kc
    if window_xy is not None:
        Kr = Kc.clone()
        Kr[:, 0, 2] -= window_xy[:, 0].to(torch.float32)
        Kr[:, 1, 2] -= window_xy[:, 1].to(torch.float32)
    out = _render.render_depth(meshes, torch.cat((mesh_index, mesh_index)), torch.cat((Re, Rg)), torch.cat((te, tg)), torch.cat((Kr, Kr)), (h, w),
                               near=near, far=far, pixel_center=pixel_center)
    info = torch.stack((out.info[:B], out.info[B:]), -1)
    known = (mesh_index >= 0) & (mesh_index < meshes.n_meshes)
    idx = torch.where(known, _A.scene_index(scene_index, S, B, dev), torch.full_like(mesh_index, -1))  # an unknown mesh: refused by the score as well
    res = vsd_from_depth(out.depth[:B], out.depth[B:], Dt, Kc, delta=delta, taus=taus, diameter=diameter, scene_index=idx, window_xy=window_xy,
                         pixel_center=pixel_center)
    return VsdRendered(res.errors, res.counts, info)


def vsd_from_states(meshes, mesh_index, states_est, states_gt, K, depth_test, **kw) -> VsdRendered:
    """`compute_vsd` from (B,7) quaternion representations (the output of `cer_solver.solve`), as `metrics.sym_pose_errors_from_states`."""
    from .transforms import quaternion_rep_to_RT

    Re, te = quaternion_rep_to_RT(states_est)
    Rg, tg = quaternion_rep_to_RT(states_gt)
    return compute_vsd(meshes, mesh_index, Re, te, Rg, tg, K, depth_test, **kw)
