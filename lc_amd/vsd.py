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

from . import _lib
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


_LIB = None
_SIGNATURES = {
    "lc_amd_vsd_version": (c_int, []),
    "lc_amd_vsd_last_error": (ctypes.c_char_p, []),
    "lc_amd_vsd_source_hash": (ctypes.c_char_p, []),
    "lc_vsd_score_f32": (c_int, [c_void_p] * 6 + [ctypes.POINTER(c_float), c_int, c_float, c_void_p] + [c_int] * 6 + [c_float] * 2 + [c_void_p] * 3),
}


def load(build_if_missing: bool = True):
    """liblc_amd_vsd.so, loaded on first use by `_lib.load_target`: a library built from other sources than the ones next to it is
    rebuilt, or refused where hipcc is absent (unless LC_AMD_ALLOW_STALE=1)."""
    global _LIB
    if _LIB is None:
        _LIB = _lib.load_target(_build.VSD, _SIGNATURES, build_if_missing)
    return _LIB


def _f32(name: str, t, shape) -> Tensor:
    """Type, element type and shape (None: any size)."""
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.vsd: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"lc_amd.vsd: {name} must be float32, got {t.dtype}")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError(f"lc_amd.vsd: {name} has shape {tuple(t.shape)}, expected ({', '.join('*' if d is None else str(d) for d in shape)})")
    return t


def _i32(name: str, t, shape) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.vsd: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"lc_amd.vsd: {name} must be int32 or int64, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"lc_amd.vsd: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _scalars(delta, taus):
    """(delta, taus) as Python floats; every rule that needs no tensor."""
    if isinstance(delta, bool) or not isinstance(delta, (int, float)):
        raise TypeError(f"lc_amd.vsd: delta must be a number, got {type(delta)}")
    if not math.isfinite(delta) or delta < 0:
        raise ValueError(f"lc_amd.vsd: delta must be finite and not negative, got {delta}")
    if isinstance(taus, (Tensor, str)) or not hasattr(taus, "__iter__"):
        raise TypeError(f"lc_amd.vsd: taus must be a sequence of numbers on the host, got {type(taus)}")
    taus = list(taus)
    if any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in taus):
        raise TypeError("lc_amd.vsd: taus must be a sequence of numbers on the host")
    if not 1 <= len(taus) <= MAX_TAUS:
        raise ValueError(f"lc_amd.vsd: 1 to {MAX_TAUS} taus, got {len(taus)}")
    if not all(math.isfinite(x) for x in taus):
        raise ValueError("lc_amd.vsd: taus must be finite")
    return float(delta), [float(x) for x in taus]


def _center(pixel_center):
    if not hasattr(pixel_center, "__len__") or len(pixel_center) != 2:
        raise ValueError(f"lc_amd.vsd: pixel_center is a pair (cx, cy), got {pixel_center!r}")
    return float(pixel_center[0]), float(pixel_center[1])


def _on(dev, **named):
    for name, t in named.items():
        if t is not None and t.device != dev:
            raise RuntimeError(f"lc_amd.vsd: {name} is on {t.device}, depth_est is on {dev}")


def _scenes(depth_test, scene_index, B: int):
    """depth_test as (S,H,W) and the rule for a missing scene_index: one scene serves every pose, B scenes serve one pose each."""
    if isinstance(depth_test, Tensor) and depth_test.dim() == 2:
        depth_test = depth_test[None]
    Dt = _f32("depth_test", depth_test, (None, None, None))
    S = int(Dt.shape[0])
    if scene_index is None:
        if S not in (1, B):
            raise ValueError(f"lc_amd.vsd: scene_index is needed to tell which of the {S} scenes each of the {B} poses belongs to")
    else:
        _i32("scene_index", scene_index, (B,))
    return Dt, S


def _scene_index(scene_index, S: int, B: int, dev) -> Tensor:
    if scene_index is None:
        return torch.zeros(B, device=dev, dtype=torch.int32) if S == 1 else torch.arange(B, device=dev, dtype=torch.int32)
    return scene_index.to(torch.int32).contiguous()


@torch.no_grad()
def vsd_from_depth(depth_est, depth_gt, depth_test, K, *, delta, taus, diameter=None, scene_index=None, window_xy=None,
                   pixel_center=(0.0, 0.0)) -> VsdResult:
    """depth_est, depth_gt (B,h,w); depth_test (H,W) or (S,H,W) with scene_index (B,) int32 / int64 (default: the one scene, or scene b
    for pose b when S = B); K (3,3) or (B,3,3); diameter (B,) or None (the taus are then absolute); window_xy (B,2) int32 / int64 = (x0,y0)
    of the (h,w) maps in the (H,W) frame, or None for full-frame maps."""
    delta, taus = _scalars(delta, taus)
    pcx, pcy = _center(pixel_center)
    De = _f32("depth_est", depth_est, (None, None, None))
    B, h, w = (int(n) for n in De.shape)
    Dg = _f32("depth_gt", depth_gt, (B, h, w))
    Dt, S = _scenes(depth_test, scene_index, B)
    H, W = int(Dt.shape[1]), int(Dt.shape[2])
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3):
        K = K.expand(B, 3, 3)
    Kc = _f32("K", K, (B, 3, 3))
    if diameter is not None:
        _f32("diameter", diameter, (B,))
    if window_xy is not None:
        _i32("window_xy", window_xy, (B, 2))
        if not (h <= H and w <= W):
            raise ValueError(f"lc_amd.vsd: a {h} x {w} window does not fit the {H} x {W} frame")
    elif (h, w) != (H, W):
        raise ValueError(f"lc_amd.vsd: without window_xy the rendered maps ({h} x {w}) must have the frame's size ({H} x {W})")
    if not (1 <= h and 1 <= w and H <= MAX_SIZE and W <= MAX_SIZE):
        raise ValueError(f"lc_amd.vsd: map sizes of 1 to {MAX_SIZE}, got {h} x {w} in {H} x {W}")
    De = _lib.require_hip_f32("depth_est", De)
    dev = De.device
    _on(dev, depth_gt=Dg, depth_test=Dt, K=Kc, diameter=diameter, scene_index=scene_index, window_xy=window_xy)
    Dg, Dt, Kc = Dg.contiguous(), Dt.contiguous(), Kc.contiguous()
    diam = None if diameter is None else diameter.contiguous()
    win = None if window_xy is None else window_xy.to(torch.int32).contiguous()
    T = len(taus)
    counts = torch.empty(B, T + 3, device=dev, dtype=torch.int32)
    errors = torch.empty(B, T, device=dev, dtype=torch.float32)
    if B:
        idx = _scene_index(scene_index, S, B, dev)
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_vsd_score_f32(_lib.ptr(De), _lib.ptr(Dg), _lib.ptr(Dt), _lib.ptr(idx), _lib.ptr(Kc), _lib.ptr(diam), (c_float * T)(*taus), T,
                                      delta, _lib.ptr(win), B, h, w, S, H, W, pcx, pcy, _lib.ptr(counts), _lib.ptr(errors), _lib.stream_ptr(dev))
        if rc != 0:
            raise RuntimeError(f"lc_amd.lc_vsd_score_f32 failed (code {rc}): {lib.lc_amd_vsd_last_error().decode(errors='replace')}")
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
    te = _f32("t_est", t_est.reshape(-1, 3) if isinstance(t_est, Tensor) else t_est, (None, 3))
    B = int(te.shape[0])
    tg = _f32("t_gt", t_gt.reshape(-1, 3) if isinstance(t_gt, Tensor) else t_gt, (B, 3))
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3):
        K = K.expand(B, 3, 3)
    Kc = _f32("K", K, (B, 3, 3))
    if diameter is not None:
        _f32("diameter", diameter, (B,))
    _on(te.device, t_gt=tg, K=Kc, diameter=diameter)
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
    _center(pixel_center)
    if not isinstance(mesh_index, Tensor) or mesh_index.dtype != torch.int32:
        raise TypeError("lc_amd.vsd: mesh_index must be an int32 tensor on the GPU (MeshSet.index_of)")
    if mesh_index.dim() != 1:
        raise ValueError(f"lc_amd.vsd: mesh_index has shape {tuple(mesh_index.shape)}, expected (B,)")
    B = int(mesh_index.shape[0])
    Re, Rg = _f32("R_est", R_est, (B, 3, 3)), _f32("R_gt", R_gt, (B, 3, 3))
    for name, t in (("t_est", t_est), ("t_gt", t_gt)):
        if isinstance(t, Tensor) and tuple(t.shape) not in ((B, 3), (B, 3, 1)):
            raise ValueError(f"lc_amd.vsd: {name} has shape {tuple(t.shape)}, expected {(B, 3)} or {(B, 3, 1)}")
    te = _f32("t_est", t_est.reshape(B, 3) if isinstance(t_est, Tensor) else t_est, (B, 3))
    tg = _f32("t_gt", t_gt.reshape(B, 3) if isinstance(t_gt, Tensor) else t_gt, (B, 3))
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3):
        K = K.expand(B, 3, 3)
    Kc = _f32("K", K, (B, 3, 3))
    Dt, S = _scenes(depth_test, scene_index, B)
    H, W = int(Dt.shape[1]), int(Dt.shape[2])
    if (window_hw is None) != (window_xy is None):
        raise ValueError("lc_amd.vsd: window_hw and window_xy go together")
    if window_xy is not None:
        h, w = int(window_hw[0]), int(window_hw[1])
        _i32("window_xy", window_xy, (B, 2))
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"lc_amd.vsd: a {h} x {w} window does not fit the {H} x {W} frame")
    else:
        h, w = H, W
    if diameter is not None:
        _f32("diameter", diameter, (B,))
    dev = meshes.device
    for name, t in (("mesh_index", mesh_index), ("R_est", Re), ("R_gt", Rg), ("t_est", te), ("t_gt", tg), ("K", Kc), ("depth_test", Dt),
                    ("scene_index", scene_index), ("diameter", diameter), ("window_xy", window_xy)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"lc_amd.vsd: {name} is on {t.device}, the meshes are on {dev} (there is no CPU fallback in the product path)")
    Kr = Kc
    if window_xy is not None:
        Kr = Kc.clone()
        Kr[:, 0, 2] -= window_xy[:, 0].to(torch.float32)
        Kr[:, 1, 2] -= window_xy[:, 1].to(torch.float32)
    out = _render.render_depth(meshes, torch.cat((mesh_index, mesh_index)), torch.cat((Re, Rg)), torch.cat((te, tg)), torch.cat((Kr, Kr)), (h, w),
                               near=near, far=far, pixel_center=pixel_center)
    info = torch.stack((out.info[:B], out.info[B:]), -1)
    known = (mesh_index >= 0) & (mesh_index < meshes.n_meshes)
    idx = torch.where(known, _scene_index(scene_index, S, B, dev), torch.full_like(mesh_index, -1))  # an unknown mesh: refused by the score as well
    res = vsd_from_depth(out.depth[:B], out.depth[B:], Dt, Kc, delta=delta, taus=taus, diameter=diameter, scene_index=idx, window_xy=window_xy,
                         pixel_center=pixel_center)
    return VsdRendered(res.errors, res.counts, info)


def vsd_from_states(meshes, mesh_index, states_est, states_gt, K, depth_test, **kw) -> VsdRendered:
    """`compute_vsd` from (B,7) quaternion representations (the output of `cer_solver.solve`), as `metrics.sym_pose_errors_from_states`."""
    from .transforms import quaternion_rep_to_RT

    Re, te = quaternion_rep_to_RT(states_est)
    Rg, tg = quaternion_rep_to_RT(states_gt)
    return compute_vsd(meshes, mesh_index, Re, te, Rg, tg, K, depth_test, **kw)
