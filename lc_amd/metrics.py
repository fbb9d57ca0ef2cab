"""Batched pose-error metrics on the GPU: `lib/utils/evaluate.py:333-339 compute_pose_errors`
(= `lib/utils/error6d.py` add / adi / re / te) for a whole test set in one launch, and the symmetry-aware BOP errors of
`error6d.py:36-84,157-172` (mssd, mspd, proj) with each object's symmetries read from a `SymmetrySet`'s device table."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_void_p

import torch
from torch import Tensor

from . import _lib
from . import build as _build
from .symmetry import SymmetrySet
from .transforms import quaternion_rep_to_RT


def compute_pose_errors(R_est: Tensor, t_est: Tensor, R_gt: Tensor, t_gt: Tensor, pts: Tensor, pts_off: Tensor = None,
                        pts_cnt: Tensor = None, want_adi: bool = True) -> dict:
    """R_* (B,3,3), t_* (B,3) or (B,3,1), pts (M,3) [or packed (P,3) with per-pose pts_off/pts_cnt (B,) int32].
    Returns dict(adi, add, re, te) of (B,) tensors -- the keys of the reference's `compute_pose_errors`."""
    lib = _lib.load()
    Re = _lib.require_hip_f32("R_est", R_est)
    Rg = _lib.require_hip_f32("R_gt", R_gt)
    te = _lib.require_hip_f32("t_est", t_est.reshape(-1, 3))
    tg = _lib.require_hip_f32("t_gt", t_gt.reshape(-1, 3))
    P = _lib.require_hip_f32("pts", pts)
    B = Re.shape[0]
    dev = Re.device
    if pts_off is not None:
        pts_off = pts_off.to(device=dev, dtype=torch.int32).contiguous()
        pts_cnt = pts_cnt.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(B, 4, device=dev, dtype=torch.float32)
    with _lib.on_device(dev):
        rc = lib.lc_pose_errors_f32(_lib.ptr(Re), _lib.ptr(te), _lib.ptr(Rg), _lib.ptr(tg), _lib.ptr(P), _lib.ptr(pts_off), _lib.ptr(pts_cnt),
                                    B, P.shape[0], int(want_adi), _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(rc, "lc_pose_errors_f32")
    return dict(adi=out[:, 0], add=out[:, 1], re=out[:, 2], te=out[:, 3])


def pose_errors_from_states(states_est: Tensor, states_gt: Tensor, pts: Tensor, **kw) -> dict:
    """Same, from (B,7) quaternion representations (the output of `cer_solver.solve`, `test.py:174`)."""
    Re, te = quaternion_rep_to_RT(states_est)
    Rg, tg = quaternion_rep_to_RT(states_gt)
    return compute_pose_errors(Re, te, Rg, tg, pts, **kw)


_SYMERR_LIB = None
_SYMERR_SIGNATURES = {
    "lc_amd_symerr_version": (c_int, []),
    "lc_amd_symerr_last_error": (ctypes.c_char_p, []),
    "lc_amd_symerr_source_hash": (ctypes.c_char_p, []),
    "lc_sym_pose_errors_workspace_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "lc_sym_pose_errors_f32": (c_int, [c_void_p] * 8 + [c_int] + [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3 + [ctypes.c_size_t, c_void_p]),
}


def load_symerr(build_if_missing: bool = True):
    """liblc_amd_symerr.so (C ABI in include/lc_amd_symerr.h), loaded on first use by `_lib.load_target`: a library built from other sources
    than the ones next to it is rebuilt, or refused where hipcc is absent (unless LC_AMD_ALLOW_STALE=1)."""
    global _SYMERR_LIB
    if _SYMERR_LIB is None:
        _SYMERR_LIB = _lib.load_target(_build.SYMERR, _SYMERR_SIGNATURES, build_if_missing)
    return _SYMERR_LIB


_SYM_WS = {}  # (device index, bytes rounded up to a power of two) -> workspace; never freed: a captured graph may hold its address


def _sym_workspace(dev, nbytes: int) -> Tensor:
    size = 1 << max(8, (nbytes - 1).bit_length())
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), size)
    ws = _SYM_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():  # a buffer from the graph's own pool must not outlive the capture in this cache
            raise RuntimeError("lc_amd.metrics: call compute_sym_pose_errors once with these sizes before capturing it in a graph")
        ws = _SYM_WS[key] = torch.empty(size // 8, device=dev, dtype=torch.int64)
    return ws


def _hip_i32(name: str, t, B: int, dev) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.metrics: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"lc_amd.metrics: {name} must be int32 or int64, got {t.dtype}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"lc_amd.metrics: {name} has shape {tuple(t.shape)}, expected {(B,)}")
    if t.device != dev:
        raise RuntimeError(f"lc_amd.metrics: {name} is on {t.device}, the poses are on {dev}")
    return t.to(torch.int32).contiguous()


def _f32(name: str, t, shape, dev=None) -> Tensor:
    """Type, element type, shape (None: any size) and the device of the poses; _lib.require_hip_f32 follows once every tensor has passed."""
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.metrics: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"lc_amd.metrics: {name} must be float32 (reference I/O precision), got {t.dtype}")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError(f"lc_amd.metrics: {name} has shape {tuple(t.shape)}, expected ({', '.join('*' if d is None else str(d) for d in shape)})")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"lc_amd.metrics: {name} is on {t.device}, the poses are on {dev}")
    return t


def compute_sym_pose_errors(R_est: Tensor, t_est: Tensor, R_gt: Tensor, t_gt: Tensor, cam_K: Tensor, pts: Tensor = None, syms: SymmetrySet = None,
                            obj_index: Tensor = None, pts_off: Tensor = None, pts_cnt: Tensor = None, meshes=None, mesh_index: Tensor = None) -> dict:
    """MSSD, MSPD and proj of B pose pairs in one call (two launches, no host synchronisation, capturable in a graph).

    R_* (B,3,3), t_* (B,3) or (B,3,1), cam_K (3,3) or (B,3,3) float32 on the device; `syms` the SymmetrySet of the objects and `obj_index`
    (B,) int32 / int64 the table index of each pose's object (`syms.index_of(obj_ids)`; -1 or any index outside the set: the pose is
    refused on the device).  Vertices: `pts` (M,3) for every pose, or packed (P,3) with `pts_off` / `pts_cnt` (B,), or `meshes=` a
    `lc_amd.render.MeshSet`, whose vertex buffer and per-mesh ranges are read on the device through `mesh_index` (B,)
    (`meshes.index_of(obj_ids)`, -1 refused; default: `obj_index`, for a MeshSet that lists the objects in the SymmetrySet's order).
    Returns dict(mssd, mspd, proj (B,) float32; mssd_sym, mspd_sym (B,) int32: the symmetry that gave each minimum, counted inside the
    object's own transforms, the lowest one among equals).  A refused pose has NaN errors and -1 indices."""
    if not isinstance(syms, SymmetrySet):
        raise TypeError(f"lc_amd.metrics: syms must be a lc_amd.symmetry.SymmetrySet, got {type(syms)}")
    if isinstance(R_est, Tensor) and syms.device != R_est.device:
        raise RuntimeError(f"lc_amd.metrics: the SymmetrySet is on {syms.device}, the poses are on {R_est.device}")
    Re = _f32("R_est", R_est, (None, 3, 3))
    dev, B = Re.device, int(Re.shape[0])
    Rg = _f32("R_gt", R_gt, (B, 3, 3), dev)
    for name, t in (("t_est", t_est), ("t_gt", t_gt)):
        if isinstance(t, Tensor) and tuple(t.shape) not in ((B, 3), (B, 3, 1)):
            raise ValueError(f"lc_amd.metrics: {name} has shape {tuple(t.shape)}, expected {(B, 3)} or {(B, 3, 1)}")
    te = _f32("t_est", t_est.reshape(B, 3) if isinstance(t_est, Tensor) else t_est, (B, 3), dev)
    tg = _f32("t_gt", t_gt.reshape(B, 3) if isinstance(t_gt, Tensor) else t_gt, (B, 3), dev)
    if isinstance(cam_K, Tensor) and tuple(cam_K.shape) == (3, 3):
        cam_K = cam_K.expand(B, 3, 3)  # a view; made contiguous on the device below: nothing is read back
    Kc = _f32("cam_K", cam_K, (B, 3, 3), dev)
    Re, Rg, te, tg, Kc = (_lib.require_hip_f32(n, t) for n, t in (("R_est", Re), ("R_gt", Rg), ("t_est", te), ("t_gt", tg), ("cam_K", Kc)))
    lib = load_symerr()
    idx = _hip_i32("obj_index", obj_index, B, dev)
    if meshes is not None:
        if pts is not None or pts_off is not None or pts_cnt is not None:
            raise ValueError("lc_amd.metrics: give the vertices either as pts [, pts_off, pts_cnt] or as meshes=, not both")
        if not hasattr(meshes, "verts") or not hasattr(meshes, "table"):
            raise TypeError(f"lc_amd.metrics: meshes must be a lc_amd.render.MeshSet, got {type(meshes)}")
        if meshes.device != dev:
            raise RuntimeError(f"lc_amd.metrics: the MeshSet is on {meshes.device}, the poses are on {dev}")
        m = (idx if mesh_index is None else _hip_i32("mesh_index", mesh_index, B, dev)).long()
        known = (m >= 0) & (m < meshes.n_meshes)
        rows = meshes.table[torch.where(known, m, torch.zeros_like(m))]  # (B,4): vert_off, n_vert, face_off, n_face
        zero = torch.zeros_like(rows[:, 0])
        pts_off, pts_cnt = torch.where(known, rows[:, 0], zero).contiguous(), torch.where(known, rows[:, 1], zero).contiguous()
        P = meshes.verts
    else:
        if mesh_index is not None:
            raise ValueError("lc_amd.metrics: mesh_index goes with meshes=")
        if pts is None:
            raise ValueError("lc_amd.metrics: the vertices are missing: pts [, pts_off, pts_cnt] or meshes=")
        if (pts_off is None) != (pts_cnt is None):
            raise ValueError("lc_amd.metrics: pts_off and pts_cnt go together")
        P = pts
        if pts_off is not None:
            pts_off, pts_cnt = _hip_i32("pts_off", pts_off, B, dev), _hip_i32("pts_cnt", pts_cnt, B, dev)
    P = _lib.require_hip_f32("pts", _f32("pts", P, (None, 3), dev))
    if P.shape[0] < 1:
        raise ValueError("lc_amd.metrics: pts holds no vertex")
    err = torch.empty(B, 3, device=dev, dtype=torch.float32)
    arg = torch.empty(B, 2, device=dev, dtype=torch.int32)
    if B:
        nbytes = int(lib.lc_sym_pose_errors_workspace_bytes(B, syms.max_k))
        ws = _sym_workspace(dev, nbytes)
        with _lib.on_device(dev):
            rc = lib.lc_sym_pose_errors_f32(_lib.ptr(Re), _lib.ptr(te), _lib.ptr(Rg), _lib.ptr(tg), _lib.ptr(Kc), _lib.ptr(P), _lib.ptr(pts_off),
                                            _lib.ptr(pts_cnt), P.shape[0], _lib.ptr(idx), _lib.ptr(syms.table), _lib.ptr(syms.obj_off),
                                            _lib.ptr(syms.obj_k), syms.n_obj, syms.total, syms.max_k, B, _lib.ptr(err), _lib.ptr(arg), _lib.ptr(ws),
                                            ws.numel() * 8, _lib.stream_ptr(dev))
        if rc != 0:
            raise RuntimeError(f"lc_amd.lc_sym_pose_errors_f32 failed (code {rc}): {lib.lc_amd_symerr_last_error().decode(errors='replace')}")
    return dict(mssd=err[:, 0], mspd=err[:, 1], proj=err[:, 2], mssd_sym=arg[:, 0], mspd_sym=arg[:, 1])


def sym_pose_errors_from_states(states_est: Tensor, states_gt: Tensor, cam_K: Tensor, *args, **kw) -> dict:
    """Same, from (B,7) quaternion representations, as `pose_errors_from_states`."""
    Re, te = quaternion_rep_to_RT(states_est)
    Rg, tg = quaternion_rep_to_RT(states_gt)
    return compute_sym_pose_errors(Re, te, Rg, tg, cam_K, *args, **kw)
