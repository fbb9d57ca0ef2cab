"""Batched pose-error metrics on the GPU: `lib/utils/evaluate.py:333-339 compute_pose_errors`
(= `lib/utils/error6d.py` add / adi / re / te) for a whole test set in one launch, and the symmetry-aware BOP errors of
`error6d.py:36-84,157-172` (mssd, mspd, proj) with each object's symmetries read from a `SymmetrySet`'s device table."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_void_p

import torch
from torch import Tensor

from . import _args, _lib
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


_SYMERR = _lib.SideLibrary(_build.SYMERR, {
    "lc_sym_pose_errors_workspace_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "lc_sym_pose_errors_f32": (c_int, [c_void_p] * 8 + [c_int] + [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3 + [ctypes.c_size_t, c_void_p]),
})
_SYMERR_SIGNATURES, load_symerr = _SYMERR.signatures, _SYMERR.load  # liblc_amd_symerr.so (C ABI in include/lc_amd_symerr.h)
_A = _args.Args("metrics")
_POSES_ON = "the poses are on {}"


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
    _A.same_device(dev, _POSES_ON, **{name: _A.i32(name, t, (B,))})
    return t.to(torch.int32).contiguous()


def _f32(name: str, t, shape, dev=None) -> Tensor:
    """Type, element type (the 16-bit floats pass: _lib.require_hip_f32 up-casts them once every tensor has passed), shape (None: any
    size) and the device of the poses."""
    _A.tensor(name, t, (torch.float32, torch.float16, torch.bfloat16), "float32 (reference I/O precision)", shape)
    if dev is not None:
        _A.same_device(dev, _POSES_ON, **{name: t})
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
    dev = R_est.device if isinstance(R_est, Tensor) else None  # (anything else is refused by the first rule below)
    B, (Re, Rg), (te, tg), Kc = _A.pose_batch(None, dict(R_est=R_est, R_gt=R_gt), dict(t_est=t_est, t_gt=t_gt), cam_K, "cam_K",
                                              lambda name, t, shape: _f32(name, t, shape, dev))
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
            _SYMERR.fail("lc_sym_pose_errors_f32", rc)
    return dict(mssd=err[:, 0], mspd=err[:, 1], proj=err[:, 2], mssd_sym=arg[:, 0], mspd_sym=arg[:, 1])


def sym_pose_errors_from_states(states_est: Tensor, states_gt: Tensor, cam_K: Tensor, *args, **kw) -> dict:
    """Same, from (B,7) quaternion representations, as `pose_errors_from_states`."""
    Re, te = quaternion_rep_to_RT(states_est)
    Rg, tg = quaternion_rep_to_RT(states_gt)
    return compute_sym_pose_errors(Re, te, Rg, tg, cam_K, *args, **kw)
