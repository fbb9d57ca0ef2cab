"""Per-object model preparation on the device (lc_amd/csrc/models/lc_models.hip, lc_amd/_C/liblc_amd_models.so; C ABI and the exact
definitions in include/lc_amd_models.h, `lc_model_prepare_f32`): what BOP's `models_info.json` and the sparse heads' `cfg_global.fps` pickle hold.

    prepare(meshes: MeshSet, fps_count=0, *, want_diameter=True) -> ModelInfo(lo, hi, diameter, pair, fps, fps_index)
    to_models_info(info, obj_ids) -> {obj_id: dict(diameter, min_x, min_y, min_z, size_x, size_y, size_z)}
    to_fps_dict(info, obj_ids)    -> {obj_id: (count, 3) float32 ndarray}     (the format of the reference's assets/fps/lmo.pkl)

All in IEEE fp32, every operation rounded on its own, d2(a, b) = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2:
`lo` / `hi` are the component-wise extents; `diameter` is sqrt of the largest d2 over all vertex pairs i < j and `pair` that pair
(ties: smallest i, then smallest j; one vertex: 0 and (0, 0)); `fps` / `fps_index` are `fps_count` farthest points seeded at the
box centre (lo + hi) * 0.5 -- each pick is the vertex farthest from the centre and the picks so far, lowest index on ties -- so the
first n rows of a result are the n-point result (the loader slices `fps[obj_id][:sparse_cnt]`).  The same meshes give the same
bits on every call.  Runs on the current stream, never waits for the device, can be captured into a graph.  There is no CPU
fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_size_t, c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import build as _build
from .render import MeshSet  # (importing it does not load the render library)

DIAM_TILE = 256        # LC_MODEL_DIAM_TILE: vertices along the edge of one tile of the pair matrix
FPS_RESIDENT = 8192    # LC_MODEL_FPS_RESIDENT: up to here a mesh's coordinates and distances stay in registers during the selection

_SO = _lib.SideLibrary(_build.MODELS, {
    "lc_model_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    # the mesh table is passed twice: on the device, and as a HOST int array the argument rules are checked from
    "lc_model_prepare_f32": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_int), c_int, c_int, c_int] + [c_void_p] * 7 + [c_size_t, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load


class ModelInfo(NamedTuple):
    lo: Tensor                    # (n,3) float32
    hi: Tensor                    # (n,3) float32
    diameter: Optional[Tensor]    # (n,) float32 (want_diameter)
    pair: Optional[Tensor]        # (n,2) int32 vertex indices of the diameter, local to each mesh (want_diameter)
    fps: Optional[Tensor]         # (n,fps_count,3) float32 (fps_count > 0)
    fps_index: Optional[Tensor]   # (n,fps_count) int32 (fps_count > 0)


def workspace_bytes(n_meshes: int, max_verts: int, fps_count: int) -> int:
    """The formula of include/lc_amd_models.h, restated: the library's own answer is `lc_model_workspace_bytes`."""
    if n_meshes <= 0 or max_verts <= 0:
        return 0
    t = -(-max_verts // DIAM_TILE)
    mind = 4 * n_meshes * (-(-max_verts // 4) * 4) if fps_count > 0 and max_verts > FPS_RESIDENT else 0
    return 16 * n_meshes * (t * (t + 1) // 2) + mind


@torch.no_grad()
def prepare(meshes: MeshSet, fps_count: int = 0, *, want_diameter: bool = True, want_extents: bool = True) -> ModelInfo:
    if not isinstance(meshes, MeshSet):
        raise TypeError(f"lc_amd.models: meshes must be a MeshSet, got {type(meshes)}")
    fps_count = int(fps_count)
    counts = meshes.table_host[:, 1]
    if fps_count < 0:
        raise ValueError(f"lc_amd.models: fps_count must not be negative, got {fps_count}")
    if int(counts.min()) < 1:
        raise ValueError(f"lc_amd.models: mesh {int(counts.argmin())} has no vertices")
    if fps_count > int(counts.min()):
        k = int(counts.argmin())
        raise ValueError(f"lc_amd.models: fps_count {fps_count} exceeds the {int(counts[k])} vertices of mesh {k} (object {meshes.obj_ids[k]})")
    if not (want_diameter or want_extents or fps_count):
        raise ValueError("lc_amd.models: nothing to compute")
    n, max_verts, dev = meshes.n_meshes, int(counts.max()), meshes.device
    lib = load()
    lo = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_extents else None
    hi = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_extents else None
    diameter = torch.empty(n, device=dev, dtype=torch.float32) if want_diameter else None
    pair = torch.empty(n, 2, device=dev, dtype=torch.int32) if want_diameter else None
    fps = torch.empty(n, fps_count, 3, device=dev, dtype=torch.float32) if fps_count else None
    fps_index = torch.empty(n, fps_count, device=dev, dtype=torch.int32) if fps_count else None
    nbytes = int(lib.lc_model_workspace_bytes(n, max_verts, fps_count))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    table_host = np.ascontiguousarray(meshes.table_host, dtype=np.int32)
    with _lib.on_device(dev):
        rc = lib.lc_model_prepare_f32(_lib.ptr(meshes.verts), _lib.ptr(meshes.table), table_host.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n,
                                      max_verts, fps_count, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(diameter), _lib.ptr(pair), _lib.ptr(fps),
                                      _lib.ptr(fps_index), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("models.prepare", rc)
    return ModelInfo(lo, hi, diameter, pair, fps, fps_index)


def _ids(info: ModelInfo, obj_ids):
    obj_ids = [int(o) for o in obj_ids]
    n = next(t for t in info if t is not None).shape[0]
    if len(obj_ids) != n:
        raise ValueError(f"lc_amd.models: {len(obj_ids)} object ids for {n} meshes")
    return obj_ids


def to_models_info(info: ModelInfo, obj_ids) -> dict:
    """BOP's models_info.json as a dict keyed by object id: `diameter`, `min_x/y/z`, `size_x/y/z` (size = hi - lo in fp64 of the fp32
    extents), in the unit of the vertices."""
    obj_ids = _ids(info, obj_ids)
    if info.lo is None or info.hi is None or info.diameter is None:
        raise ValueError("lc_amd.models: to_models_info needs the extents and the diameter")
    lo, hi, dia = (np.asarray(t.detach().cpu().numpy() if isinstance(t, Tensor) else t, dtype=np.float64) for t in (info.lo, info.hi, info.diameter))
    out = {}
    for k, oid in enumerate(obj_ids):
        out[oid] = dict(diameter=float(dia[k]), min_x=float(lo[k, 0]), min_y=float(lo[k, 1]), min_z=float(lo[k, 2]),
                        size_x=float(hi[k, 0] - lo[k, 0]), size_y=float(hi[k, 1] - lo[k, 1]), size_z=float(hi[k, 2] - lo[k, 2]))
    return out


def to_fps_dict(info: ModelInfo, obj_ids) -> dict:
    """{obj_id: (count, 3) float32 ndarray}: what `dataset.py:232-236` unpickles into `cfg_global.fps`."""
    obj_ids = _ids(info, obj_ids)
    if info.fps is None:
        raise ValueError("lc_amd.models: to_fps_dict needs the farthest points (fps_count > 0)")
    pts = np.asarray(info.fps.detach().cpu().numpy() if isinstance(info.fps, Tensor) else info.fps, dtype=np.float32)
    return {oid: np.ascontiguousarray(pts[k]) for k, oid in enumerate(obj_ids)}
