"""The oriented model box on the device (lc_amd/csrc/obox/lc_obox.hip, lc_amd/_C/liblc_amd_obox.so; C ABI and the exact definitions in
include/lc_amd_obox.h, `lc_obox_search_f32`): what the reference's `models_xform.json` holds per object (model_transform.py:21-42).

    oriented_box(meshes: MeshSet, *, axis=None, levels=6) -> OrientedBox(xform, noc_scale, volume, aabb_volume, path, info)
    to_models_xform(box, obj_ids) -> {"<obj_id>": {"xform": 16 numbers row-major, "xformed_noc_scale": 3 numbers}}
    delta_table(axis, levels)     -> (deltas (n_level0 + levels * n_refine, 4) float64, n_level0, n_refine)
    workspace_bytes(n_meshes, axis=None, levels=6)

The rotation is SEARCHED: over a stated hierarchical grid of rotations (all orientations modulo the cube's 24, or the turns about one model
axis), the candidate whose bounding box of the rotated vertices has the least volume; every level refines around the winner of the one
before with half the step.  It is not a proven global minimum.  A candidate's matrix is formed in fp64 and rounded once to fp32; its score
is fp32, every operation rounded on its own; ties go to the lowest index.  `xform` is `[R | t; 0 0 0 1]` with `t = -centre` of the box,
`noc_scale` the half-extents, `volume` the winning score, `aabb_volume` the identity's, `path` the winning index of every level, `info` 1 for
a mesh with a coordinate that is not finite.  The same meshes give the same bits on every call.  Runs on the current stream, never waits for
the device, reads nothing back, can be captured into a graph.  There is no CPU fallback (tests/obox_oracle.py is the numpy restatement).
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_int, c_size_t, c_void_p
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import build as _build
from .render import MeshSet  # (importing it does not load the render library)

TILE = 256              # LC_OBOX_TILE: vertices of one LDS tile
SPLIT = 1024            # LC_OBOX_SPLIT: vertices of one workgroup's chunk; a larger mesh is split over workgroups
MAX_LEVELS = 16         # LC_OBOX_MAX_LEVELS
MAX_CAND = 65536        # LC_OBOX_MAX_CAND
STEP0_DEG = 9           # LC_OBOX_STEP0_DEG: the step of level 0, pi / 20
GRID_RADIUS = 7         # LC_OBOX_GRID_RADIUS: level 0 holds the rotation vectors of at most this many steps
LEVEL0_COUNT = 1419     # LC_OBOX_LEVEL0_COUNT
AXIS_LEVEL0_COUNT = 10  # LC_OBOX_AXIS_LEVEL0_COUNT
DEFAULT_LEVELS = 6
STEP0 = math.pi / 20.0

_SO = _lib.SideLibrary(_build.OBOX, {
    "lc_obox_workspace_bytes": (c_size_t, [c_int, c_int]),
    # the mesh table is passed twice: on the device, and as a HOST int array the argument rules are checked from
    "lc_obox_search_f32": (c_int, [c_void_p, c_int, c_void_p, ctypes.POINTER(c_int), c_int, c_int, c_void_p, c_int, c_int, c_int] + [c_void_p] * 7 +
                           [c_size_t, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load


class OrientedBox(NamedTuple):
    xform: Tensor        # (n,4,4) float32: [R | t; 0 0 0 1]
    noc_scale: Tensor    # (n,3) float32: half-extents of the box in the transformed frame
    volume: Tensor       # (n,) float32: the winning score
    aabb_volume: Tensor  # (n,) float32: the score of the identity
    path: Tensor         # (n,levels+1) int32: the winning candidate of every level
    info: Tensor         # (n,) int32: 0, or 1 for a coordinate that is not finite


def _axis(axis):
    if axis is None:
        return None
    if isinstance(axis, str) and axis in ("x", "y", "z"):
        return "xyz".index(axis)
    if isinstance(axis, (int, np.integer)) and not isinstance(axis, bool) and 0 <= int(axis) <= 2:
        return int(axis)
    raise ValueError(f"lc_amd.obox: axis must be None, 0, 1, 2 or 'x', 'y', 'z', got {axis!r}")


def _levels(levels):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"lc_amd.obox: levels must be an integer in 0..{MAX_LEVELS}, got {levels!r}")
    return int(levels)


def _vectors(axis, reach, ball):
    """The integer rotation vectors of a table by ascending (n2, i, j, k): all with components in -reach..reach (and n2 <= ball), or those
    along `axis` alone."""
    span = range(-reach, reach + 1)
    if axis is None:
        pts = [(i, j, k) for i in span for j in span for k in span]
    else:
        pts = [tuple(s if a == axis else 0 for a in range(3)) for s in span]
    pts = [p for p in pts if ball is None or p[0] * p[0] + p[1] * p[1] + p[2] * p[2] <= ball]
    return sorted(pts, key=lambda p: (p[0] * p[0] + p[1] * p[1] + p[2] * p[2], p))


def _quats(vectors, step):
    out = np.zeros((len(vectors), 4), np.float64)
    for r, (i, j, k) in enumerate(vectors):
        n2 = i * i + j * j + k * k
        if n2 == 0:
            out[r] = (1.0, 0.0, 0.0, 0.0)
            continue
        root = math.sqrt(float(n2))
        h = (step * root) * 0.5
        f = math.sin(h) / root
        out[r] = (math.cos(h), i * f, j * f, k * f)
    return out


def delta_table(axis=None, levels: int = DEFAULT_LEVELS):
    """The stated tables of include/lc_amd_obox.h as one (n_level0 + levels * n_refine, 4) float64 array of unit quaternions (w, x, y, z),
    with n_level0 and n_refine."""
    axis, levels = _axis(axis), _levels(levels)
    if axis is None:
        level0 = _vectors(None, GRID_RADIUS, GRID_RADIUS * GRID_RADIUS)
    else:
        level0 = [tuple(s if a == axis else 0 for a in range(3)) for s in range(AXIS_LEVEL0_COUNT)]
    refine = _vectors(axis, 2, None)
    parts = [_quats(level0, STEP0)] + [_quats(refine, STEP0 / 2.0 ** l) for l in range(1, levels + 1)]
    return np.ascontiguousarray(np.concatenate(parts, 0)), len(level0), len(refine)


def workspace_bytes(n_meshes: int, axis=None, levels: int = DEFAULT_LEVELS) -> int:
    """The formula of include/lc_amd_obox.h for the stated tables, restated: the library's own answer is `lc_obox_workspace_bytes`."""
    axis, levels = _axis(axis), _levels(levels)
    if n_meshes <= 0:
        return 0
    n0, n1 = (LEVEL0_COUNT, 125) if axis is None else (AXIS_LEVEL0_COUNT, 5)
    max_cand = max(n0, n1) if levels else n0
    return 32 * n_meshes + -(-4 * n_meshes // 16) * 16 + 24 * n_meshes * max_cand


_TABLES = {}


def _device_table(axis, levels, dev):
    key = (axis, levels, str(dev))
    if key not in _TABLES:
        deltas, n0, n1 = delta_table(axis, levels)
        _TABLES[key] = (torch.from_numpy(deltas).to(dev), n0, n1)
    return _TABLES[key]


@torch.no_grad()
def oriented_box(meshes: MeshSet, *, axis=None, levels: int = DEFAULT_LEVELS) -> OrientedBox:
    if not isinstance(meshes, MeshSet):
        raise TypeError(f"lc_amd.obox: meshes must be a MeshSet, got {type(meshes)}")
    axis, levels = _axis(axis), _levels(levels)
    counts = meshes.table_host[:, 1]
    if int(counts.min()) < 1:
        raise ValueError(f"lc_amd.obox: mesh {int(counts.argmin())} has no vertices")
    n, max_verts, dev = meshes.n_meshes, int(counts.max()), meshes.device
    lib = load()
    deltas, n0, n1 = _device_table(axis, levels, dev)  # (uploaded on the first call of a kind: capture a graph after a warm-up call)
    xform = torch.empty(n, 4, 4, device=dev, dtype=torch.float32)
    noc_scale = torch.empty(n, 3, device=dev, dtype=torch.float32)
    volume = torch.empty(n, device=dev, dtype=torch.float32)
    aabb_volume = torch.empty(n, device=dev, dtype=torch.float32)
    path = torch.empty(n, levels + 1, device=dev, dtype=torch.int32)
    info = torch.empty(n, device=dev, dtype=torch.int32)
    nbytes = int(lib.lc_obox_workspace_bytes(n, max(n0, n1) if levels else n0))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    table_host = np.ascontiguousarray(meshes.table_host, dtype=np.int32)
    with _lib.on_device(dev):
        rc = lib.lc_obox_search_f32(_lib.ptr(meshes.verts), meshes.total_verts, _lib.ptr(meshes.table), table_host.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                    n, max_verts, _lib.ptr(deltas), n0, n1, levels, _lib.ptr(xform), _lib.ptr(noc_scale), _lib.ptr(volume),
                                    _lib.ptr(aabb_volume), _lib.ptr(path), _lib.ptr(info), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("obox.oriented_box", rc)
    return OrientedBox(xform, noc_scale, volume, aabb_volume, path, info)


def _host(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, Tensor) else t)


def to_models_xform(box, obj_ids) -> dict:
    """The reference's models_xform.json as a dict: the object id as a string -> {"xform": 16 numbers row-major, "xformed_noc_scale": 3
    numbers}.  Every number is the fp32 value as the Python float of the same value, which `json` prints so that it reads back exactly:
    `np.float32(json)` gives the same bits (`model_transform.py:35-37` reads the file as float32)."""
    obj_ids = [int(o) for o in obj_ids]
    xform, scale = _host(box.xform).astype(np.float32, copy=False), _host(box.noc_scale).astype(np.float32, copy=False)
    if xform.ndim != 3 or xform.shape[1:] != (4, 4) or scale.shape != (xform.shape[0], 3):
        raise ValueError(f"lc_amd.obox: xform must be (n,4,4) and noc_scale (n,3), got {xform.shape} and {scale.shape}")
    if len(obj_ids) != xform.shape[0] or len(set(obj_ids)) != len(obj_ids):
        raise ValueError(f"lc_amd.obox: {len(obj_ids)} object ids for {xform.shape[0]} meshes (each once)")
    return {str(o): {"xform": [float(x) for x in xform[k].reshape(16)], "xformed_noc_scale": [float(x) for x in scale[k]]} for k, o in enumerate(obj_ids)}
