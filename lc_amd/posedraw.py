"""A synthetic scene's object poses: the contract in host numpy, and the kernel that draws the same numbers on the device from the seed word
(lc_amd/csrc/posedraw/lc_posedraw.hip, lc_amd/_C/liblc_amd_posedraw.so; C ABI in include/lc_amd_posedraw.h).  What a host loop in front of
the renderer would do for an `imgn`-style split -- draw a rotation per object, place the objects so that they neither interpenetrate nor
leave the frame, upload -- as one launch behind which `shade.render_scene`, `gtinfo.gt_info_from_depth` and the training inputs follow
without the host (lc_amd/synthscene.py chains them).

    draw_scene_poses_host(cfg, seed, scene_ids, mesh_index, radius, cam_K) -> ScenePoses             host numpy: the definition
    draw_scene_poses(cfg, *, seed, scene_id, mesh_index, radius, cam_K) -> ScenePoses                device tensors, one launch
    mesh_radii(meshes) -> (n_meshes,) float32                                                        largest vertex norm, rounded up
    shoemake_libm(u0, u1, u2) -> (...,3,3) float64                                                   the same rotation by numpy's libm

Every number is defined bit for bit, as lc_amd/geometry.py defines its own: fp64 with every product, sum, quotient and square root
rounded on its own, in the order `draw_scene_poses_host` writes them, no FMA, the outputs rounded to fp32 once.  The random numbers are
`augment.u(seed, scene_id, OP_POSE, i)` with i = (m TRIES + k) 8 + d for slot m, try k and draw d: the sample is the scene's id, so a
scene is the same in any batch.  Cosine and sine are `geometry.cos_sin_turns` -- the stated polynomial, never libm -- at u / 2: that
function takes the angle 4 pi x, and x = u / 2 = n / 2^25 with n < 2^24 is reduced as exactly as u itself (tau = 2 x = u, 8 tau and its
fractional part hold 24 bits at the most).

Placement is rejection by at most TRIES tries per slot against the bounding spheres of the slots placed before it; it is stated, not
proven to find a placement that exists.  A slot that is not placed (info < 0) has zeros for R and t and -1 in `mesh_index_out`, which is
what the later stages are given: `render.render_depth` and everything behind it refuse a row whose mesh is unknown, so such a slot gets
no pixel and no record without any new rule.

`draw_scene_poses` reads its seed from one 64-bit word on the device (or takes a whole number), never waits for the device, allocates
its outputs only and can be captured into a graph.  HIP tensors only: there is no CPU fallback -- the host function is the definition,
not a route.
"""
from __future__ import annotations

import math
from ctypes import c_double, c_int, c_void_p
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import augment as _aug
from . import build as _build
from .geometry import cos_sin_turns

MAX_INSTANCES = 64      # LC_POSEDRAW_MAX_INSTANCES
TRIES = 64              # LC_POSEDRAW_TRIES
MAX_SCENES = 1048576    # LC_POSEDRAW_MAX_SCENES
OP_POSE = _aug.OP_HOST + 16  # LC_POSEDRAW_OP_POSE: behind sampler.OP_SPARE and OP_PERM
PLACED, NO_ROOM, REFUSED, EMPTY = 0, -1, -2, -3  # the values of `info`


@dataclass(frozen=True)
class PoseDrawConfig:
    """z_range = (z_min, z_max) of the instances' origins, in the poses' unit; centre_box = (x0, y0, x1, y1) in pixels, within which an
    instance's projected origin is drawn (it may exceed the frame, which gives truncated objects); gap >= 0, the least distance between two
    spheres' surfaces; near, the rasteriser's near plane: a mesh whose sphere reaches it (z_min - r <= near) is refused."""
    z_range: tuple
    centre_box: tuple
    gap: float = 0.0
    near: float = 0.01


class ScenePoses(NamedTuple):
    """numpy arrays (`draw_scene_poses_host`) or device tensors (`draw_scene_poses`)."""
    R: object               # (S,M,3,3) float32, zeros where info != 0
    t: object               # (S,M,3) float32, zeros where info != 0
    tries: object           # (S,M) int32: the try taken; TRIES where info = -1, 0 where info = -2 or -3
    info: object            # (S,M) int32: 0 placed, -1 no good try, -2 refused without a draw, -3 an empty slot
    mesh_index_out: object  # (S,M) int32: mesh_index where info = 0, else -1


_A = _args.Args("posedraw")


def _config(cfg):
    """-> (z_min, z_max, x0, y0, x1, y1, gap, near) as Python floats, checked."""
    if not isinstance(cfg, PoseDrawConfig):
        raise TypeError(f"lc_amd.posedraw: cfg must be a PoseDrawConfig, got {type(cfg)}")
    z_min, z_max = _A.pair("z_range", cfg.z_range)
    box = cfg.centre_box
    if isinstance(box, (Tensor, str)) or not hasattr(box, "__len__") or len(box) != 4:
        raise ValueError(f"lc_amd.posedraw: centre_box is (x0, y0, x1, y1), got {box!r}")
    vals = []
    for name, v in (("z_range", z_min), ("z_range", z_max), ("centre_box", box[0]), ("centre_box", box[1]), ("centre_box", box[2]), ("centre_box", box[3]),
                    ("gap", cfg.gap), ("near", cfg.near)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"lc_amd.posedraw: {name} must hold numbers, got {type(v)}")
        if not math.isfinite(v):
            raise ValueError(f"lc_amd.posedraw: {name} must be finite, got {v}")
        vals.append(float(v))
    z_min, z_max, x0, y0, x1, y1, gap, near = vals
    if z_min > z_max:
        raise ValueError(f"lc_amd.posedraw: z_range = (z_min, z_max) with z_min <= z_max, got {cfg.z_range!r}")
    if x0 > x1 or y0 > y1:
        raise ValueError(f"lc_amd.posedraw: centre_box = (x0, y0, x1, y1) is empty, got {tuple(box)!r}")
    if gap < 0:
        raise ValueError(f"lc_amd.posedraw: gap must not be negative, got {gap}")
    return tuple(vals)


def _slots(M: int):
    if not 1 <= M <= MAX_INSTANCES:
        raise ValueError(f"lc_amd.posedraw: 1 to {MAX_INSTANCES} slots per scene, got M = {M}")


def _quat_to_R(x, y, z, w):
    """The written quaternion-to-matrix formula, term by term: nine products, then one sum or difference and the doubling (exact) each."""
    xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    R = np.empty(np.shape(x) + (3, 3), dtype=np.float64)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)
    return R


def shoemake(u0, u1, u2):
    """The contract's rotation, fp64: q = (sqrt(1 - u0) sin 2 pi u1, sqrt(1 - u0) cos 2 pi u1, sqrt(u0) sin 2 pi u2, sqrt(u0) cos 2 pi u2)
    with `cos_sin_turns` at u / 2 and the correctly rounded square root, then `_quat_to_R`."""
    u0, u1, u2 = (np.asarray(v, dtype=np.float64) for v in (u0, u1, u2))
    a, b = np.sqrt(1.0 - u0), np.sqrt(u0)
    c1, s1 = cos_sin_turns(u1 * 0.5)
    c2, s2 = cos_sin_turns(u2 * 0.5)
    return _quat_to_R(a * s1, a * c1, b * s2, b * c2)


def shoemake_libm(u0, u1, u2):
    """Shoemake's formula by numpy's own sine and cosine: what the contract's polynomial is compared with, never a definition."""
    u0, u1, u2 = (np.asarray(v, dtype=np.float64) for v in (u0, u1, u2))
    a, b = np.sqrt(1.0 - u0), np.sqrt(u0)
    t1, t2 = 2.0 * np.pi * u1, 2.0 * np.pi * u2
    return _quat_to_R(a * np.sin(t1), a * np.cos(t1), b * np.sin(t2), b * np.cos(t2))


def rotation_draws(seed, scene_id, m):
    """(u0, u1, u2) of slot m of a scene: try 0, draws 0, 1, 2."""
    i0 = (np.asarray(m, dtype=np.int64) * TRIES) * 8
    return tuple(_aug.u(seed, scene_id, OP_POSE, i0 + d) for d in range(3))


def candidates(cfg_values, seed, scene_id, m, K):
    """The TRIES candidate positions of slot m of one scene as (TRIES,3) fp64; K (3,3) fp64, widened from fp32."""
    z_min, z_max, x0, y0, x1, y1 = cfg_values[:6]
    i0 = (m * TRIES + np.arange(TRIES, dtype=np.int64)) * 8
    u3, u4, u5 = (_aug.u(seed, scene_id, OP_POSE, i0 + d) for d in (3, 4, 5))
    px = x0 + u3 * (x1 - x0)
    py = y0 + u4 * (y1 - y0)
    z = z_min + u5 * (z_max - z_min)
    yn = (py - K[1, 2]) / K[1, 1]
    xn = ((px - K[0, 2]) - K[0, 1] * yn) / K[0, 0]
    return np.stack((xn * z, yn * z, z), axis=1)


def draw_scene_poses_host(cfg: PoseDrawConfig, seed, scene_ids, mesh_index, radius, cam_K, return_fp64=False) -> ScenePoses:
    """The definition, in host numpy.  scene_ids (S,) int32; mesh_index (S,M) int32, -1 an empty slot; radius (n_meshes,) float32, the
    bounding-sphere radius of each mesh about the model origin in the poses' unit (finite, not negative); cam_K (3,3) or (S,3,3), rounded
    to float32 first (what the device reads) and widened to fp64, skew honoured.

    info, decided before anything is drawn: -3 for mesh_index = -1; -2 for an unknown mesh (below -1 or >= n_meshes), for
    `z_min - r <= near`, and for a K with an entry that is not finite or with K00 or K11 zero.
    Rotation of slot m: `shoemake(u0, u1, u2)` of try 0, draws 0, 1, 2.  Position of slot m at try k: `candidates`.
    Placement, in order m = 0, 1, ...: try k is good when for every earlier PLACED slot j of the scene
    (dx dx + dy dy) + dz dz >= s s with s = (r_m + r_j) + gap, on the fp64 positions; the slot takes the good try of lowest k
    (info 0, tries k) or none (info -1, tries TRIES: it is left out of the scene and blocks no later slot).
    R, t: the fp64 values rounded to float32 once, zeros where info != 0; mesh_index_out = mesh_index where info = 0, else -1.
    `return_fp64` adds the fp64 positions (S,M,3), NaN where info != 0, behind the tuple: (ScenePoses, positions)."""
    values = _config(cfg)
    z_min, gap, near = values[0], values[6], values[7]
    seed = _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    ids = np.asarray(scene_ids)
    mi = np.asarray(mesh_index)
    rad = np.asarray(radius)
    for name, a, kind in (("scene_ids", ids, np.int32), ("mesh_index", mi, np.int32), ("radius", rad, np.float32)):
        if a.dtype != kind:
            raise TypeError(f"lc_amd.posedraw: {name} must be {np.dtype(kind).name}, got {a.dtype}")
    if ids.ndim != 1:
        raise ValueError(f"lc_amd.posedraw: scene_ids has shape {ids.shape}, expected (S,)")
    S = len(ids)
    if mi.ndim != 2 or mi.shape[0] != S:
        raise ValueError(f"lc_amd.posedraw: mesh_index has shape {mi.shape}, expected ({S}, M)")
    M = int(mi.shape[1])
    _slots(M)
    if rad.ndim != 1 or len(rad) < 1:
        raise ValueError(f"lc_amd.posedraw: radius has shape {rad.shape}, expected (n_meshes,)")
    if not np.isfinite(rad).all() or (rad < 0).any():
        raise ValueError("lc_amd.posedraw: radius must be finite and not negative")
    K32 = np.asarray(cam_K, dtype=np.float32)
    if K32.shape not in ((3, 3), (S, 3, 3)):
        raise ValueError(f"lc_amd.posedraw: cam_K has shape {K32.shape}, expected (3, 3) or ({S}, 3, 3)")
    Ks = np.broadcast_to(K32, (S, 3, 3)).astype(np.float64)
    r64 = rad.astype(np.float64)

    R = np.zeros((S, M, 3, 3), dtype=np.float32)
    t = np.zeros((S, M, 3), dtype=np.float32)
    tries = np.zeros((S, M), dtype=np.int32)
    info = np.full((S, M), EMPTY, dtype=np.int32)
    out = np.full((S, M), -1, dtype=np.int32)
    pos = np.full((S, M, 3), np.nan, dtype=np.float64)
    with np.errstate(all="ignore"):
        for s in range(S):
            K = Ks[s]
            K_ok = bool(np.isfinite(K).all() and K[0, 0] != 0.0 and K[1, 1] != 0.0)
            placed = []  # (position, radius) of the scene's placed slots
            for m in range(M):
                k = int(mi[s, m])
                if k == -1:
                    continue
                if not (0 <= k < len(rad)) or not K_ok or not (z_min - r64[k] > near):
                    info[s, m] = REFUSED
                    continue
                cand = candidates(values, seed, ids[s], m, K)
                good = np.ones(TRIES, dtype=bool)
                for pj, rj in placed:
                    sep = (r64[k] + rj) + gap
                    d = cand - pj
                    good &= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] >= sep * sep
                if not good.any():
                    info[s, m], tries[s, m] = NO_ROOM, TRIES
                    continue
                take = int(np.argmax(good))
                placed.append((cand[take], r64[k]))
                info[s, m], tries[s, m], out[s, m] = PLACED, take, k
                pos[s, m] = cand[take]
                t[s, m] = cand[take].astype(np.float32)
                R[s, m] = shoemake(*rotation_draws(seed, ids[s], m)).astype(np.float32)
    res = ScenePoses(R, t, tries, info, out)
    return (res, pos) if return_fp64 else res


def mesh_radii(meshes) -> np.ndarray:
    """(n_meshes,) float32: each mesh's largest vertex norm about the model origin, formed in fp64 from the set's float32 vertices and
    rounded UP to float32, so that the sphere holds every vertex.  `meshes`: a `render.MeshSet` (read back once) or a list of
    (verts, faces) arrays."""
    from . import render as _render

    if isinstance(meshes, _render.MeshSet):
        verts = meshes.verts.cpu().numpy()
        per_mesh = [verts[vo:vo + nv] for vo, nv, _, _ in meshes.table_host.tolist()]
    else:
        per_mesh = [np.asarray(v.detach().cpu().numpy() if isinstance(v, Tensor) else v, dtype=np.float32) for v, _ in meshes]
    out = np.zeros(len(per_mesh), dtype=np.float32)
    for k, v in enumerate(per_mesh):
        if len(v):
            r = float(np.sqrt((v.astype(np.float64) ** 2).sum(axis=1).max())) * (1.0 + 2.0 ** -50)  # above the fp64 rounding of the norm
            r32 = np.float32(r)
            out[k] = r32 if float(r32) >= r else np.nextafter(r32, np.float32(np.inf))
    return out


# ---- the device --------------------------------------------------------------------------------------------------------------------
_SO = _lib.SideLibrary(_build.POSEDRAW, {
    "lc_posedraw_scenes_f32": (c_int, [c_double] * 8 + [c_void_p] * 4 + [c_int, c_void_p] + [c_int] * 3 + [c_void_p] * 6),
})
_SIGNATURES, load = _SO.signatures, _SO.load


@torch.no_grad()
def draw_scene_poses(cfg: PoseDrawConfig, *, seed, scene_id, mesh_index, radius, cam_K) -> ScenePoses:
    """`draw_scene_poses_host(cfg, seed, scene_id, mesh_index, radius, cam_K)` as device tensors, bit for bit, in one launch
    (`lc_posedraw_scenes_f32` of include/lc_amd_posedraw.h).

    seed: a whole number below 2^64, or a device tensor of one uint64 / int64 element that the KERNEL reads (`augment.augment_drawn`'s
    rule: the same word serves every drawn stage).  scene_id (S,) int32, mesh_index (S,M) int32 with M of 1 to MAX_INSTANCES, radius
    (n_meshes,) float32 and cam_K (3,3) or (S,3,3) float32, all on the device.  The radii cannot be looked at without waiting for the
    device: a slot whose radius is negative or not finite is refused by the kernel (info = -2) where the host function raises."""
    values = _config(cfg)
    scene_id = _A.tensor("scene_id", scene_id, (torch.int32,), "int32", (None,))
    S = int(scene_id.shape[0])
    if S > MAX_SCENES:
        raise ValueError(f"lc_amd.posedraw: at most {MAX_SCENES} scenes, got {S}")
    mesh_index = _A.tensor("mesh_index", mesh_index, (torch.int32,), "int32", (S, None))
    M = int(mesh_index.shape[1])
    _slots(M)
    radius = _A.f32("radius", radius, (None,))
    n_meshes = int(radius.shape[0])
    if n_meshes < 1:
        raise ValueError("lc_amd.posedraw: radius holds one value per mesh, at least one")
    one_camera = isinstance(cam_K, Tensor) and tuple(cam_K.shape) == (3, 3)
    cam_K = _A.f32("cam_K", cam_K, (3, 3) if one_camera else (S, 3, 3))
    if not isinstance(seed, Tensor):
        _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    elif seed.dtype not in (torch.uint64, torch.int64) or seed.numel() != 1:
        raise TypeError(f"lc_amd.posedraw: a seed tensor holds one uint64 or int64 element, got {seed.dtype} of shape {tuple(seed.shape)}")
    if not scene_id.is_cuda:
        raise RuntimeError(f"lc_amd.posedraw: scene_id is on {scene_id.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = scene_id.device
    _A.same_device(dev, "scene_id on {}", mesh_index=mesh_index, radius=radius, cam_K=cam_K)
    word = _aug._seed_word(seed, dev)
    sid, mi, rad, K = scene_id.contiguous(), mesh_index.contiguous(), radius.contiguous(), cam_K.contiguous()

    def made(shape, dtype):
        return torch.empty(shape, device=dev, dtype=dtype)

    R, t = made((S, M, 3, 3), torch.float32), made((S, M, 3), torch.float32)
    tries, info, out = made((S, M), torch.int32), made((S, M), torch.int32), made((S, M), torch.int32)
    if S:
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_posedraw_scenes_f32(*values, _lib.ptr(word), _lib.ptr(sid), _lib.ptr(mi), _lib.ptr(rad), n_meshes, _lib.ptr(K), 0 if one_camera else 9,
                                            S, M, _lib.ptr(R), _lib.ptr(t), _lib.ptr(tries), _lib.ptr(info), _lib.ptr(out), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("posedraw.draw_scene_poses", rc)
    return ScenePoses(R, t, tries, info, out)
