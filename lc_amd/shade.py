"""Shaded colour images of posed meshes on the device (lc_amd/csrc/shade/lc_shade.hip, lc_amd/_C/liblc_amd_shade.so; C ABI and the exact
definition of every byte in include/lc_amd_shade.h): what the reference draws with its vendored OpenGL renderer for the rendered,
background-less `imgn` split (`tools/lib/meshrenderer/meshrenderer_phong.py:125-165`, `dataset.py:413`).

    vertex_normals(verts, faces) -> (Nv,3) float32                     area-weighted vertex normals, on the host, once per dataset
    Appearance(meshes, colors=None, normals=None)                      per-vertex colours and normals of a MeshSet on the device
    shade(meshes, appearance, face, mesh_index, R, t, K, *, light, phong, ...) -> out (B,h,w,3) uint8
    shade_scene(meshes, appearance, frames, instance, face, mesh_index, scene_index, R, t, K, *, light, phong, ...) -> frames, in place
    render_color(meshes, appearance, mesh_index, R, t, K, size_hw, *, near, far, light, phong, background=None) -> (frames, Rendered)
    render_scene(meshes, appearance, mesh_index, scene_index, R, t, K, frame_hw, n_scenes, *, near, far, light, phong, background=None)
        -> (frames (S,H,W,3) uint8, SceneDepth)

The rasteriser says which face a pixel sees (`render.render_depth(want_face=True)`), the composition which instance
(`gtinfo.compose_scene_depth(want_instance=True)`); the shading pass interpolates colour, normal and position with perspective-correct
weights and lights them with a Phong model of exponent 1 and a one-sided normal, all in fp64 with every operation rounded on its own.
Only hit pixels are written: the frames keep whatever they held elsewhere -- zeros, a photograph, a `BackgroundStore` cut.  The frames are
(…,H,W,3) uint8, what `crops.warp_affine` and `train_inputs.train_inputs` read; a scene's depth and instance maps feed
`gtinfo.gt_info_from_depth`.

`light` is the light's position in camera coordinates (x right, y down, z forward) and `phong` = (ka, kd, ks), each (3,) for every row
or (B,3), as float32 tensors on the device or as three numbers.  Randomised lighting is the caller's tensors, made with `torch.rand` on the
device: a replayed graph then lights anew (numbers, not tensors, are uploaded at the call and cannot be captured).

HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device, allocates its
outputs only and can be captured into a graph.  `info` (B,) int32: 0, 1 where a pixel of the row was refused (a face or vertex index
outside its mesh; in a scene a window pixel outside the maps or a row of another scene), -1 for a refused row (an unknown mesh).
"""
from __future__ import annotations

from ctypes import c_float, c_int, c_void_p

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build
from . import gtinfo as _gtinfo
from . import render as _render
from .render import MeshSet

MAX_SIZE = 16384  # LC_SHADE_MAX_SIZE
DEFAULT_LIGHT = (400.0, -400.0, -400.0)  # the reference's (400, 400, 400) of its OpenGL camera (y up, z backward) in this camera frame
DEFAULT_PHONG = (0.4, 0.8, 0.3)          # ambient, diffuse, specular

_MESH = [c_void_p] * 5 + [c_int] * 3
_SO = _lib.SideLibrary(_build.SHADE, {
    "lc_shade_instances_u8": (c_int, _MESH + [c_void_p] * 7 + [c_int] * 3 + [c_float] * 2 + [c_void_p] * 3),
    "lc_shade_scene_u8": (c_int, _MESH + [c_void_p] * 9 + [c_int] * 3 + [c_float] * 2 + [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 2),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("shade")


def vertex_normals(verts, faces) -> np.ndarray:
    """(Nv,3) float32: every face's cross product (V1 - V0) x (V2 - V0) -- twice its area along its normal -- added to its three vertices
    in face order, the sum normalised in fp64 and rounded to fp32; a vertex whose sum is zero (no face, or faces that cancel) stays zero."""
    V = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError(f"lc_amd.shade: face indices must lie in [0, {len(V)}), got [{F.min()}, {F.max()}]")
    cross = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    acc = np.zeros_like(V)
    for k in range(3):
        np.add.at(acc, F[:, k], cross)
    length = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
    with np.errstate(all="ignore"):
        unit = np.where(length[:, None] > 0, acc / length[:, None], 0.0)
    return unit.astype(np.float32)


class Appearance:
    """What the shading pass needs beside a MeshSet's geometry: `colors` (total_verts,3) uint8 and `normals` (total_verts,3) float32 on the
    device, concatenated in the set's order.  `colors` and `normals` are lists with one (Nv,3) array or tensor (or None) per mesh;
    colors None means mid-grey 128, normals None means `vertex_normals` of the mesh.  Validated on the host, uploaded once."""

    def __init__(self, meshes: MeshSet, colors=None, normals=None):
        if not isinstance(meshes, MeshSet):
            raise TypeError(f"lc_amd.shade: meshes must be a MeshSet, got {type(meshes)}")
        n = meshes.n_meshes
        for name, seq in (("colors", colors), ("normals", normals)):
            if seq is not None and (isinstance(seq, (Tensor, np.ndarray)) or not hasattr(seq, "__len__") or len(seq) != n):
                raise ValueError(f"lc_amd.shade: {name} is a list of one (Nv,3) array per mesh ({n}), or None")
        verts = faces = None
        cs, ns = [], []
        for k, (vo, nv, fo, nf) in enumerate(meshes.table_host.tolist()):
            c = None if colors is None else colors[k]
            if c is None:
                c = np.full((nv, 3), 128, dtype=np.uint8)
            else:
                c = np.ascontiguousarray(c.detach().cpu().numpy() if isinstance(c, Tensor) else c)
                if c.dtype != np.uint8:
                    raise TypeError(f"lc_amd.shade: mesh {k}: colors must be uint8, got {c.dtype}")
                if c.shape != (nv, 3):
                    raise ValueError(f"lc_amd.shade: mesh {k}: colors has shape {c.shape}, expected {(nv, 3)}")
            m = None if normals is None else normals[k]
            if m is None:
                if verts is None:  # the set's own arrays, read back once
                    verts, faces = meshes.verts.cpu().numpy(), meshes.faces.cpu().numpy()
                m = vertex_normals(verts[vo:vo + nv], faces[fo:fo + nf])
            else:
                m = np.ascontiguousarray(m.detach().cpu().numpy() if isinstance(m, Tensor) else m)
                if not np.issubdtype(m.dtype, np.floating):
                    raise TypeError(f"lc_amd.shade: mesh {k}: normals must hold floats, got {m.dtype}")
                if m.shape != (nv, 3):
                    raise ValueError(f"lc_amd.shade: mesh {k}: normals has shape {m.shape}, expected {(nv, 3)}")
                m = m.astype(np.float32)
                if not np.isfinite(m).all():
                    raise ValueError(f"lc_amd.shade: mesh {k}: normals must be finite")
            cs.append(c)
            ns.append(m)
        self.meshes = meshes
        self.colors_host, self.normals_host = np.concatenate(cs, 0).reshape(-1, 3), np.concatenate(ns, 0).reshape(-1, 3)
        self.colors = torch.from_numpy(self.colors_host).to(meshes.device)
        self.normals = torch.from_numpy(self.normals_host).to(meshes.device)


def _per_row(name: str, v, B: int, dev) -> Tensor:
    """light or phong as a contiguous (B,3) float32 tensor on the device: a tensor of (3,) or (B,3), or three numbers."""
    if not isinstance(v, Tensor):
        vals = np.asarray(v, dtype=np.float64).reshape(-1) if hasattr(v, "__len__") and not isinstance(v, str) else None
        if vals is None or vals.shape != (3,) or not np.isfinite(vals).all():
            raise ValueError(f"lc_amd.shade: {name} is three finite numbers or a float32 tensor of shape (3,) or {(B, 3)}, got {v!r}")
        v = torch.tensor(vals.astype(np.float32), device=dev)
    v = _lib.require_hip_f32(name, v)
    if tuple(v.shape) == (3,):
        v = v.expand(B, 3)
    _A.rows(name, v, (B, 3))
    return v.contiguous()


def _rows(meshes, appearance, face, mesh_index, R, t, K, light, phong, pixel_center):
    """The rules the two forms share -> (B, h, w, dev, the contiguous row tensors, (cx, cy))."""
    if not isinstance(meshes, MeshSet):
        raise TypeError(f"lc_amd.shade: meshes must be a MeshSet, got {type(meshes)}")
    if not isinstance(appearance, Appearance):
        raise TypeError(f"lc_amd.shade: appearance must be an Appearance, got {type(appearance)}")
    if appearance.meshes is not meshes:
        raise ValueError("lc_amd.shade: appearance was made for another MeshSet")
    face = _A.tensor("face", face, (torch.int32,), "int32", (None, None, None))
    B, h, w = (int(n) for n in face.shape)
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f"lc_amd.shade: map sizes of 1 to {MAX_SIZE}, got {h} x {w}")
    def f32(name, x, shape):
        x = _lib.require_hip_f32(name, x)
        _A.rows(name, x, shape)
        return x

    rows, (R,), (t,), K = _A.pose_batch(mesh_index, {"R": R}, {"t": t}, K, f32=f32)
    if rows != B:
        raise ValueError(f"lc_amd.shade: mesh_index has shape {tuple(mesh_index.shape)}, expected {(B,)}")
    cx, cy = _A.center(pixel_center)
    dev = meshes.device
    if not face.is_cuda:
        raise RuntimeError(f"lc_amd.shade: face is on {face.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    light, phong = _per_row("light", light, B, dev), _per_row("phong", phong, B, dev)
    _A.same_device(dev, _args.MESHES_ON, face=face, mesh_index=mesh_index, R=R, t=t, K=K, light=light, phong=phong)
    return B, h, w, dev, (mesh_index.contiguous(), R, t, K.contiguous(), light, phong, face.contiguous()), (cx, cy)


def _mesh_args(meshes, appearance):
    return (_lib.ptr(meshes.verts), _lib.ptr(appearance.normals), _lib.ptr(appearance.colors), _lib.ptr(meshes.faces), _lib.ptr(meshes.table),
            meshes.n_meshes, meshes.total_verts, meshes.total_faces)


def _info(info, B: int, dev) -> Tensor:
    if info is None:
        return torch.empty(B, device=dev, dtype=torch.int32)
    info = _A.tensor("info", info, (torch.int32,), "int32", (B,))
    _A.same_device(dev, _args.MESHES_ON, info=info)
    if not info.is_contiguous():
        raise ValueError("lc_amd.shade: info must be contiguous")
    return info


@torch.no_grad()
def shade(meshes: MeshSet, appearance: Appearance, face, mesh_index, R, t, K, *, light, phong, pixel_center=(0.5, 0.5), out=None, info=None) -> Tensor:
    """out (B,h,w,3) uint8: the hit pixels of `face` (B,h,w) int32 (`render_depth(..., want_face=True).face`, rendered with the same
    mesh_index, R, t, K and pixel_center) shaded; every other pixel keeps the byte `out` held (a new `out` is zeros).  `info` (B,) int32, if
    given, receives the rows' records (see the module's head)."""
    B, h, w, dev, rows, (cx, cy) = _rows(meshes, appearance, face, mesh_index, R, t, K, light, phong, pixel_center)
    if out is None:
        out = torch.zeros(B, h, w, 3, device=dev, dtype=torch.uint8)
    else:
        out = _A.tensor("out", out, (torch.uint8,), "uint8", (B, h, w, 3))
        _A.same_device(dev, _args.MESHES_ON, out=out)
        if not out.is_contiguous():
            raise ValueError(f"lc_amd.shade: out must be contiguous (hit pixels are written in place), got strides {tuple(out.stride())}")
    info = _info(info, B, dev)
    if B:
        with _lib.on_device(dev):
            rc = load().lc_shade_instances_u8(*_mesh_args(meshes, appearance), *(_lib.ptr(x) for x in rows), B, h, w, cx, cy, _lib.ptr(out), _lib.ptr(info),
                                              _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("shade.shade", rc)
    return out


@torch.no_grad()
def shade_scene(meshes: MeshSet, appearance: Appearance, frames, instance, face, mesh_index, scene_index, R, t, K, *, light, phong, origin_xy=None,
                pixel_center=(0.5, 0.5), info=None) -> Tensor:
    """IN PLACE in frames (S,H,W,3) uint8, contiguous: frame pixel (X,Y) of scene s takes row b = instance[s,Y,X] (`compose_scene_depth(...,
    want_instance=True).instance`; -1: untouched) and is shaded as window pixel (X - x0_b, Y - y0_b) of row b's `face` map with the row's
    mesh, pose, K, light and phong.  origin_xy (B,2) int32 / int64 places the (h,w) maps in the frame, anywhere; None: full-frame maps.
    scene_index (B,) int32 / int64.  -> frames."""
    B, h, w, dev, rows, (cx, cy) = _rows(meshes, appearance, face, mesh_index, R, t, K, light, phong, pixel_center)
    frames = _A.tensor("frames", frames, (torch.uint8,), "uint8", (None, None, None, 3))
    S, H, W = (int(n) for n in frames.shape[:3])
    if S < 1 or not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f"lc_amd.shade: at least one frame, of sizes of 1 to {MAX_SIZE}, got {S} of {H} x {W}")
    instance = _A.tensor("instance", instance, (torch.int32,), "int32", (S, H, W))
    _A.i32("scene_index", scene_index, (B,))
    if origin_xy is not None:
        _A.i32("origin_xy", origin_xy, (B, 2))
    elif (h, w) != (H, W):
        raise ValueError(f"lc_amd.shade: without origin_xy the maps ({h} x {w}) must have the frame's size ({H} x {W})")
    if not frames.is_contiguous():
        raise ValueError(f"lc_amd.shade: frames must be contiguous (hit pixels are written in place), got strides {tuple(frames.stride())}")
    _A.same_device(dev, _args.MESHES_ON, frames=frames, instance=instance, scene_index=scene_index, origin_xy=origin_xy)
    idx = scene_index.to(torch.int32).contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    inst = instance.contiguous()
    info = _info(info, B, dev)
    if B:
        mesh_index, Rc, tc, Kc, light, phong, face = rows
        with _lib.on_device(dev):
            rc = load().lc_shade_scene_u8(*_mesh_args(meshes, appearance), _lib.ptr(mesh_index), _lib.ptr(idx), _lib.ptr(Rc), _lib.ptr(tc), _lib.ptr(Kc),
                                          _lib.ptr(light), _lib.ptr(phong), _lib.ptr(face), _lib.ptr(org), B, h, w, cx, cy, _lib.ptr(inst), _lib.ptr(frames),
                                          S, H, W, _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("shade.shade_scene", rc)
    return frames


def _canvas(background, shape, dev) -> Tensor:
    """The frames the shading writes into: zeros, or a copy of `background` (the caller's tensor is left as it is)."""
    if background is None:
        return torch.zeros(shape, device=dev, dtype=torch.uint8)
    background = _A.tensor("background", background, (torch.uint8,), "uint8", shape)
    _A.same_device(dev, _args.MESHES_ON, background=background)
    return background.clone(memory_format=torch.contiguous_format)


@torch.no_grad()
def render_color(meshes: MeshSet, appearance: Appearance, mesh_index, R, t, K, size_hw, *, near, far, light, phong, background=None,
                 pixel_center=(0.5, 0.5)):
    """(frames (B,H,W,3) uint8, Rendered): `render.render_depth(..., want_face=True)` and `shade` over zeros, or over a copy of
    `background` (B,H,W,3) uint8."""
    if not isinstance(appearance, Appearance):
        raise TypeError(f"lc_amd.shade: appearance must be an Appearance, got {type(appearance)}")
    rendered = _render.render_depth(meshes, mesh_index, R, t, K, size_hw, near=near, far=far, pixel_center=pixel_center, want_face=True)
    out = _canvas(background, (*rendered.face.shape, 3), meshes.device)
    return shade(meshes, appearance, rendered.face, mesh_index, R, t, K, light=light, phong=phong, pixel_center=pixel_center, out=out), rendered


@torch.no_grad()
def render_scene(meshes: MeshSet, appearance: Appearance, mesh_index, scene_index, R, t, K, frame_hw, n_scenes, *, near, far, light, phong,
                 background=None, pixel_center=(0.5, 0.5)):
    """(frames (S,H,W,3) uint8, SceneDepth): every instance rendered into the full frame, the scenes composed from those renders
    (`gtinfo.compose_scene_depth(..., want_instance=True)`: per pixel the nearest instance), then `shade_scene` over zeros or over a copy
    of `background` (S,H,W,3) uint8.  K (3,3) or (B,3,3)."""
    if not isinstance(appearance, Appearance):
        raise TypeError(f"lc_amd.shade: appearance must be an Appearance, got {type(appearance)}")
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3) and isinstance(mesh_index, Tensor):
        K = K.expand(int(mesh_index.shape[0]), 3, 3).contiguous()
    rendered = _render.render_depth(meshes, mesh_index, R, t, K, frame_hw, near=near, far=far, pixel_center=pixel_center, want_face=True)
    scene = _gtinfo.compose_scene_depth(rendered.depth, scene_index, (int(frame_hw[0]), int(frame_hw[1])), n_scenes, want_instance=True)
    frames = _canvas(background, (*scene.depth.shape, 3), meshes.device)
    shade_scene(meshes, appearance, frames, scene.instance, rendered.face, mesh_index, scene_index, R, t, K, light=light, phong=phong,
                pixel_center=pixel_center)
    return frames, scene
