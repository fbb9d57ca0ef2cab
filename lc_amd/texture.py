"""Shaded colour images of posed, TEXTURED meshes on the device (lc_amd/csrc/texture/lc_texture.hip, lc_amd/_C/liblc_amd_texture.so; C ABI
and the exact definition of every byte in include/lc_amd_texture.h): `lc_amd.shade`'s pass with the albedo of a pixel sampled from the
mesh's texture at per-corner texture coordinates, for the object sets that ship a PLY with `texture_u` / `texture_v` and a texture image
(the reference reads those with `tools/lib/pysixd/inout.py:505-617`).

    TextureStore.from_images(images, device, levels=None)               every texture and its mip chain in one resident buffer, once per dataset
    TexturedAppearance(meshes, uvs, tex_index, textures, colors=None, normals=None)
    shade(meshes, appearance, face, mesh_index, R, t, K, *, light, phong, wrap=0, lod=True, ...) -> out (B,h,w,3) uint8
    shade_scene(meshes, appearance, frames, instance, face, mesh_index, scene_index, R, t, K, *, light, phong, wrap=0, lod=True, ...) -> frames
    render_color(meshes, appearance, mesh_index, R, t, K, size_hw, *, near, far, light, phong, wrap=0, lod=True, background=None) -> (frames, Rendered)
    render_scene(meshes, appearance, mesh_index, scene_index, R, t, K, frame_hw, n_scenes, *, near, far, light, phong, ...) -> (frames, SceneDepth)
    read_ply_textured(path) -> TexturedPly                              host only: a PLY's geometry, per-corner uv and texture file name

The four functions mirror those of `lc_amd.shade` and write the same frames.  A mesh whose `tex_index` is -1 takes its per-vertex
colours and its pixels are `lc_amd.shade`'s, byte for byte.  `wrap`: 0 / "clamp" or 1 / "repeat", for every row, or an int32 tensor (B,).
`lod=True` picks one mip level per pixel from the texture coordinates of the neighbouring samples and samples it bilinearly (OpenGL's
GL_LINEAR_MIPMAP_NEAREST); `lod=False` samples level 0.  v = 0 is the LAST row of the image as given (OpenGL's convention for an image
loaded top row first); pass 1 - v for the other one.  Images are decoded by the caller: a texture is an (Ht,Wt,3) uint8 array.

HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device, allocates its
outputs only and can be captured into a graph.  `info` (B,) int32: 0, 1 where a pixel of the row was refused (what `lc_amd.shade`
refuses, and texture coordinates that are not finite or lead 2^30 texels away), -1 for a refused row (an unknown mesh or texture, a wrap
that is neither 0 nor 1).
"""
from __future__ import annotations

from ctypes import c_float, c_int, c_longlong, c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build
from . import gtinfo as _gtinfo
from . import render as _render
from . import shade as _shade
from .render import MeshSet
from .shade import DEFAULT_LIGHT, DEFAULT_PHONG, vertex_normals  # noqa: F401

MAX_SIZE = 16384        # of a map or frame side, as lc_amd.shade has it
TEX_MAX_SIZE = 16384    # LC_TEX_MAX_SIZE
TEX_MAX_LEVELS = 15     # LC_TEX_MAX_LEVELS
WRAP = {"clamp": 0, "repeat": 1}

_MESH = [c_void_p] * 7 + [c_int] * 3 + [c_void_p] * 2 + [c_int, c_longlong]
_SO = _lib.SideLibrary(_build.TEXTURE, {
    "lc_tex_build_mips_u8": (c_int, [c_void_p, c_longlong, c_void_p, c_int, c_void_p]),
    "lc_texshade_instances_u8": (c_int, _MESH + [c_void_p] * 8 + [c_int] * 3 + [c_float] * 2 + [c_int] + [c_void_p] * 3),
    "lc_texshade_scene_u8": (c_int, _MESH + [c_void_p] * 10 + [c_int] * 3 + [c_float] * 2 + [c_int] + [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 2),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("texture")


def level_sizes(Ht: int, Wt: int, n_levels: int) -> list:
    """[(H_L, W_L)] of the first n_levels levels: each side halves, rounding down, and stays at 1."""
    out = []
    for _ in range(n_levels):
        out.append((Ht, Wt))
        Ht, Wt = max(1, Ht >> 1), max(1, Wt >> 1)
    return out


class TextureStore:
    """Every texture of a dataset in one byte buffer on the device: `texels` (total_texels,4) uint8, a texel (R, G, B, 0); `table` (n_tex,4)
    int64 = (offset of level 0 in texels, Ht, Wt, n_levels), level L+1 directly behind level L.  Level 0 is uploaded; the others are written
    on the device (`lc_tex_build_mips_u8`) on the current stream."""

    def __init__(self, texels: Tensor, table_host: np.ndarray):
        self.texels, self.table_host = texels, table_host
        self.table = torch.from_numpy(table_host).to(texels.device)
        self.n_tex, self.total_texels, self.device = len(table_host), int(texels.shape[0]), texels.device

    @classmethod
    def from_images(cls, images, device, levels=None) -> "TextureStore":
        """images: a list of (Ht,Wt,3) uint8 arrays of their own sizes, row 0 the first row of the image.  levels None: every texture's
        full chain down to 1 x 1; a number: at most that many levels (1: level 0 only)."""
        if isinstance(images, (np.ndarray, Tensor)) or not hasattr(images, "__len__"):
            raise ValueError("lc_amd.texture: images is a list of (Ht,Wt,3) uint8 arrays")
        if levels is not None:
            levels = _A.whole("levels", levels, 1, TEX_MAX_LEVELS)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"lc_amd.texture: the store lives on the MI355X, got device {device} (there is no CPU fallback in the product path)")
        table, off, imgs = [], 0, []
        for k, im in enumerate(images):
            im = np.ascontiguousarray(im.detach().cpu().numpy() if isinstance(im, Tensor) else im)
            if im.dtype != np.uint8:
                raise TypeError(f"lc_amd.texture: image {k} must be uint8, got {im.dtype}")
            if im.ndim != 3 or im.shape[2] != 3 or not (1 <= im.shape[0] <= TEX_MAX_SIZE and 1 <= im.shape[1] <= TEX_MAX_SIZE):
                raise ValueError(f"lc_amd.texture: image {k} has shape {im.shape}, expected (Ht,Wt,3) with sides of 1 to {TEX_MAX_SIZE}")
            Ht, Wt = int(im.shape[0]), int(im.shape[1])
            n = max(Ht, Wt).bit_length()  # the full chain: down to 1 x 1
            n = n if levels is None else min(n, levels)
            table.append((off, Ht, Wt, n))
            off += sum(h * w for h, w in level_sizes(Ht, Wt, n))
            imgs.append(im)
        host = np.zeros((off, 4), dtype=np.uint8)
        for (o, Ht, Wt, _), im in zip(table, imgs):
            host[o:o + Ht * Wt, :3] = im.reshape(-1, 3)
        store = cls(torch.from_numpy(host).to(device), np.asarray(table, dtype=np.int64).reshape(-1, 4))
        if store.n_tex:
            with _lib.on_device(store.device):
                rc = load().lc_tex_build_mips_u8(_lib.ptr(store.texels), store.total_texels, c_void_p(store.table_host.ctypes.data), store.n_tex,
                                                 _lib.stream_ptr(store.device))
            if rc != 0:
                _SO.fail("texture.TextureStore.from_images", rc)
        return store

    def level(self, k: int, L: int) -> Tensor:
        """Level L of texture k as an (H_L, W_L, 3) uint8 view of the buffer."""
        off, Ht, Wt, n = (int(v) for v in self.table_host[k])
        if not 0 <= L < n:
            raise IndexError(f"lc_amd.texture: texture {k} has {n} levels, asked for level {L}")
        sizes = level_sizes(Ht, Wt, n)
        off += sum(h * w for h, w in sizes[:L])
        h, w = sizes[L]
        return self.texels[off:off + h * w, :3].reshape(h, w, 3)


def corner_uv(uv, faces, n_vert: int) -> np.ndarray:
    """(Nf,3,2) float32 from per-corner (Nf,3,2) coordinates as they are, or from per-vertex (Nv,2) ones gathered by `faces` (Nf,3)."""
    faces = np.asarray(faces).reshape(-1, 3)
    uv = np.asarray(uv.detach().cpu().numpy() if isinstance(uv, Tensor) else uv)
    if not np.issubdtype(uv.dtype, np.floating):
        raise TypeError(f"lc_amd.texture: uv must hold floats, got {uv.dtype}")
    if uv.shape == (len(faces), 3, 2):
        return np.ascontiguousarray(uv, dtype=np.float32)
    if uv.shape == (n_vert, 2):
        return np.ascontiguousarray(uv[faces.astype(np.int64)], dtype=np.float32)
    raise ValueError(f"lc_amd.texture: uv has shape {uv.shape}, expected per-corner {(len(faces), 3, 2)} or per-vertex {(n_vert, 2)}")


class TexturedAppearance:
    """What the textured pass needs beside a MeshSet's geometry: `uv` (total_faces,3,2) float32, per face corner and aligned with the set's
    `faces`; `tex_index` (n_meshes,) int32 into `textures` (a TextureStore), -1 for a mesh without a texture; `colors` and `normals` as
    `shade.Appearance` builds them (the colours serve the meshes without a texture).  `uvs`: a list with one array per mesh, per corner
    (Nf,3,2) or per vertex (Nv,2), or None for a mesh without a texture (zeros).  Validated on the host, uploaded once."""

    def __init__(self, meshes: MeshSet, uvs, tex_index, textures: TextureStore, colors=None, normals=None):
        base = _shade.Appearance(meshes, colors, normals)
        if not isinstance(textures, TextureStore):
            raise TypeError(f"lc_amd.texture: textures must be a TextureStore, got {type(textures)}")
        n = meshes.n_meshes
        if isinstance(uvs, (Tensor, np.ndarray)) or not hasattr(uvs, "__len__") or len(uvs) != n:
            raise ValueError(f"lc_amd.texture: uvs is a list of one array per mesh ({n})")
        ti = np.asarray(tex_index.detach().cpu().numpy() if isinstance(tex_index, Tensor) else tex_index)
        if ti.shape != (n,) or not np.issubdtype(ti.dtype, np.integer):
            raise ValueError(f"lc_amd.texture: tex_index holds one whole number per mesh ({n}), got {tex_index!r}")
        if ti.size and (ti.min() < -1 or ti.max() >= textures.n_tex):
            raise ValueError(f"lc_amd.texture: tex_index must lie in [-1, {textures.n_tex}), got [{ti.min()}, {ti.max()}]")
        faces = meshes.faces.cpu().numpy()
        per_mesh = []
        for k, (vo, nv, fo, nf) in enumerate(meshes.table_host.tolist()):
            if uvs[k] is None:
                if ti[k] >= 0:
                    raise ValueError(f"lc_amd.texture: mesh {k} has texture {ti[k]} and no uv")
                per_mesh.append(np.zeros((nf, 3, 2), dtype=np.float32))
                continue
            try:
                per_mesh.append(corner_uv(uvs[k], faces[fo:fo + nf], nv))
            except (TypeError, ValueError) as e:
                raise type(e)(str(e).replace("lc_amd.texture: ", f"lc_amd.texture: mesh {k}: ")) from None
        if meshes.device != textures.device:
            raise ValueError(f"lc_amd.texture: the textures are on {textures.device}, the meshes on {meshes.device}")
        self.meshes, self.textures, self.base = meshes, textures, base
        self.colors, self.normals, self.colors_host, self.normals_host = base.colors, base.normals, base.colors_host, base.normals_host
        self.uv_host = np.concatenate(per_mesh, 0).reshape(-1, 3, 2) if per_mesh else np.zeros((0, 3, 2), np.float32)
        self.tex_index_host = ti.astype(np.int32)
        self.uv = torch.from_numpy(self.uv_host).to(meshes.device)
        self.tex_index = torch.from_numpy(self.tex_index_host).to(meshes.device)


def _per_row(name: str, v, B: int, dev) -> Tensor:
    """light or phong as a contiguous (B,3) float32 tensor on the device: a tensor of (3,) or (B,3), or three numbers."""
    if not isinstance(v, Tensor):
        vals = np.asarray(v, dtype=np.float64).reshape(-1) if hasattr(v, "__len__") and not isinstance(v, str) else None
        if vals is None or vals.shape != (3,) or not np.isfinite(vals).all():
            raise ValueError(f"lc_amd.texture: {name} is three finite numbers or a float32 tensor of shape (3,) or {(B, 3)}, got {v!r}")
        v = torch.tensor(vals.astype(np.float32), device=dev)
    v = _lib.require_hip_f32(name, v)
    if tuple(v.shape) == (3,):
        v = v.expand(B, 3)
    _A.rows(name, v, (B, 3))
    return v.contiguous()


def _wrap(wrap, B: int, dev) -> Tensor:
    """wrap as a contiguous (B,) int32 tensor on the device: 0 / "clamp", 1 / "repeat", or the caller's tensor."""
    if isinstance(wrap, Tensor):
        wrap = _A.tensor("wrap", wrap, (torch.int32,), "int32", (B,))
        _A.same_device(dev, _args.MESHES_ON, wrap=wrap)
        return wrap.contiguous()
    code = WRAP.get(wrap, wrap) if isinstance(wrap, str) else wrap
    if isinstance(code, bool) or code not in (0, 1):
        raise ValueError(f'lc_amd.texture: wrap is 0 or "clamp", 1 or "repeat", or an int32 tensor of shape {(B,)}, got {wrap!r}')
    return torch.full((B,), int(code), device=dev, dtype=torch.int32)


def _rows(meshes, appearance, face, mesh_index, R, t, K, light, phong, wrap, lod, pixel_center):
    """The rules the two forms share -> (B, h, w, dev, the contiguous row tensors, (cx, cy), lod)."""
    if not isinstance(meshes, MeshSet):
        raise TypeError(f"lc_amd.texture: meshes must be a MeshSet, got {type(meshes)}")
    if not isinstance(appearance, TexturedAppearance):
        raise TypeError(f"lc_amd.texture: appearance must be a TexturedAppearance, got {type(appearance)}")
    if appearance.meshes is not meshes:
        raise ValueError("lc_amd.texture: appearance was made for another MeshSet")
    if not isinstance(lod, (bool, np.bool_)):
        raise TypeError(f"lc_amd.texture: lod must be True or False, got {lod!r}")
    face = _A.tensor("face", face, (torch.int32,), "int32", (None, None, None))
    B, h, w = (int(n) for n in face.shape)
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f"lc_amd.texture: map sizes of 1 to {MAX_SIZE}, got {h} x {w}")

    def f32(name, x, shape):
        x = _lib.require_hip_f32(name, x)
        _A.rows(name, x, shape)
        return x

    rows, (R,), (t,), K = _A.pose_batch(mesh_index, {"R": R}, {"t": t}, K, f32=f32)
    if rows != B:
        raise ValueError(f"lc_amd.texture: mesh_index has shape {tuple(mesh_index.shape)}, expected {(B,)}")
    cx, cy = _A.center(pixel_center)
    dev = meshes.device
    if not face.is_cuda:
        raise RuntimeError(f"lc_amd.texture: face is on {face.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    light, phong, wrap = _per_row("light", light, B, dev), _per_row("phong", phong, B, dev), _wrap(wrap, B, dev)
    _A.same_device(dev, _args.MESHES_ON, face=face, mesh_index=mesh_index, R=R, t=t, K=K, light=light, phong=phong)
    return B, h, w, dev, (mesh_index.contiguous(), R, t, K.contiguous(), light, phong, wrap, face.contiguous()), (cx, cy), int(bool(lod))


def _mesh_args(meshes, ap):
    tx = ap.textures
    return (_lib.ptr(meshes.verts), _lib.ptr(ap.normals), _lib.ptr(ap.colors), _lib.ptr(meshes.faces), _lib.ptr(ap.uv), _lib.ptr(meshes.table),
            _lib.ptr(ap.tex_index), meshes.n_meshes, meshes.total_verts, meshes.total_faces, _lib.ptr(tx.texels), _lib.ptr(tx.table), tx.n_tex,
            tx.total_texels)


def _info(info, B: int, dev) -> Tensor:
    if info is None:
        return torch.empty(B, device=dev, dtype=torch.int32)
    info = _A.tensor("info", info, (torch.int32,), "int32", (B,))
    _A.same_device(dev, _args.MESHES_ON, info=info)
    if not info.is_contiguous():
        raise ValueError("lc_amd.texture: info must be contiguous")
    return info


@torch.no_grad()
def shade(meshes: MeshSet, appearance: TexturedAppearance, face, mesh_index, R, t, K, *, light, phong, wrap=0, lod=True, pixel_center=(0.5, 0.5),
          out=None, info=None) -> Tensor:
    """out (B,h,w,3) uint8: the hit pixels of `face` (B,h,w) int32 (`render_depth(..., want_face=True).face`, rendered with the same
    mesh_index, R, t, K and pixel_center) shaded; every other pixel keeps the byte `out` held (a new `out` is zeros).  `info` (B,) int32, if
    given, receives the rows' records (see the module's head)."""
    B, h, w, dev, rows, (cx, cy), lod = _rows(meshes, appearance, face, mesh_index, R, t, K, light, phong, wrap, lod, pixel_center)
    if out is None:
        out = torch.zeros(B, h, w, 3, device=dev, dtype=torch.uint8)
    else:
        out = _A.tensor("out", out, (torch.uint8,), "uint8", (B, h, w, 3))
        _A.same_device(dev, _args.MESHES_ON, out=out)
        if not out.is_contiguous():
            raise ValueError(f"lc_amd.texture: out must be contiguous (hit pixels are written in place), got strides {tuple(out.stride())}")
    info = _info(info, B, dev)
    if B:
        with _lib.on_device(dev):
            rc = load().lc_texshade_instances_u8(*_mesh_args(meshes, appearance), *(_lib.ptr(x) for x in rows), B, h, w, cx, cy, lod, _lib.ptr(out),
                                                 _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("texture.shade", rc)
    return out


@torch.no_grad()
def shade_scene(meshes: MeshSet, appearance: TexturedAppearance, frames, instance, face, mesh_index, scene_index, R, t, K, *, light, phong, wrap=0,
                lod=True, origin_xy=None, pixel_center=(0.5, 0.5), info=None) -> Tensor:
    """IN PLACE in frames (S,H,W,3) uint8, contiguous: frame pixel (X,Y) of scene s takes row b = instance[s,Y,X] (-1: untouched) and is
    shaded as window pixel (X - x0_b, Y - y0_b) of row b's `face` map, as `lc_amd.shade.shade_scene` has it.  -> frames."""
    B, h, w, dev, rows, (cx, cy), lod = _rows(meshes, appearance, face, mesh_index, R, t, K, light, phong, wrap, lod, pixel_center)
    frames = _A.tensor("frames", frames, (torch.uint8,), "uint8", (None, None, None, 3))
    S, H, W = (int(n) for n in frames.shape[:3])
    if S < 1 or not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f"lc_amd.texture: at least one frame, of sizes of 1 to {MAX_SIZE}, got {S} of {H} x {W}")
    instance = _A.tensor("instance", instance, (torch.int32,), "int32", (S, H, W))
    _A.i32("scene_index", scene_index, (B,))
    if origin_xy is not None:
        _A.i32("origin_xy", origin_xy, (B, 2))
    elif (h, w) != (H, W):
        raise ValueError(f"lc_amd.texture: without origin_xy the maps ({h} x {w}) must have the frame's size ({H} x {W})")
    if not frames.is_contiguous():
        raise ValueError(f"lc_amd.texture: frames must be contiguous (hit pixels are written in place), got strides {tuple(frames.stride())}")
    _A.same_device(dev, _args.MESHES_ON, frames=frames, instance=instance, scene_index=scene_index, origin_xy=origin_xy)
    idx = scene_index.to(torch.int32).contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    inst = instance.contiguous()
    info = _info(info, B, dev)
    if B:
        mesh_index, Rc, tc, Kc, light, phong, wrap, face = rows
        with _lib.on_device(dev):
            rc = load().lc_texshade_scene_u8(*_mesh_args(meshes, appearance), _lib.ptr(mesh_index), _lib.ptr(idx), _lib.ptr(Rc), _lib.ptr(tc), _lib.ptr(Kc),
                                             _lib.ptr(light), _lib.ptr(phong), _lib.ptr(wrap), _lib.ptr(face), _lib.ptr(org), B, h, w, cx, cy, lod,
                                             _lib.ptr(inst), _lib.ptr(frames), S, H, W, _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("texture.shade_scene", rc)
    return frames


def _canvas(background, shape, dev) -> Tensor:
    """The frames the shading writes into: zeros, or a copy of `background` (the caller's tensor is left as it is)."""
    if background is None:
        return torch.zeros(shape, device=dev, dtype=torch.uint8)
    background = _A.tensor("background", background, (torch.uint8,), "uint8", shape)
    _A.same_device(dev, _args.MESHES_ON, background=background)
    return background.clone(memory_format=torch.contiguous_format)


@torch.no_grad()
def render_color(meshes: MeshSet, appearance: TexturedAppearance, mesh_index, R, t, K, size_hw, *, near, far, light, phong, wrap=0, lod=True,
                 background=None, pixel_center=(0.5, 0.5)):
    """(frames (B,H,W,3) uint8, Rendered): `render.render_depth(..., want_face=True)` and `shade` over zeros, or over a copy of
    `background` (B,H,W,3) uint8."""
    if not isinstance(appearance, TexturedAppearance):
        raise TypeError(f"lc_amd.texture: appearance must be a TexturedAppearance, got {type(appearance)}")
    rendered = _render.render_depth(meshes, mesh_index, R, t, K, size_hw, near=near, far=far, pixel_center=pixel_center, want_face=True)
    out = _canvas(background, (*rendered.face.shape, 3), meshes.device)
    return shade(meshes, appearance, rendered.face, mesh_index, R, t, K, light=light, phong=phong, wrap=wrap, lod=lod, pixel_center=pixel_center,
                 out=out), rendered


@torch.no_grad()
def render_scene(meshes: MeshSet, appearance: TexturedAppearance, mesh_index, scene_index, R, t, K, frame_hw, n_scenes, *, near, far, light, phong,
                 wrap=0, lod=True, background=None, pixel_center=(0.5, 0.5)):
    """(frames (S,H,W,3) uint8, SceneDepth): every instance rendered into the full frame, the scenes composed from those renders
    (`gtinfo.compose_scene_depth(..., want_instance=True)`), then `shade_scene` over zeros or over a copy of `background` (S,H,W,3)
    uint8.  K (3,3) or (B,3,3)."""
    if not isinstance(appearance, TexturedAppearance):
        raise TypeError(f"lc_amd.texture: appearance must be a TexturedAppearance, got {type(appearance)}")
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3) and isinstance(mesh_index, Tensor):
        K = K.expand(int(mesh_index.shape[0]), 3, 3).contiguous()
    rendered = _render.render_depth(meshes, mesh_index, R, t, K, frame_hw, near=near, far=far, pixel_center=pixel_center, want_face=True)
    scene = _gtinfo.compose_scene_depth(rendered.depth, scene_index, (int(frame_hw[0]), int(frame_hw[1])), n_scenes, want_instance=True)
    frames = _canvas(background, (*scene.depth.shape, 3), meshes.device)
    shade_scene(meshes, appearance, frames, scene.instance, rendered.face, mesh_index, scene_index, R, t, K, light=light, phong=phong, wrap=wrap, lod=lod,
                pixel_center=pixel_center)
    return frames, scene


class TexturedPly(NamedTuple):
    verts: np.ndarray               # (Nv,3) float32
    faces: np.ndarray               # (Nf,3) int32
    colors: Optional[np.ndarray]    # (Nv,3) uint8 where the vertices have red, green, blue
    normals: Optional[np.ndarray]   # (Nv,3) float32 where they have nx, ny, nz
    uv: Optional[np.ndarray]        # (Nf,3,2) float32: the face's `texcoord` list, else the vertices' texture_u / texture_v gathered to corners
    texture_file: Optional[str]     # the name after `comment TextureFile`


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_textured(path) -> TexturedPly:
    """A triangle mesh from an ascii or binary_little_endian PLY, with what a textured model carries (host only; `gen_z.read_ply` reads
    geometry alone): per-vertex colours and normals where present, texture coordinates per face corner, the texture's file name."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header")
    if not blob.startswith(b"ply") or end < 0:
        raise ValueError(f"lc_amd.texture: {path} is not a PLY file")
    body = blob.index(b"\n", end) + 1
    fmt, texture_file, elements = None, None, []
    for line in blob[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "comment" and len(w) >= 3 and w[1] == "TextureFile":
            texture_file = line.split("TextureFile", 1)[1].strip()
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"lc_amd.texture: {path}: a property in front of every element")
            kinds = w[2:4] if w[1] == "list" else w[1:2]
            if any(k not in _PLY_TYPES for k in kinds):
                raise ValueError(f"lc_amd.texture: {path}: unknown property type in {line!r}")
            elements[-1][2].append((w[-1], None, _PLY_TYPES[w[1]]) if w[1] != "list" else (w[-1], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"lc_amd.texture: {path}: format {fmt!r}; ascii and binary_little_endian are read")
    tokens, pos = (blob[body:].split(), 0) if fmt == "ascii" else (None, body)
    data = {}
    for name, count, props in elements:
        if all(cnt is None for _, cnt, _ in props):  # fixed-size records: one structured read
            dt = np.dtype([(p, "<" + ty) for p, _, ty in props])
            if fmt == "ascii":
                flat = tokens[pos:pos + count * len(props)]
                if len(flat) != count * len(props):
                    raise ValueError(f"lc_amd.texture: {path}: element {name} is cut short")
                pos += len(flat)
                table = np.array(flat, dtype=np.float64).reshape(count, len(props))
                rec = np.zeros(count, dtype=dt)
                for j, (p, _, _) in enumerate(props):
                    rec[p] = table[:, j]
            else:
                if pos + count * dt.itemsize > len(blob):
                    raise ValueError(f"lc_amd.texture: {path}: element {name} is cut short")
                rec = np.frombuffer(blob, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
            data[name] = {p: rec[p] for p, _, _ in props}
            continue
        cols = {p: [] for p, _, _ in props}
        for _ in range(count):
            for p, cnt, ty in props:
                try:
                    if fmt == "ascii":
                        n = 1 if cnt is None else int(tokens[pos])
                        pos += cnt is not None
                        vals = np.array(tokens[pos:pos + n], dtype=np.float64).astype(ty)
                        pos += n
                    else:
                        n = 1
                        if cnt is not None:
                            n = int(np.frombuffer(blob, dtype="<" + cnt, count=1, offset=pos)[0])
                            pos += np.dtype(cnt).itemsize
                        vals = np.frombuffer(blob, dtype="<" + ty, count=n, offset=pos)
                        pos += n * np.dtype(ty).itemsize
                    if len(vals) != n:
                        raise IndexError
                except (IndexError, ValueError):
                    raise ValueError(f"lc_amd.texture: {path}: element {name} is cut short") from None
                cols[p].append(vals if cnt is not None else vals[0])
        data[name] = cols
    vert, face = data.get("vertex"), data.get("face")
    if vert is None or not all(k in vert for k in "xyz"):
        raise ValueError(f"lc_amd.texture: {path}: no vertex element with x, y, z")
    stack = lambda keys, dt: np.stack([np.asarray(vert[k]) for k in keys], -1).astype(dt).reshape(-1, len(keys))  # noqa: E731
    verts = stack("xyz", np.float32)
    index = next((k for k in ("vertex_indices", "vertex_index") if face is not None and k in face), None)
    lists = [] if index is None else face[index]
    if any(len(f) != 3 for f in lists):
        raise ValueError(f"lc_amd.texture: {path}: every face must be a triangle")
    faces = np.asarray(lists, dtype=np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"lc_amd.texture: {path}: face indices must lie in [0, {len(verts)}), got [{faces.min()}, {faces.max()}]")
    faces = faces.astype(np.int32)
    colors = stack(("red", "green", "blue"), np.uint8) if all(k in vert for k in ("red", "green", "blue")) else None
    normals = stack(("nx", "ny", "nz"), np.float32) if all(k in vert for k in ("nx", "ny", "nz")) else None
    uv = None
    if face is not None and "texcoord" in face:
        if any(len(c) != 6 for c in face["texcoord"]):
            raise ValueError(f"lc_amd.texture: {path}: every face's texcoord list must hold six numbers")
        uv = np.asarray(face["texcoord"], dtype=np.float32).reshape(-1, 3, 2)
    elif all(k in vert for k in ("texture_u", "texture_v")):
        uv = stack(("texture_u", "texture_v"), np.float32)[faces.astype(np.int64)].reshape(-1, 3, 2)
    return TexturedPly(verts, faces, colors, normals, uv, texture_file)
