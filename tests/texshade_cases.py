"""The textured shading pass's case list (TEST INFRASTRUCTURE ONLY): small procedural scenes and generated textures, no assets.  The face
and instance maps of a case are the ORACLE's (tests/render_oracle.py, tests/shade_oracle.compose), built by tests/shade_cases._case, so
that the shading is judged apart from the rasteriser; `reference(name, flip, lod)` is tests/texshade_oracle.py's result over the SENTINEL
frame, computed once per process and shared (treat as read-only).

    quad8 / quad4 / quad2   a fronto-parallel unit quad at z = 1 with an 8 x 8 texture, drawn on 8 x 8, 4 x 4 and 2 x 2 pixels with
                            phong = (1, 0, 0): every quotient is exact, and the bytes are those of level 0, 1 and 2 with v flipped
    b{1,3}-{h}x{w}          a 12-face box (texture 0: 3 x 5), an 80-face icosphere (texture 1: 64 x 32) and an untextured quad under oblique
                            poses and a camera with skew and fx != fy, on maps of 1 x 1, 5 x 67, 40 x 48 and 37 x 53 pixels; per-corner
                            texture coordinates in [-1.5, 2.5], different across every shared vertex (seams); B = 1 is the icosphere alone
    levels                  a tilted quad whose texture coordinates are scaled so that rho2 crosses several level thresholds in one image
    scene / scene-planted   tests/shade_cases.py's two scenes of four windows partly off the frame, textured; and with its planted entries
    planted-face            face indices outside the mesh
    bad-uv                  a face whose coordinates are not finite, and one whose coordinates lead 2^30 texels away

A case's `wrap` holds one value per row; `flip` runs it with every value exchanged, so that both values meet every row.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from lc_amd import synth
from tests import camera_cases, render_cases, shade_cases, shade_oracle, texshade_oracle
from tests.shade_cases import sentinel  # noqa: F401

CAMERA = camera_cases.CAMERAS[1]  # "stress": anisotropy and skew
SIZES = ((1, 1), (5, 67), (40, 48), (37, 53))  # the last: neither side a multiple of the kernel's 16 x 16 tile


class Case(NamedTuple):
    name: str
    base: shade_cases.Case   # meshes, rows, face maps, scene
    uvs: tuple               # per mesh (Nf,3,2) float32, or None
    tex_index: np.ndarray    # (n_meshes,) int32
    images: tuple            # the textures, (Ht,Wt,3) uint8
    wrap: np.ndarray         # (B,) int32

    @property
    def tm(self) -> texshade_oracle.TexMeshes:
        ms = self.base.ms
        uv = np.concatenate([np.zeros((len(m[1]), 3, 2), np.float32) if u is None else u for m, u in zip(self.base.meshes, self.uvs)], 0)
        texels, table = texshade_oracle.store(self.images)
        return texshade_oracle.TexMeshes(ms, uv, np.asarray(self.tex_index, np.int32), texels, table)


def image(hw, seed) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(*hw, 3), dtype=np.uint8)


TEX8 = image((8, 8), 8)
TEX_SMALL, TEX_WIDE = image((3, 5), 35), image((64, 32), 6432)
UNIT_QUAD = (np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float32), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
UNIT_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float32)  # v = the model's y: 0 at the image's top row of pixels


def stress_K(size_hw, scale=1.25) -> np.ndarray:
    """A camera whose 2 x 2 block is f M with M the `stress` matrix of lc_amd.synth.CAMERAS (fx != fy, skew), centred off the middle."""
    h, w = size_hw
    K = np.eye(3)
    K[:2, :2] = scale * max(h, w) * np.asarray(synth.CAMERAS[CAMERA])
    K[0, 2], K[1, 2] = w / 2 + 0.3, h / 2 - 0.2
    return K.astype(np.float32)


def corner_uvs(n_faces, seed) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1.5, 2.5, size=(n_faces, 3, 2)).astype(np.float32)


def _three_meshes():
    box = shade_cases._mesh(*render_cases.box((0.08, 0.06, 0.05)), shade_cases._colors(8, 3))
    ico = shade_cases._mesh(*render_cases.icosphere(1, 0.1), shade_cases._colors(42, 4))
    quad = shade_cases._mesh(*shade_cases.QUAD, shade_cases.QUAD_COLORS)
    return box, ico, quad


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    quad = shade_cases._mesh(*shade_cases.QUAD, shade_cases.QUAD_COLORS)
    if name in ("quad8", "quad4", "quad2"):
        n = int(name[4:])
        mesh = shade_cases._mesh(*UNIT_QUAD, np.full((4, 3), 128, np.uint8))
        K = np.array([[n, 0, 0], [0, n, 0], [0, 0, 1]], dtype=np.float32)
        base = shade_cases._case(name, [mesh], [0], [(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))], K, (n, n), phong=(1.0, 0.0, 0.0), near=0.5, far=2.0)
        return Case(name, base, (UNIT_UV[UNIT_QUAD[1]],), np.array([0], np.int32), (TEX8,), np.array([0], np.int32))
    if name.startswith(("b1-", "b3-")):
        B, (h, w) = int(name[1]), tuple(int(v) for v in name.split("-")[1].split("x"))
        box, ico, q = _three_meshes()
        poses = [(render_cases.rot((1, 2, 0.5), 131.0), np.array([0.004, -0.006, 0.42], np.float32)),
                 (render_cases.rot((0.3, 1, 0.2), 47.0), np.array([-0.005, 0.003, 0.40], np.float32)), shade_cases.QUAD_POSE]
        rows = [0, 1, 2] if B == 3 else [1]
        base = shade_cases._case(name, [box, ico, q], rows, [poses[r] for r in rows], stress_K((h, w), 4.0 if (h, w) == (1, 1) else 1.25), (h, w),
                                 light=[[0.3, -0.4, -0.2], shade_cases.DEFAULT_LIGHT, [-1.0, 0.5, 0.1]][:B], phong=[shade_cases.DEFAULT_PHONG, [0.2, 0.9, 0.6], [0.5, 0.5, 0.5]][:B])
        return Case(name, base, (corner_uvs(12, 1), corner_uvs(80, 2), None), np.array([0, 1, -1], np.int32), (TEX_SMALL, TEX_WIDE), np.array([0, 1, 0][:B], np.int32))
    if name == "levels":  # the quad leans 75 degrees away: the far edge packs many texels into a pixel, the near edge few; the coordinates span four repeats
        pose = (render_cases.rot((0, 1, 0), 75.0), np.array([0.0, 0.0, 0.16], np.float32))
        base = shade_cases._case(name, [quad], [0], [pose], stress_K(shade_cases.WINDOW), shade_cases.WINDOW)
        return Case(name, base, (4.0 * UNIT_UV[shade_cases.QUAD[1]],), np.array([0], np.int32), (TEX_WIDE,), np.array([1], np.int32))
    if name in ("scene", "scene-planted"):
        b = shade_cases.build(name)
        return Case(name, b, (corner_uvs(20, 5), UNIT_UV[shade_cases.QUAD[1]] * np.float32(1.5)), np.array([1, 0], np.int32), (TEX_SMALL, TEX_WIDE),
                    np.array([0, 1, 1, 0], np.int32))
    if name == "planted-face":
        return Case(name, shade_cases.build(name), (corner_uvs(20, 5),), np.array([0], np.int32), (TEX_SMALL,), np.array([1], np.int32))
    if name == "bad-uv":  # the faces the image shows first and last
        b = shade_cases.build("ico20")
        uv = corner_uvs(20, 5)
        seen = np.unique(b.face[b.face >= 0])
        uv[seen[0], 1, 0] = np.inf
        uv[seen[1], 2, 1] = np.nan
        uv[seen[-1]] = np.float32(2.0 ** 31)  # times a level's size of 1 or more: beyond 2^30
        return Case(name, b, (uv,), np.array([0], np.int32), (TEX_SMALL,), np.array([0], np.int32))
    raise KeyError(name)


QUADS = ("quad8", "quad4", "quad2")
GRID = tuple(f"b{B}-{h}x{w}" for B in (1, 3) for h, w in SIZES)
NAMES = QUADS + GRID + ("levels", "scene", "scene-planted", "planted-face", "bad-uv")


def _wrap(c: Case, flip: bool):
    return 1 - c.wrap if flip else c.wrap


def shade(c: Case, flip=False, lod=True, tm=None, out=None, wrap=None):
    """The instance form of a case over the sentinel (or `out`) -> (Shaded, level)."""
    b = c.base
    out = sentinel((len(b.face), *b.size_hw, 3)) if out is None else out
    return texshade_oracle.shade(c.tm if tm is None else tm, b.face, b.mesh_index, b.R, b.t, b.K, b.light, b.phong, _wrap(c, flip) if wrap is None else wrap, lod, out,
                                 shade_cases.CENTER)


def shade_scene(c: Case, flip=False, lod=True) -> shade_oracle.Shaded:
    b, sc = c.base, c.base.scene
    return texshade_oracle.shade_scene(c.tm, sentinel((sc.S, *sc.frame_hw, 3)), sc.instance, b.face, b.mesh_index, sc.scene_index, b.R, b.t, b.K, b.light, b.phong,
                                       _wrap(c, flip), lod, sc.origin_xy, shade_cases.CENTER)


@functools.lru_cache(maxsize=None)
def reference(name: str, flip=False, lod=True):
    """(Shaded, level) of the instance form."""
    return shade(build(name), flip, lod)


@functools.lru_cache(maxsize=None)
def scene_reference(name: str, flip=False, lod=True) -> shade_oracle.Shaded:
    return shade_scene(build(name), flip, lod)
