"""The shading pass's case list (TEST INFRASTRUCTURE ONLY): small procedural scenes, no assets.  The face and instance maps of a case are the
ORACLE's (tests/render_oracle.py, tests/shade_oracle.compose), some with planted entries, so that the shading is judged apart from the
rasteriser; `reference(name)` is tests/shade_oracle.py's result over the SENTINEL frame, computed once per process and shared.

Two conditions hold for every case and are asserted by tests/test_shade_host.py:
  * every value `I c` before the final rounding stays 2^-20 clear of a half-integer -- but in `grid-square`, whose arithmetic is exact by
    construction (a quad on the rasteriser's grid with a span of 8 px at depth 1, so that the weights are eighths, colours that are multiples of 4 and phong = (1, 0, 0)):
    there a value may lie EXACTLY on a half, which no order of evaluation can move and which is what tells half-to-even from half-up;
  * every vertex a face map uses keeps tests/render_oracle.py's margin of 2^-30 px from a snapping boundary.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

from lc_amd.shade import DEFAULT_LIGHT, DEFAULT_PHONG, vertex_normals
from tests import render_cases, render_grid, render_oracle, shade_oracle

NEAR, FAR = 0.01, 6.5
CENTER = (0.5, 0.5)


class Scene(NamedTuple):
    S: int
    frame_hw: tuple
    scene_index: np.ndarray          # (B,) int32
    origin_xy: Optional[np.ndarray]  # (B,2) int32, None: full-frame maps
    instance: np.ndarray             # (S,H,W) int32
    depth: np.ndarray                # (S,H,W) float32


class Case(NamedTuple):
    name: str
    meshes: tuple            # ((verts, faces, normals, colors), ...)
    mesh_index: np.ndarray   # (B,) int32
    R: np.ndarray            # (B,3,3) float32
    t: np.ndarray            # (B,3)
    K: np.ndarray            # (B,3,3)
    light: np.ndarray        # (B,3)
    phong: np.ndarray        # (B,3)
    size_hw: tuple
    near: float
    far: float
    face: np.ndarray         # (B,h,w) int32
    renders: tuple           # the render_oracle.Ref of every row (None for a refused row)
    exact_halves: bool
    scene: Optional[Scene]

    @property
    def ms(self) -> shade_oracle.Meshes:
        return shade_oracle.concat(self.meshes)


def sentinel(shape) -> np.ndarray:
    """Bytes that no shaded pixel is likely to repeat by accident and that differ between neighbours: 1 to 251."""
    idx = np.indices(shape).astype(np.int64)
    mult = (5, 13, 7, 31, 3)[-len(shape):]
    return (sum(m * i for m, i in zip(mult, idx)) % 251 + 1).astype(np.uint8)


def _colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)


def _mesh(v, f, colors, normals=None):
    v, f = np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)
    return v, f, (vertex_normals(v, f) if normals is None else np.asarray(normals, dtype=np.float32)), np.asarray(colors, dtype=np.uint8)


def _rows(vals, B):
    a = np.asarray(vals, dtype=np.float32)
    return np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape[-1:]) if a.ndim == 1 else a)


def _case(name, meshes, mesh_index, poses, K, size_hw, *, light=DEFAULT_LIGHT, phong=DEFAULT_PHONG, near=NEAR, far=FAR, exact_halves=False, scene=None,
          plant=None) -> Case:
    """Renders every row with the oracle; `scene` = (S, frame_hw, scene_index, origin_xy) composes them; `plant(face, instance)` edits the maps."""
    B = len(mesh_index)
    K = np.asarray(K, dtype=np.float32)
    K = np.ascontiguousarray(np.broadcast_to(K, (B, 3, 3)))
    R = np.stack([np.asarray(p[0], dtype=np.float32) for p in poses])
    t = np.stack([np.asarray(p[1], dtype=np.float32) for p in poses])
    renders, face = [], np.full((B, *size_hw), -1, dtype=np.int32)
    for b, mi in enumerate(mesh_index):
        if not 0 <= mi < len(meshes):
            renders.append(None)
            continue
        renders.append(render_oracle.render(meshes[mi][0], meshes[mi][1], R[b], t[b], K[b], size_hw, near, far, CENTER))
        face[b] = renders[-1].face
    sc = None
    if scene is not None:
        S, frame_hw, scene_index, origin_xy = scene
        depth = np.stack([np.zeros(size_hw, np.float32) if r is None else r.depth for r in renders])
        d, inst = shade_oracle.compose(depth, scene_index, origin_xy, frame_hw, S)
        sc = Scene(S, tuple(frame_hw), np.asarray(scene_index, dtype=np.int32), None if origin_xy is None else np.asarray(origin_xy, dtype=np.int32), inst, d)
    if plant is not None:
        plant(face, None if sc is None else sc.instance)
    return Case(name, tuple(meshes), np.asarray(mesh_index, dtype=np.int32), R, t, K, _rows(light, B), _rows(phong, B), tuple(size_hw), near, far, face,
                tuple(renders), exact_halves, sc)


def _grid_square():
    """Two faces on the rasteriser's grid (tests/render_grid.py): corners on the samples of pixels 2 and 10, depth 1, identity camera."""
    return render_grid.scene("shade-grid-square", *render_grid.quad(render_grid.S(2), render_grid.S(2), render_grid.S(10), render_grid.S(10)), (16, 16),
                             cam=render_grid.CAMERAS[0])


GRID_COLORS = np.array([[0, 4, 96], [4, 0, 100], [96, 228, 0], [64, 100, 32]], dtype=np.uint8)  # multiples of 4, odd and even: the weights are eighths
TILT = render_cases.rot((0, 1, 0), 60.0)
QUAD = (np.array([[-0.1, -0.1, 0], [0.1, -0.1, 0], [0.1, 0.1, 0], [-0.1, 0.1, 0]], dtype=np.float32), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
QUAD_COLORS = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 40]], dtype=np.uint8)
QUAD_POSE = (TILT, np.array([0.004, -0.003, 0.35], dtype=np.float32))
ICO = render_cases.icosphere(0, 0.1)  # 12 vertices, 20 faces
ICO_POSE = (render_cases.POSES["ico"].R, render_cases.POSES["ico"].t)
SMALL, ODD, FRAME, WINDOW = (16, 16), (37, 53), (48, 64), (40, 48)
FRAME_K = render_cases.camera(FRAME)


def _window_K(origin):
    """The frame's camera seen from a window at `origin`: pixel (x, y) of the window is frame pixel (x + x0, y + y0)."""
    K = FRAME_K.copy()
    K[0, 2] -= np.float32(origin[0])
    K[1, 2] -= np.float32(origin[1])
    return K


def _scene_rows():
    """Four instances, two per scene, overlapping pairwise: an icosahedron in front of a tilted quad, and the reverse."""
    poses = [(ICO_POSE[0], np.array([-0.02, 0.01, 0.40], np.float32)), (TILT, np.array([0.09, 0.02, 0.52], np.float32)),
             (TILT, np.array([-0.03, -0.02, 0.45], np.float32)), (ICO_POSE[0], np.array([-0.06, 0.03, 0.60], np.float32))]
    return [1, 0, 0, 1], poses, np.array([0, 0, 1, 1], dtype=np.int32)


def _plant_scene(face, instance):
    instance[0, 0, 0] = 4        # an instance >= B: names no row
    instance[0, 0, 1] = -2       # below -1: names no row
    instance[1, 47, 63] = 0      # a row of scene 0 named by a pixel of scene 1
    instance[0, 47, 0] = 1       # a frame pixel outside row 1's window (its origin is (24, 12))


def _plant_face(face, instance):
    ys, xs = np.nonzero(face[0] >= 0)
    face[0, ys[0], xs[0]] = 20   # = n_face
    face[0, ys[-1], xs[-1]] = -2  # below the miss
    face[0, 0, 0] = 1 << 30


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    ico = _mesh(*ICO, _colors(12, 1))
    quad = _mesh(*QUAD, QUAD_COLORS)
    if name in ("grid-square", "light-on-surface"):
        sc = _grid_square()
        mesh = _mesh(sc.verts, sc.faces, GRID_COLORS)
        if name == "grid-square":
            return _case(name, [mesh], [0], [(sc.R, sc.t)], sc.K, sc.size_hw, phong=(1.0, 0.0, 0.0), near=sc.near, far=sc.far, exact_halves=True)
        # the sample of pixel (4, 6) lies at ((4.5, 6.5) / 64, 1) in camera space, exactly: the light sits on it
        return _case(name, [mesh], [0], [(sc.R, sc.t)], sc.K, sc.size_hw, light=(4.5 / 64, 6.5 / 64, 1.0), near=sc.near, far=sc.far)
    if name == "tilted-quad":
        return _case(name, [quad], [0], [QUAD_POSE], render_cases.camera(ODD), ODD)
    if name == "ico20":
        return _case(name, [ico], [0], [ICO_POSE], render_cases.camera(ODD), ODD)
    if name == "batch":  # three rows over two meshes (vert_off != 0 for the quad) and a row without a mesh
        return _case(name, [ico, quad], [1, 0, -1, 1], [QUAD_POSE, ICO_POSE, ICO_POSE, (render_cases.rot((1, 1, 0), 40.0), QUAD_POSE[1])],
                     render_cases.camera(ODD), ODD, light=[[0.3, -0.4, -0.2], DEFAULT_LIGHT, DEFAULT_LIGHT, [-1.0, 0.5, 0.1]],
                     phong=[DEFAULT_PHONG, [0.2, 0.9, 0.6], DEFAULT_PHONG, [0.5, 0.5, 0.5]])
    if name == "planted-face":
        return _case(name, [ico], [0], [ICO_POSE], render_cases.camera(SMALL), SMALL, plant=_plant_face)
    if name == "back-facing":  # normals that point away from the camera and the light: d = 0
        away = np.tile(TILT.astype(np.float64).T @ np.array([0.0, 0.0, 1.0]), (4, 1))
        return _case(name, [_mesh(*QUAD, QUAD_COLORS, away)], [0], [QUAD_POSE], render_cases.camera(SMALL), SMALL, light=(0.1, -0.2, 0.0))
    if name == "zero-normal":
        return _case(name, [_mesh(*QUAD, QUAD_COLORS, np.zeros((4, 3)))], [0], [QUAD_POSE], render_cases.camera(SMALL), SMALL, light=(0.1, -0.2, 0.9))
    if name == "saturated":
        return _case(name, [_mesh(*ICO, 255 - _colors(12, 2) // 3)], [0], [ICO_POSE], render_cases.camera(SMALL), SMALL, light=(0.1, -0.1, 0.0), phong=(1.5, 1.0, 0.5))
    if name in ("scene", "scene-planted"):
        mi, poses, sidx = _scene_rows()
        origins = np.array([[-8, -6], [24, 12], [-5, 20], [10, 4]], dtype=np.int32)  # negative; 24 + 48 > 64; 20 + 40 > 48
        return _case(name, [ico, quad], mi, poses, np.stack([_window_K(o) for o in origins]), WINDOW, scene=(2, FRAME, sidx, origins),
                     plant=_plant_scene if name == "scene-planted" else None)
    if name == "scene-full":  # the same instances in full-frame maps, no origins: what render_scene draws
        mi, poses, sidx = _scene_rows()
        return _case(name, [ico, quad], mi, poses, FRAME_K, FRAME, scene=(2, FRAME, sidx, None))
    raise KeyError(name)


NAMES = ("grid-square", "tilted-quad", "ico20", "batch", "planted-face", "back-facing", "zero-normal", "light-on-surface", "saturated", "scene",
         "scene-planted", "scene-full")
END_TO_END = ("ico20", "scene-full")  # rendered by the device's own rasteriser in tests/test_gpu_shade.py


def shade(case: Case, mistake=None, out=None) -> shade_oracle.Shaded:
    """The instance form of a case over the sentinel (or `out`)."""
    out = sentinel((len(case.face), *case.size_hw, 3)) if out is None else out
    return shade_oracle.shade(case.ms, case.face, case.mesh_index, case.R, case.t, case.K, case.light, case.phong, out, CENTER, mistake)


def shade_scene(case: Case, mistake=None) -> shade_oracle.Shaded:
    sc = case.scene
    return shade_oracle.shade_scene(case.ms, sentinel((sc.S, *sc.frame_hw, 3)), sc.instance, case.face, case.mesh_index, sc.scene_index, case.R, case.t, case.K,
                                    case.light, case.phong, sc.origin_xy, CENTER, mistake)


def tie_masks(case: Case) -> np.ndarray:
    """(B,h,w) bool: tests/render_oracle.tie_pixels of every row's render, at the tolerance the rasteriser's own test compares z with."""
    return np.stack([np.zeros(case.size_hw, bool) if r is None else render_oracle.tie_pixels(r, render_oracle.z_tolerance(r)) for r in case.renders])


def scene_tie_mask(case: Case) -> np.ndarray:
    """(S,H,W) bool of a case with full-frame maps: the winning row's tie pixels, and the pixels where the two nearest rows of the scene
    lie within the larger of their z tolerances of each other (the device's z may differ from the oracle's by that much)."""
    sc = case.scene
    assert sc.origin_xy is None
    ties, out = tie_masks(case), np.zeros(sc.instance.shape, bool)
    tol = max(render_oracle.z_tolerance(r) for r in case.renders if r is not None)
    for s in range(sc.S):
        rows = [b for b in range(len(case.face)) if sc.scene_index[b] == s and case.renders[b] is not None]
        z = np.stack([np.where(case.renders[b].mask, case.renders[b].z64, np.inf) for b in rows])
        z.sort(0)
        with np.errstate(all="ignore"):
            out[s] = np.isfinite(z[1]) & (z[1] - z[0] <= tol * z[0]) if len(rows) > 1 else False
        for b in rows:
            out[s] |= ties[b] & (sc.instance[s] == b)
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str) -> shade_oracle.Shaded:
    """The instance form's reference (treat as read-only)."""
    return shade(build(name))


@functools.lru_cache(maxsize=None)
def scene_reference(name: str) -> shade_oracle.Shaded:
    """The scene form's reference of a case with a scene (treat as read-only)."""
    return shade_scene(build(name))
