"""Annotated synthetic scenes from one seed word: the drawn poses (lc_amd/posedraw.py) chained in front of the existing render, compose,
shade and annotate stages, all on the device.

    synth_scenes(meshes, appearance, radius, cfg, *, seed, scene_id, mesh_index, cam_K, frame_hw, near, far, light, phong, delta,
                 background=None) -> SynthScenes(frames, scene, gt, poses, scene_index, render_info)
    render_and_annotate(meshes, appearance, drawn, cam_K, frame_hw, *, near, far, light, phong, delta, background=None) -> SynthScenes

The stages, in order:
    1. `posedraw.draw_scene_poses`: R, t and `mesh_index_out` of S scenes of M slots from (cfg, seed, scene_id);
    2. the B = S M rows in scene order, row s M + m of scene s;
    3. `shade.render_scene` (an `Appearance`) or `texture.render_scene` (a `TexturedAppearance`): the frames and the composed depth;
    4. `gtinfo.gt_info_from_depth` of the instances' renders against that depth: counts, boxes, visible masks.

Nothing is formed on the host and nothing is read back; the call allocates its stages' outputs only, never waits for the device and can
be captured with `torch.cuda.graph`: one replay after `seed.add_(1)` gives a new annotated scene.  No pixel code lives here.

Two things the stages do not offer as the chain would want them: `render_scene` does not hand back the instances'
own renders, which stage 4 compares with the scene, so `render.render_depth` runs once more on the same rows -- the same launch on the same
inputs, hence the same bits as the renders the scene was composed from; and the record's kernel refuses a row by its scene index, not
by its mesh, so a slot that was not placed is given the scene index -1 there, as `gtinfo.compute_gt_info` does for an unknown mesh.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor

from . import gtinfo as _gtinfo
from . import posedraw as _posedraw
from . import render as _render
from . import shade as _shade
from . import texture as _texture
from .gtinfo import GtInfo, SceneDepth
from .posedraw import PoseDrawConfig, ScenePoses

PIXEL_CENTER = (0.5, 0.5)  # the rasteriser's and the shading pass's default: the chain renders, shades and annotates at one convention


class SynthScenes(NamedTuple):
    frames: Tensor       # (S,H,W,3) uint8
    scene: SceneDepth    # depth (S,H,W) float32, instance (S,H,W) int32 (row s M + m, -1 where nothing is hit), info (B,)
    gt: GtInfo           # info (B,12) int32 and mask_visib (B,H,W) bool; `gt.visib_fract()`; a slot that was not placed: -1 throughout
    poses: ScenePoses    # R (B,3,3), t (B,3), tries (B,), info (B,), mesh_index_out (B,): the drawn poses, flattened to the B rows
    scene_index: Tensor  # (B,) int32: the scene of each row
    render_info: Tensor  # (B,) int32: the rasteriser's info (faces dropped at the near plane; -1: a slot that was not placed)


def flatten(poses: ScenePoses) -> ScenePoses:
    """(S,M,...) -> (S M,...), views."""
    S, M = poses.info.shape
    B = S * M
    return ScenePoses(poses.R.reshape(B, 3, 3), poses.t.reshape(B, 3), poses.tries.reshape(B), poses.info.reshape(B), poses.mesh_index_out.reshape(B))


@torch.no_grad()
def render_and_annotate(meshes, appearance, drawn: ScenePoses, cam_K, frame_hw, *, near, far, light, phong, delta, background=None) -> SynthScenes:
    """Stages 2 to 4 on poses of shape (S,M,...) that are already on the device, drawn there or uploaded: what `synth_scenes` runs behind
    its draw, and what a host route would run behind its upload (scripts/bench_posedraw.py times both)."""
    if not isinstance(meshes, _render.MeshSet):
        raise TypeError(f"lc_amd.synthscene: meshes must be a MeshSet, got {type(meshes)}")
    if isinstance(appearance, _texture.TexturedAppearance):
        render_scene = _texture.render_scene
    elif isinstance(appearance, _shade.Appearance):
        render_scene = _shade.render_scene
    else:
        raise TypeError(f"lc_amd.synthscene: appearance must be an Appearance or a TexturedAppearance, got {type(appearance)}")
    H, W = int(frame_hw[0]), int(frame_hw[1])
    S, M = (int(n) for n in drawn.info.shape)
    dev = drawn.info.device
    poses = flatten(drawn)
    B = S * M
    scene_index = torch.arange(S, device=dev, dtype=torch.int32)[:, None].expand(S, M).reshape(B)  # views and one copy: no wait
    K = (cam_K.expand(S, 3, 3) if tuple(cam_K.shape) == (3, 3) else cam_K)[:, None].expand(S, M, 3, 3).reshape(B, 3, 3)
    frames, scene = render_scene(meshes, appearance, poses.mesh_index_out, scene_index, poses.R, poses.t, K, (H, W), S, near=near, far=far, light=light,
                                 phong=phong, background=background, pixel_center=PIXEL_CENTER)
    inst = _render.render_depth(meshes, poses.mesh_index_out, poses.R, poses.t, K, (H, W), near=near, far=far, pixel_center=PIXEL_CENTER)
    idx = torch.where(poses.mesh_index_out >= 0, scene_index, torch.full_like(scene_index, -1))  # a slot that was not placed: refused by the record as well
    gt = _gtinfo.gt_info_from_depth(inst.depth, scene.depth, K, delta=delta, scene_index=idx, pixel_center=PIXEL_CENTER)
    return SynthScenes(frames, scene, gt, poses, scene_index, inst.info)


@torch.no_grad()
def synth_scenes(meshes, appearance, radius, cfg: PoseDrawConfig, *, seed, scene_id, mesh_index, cam_K, frame_hw, near, far, light, phong, delta,
                 background=None) -> SynthScenes:
    """meshes: a `render.MeshSet`; appearance: a `shade.Appearance` or a `texture.TexturedAppearance` of it; radius (n_meshes,) float32 on
    the device (`posedraw.mesh_radii`); cfg, seed, scene_id (S,), mesh_index (S,M) and cam_K (3,3) or (S,3,3) as `draw_scene_poses` takes
    them; frame_hw = (H, W); near, far, light, phong, background as `render_scene`; delta as `gt_info_from_depth`."""
    if not isinstance(meshes, _render.MeshSet):
        raise TypeError(f"lc_amd.synthscene: meshes must be a MeshSet, got {type(meshes)}")
    if not isinstance(appearance, (_shade.Appearance, _texture.TexturedAppearance)):
        raise TypeError(f"lc_amd.synthscene: appearance must be an Appearance or a TexturedAppearance, got {type(appearance)}")
    if isinstance(radius, Tensor) and radius.dim() == 1 and int(radius.shape[0]) != meshes.n_meshes:
        raise ValueError(f"lc_amd.synthscene: radius holds {int(radius.shape[0])} values, the set {meshes.n_meshes} meshes")
    drawn = _posedraw.draw_scene_poses(cfg, seed=seed, scene_id=scene_id, mesh_index=mesh_index, radius=radius, cam_K=cam_K)
    return render_and_annotate(meshes, appearance, drawn, cam_K, frame_hw, near=near, far=far, light=light, phong=phong, delta=delta, background=background)
