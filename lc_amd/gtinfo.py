"""BOP's ground-truth visibility annotations on the device (lc_amd/csrc/gtinfo/lc_gtinfo.hip, lc_amd/_C/liblc_amd_gtinfo.so; C ABI and
the exact definition of every output in include/lc_amd_gtinfo.h): what the BOP toolkit's calc_gt_masks.py and calc_gt_info.py write per
instance -- `mask_visib`, `px_count_all`, `px_count_valid`, `px_count_visib`, `visib_fract`, `bbox_obj`, `bbox_visib` -- from one render
of the instance and the scene's depth.

    gt_info_from_depth(depth_gt, depth_test, K, *, delta, ...) -> GtInfo(info, mask_visib)
        the record alone, for renders from any renderer
    compose_scene_depth(depth_inst, scene_index, frame_hw, n_scenes, ...) -> SceneDepth(depth, instance, info)
        a scene's depth as the per-pixel nearest of its instances' renders (synthetic scenes have no measured depth)
    compute_gt_info(meshes, mesh_index, R, t, K, depth_test, *, frame_hw, delta, near, far, ...) -> GtRendered
        one `render.render_depth` call into the window, the scene composed from those renders when depth_test is None, then the record
    bop_records(result, *, bbox_plus_one=False) -> [dict]
        BOP's keys, on the host: the only function here that reads back

`info` (B,12) int32: px_count_all, px_count_valid, px_count_visib, edge, the inclusive box x_min, y_min, x_max, y_max of the silhouette and
that of its visible part, both in frame coordinates; an empty box is four times -1.  `edge` > 0 says that the window may have cut the
silhouette: px_count_all and the first box are then lower bounds.  A refused row (scene_index outside the scenes, an origin beyond
MAX_ORIGIN, an unknown mesh) is -1 throughout with a zero mask.  Everything is an integer sum, minimum or maximum: the same bits for any
batch, order and launch.

The window: `origin_xy` (B,2) = (x0, y0) places the (h,w) maps in the (H,W) frame; it may be negative and the window may reach outside
the frame or be larger than it.  BOP measures the whole silhouette of a truncated object in a 3H x 3W render: origin (-W,-H), or
`margin=(W, H)` of `compute_gt_info`.  An object-centred window (`vsd.window_origins`) is the cheap form.

`pixel_center` = (0, 0), the default, gives pixel (x,y) the K-coordinates (x,y): the convention of BOP's depth-to-distance conversion.

float32 HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device,
allocates its outputs and the composition's workspace only and can be captured into a graph.
"""
from __future__ import annotations

from ctypes import c_float, c_int, c_size_t, c_void_p
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

COLUMNS = 12             # LC_GTINFO_COLUMNS
MAX_FRAME = 16384        # LC_GTINFO_MAX_FRAME
MAX_WINDOW = 49152       # LC_GTINFO_MAX_WINDOW
MAX_ORIGIN = 16777216    # LC_GTINFO_MAX_ORIGIN
TILE_W, TILE_H = 256, 16  # LC_GTINFO_TILE_W, LC_GTINFO_TILE_H: the window pixels one workgroup reduces
PX_ALL, PX_VALID, PX_VISIB, EDGE = 0, 1, 2, 3
BOX_OBJ, BOX_VISIB = slice(4, 8), slice(8, 12)


class GtInfo(NamedTuple):
    info: Tensor                  # (B,12) int32
    mask_visib: Optional[Tensor]  # (B,h,w) bool, window coordinates (want_mask)

    def visib_fract(self) -> Tensor:
        return _visib_fract(self.info)


class SceneDepth(NamedTuple):
    depth: Tensor               # (S,H,W) float32, 0 where nothing is hit
    instance: Optional[Tensor]  # (S,H,W) int32: the winning row, -1 where nothing is hit (want_instance)
    info: Tensor                # (B,) int32: 0, -1 for a skipped row


class GtRendered(NamedTuple):
    info: Tensor                 # (B,12) int32
    mask_visib: Tensor           # (B,h,w) bool, window coordinates
    depth_gt: Tensor             # (B,h,w) float32: the renders; `depth_gt > 0` is BOP's `mask`
    origin_xy: Tensor            # (B,2) int32: where the windows lie
    render_info: Tensor          # (B,) int32: the renderer's info (faces dropped at the near plane; -1: unknown mesh)
    scene: Optional[SceneDepth]  # the composed scene (depth_test=None)

    def visib_fract(self) -> Tensor:
        return _visib_fract(self.info)


def _visib_fract(info: Tensor) -> Tensor:
    """px_count_visib / px_count_all as float64 on the device, 0 where the denominator is 0 (and on a refused row)."""
    n_all, n_vis = info[:, PX_ALL].double(), info[:, PX_VISIB].double()
    return torch.where(info[:, PX_ALL] > 0, n_vis / n_all.clamp(min=1.0), torch.zeros_like(n_all))


_SO = _lib.SideLibrary(_build.GTINFO, {
    "lc_gtinfo_f32": (c_int, [c_void_p] * 5 + [c_int] * 6 + [c_float] * 3 + [c_void_p] * 3),
    "lc_scene_compose_workspace_bytes": (c_size_t, [c_int] * 3),
    "lc_scene_compose_f32": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 4 + [c_size_t, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("gtinfo")


def _size(name: str, hw, limit: int):
    h, w = _A.pair(name, hw)
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, int) or not isinstance(w, int):
        raise TypeError(f"lc_amd.gtinfo: {name} holds two whole numbers, got {hw!r}")
    if not (1 <= h <= limit and 1 <= w <= limit):
        raise ValueError(f"lc_amd.gtinfo: {name} of 1 to {limit}, got {h} x {w}")
    return h, w


def _window(h: int, w: int, H: int, W: int, origin_xy, B: int, placed: bool = False):
    """The size rules of a window in a frame (placed: by the caller itself, with no origin_xy to check)."""
    _size("the frame", (H, W), MAX_FRAME)
    _size("the window", (h, w), MAX_WINDOW)
    if h * w >= 2 ** 31:
        raise ValueError(f"lc_amd.gtinfo: a window of {h} x {w} pixels overflows the int32 counts")
    if origin_xy is not None:
        _A.i32("origin_xy", origin_xy, (B, 2))
    elif not placed and (h, w) != (H, W):
        raise ValueError(f"lc_amd.gtinfo: without origin_xy the maps ({h} x {w}) must have the frame's size ({H} x {W})")


@torch.no_grad()
def gt_info_from_depth(depth_gt, depth_test, K, *, delta, scene_index=None, origin_xy=None, pixel_center=(0.0, 0.0), want_mask=True) -> GtInfo:
    """depth_gt (B,h,w); depth_test (H,W) or (S,H,W) with scene_index (B,) int32 / int64 (default: the one scene, or scene b for instance b
    when S = B); K (3,3) or (B,3,3); origin_xy (B,2) int32 / int64 = (x0,y0) of the (h,w) maps in the (H,W) frame, anywhere, or None for
    full-frame maps."""
    delta = _A.delta(delta)
    pcx, pcy = _A.center(pixel_center)
    Dg = _A.f32("depth_gt", depth_gt, (None, None, None))
    B, h, w = (int(n) for n in Dg.shape)
    Dt, S = _A.scenes(depth_test, scene_index, B, "instances")
    H, W = int(Dt.shape[1]), int(Dt.shape[2])
    Kc = _A.cam_K("K", K, B)
    _window(h, w, H, W, origin_xy, B)
    Dg = _lib.require_hip_f32("depth_gt", Dg)
    dev = Dg.device
    _A.same_device(dev, "depth_gt is on {}", depth_test=Dt, K=Kc, scene_index=scene_index, origin_xy=origin_xy)
    Dt, Kc = Dt.contiguous(), Kc.contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    info = torch.empty(B, COLUMNS, device=dev, dtype=torch.int32)
    mask = torch.empty(B, h, w, device=dev, dtype=torch.bool) if want_mask else None
    if B:
        idx = _A.scene_index(scene_index, S, B, dev)
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_gtinfo_f32(_lib.ptr(Dg), _lib.ptr(org), _lib.ptr(Dt), _lib.ptr(idx), _lib.ptr(Kc), B, h, w, S, H, W, pcx, pcy, delta,
                                   _lib.ptr(info), _lib.ptr(mask), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("lc_gtinfo_f32", rc)
    return GtInfo(info, mask)


@torch.no_grad()
def compose_scene_depth(depth_inst, scene_index, frame_hw, n_scenes, *, origin_xy=None, want_instance=False) -> SceneDepth:
    """depth_inst (B,h,w): the instances' renders; scene_index (B,) int32 / int64; frame_hw = (H,W); n_scenes = S; origin_xy as in
    `gt_info_from_depth`.  The depth of scene s at a pixel is the smallest z with 0 < z < inf of the rows of s that cover it, the lowest
    row among equal z."""
    H, W = _size("frame_hw", frame_hw, MAX_FRAME)
    if isinstance(n_scenes, bool) or not isinstance(n_scenes, int):
        raise TypeError(f"lc_amd.gtinfo: n_scenes must be a whole number, got {type(n_scenes)}")
    if n_scenes < 1:
        raise ValueError(f"lc_amd.gtinfo: at least one scene, got n_scenes = {n_scenes}")
    Di = _A.f32("depth_inst", depth_inst, (None, None, None))
    B, h, w = (int(n) for n in Di.shape)
    _A.i32("scene_index", scene_index, (B,))
    _window(h, w, H, W, origin_xy, B)
    Di = _lib.require_hip_f32("depth_inst", Di)
    dev = Di.device
    _A.same_device(dev, "depth_inst is on {}", scene_index=scene_index, origin_xy=origin_xy)
    idx = scene_index.to(torch.int32).contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    depth = torch.empty(n_scenes, H, W, device=dev, dtype=torch.float32)
    inst = torch.empty(n_scenes, H, W, device=dev, dtype=torch.int32) if want_instance else None
    info = torch.empty(B, device=dev, dtype=torch.int32)
    lib = load()
    nbytes = int(lib.lc_scene_compose_workspace_bytes(n_scenes, H, W))
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    with _lib.on_device(dev):
        rc = lib.lc_scene_compose_f32(_lib.ptr(Di) if B else None, _lib.ptr(org) if B else None, _lib.ptr(idx) if B else None, B, h, w, n_scenes, H, W,
                                      _lib.ptr(depth), _lib.ptr(inst), _lib.ptr(info) if B else None, _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("lc_scene_compose_f32", rc)
    return SceneDepth(depth, inst, info)


@torch.no_grad()
def compute_gt_info(meshes, mesh_index, R, t, K, depth_test, *, frame_hw=None, margin=None, window_hw=None, window_xy=None, delta, near, far,
                    scene_index=None, n_scenes=None, pixel_center=(0.0, 0.0)) -> GtRendered:
    """Render and annotate.  meshes: a `render.MeshSet`; mesh_index (B,) int32 on the device (`meshes.index_of(obj_ids)`; an unknown mesh
    refuses the row); R (B,3,3), t (B,3) or (B,3,1), K (3,3) or (B,3,3); depth_test, scene_index and delta as in `gt_info_from_depth`.

    The window.  Default: the frame.  margin = (mx, my) widens it by mx columns and my rows on every side, the same for every row
    (margin = (W, H) is BOP's 3H x 3W render); or window_hw = (h,w) with window_xy (B,2) int32 / int64 puts a window per row anywhere.  The
    render uses K with K02 - x0 and K12 - y0 (formed in fp32: exact for an integer-valued principal point, where a window's render is the
    frame's render cropped), the record the given K and the origin.

    depth_test = None is the synthetic case: frame_hw = (H,W) is needed, and the scenes' depth is first composed from these same renders
    (`compose_scene_depth`; every row one scene, or scene_index with n_scenes) and returned as `scene`.  An instance is then hidden exactly
    where another one of its scene is nearer by more than delta."""
    from . import render as _render

    if not isinstance(meshes, _render.MeshSet):
        raise TypeError(f"lc_amd.gtinfo: meshes must be a lc_amd.render.MeshSet, got {type(meshes)}")
    delta = _A.delta(delta)
    _A.center(pixel_center)
    B, (Rc,), (tc,), Kc = _A.pose_batch(mesh_index, dict(R=R), dict(t=t), K)
    if depth_test is None:
        if frame_hw is None:
            raise ValueError("lc_amd.gtinfo: without depth_test the scene is composed from the renders, and frame_hw = (H, W) is needed")
        H, W = _size("frame_hw", frame_hw, MAX_FRAME)
        Dt = None
        if scene_index is None:
            if n_scenes not in (None, 1):
                raise ValueError(f"lc_amd.gtinfo: scene_index is needed to tell which of the {n_scenes} scenes each instance belongs to")
            S = 1
        else:
            _A.i32("scene_index", scene_index, (B,))
            if isinstance(n_scenes, bool) or not isinstance(n_scenes, int) or n_scenes < 1:
                raise ValueError("lc_amd.gtinfo: with scene_index and no depth_test, n_scenes says how many scenes to compose")
            S = n_scenes
    else:
        Dt, S = _A.scenes(depth_test, scene_index, B, "instances")
        H, W = int(Dt.shape[1]), int(Dt.shape[2])
        if frame_hw is not None and tuple(_size("frame_hw", frame_hw, MAX_FRAME)) != (H, W):
            raise ValueError(f"lc_amd.gtinfo: frame_hw = {tuple(frame_hw)} but depth_test is {H} x {W}")
        if n_scenes not in (None, S):
            raise ValueError(f"lc_amd.gtinfo: n_scenes = {n_scenes} but depth_test holds {S} scenes")
    if (window_hw is None) != (window_xy is None):
        raise ValueError("lc_amd.gtinfo: window_hw and window_xy go together")
    if margin is not None and window_hw is not None:
        raise ValueError("lc_amd.gtinfo: margin or window_hw with window_xy, not both")
    dev = meshes.device
    if window_xy is not None:
        h, w = _size("window_hw", window_hw, MAX_WINDOW)
        _A.i32("window_xy", window_xy, (B, 2))
    else:
        mx, my = _A.pair("margin", (0, 0) if margin is None else margin)
        if isinstance(mx, bool) or isinstance(my, bool) or not isinstance(mx, int) or not isinstance(my, int) or mx < 0 or my < 0:
            raise ValueError(f"lc_amd.gtinfo: margin = (mx, my) holds two whole numbers that are not negative, got {margin!r}")
        h, w = H + 2 * my, W + 2 * mx
    _window(h, w, H, W, window_xy, B, placed=True)
    _A.same_device(dev, _args.MESHES_ON, mesh_index=mesh_index, R=Rc, t=tc, K=Kc, depth_test=Dt, scene_index=scene_index, window_xy=window_xy)
    if window_xy is not None:
        origin = window_xy.to(torch.int32).contiguous()
    else:
        origin = torch.cat((torch.full((B, 1), -mx, device=dev, dtype=torch.int32), torch.full((B, 1), -my, device=dev, dtype=torch.int32)), 1)  # (fills: capturable)
    Kr = Kc.clone()
    Kr[:, 0, 2] -= origin[:, 0].to(torch.float32)
    Kr[:, 1, 2] -= origin[:, 1].to(torch.float32)
    out = _render.render_depth(meshes, mesh_index, Rc, tc, Kr, (h, w), near=near, far=far, pixel_center=pixel_center)
    known = (mesh_index >= 0) & (mesh_index < meshes.n_meshes)
    idx = torch.where(known, _A.scene_index(scene_index, S, B, dev), torch.full_like(mesh_index, -1))  # an unknown mesh: refused by the record as well
    scene = None
    if Dt is None:
        scene = compose_scene_depth(out.depth, idx, (H, W), S, origin_xy=origin, want_instance=True)
        Dt = scene.depth
    res = gt_info_from_depth(out.depth, Dt, Kc, delta=delta, scene_index=idx, origin_xy=origin, pixel_center=pixel_center)
    return GtRendered(res.info, res.mask_visib, out.depth, origin, out.info, scene)


def bop_records(result, *, bbox_plus_one=False):
    """The records of `scene_gt_info.json`, one dict per row, from a `GtInfo`, a `GtRendered` or an `info` tensor: the ONE read-back of
    this module.  bbox_obj and bbox_visib are [x, y, w, h] with w = x_max - x_min and h = y_max - y_min as the BOP toolkit forms them, or
    with + 1 each (bbox_plus_one: the width in pixels, as the reference's own mask-to-box helper counts it).  Both boxes are [-1, -1, -1, -1] when
    px_count_visib is 0 -- this project's rule (include/lc_amd_gtinfo.h); visib_fract is formed from the two integers as a Python
    float, 0.0 when px_count_all is 0.  A refused row gives -1 counts, -1 boxes and visib_fract 0.0."""
    info = result if isinstance(result, Tensor) else result.info
    if not isinstance(info, Tensor) or info.dim() != 2 or info.shape[1] != COLUMNS or info.dtype != torch.int32:
        raise ValueError("lc_amd.gtinfo: bop_records takes a GtInfo, a GtRendered or their (B,12) int32 info")
    one = 1 if bbox_plus_one else 0
    out = []
    for row in info.cpu().tolist():
        n_all, n_valid, n_vis = row[PX_ALL], row[PX_VALID], row[PX_VISIB]

        def box(x0, y0, x1, y1):
            return [x0, y0, x1 - x0 + one, y1 - y0 + one] if n_vis > 0 else [-1, -1, -1, -1]

        out.append(dict(bbox_obj=box(*row[BOX_OBJ]), bbox_visib=box(*row[BOX_VISIB]), px_count_all=n_all, px_count_valid=n_valid, px_count_visib=n_vis,
                        visib_fract=n_vis / float(n_all) if n_all > 0 else 0.0))
    return out
