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

import ctypes
import math
from ctypes import c_float, c_int, c_size_t, c_void_p
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
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


_LIB = None
_SIGNATURES = {
    "lc_amd_gtinfo_version": (c_int, []),
    "lc_amd_gtinfo_last_error": (ctypes.c_char_p, []),
    "lc_amd_gtinfo_source_hash": (ctypes.c_char_p, []),
    "lc_gtinfo_f32": (c_int, [c_void_p] * 5 + [c_int] * 6 + [c_float] * 3 + [c_void_p] * 3),
    "lc_scene_compose_workspace_bytes": (c_size_t, [c_int] * 3),
    "lc_scene_compose_f32": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 4 + [c_size_t, c_void_p]),
}


def load(build_if_missing: bool = True):
    """liblc_amd_gtinfo.so, loaded on first use by `_lib.load_target`: a library built from other sources than the ones next to it is
    rebuilt, or refused where hipcc is absent (unless LC_AMD_ALLOW_STALE=1)."""
    global _LIB
    if _LIB is None:
        _LIB = _lib.load_target(_build.GTINFO, _SIGNATURES, build_if_missing)
    return _LIB


def _f32(name: str, t, shape) -> Tensor:
    """Type, element type and shape (None: any size)."""
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.gtinfo: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"lc_amd.gtinfo: {name} must be float32, got {t.dtype}")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError(f"lc_amd.gtinfo: {name} has shape {tuple(t.shape)}, expected ({', '.join('*' if d is None else str(d) for d in shape)})")
    return t


def _i32(name: str, t, shape) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.gtinfo: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"lc_amd.gtinfo: {name} must be int32 or int64, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"lc_amd.gtinfo: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _delta(delta) -> float:
    if isinstance(delta, bool) or not isinstance(delta, (int, float)):
        raise TypeError(f"lc_amd.gtinfo: delta must be a number, got {type(delta)}")
    if not math.isfinite(delta) or delta < 0:
        raise ValueError(f"lc_amd.gtinfo: delta must be finite and not negative, got {delta}")
    return float(delta)


def _pair(name: str, v):
    if isinstance(v, (Tensor, str)) or not hasattr(v, "__len__") or len(v) != 2:
        raise ValueError(f"lc_amd.gtinfo: {name} is a pair, got {v!r}")
    return v[0], v[1]


def _center(pixel_center):
    cx, cy = _pair("pixel_center", pixel_center)
    return float(cx), float(cy)


def _size(name: str, hw, limit: int):
    h, w = _pair(name, hw)
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, int) or not isinstance(w, int):
        raise TypeError(f"lc_amd.gtinfo: {name} holds two whole numbers, got {hw!r}")
    if not (1 <= h <= limit and 1 <= w <= limit):
        raise ValueError(f"lc_amd.gtinfo: {name} of 1 to {limit}, got {h} x {w}")
    return h, w


def _on(dev, first: str, **named):
    for name, t in named.items():
        if t is not None and t.device != dev:
            raise RuntimeError(f"lc_amd.gtinfo: {name} is on {t.device}, {first} is on {dev}")


def _scenes(depth_test, scene_index, B: int):
    """depth_test as (S,H,W) and the rule for a missing scene_index (that of lc_amd.vsd): one scene serves every instance, B scenes serve
    one instance each."""
    if isinstance(depth_test, Tensor) and depth_test.dim() == 2:
        depth_test = depth_test[None]
    Dt = _f32("depth_test", depth_test, (None, None, None))
    S = int(Dt.shape[0])
    if scene_index is None:
        if S not in (1, B):
            raise ValueError(f"lc_amd.gtinfo: scene_index is needed to tell which of the {S} scenes each of the {B} instances belongs to")
    else:
        _i32("scene_index", scene_index, (B,))
    return Dt, S


def _scene_index(scene_index, S: int, B: int, dev) -> Tensor:
    if scene_index is None:
        return torch.zeros(B, device=dev, dtype=torch.int32) if S == 1 else torch.arange(B, device=dev, dtype=torch.int32)
    return scene_index.to(torch.int32).contiguous()


def _window(h: int, w: int, H: int, W: int, origin_xy, B: int, placed: bool = False):
    """The size rules of a window in a frame (placed: by the caller itself, with no origin_xy to check)."""
    _size("the frame", (H, W), MAX_FRAME)
    _size("the window", (h, w), MAX_WINDOW)
    if h * w >= 2 ** 31:
        raise ValueError(f"lc_amd.gtinfo: a window of {h} x {w} pixels overflows the int32 counts")
    if origin_xy is not None:
        _i32("origin_xy", origin_xy, (B, 2))
    elif not placed and (h, w) != (H, W):
        raise ValueError(f"lc_amd.gtinfo: without origin_xy the maps ({h} x {w}) must have the frame's size ({H} x {W})")


def _fail(lib, what: str, rc: int):
    raise RuntimeError(f"lc_amd.{what} failed (code {rc}): {lib.lc_amd_gtinfo_last_error().decode(errors='replace')}")


@torch.no_grad()
def gt_info_from_depth(depth_gt, depth_test, K, *, delta, scene_index=None, origin_xy=None, pixel_center=(0.0, 0.0), want_mask=True) -> GtInfo:
    """depth_gt (B,h,w); depth_test (H,W) or (S,H,W) with scene_index (B,) int32 / int64 (default: the one scene, or scene b for instance b
    when S = B); K (3,3) or (B,3,3); origin_xy (B,2) int32 / int64 = (x0,y0) of the (h,w) maps in the (H,W) frame, anywhere, or None for
    full-frame maps."""
    delta = _delta(delta)
    pcx, pcy = _center(pixel_center)
    Dg = _f32("depth_gt", depth_gt, (None, None, None))
    B, h, w = (int(n) for n in Dg.shape)
    Dt, S = _scenes(depth_test, scene_index, B)
    H, W = int(Dt.shape[1]), int(Dt.shape[2])
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3):
        K = K.expand(B, 3, 3)
    Kc = _f32("K", K, (B, 3, 3))
    _window(h, w, H, W, origin_xy, B)
    Dg = _lib.require_hip_f32("depth_gt", Dg)
    dev = Dg.device
    _on(dev, "depth_gt", depth_test=Dt, K=Kc, scene_index=scene_index, origin_xy=origin_xy)
    Dt, Kc = Dt.contiguous(), Kc.contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    info = torch.empty(B, COLUMNS, device=dev, dtype=torch.int32)
    mask = torch.empty(B, h, w, device=dev, dtype=torch.bool) if want_mask else None
    if B:
        idx = _scene_index(scene_index, S, B, dev)
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_gtinfo_f32(_lib.ptr(Dg), _lib.ptr(org), _lib.ptr(Dt), _lib.ptr(idx), _lib.ptr(Kc), B, h, w, S, H, W, pcx, pcy, delta,
                                   _lib.ptr(info), _lib.ptr(mask), _lib.stream_ptr(dev))
        if rc != 0:
            _fail(lib, "lc_gtinfo_f32", rc)
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
    Di = _f32("depth_inst", depth_inst, (None, None, None))
    B, h, w = (int(n) for n in Di.shape)
    _i32("scene_index", scene_index, (B,))
    _window(h, w, H, W, origin_xy, B)
    Di = _lib.require_hip_f32("depth_inst", Di)
    dev = Di.device
    _on(dev, "depth_inst", scene_index=scene_index, origin_xy=origin_xy)
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
        _fail(lib, "lc_scene_compose_f32", rc)
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
    delta = _delta(delta)
    _center(pixel_center)
    if not isinstance(mesh_index, Tensor) or mesh_index.dtype != torch.int32:
        raise TypeError("lc_amd.gtinfo: mesh_index must be an int32 tensor on the GPU (MeshSet.index_of)")
    if mesh_index.dim() != 1:
        raise ValueError(f"lc_amd.gtinfo: mesh_index has shape {tuple(mesh_index.shape)}, expected (B,)")
    B = int(mesh_index.shape[0])
    Rc = _f32("R", R, (B, 3, 3))
    if isinstance(t, Tensor) and tuple(t.shape) not in ((B, 3), (B, 3, 1)):
        raise ValueError(f"lc_amd.gtinfo: t has shape {tuple(t.shape)}, expected {(B, 3)} or {(B, 3, 1)}")
    tc = _f32("t", t.reshape(B, 3) if isinstance(t, Tensor) else t, (B, 3))
    if isinstance(K, Tensor) and tuple(K.shape) == (3, 3):
        K = K.expand(B, 3, 3)
    Kc = _f32("K", K, (B, 3, 3))
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
            _i32("scene_index", scene_index, (B,))
            if isinstance(n_scenes, bool) or not isinstance(n_scenes, int) or n_scenes < 1:
                raise ValueError("lc_amd.gtinfo: with scene_index and no depth_test, n_scenes says how many scenes to compose")
            S = n_scenes
    else:
        Dt, S = _scenes(depth_test, scene_index, B)
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
        _i32("window_xy", window_xy, (B, 2))
    else:
        mx, my = _pair("margin", (0, 0) if margin is None else margin)
        if isinstance(mx, bool) or isinstance(my, bool) or not isinstance(mx, int) or not isinstance(my, int) or mx < 0 or my < 0:
            raise ValueError(f"lc_amd.gtinfo: margin = (mx, my) holds two whole numbers that are not negative, got {margin!r}")
        h, w = H + 2 * my, W + 2 * mx
    _window(h, w, H, W, window_xy, B, placed=True)
    for name, x in (("mesh_index", mesh_index), ("R", Rc), ("t", tc), ("K", Kc), ("depth_test", Dt), ("scene_index", scene_index), ("window_xy", window_xy)):
        if x is not None and x.device != dev:
            raise RuntimeError(f"lc_amd.gtinfo: {name} is on {x.device}, the meshes are on {dev} (there is no CPU fallback in the product path)")
    if window_xy is not None:
        origin = window_xy.to(torch.int32).contiguous()
    else:
        origin = torch.cat((torch.full((B, 1), -mx, device=dev, dtype=torch.int32), torch.full((B, 1), -my, device=dev, dtype=torch.int32)), 1)  # (fills: capturable)
    Kr = Kc.clone()
    Kr[:, 0, 2] -= origin[:, 0].to(torch.float32)
    Kr[:, 1, 2] -= origin[:, 1].to(torch.float32)
    out = _render.render_depth(meshes, mesh_index, Rc, tc, Kr, (h, w), near=near, far=far, pixel_center=pixel_center)
    known = (mesh_index >= 0) & (mesh_index < meshes.n_meshes)
    idx = torch.where(known, _scene_index(scene_index, S, B, dev), torch.full_like(mesh_index, -1))  # an unknown mesh: refused by the record as well
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
