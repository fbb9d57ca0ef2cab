"""The training crop's geometry: its contract in host numpy, and the kernels that draw the same numbers on the device from the seed word
(lc_amd/csrc/geometry/lc_geometry.hip, lc_amd/_C/liblc_amd_geometry.so; C ABI in include/lc_amd_geometry.h).
What the reference's loader computes per instance on a host core before it touches a pixel -- `_aug_bbox` and the rotation
(`dataset.py:313-327,402`), the two `_get_affine_transform` matrices (`dataset.py:404-405`), `out_K = affine33 @ cam_K` and `out_pix_scale`
(`dataset.py:437,470`), and the background's stretch of `_switch_bg`.

    zoom_geometry_host(cfg, seed, sample_ids, bbox_xyxy, im_hw, cam_K, in_wh, out_wh, train=True) -> ZoomGeometry     host numpy
    background_geometry_host(seed, sample_ids, bg_hw, out_hw) -> (G,2,3) float32                                  = augment.background_matrices
    cos_sin_turns(u4) -> (c, s)                                                                                   the stated polynomial
    zoom_geometry(cfg, *, seed, sample_id, bbox_xyxy, im_hw, cam_K, in_wh, out_wh, train=True, want_info=False) -> ZoomGeometry   device tensors
    background_geometry(*, seed, sample_id, bg_hw, out_hw) -> (B,2,3) float32                                     device tensor

The matrices feed fixed-point warps, where a last-place difference moves a pixel, so every number is defined bit for bit: fp64 with
every product, sum and quotient rounded on its own, in the order written in `zoom_geometry_host`, the random numbers those of
`augment.draw_zoom` (`augment.u(seed, id, OP_ZOOM, 0..4)`), and the rotation's cosine and sine a stated polynomial on an exactly reduced
argument instead of a libm call (`cos_sin_turns`): what libm returns differs from machine to machine and from the device's.  The host
functions touch no device; `zoom_geometry` and `background_geometry` are one launch each that equals them bit for bit, reads its seed
from one 64-bit word on the device, never waits for the device and allocates its outputs only: a captured graph draws new geometry at
every replay once the word has changed (lc_amd/train_inputs.py chains the loader's stages behind it).  HIP tensors only: there is no
CPU fallback -- the host functions are the definition, not a route.
"""
from __future__ import annotations

import math
from ctypes import c_double, c_int, c_void_p
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import augment as _aug
from . import build as _build
from .augment import AugmentConfig

MAX_SIZE = 16384  # LC_GEOMETRY_MAX_SIZE = LC_CROP_MAX_SIZE

OP_STEP_INDEX = 5  # step_id is key(OP_ZOOM, 5): the draws of `draw_zoom` are 0..4
PI_4 = float.fromhex("0x1.921fb54442d18p-1")  # fl(pi / 4)
# (-1)^(k/2) / k! rounded to fp64, k = 3, 5, ..., 17 and k = 2, 4, ..., 16
SIN_C = tuple(float.fromhex(h) for h in (
    "-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19", "-0x1.ae64567f544e4p-26",
    "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41", "0x1.952c77030ad4ap-49"))
COS_C = tuple(float.fromhex(h) for h in (
    "-0x1.0000000000000p-1", "0x1.5555555555555p-5", "-0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-16", "-0x1.27e4fb7789f5cp-22",
    "0x1.1eed8eff8d898p-29", "-0x1.93974a8c07c9dp-37", "0x1.ae7f3e733b81fp-45"))
# the octant table: (c, s) of octant o = floor(8 f) as (sign, which) pairs over (S, C) of the reduced argument
OCTANTS = ((("+", "C"), ("+", "S")), (("+", "S"), ("+", "C")), (("-", "S"), ("+", "C")), (("-", "C"), ("+", "S")),
           (("-", "C"), ("-", "S")), (("-", "S"), ("-", "C")), (("+", "S"), ("-", "C")), (("+", "C"), ("-", "S")))

_NAN32 = np.float32(np.nan)


class ZoomGeometry(NamedTuple):
    """numpy arrays (`zoom_geometry_host`) or device tensors (`zoom_geometry`).  `centre`, `scale`, `rot` and `cs` are fp64 and for
    information (`rot` = (4 u4) pi where the rotation's gate is open: the angle `affine_from_box` would be given, host only -- the device
    has no use for it and leaves None; `cs` = the (c, s) the matrices are made of).  `zoom_geometry` makes the three others with
    `want_info` only."""
    in_affine: object      # (B,2,3) float32, frame -> network input
    out_affine: object     # (B,2,3) float32, frame -> output map
    out_K: object          # (B,3,3) float32
    out_pix_scale: object  # (B,) float32
    step_id: object        # (B,) int32 >= 0: `mask_crops`' sample_id of this step
    info: object           # (B,) int32: 0, or -1 for a refused row (all of the above but step_id are NaN)
    centre: object         # (B,2) float64
    scale: object          # (B,) float64
    rot: object            # (B,) float64
    cs: object             # (B,2) float64


def cos_sin_turns(u4):
    """(c, s) = (cos, sin) of the angle 4 pi u4 for u4 = k / 2^24, vectorised fp64 with every operation rounded on its own:
    tau = 2 u4, f = tau - floor(tau), o = floor(8 f), g = 8 f - o, for odd o g <- 1 - g (all exact); a = g * fl(pi / 4);
    z = a * a; S = a * (1 + z (s3 + z (s5 + ... + z s17))) and C = 1 + z (c2 + z (c4 + ... + z c16)) by Horner's rule from the highest
    coefficient down, each step one product and one sum; (c, s) from (+-S, +-C) by OCTANTS[o].  a = 0 gives S = 0 and C = 1 exactly."""
    u4 = np.asarray(u4, dtype=np.float64)
    tau = 2.0 * u4
    f = tau - np.floor(tau)
    o = np.floor(8.0 * f)
    g = 8.0 * f - o
    o = o.astype(np.int64)
    g = np.where(o & 1, 1.0 - g, g)
    a = g * PI_4
    z = a * a
    p = np.full_like(z, SIN_C[-1])
    for coef in SIN_C[-2::-1]:
        p = p * z + coef
    S = a * (p * z + 1.0)
    q = np.full_like(z, COS_C[-1])
    for coef in COS_C[-2::-1]:
        q = q * z + coef
    C = q * z + 1.0
    val = {"S": S, "C": C}
    c, s = np.empty_like(z), np.empty_like(z)
    for k, ((sc, wc), (ss, ws)) in enumerate(OCTANTS):
        m = o == k
        c[m] = (val[wc] if sc == "+" else -val[wc])[m]
        s[m] = (val[ws] if ss == "+" else -val[ws])[m]
    return c, s


def _affine(k, c, s, cx, cy, dst_w, dst_h):
    """The forward matrix of `crops.affine_from_box`, term for term in Python's evaluation order, as (B,2,3) fp64."""
    dx, dy = dst_w * 0.5, dst_h * 0.5
    M = np.empty((len(k), 2, 3), dtype=np.float64)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = k * c, k * s, dx - (k * c * cx + k * s * cy)
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = -k * s, k * c, dy - (-k * s * cx + k * c * cy)
    return M


def zoom_geometry_host(cfg: AugmentConfig, seed, sample_ids, bbox_xyxy, im_hw, cam_K, in_wh, out_wh, train=True) -> ZoomGeometry:
    """The definition, in host numpy.  bbox_xyxy (B,4) and cam_K (B,3,3) or (3,3) are rounded to float32 first (what
    the device reads) and widened to fp64; im_hw = (H, W) of the frames; in_wh and out_wh = (w, h) of the network's input and output.

    centre, scale: `augment.draw_zoom`'s expressions in its order (train), or the box centre and `max(w, h, 1) * dzi_pad_scale`
    without a draw (not train).  (c, s) = `cos_sin_turns(u4)` where u3 < rotate_prob (train), else (1, 0).
    in_affine / out_affine = fp32(`_affine(dst_w / scale, c, s, centre, dst_w, dst_h)`) with in_wh / out_wh.
    out_K rows 0-1 = fp32((A[i,0] K[0,j] + A[i,1] K[1,j]) + A[i,2] K[2,j]) with the fp32 out_affine A and K widened; row 2 = K's.
    out_pix_scale = fp32(scale / out_w).  step_id = key(seed, id, OP_ZOOM, 5) & 0x7FFFFFFF.
    info = -1 for a row with a non-finite box or K entry, or with scale not finite or <= 0: its centre, scale, matrices, out_K and
    out_pix_scale are NaN."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    B = len(ids)
    box = np.asarray(bbox_xyxy, dtype=np.float32).reshape(B, 4).astype(np.float64)
    K32 = np.ascontiguousarray(np.broadcast_to(np.asarray(cam_K, dtype=np.float32), (B, 3, 3)))
    K = K32.astype(np.float64)
    in_w, in_h, out_w, out_h = float(in_wh[0]), float(in_wh[1]), float(out_wh[0]), float(out_wh[1])
    with np.errstate(all="ignore"):
        if train:
            centre, scale, rot = _aug.draw_zoom(cfg, seed, ids, box, im_hw)
            u3, u4 = _aug.u(seed, ids, _aug.OP_ZOOM, 3), _aug.u(seed, ids, _aug.OP_ZOOM, 4)
            gate = u3 < cfg.rotate_prob
            c, s = cos_sin_turns(u4)
            c, s = np.where(gate, c, 1.0), np.where(gate, s, 0.0)
        else:
            x1, y1, x2, y2 = box.T
            centre = np.stack((0.5 * (x1 + x2), 0.5 * (y1 + y2)), axis=1)
            w, h = x2 - x1, y2 - y1
            scale = np.where(w > h, w, h)
            scale = np.where(scale > 1.0, scale, 1.0) * cfg.dzi_pad_scale
            rot, c, s = np.zeros(B), np.ones(B), np.zeros(B)
        bad = ~(np.isfinite(box).all(axis=1) & np.isfinite(K).all(axis=(1, 2)) & np.isfinite(scale) & (scale > 0))
        cx, cy = centre[:, 0], centre[:, 1]
        in_affine = _affine(in_w / scale, c, s, cx, cy, in_w, in_h).astype(np.float32)
        out_affine = _affine(out_w / scale, c, s, cx, cy, out_w, out_h).astype(np.float32)
        A = out_affine.astype(np.float64)
        out_K = K32.copy()
        for i in range(2):
            for j in range(3):
                out_K[:, i, j] = ((A[:, i, 0] * K[:, 0, j] + A[:, i, 1] * K[:, 1, j]) + A[:, i, 2] * K[:, 2, j]).astype(np.float32)
        pix = (scale / out_w).astype(np.float32)
    centre, scale = np.where(bad[:, None], np.nan, centre), np.where(bad, np.nan, scale)
    in_affine[bad], out_affine[bad], out_K[bad], pix[bad] = _NAN32, _NAN32, _NAN32, _NAN32
    step_id = (_aug.key(seed, ids, _aug.OP_ZOOM, OP_STEP_INDEX) & np.uint64(0x7FFFFFFF)).astype(np.int32)
    return ZoomGeometry(in_affine, out_affine, out_K, pix, step_id, np.where(bad, -1, 0).astype(np.int32), centre, scale,
                        np.asarray(rot, dtype=np.float64), np.stack((c, s), axis=1))


def background_geometry_host(seed, sample_ids, bg_hw, out_hw):
    """`augment.background_matrices`, which is the definition: (G,2,3) float32."""
    return _aug.background_matrices(seed, sample_ids, bg_hw, out_hw)


# ---- the device --------------------------------------------------------------------------------------------------------------------
_SO = _lib.SideLibrary(_build.GEOMETRY, {
    "lc_geometry_zoom_f32": (c_int, [c_double] * 4 + [c_int] * 7 + [c_void_p] * 4 + [c_int] * 2 + [c_void_p] * 10),
    "lc_geometry_background_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("geometry")  # its whole numbers may be numpy's: sizes come out of shapes and arrays here


def _rows(sample_id):
    """sample_id (B,) int32 on the device: the first tensor of both calls, which says where the launch runs."""
    sample_id = _A.tensor("sample_id", sample_id, (torch.int32,), "int32", (None,))
    return sample_id, int(sample_id.shape[0])


def _seed_arg(seed):
    """`augment._seed_word`'s rule on the seed's type, ahead of the device: a whole number below 2^64, or one 64-bit element."""
    if not isinstance(seed, Tensor):
        _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    elif seed.dtype not in (torch.uint64, torch.int64) or seed.numel() != 1:
        raise TypeError(f"lc_amd.geometry: a seed tensor holds one uint64 or int64 element, got {seed.dtype} of shape {tuple(seed.shape)}")


def _on_device(sample_id):
    if not sample_id.is_cuda:
        raise RuntimeError(f"lc_amd.geometry: sample_id is on {sample_id.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    return sample_id.device


@torch.no_grad()
def zoom_geometry(cfg: AugmentConfig, *, seed, sample_id, bbox_xyxy, im_hw, cam_K, in_wh, out_wh, train=True, want_info=False) -> ZoomGeometry:
    """`zoom_geometry_host(cfg, seed, sample_id, bbox_xyxy, im_hw, cam_K, in_wh, out_wh, train)` as device tensors, bit for bit, in one
    launch (`lc_geometry_zoom_f32` of include/lc_amd_geometry.h).

    seed: a whole number below 2^64, or a device tensor of one uint64 / int64 element that the KERNEL reads (`augment.augment_drawn`'s
    rule: the same word serves both).  sample_id (B,) int32, bbox_xyxy (B,4) float32 and cam_K (B,3,3) or (3,3) float32 on the device;
    im_hw = (H, W) of the frames, in_wh and out_wh = (w, h) of the network's input and output, whole numbers of 1 to MAX_SIZE.
    `want_info` adds `centre`, `scale` and `cs` (fp64); `rot` is always None.  A refused row (a non-finite box or K entry, a scale that
    is not finite or <= 0) has info = -1 and NaN in every float output; nothing is read back to find out."""
    if not isinstance(cfg, AugmentConfig):
        raise TypeError(f"lc_amd.geometry: cfg must be an AugmentConfig, got {type(cfg)}")
    ratios = [float(getattr(cfg, name)) for name in ("dzi_scale_ratio", "dzi_shift_ratio", "dzi_pad_scale")]
    for name, v in zip(("dzi_scale_ratio", "dzi_shift_ratio", "dzi_pad_scale"), ratios):
        if not math.isfinite(v):
            raise ValueError(f"lc_amd.geometry: {name} must be finite, got {v}")
    rotate_prob = float(cfg.rotate_prob)
    if not 0.0 <= rotate_prob <= 1.0:
        raise ValueError(f"lc_amd.geometry: rotate_prob must lie in [0, 1], got {cfg.rotate_prob}")
    if not isinstance(train, bool) or not isinstance(want_info, bool):
        raise TypeError(f"lc_amd.geometry: train and want_info are bools, got {type(train)} and {type(want_info)}")
    sample_id, B = _rows(sample_id)
    bbox_xyxy = _A.f32("bbox_xyxy", bbox_xyxy, (B, 4))
    one_camera = isinstance(cam_K, Tensor) and tuple(cam_K.shape) == (3, 3)
    cam_K = _A.f32("cam_K", cam_K, (3, 3) if one_camera else (B, 3, 3))
    im_h, im_w = _A.size_pair("im_hw", im_hw, MAX_SIZE, numpy=True)
    in_w, in_h = _A.size_pair("in_wh", in_wh, MAX_SIZE, numpy=True)
    out_w, out_h = _A.size_pair("out_wh", out_wh, MAX_SIZE, numpy=True)
    _seed_arg(seed)
    dev = _on_device(sample_id)
    _A.same_device(dev, "sample_id on {}", bbox_xyxy=bbox_xyxy, cam_K=cam_K)
    word = _aug._seed_word(seed, dev)
    sid, box, K = sample_id.contiguous(), bbox_xyxy.contiguous(), cam_K.contiguous()

    def made(shape, dtype):
        return torch.empty(shape, device=dev, dtype=dtype)

    in_affine, out_affine, out_K = made((B, 2, 3), torch.float32), made((B, 2, 3), torch.float32), made((B, 3, 3), torch.float32)
    pix, step_id, info = made((B,), torch.float32), made((B,), torch.int32), made((B,), torch.int32)
    centre, scale, cs = (made((B, 2), torch.float64), made((B,), torch.float64), made((B, 2), torch.float64)) if want_info else (None, None, None)
    if B:
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_geometry_zoom_f32(*ratios, rotate_prob, int(train), im_h, im_w, in_w, in_h, out_w, out_h, _lib.ptr(word), _lib.ptr(sid), _lib.ptr(box),
                                          _lib.ptr(K), 0 if one_camera else 9, B, _lib.ptr(in_affine), _lib.ptr(out_affine), _lib.ptr(out_K), _lib.ptr(pix),
                                          _lib.ptr(step_id), _lib.ptr(info), _lib.ptr(centre), _lib.ptr(scale), _lib.ptr(cs), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("geometry.zoom_geometry", rc)
    return ZoomGeometry(in_affine, out_affine, out_K, pix, step_id, info, centre, scale, None, cs)


@torch.no_grad()
def background_geometry(*, seed, sample_id, bg_hw, out_hw) -> Tensor:
    """`augment.background_matrices(seed, sample_id, bg_hw, out_hw)` as a (B,2,3) float32 device tensor, bit for bit, in one launch
    (`lc_geometry_background_f32`): the matrix `crops.warp_affine` takes to cut row b's region out of its background.

    seed as `zoom_geometry`'s; sample_id (B,) int32 on the device; bg_hw = (Hb, Wb), one pair of whole numbers of 1 to MAX_SIZE for
    all rows, or a (B,2) int32 device tensor, one pair per sample (any values: no row is refused); out_hw = (H, W) of the crop."""
    sample_id, B = _rows(sample_id)
    per_row = isinstance(bg_hw, Tensor)
    if per_row:
        bg_hw = _A.tensor("bg_hw", bg_hw, (torch.int32,), "int32", (B, 2))
        hb = wb = 0
    else:
        hb, wb = _A.size_pair("bg_hw", bg_hw, MAX_SIZE, numpy=True)
    H, W = _A.size_pair("out_hw", out_hw, MAX_SIZE, numpy=True)
    _seed_arg(seed)
    dev = _on_device(sample_id)
    if per_row:
        _A.same_device(dev, "sample_id on {}", bg_hw=bg_hw)
    word = _aug._seed_word(seed, dev)
    sid = sample_id.contiguous()
    pairs = bg_hw.contiguous() if per_row else None
    M = torch.empty((B, 2, 3), device=dev, dtype=torch.float32)
    if B:
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_geometry_background_f32(_lib.ptr(word), _lib.ptr(sid), hb, wb, _lib.ptr(pairs), H, W, B, _lib.ptr(M), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("geometry.background_geometry", rc)
    return M
