"""Zoom-in crops on the device: exact integer affine warps of uint8 frames (lc_amd/csrc/crop/lc_crop.hip, lc_amd/_C/liblc_amd_crop.so,
C ABI and the exact definition of the result in include/lc_amd_crop.h).

    warp_affine(frames, M, out_hw, *, frame_index=None, interp="linear", normalize=None, dtype=torch.float32, out=None, info=None)
    affine_from_box(center, scale, rot_rad, out_wh) -> (M, M_inv)
    test_item(dataset, index) -> blob        the non-training branch of the reference's loader without its warp
    finish_blob(blob) -> blob                the warp, on the device, after the transfer

What the reference's loader does per instance on the host (`dataset.py:409-411`: `cv2.warpAffine(rgb, in_affine, net_input_wh)`, then
`.to(float32).div(255)`, then `transforms.Normalize` in `test.py:163`): a frame is uploaded once as uint8 and every crop of it is cut on
the device, in OpenCV's published fixed-point scheme for 8-bit images (coordinates on a 1/1024 px grid, bilinear weights on a 1/32 px
grid, constant border 0).  That scheme is integer arithmetic, so the crop is defined bit for bit; tests/crops_oracle.py restates it.

HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device, needs no
workspace and can be captured into a graph.
"""
from __future__ import annotations

import ctypes
import logging
import math
from ctypes import c_int, c_void_p
from operator import itemgetter

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

logger = logging.getLogger(__name__)

MAX_SIZE = 16384  # LC_CROP_MAX_SIZE
INTERP = {"nearest": 0, "linear": 1}  # LC_CROP_NEAREST / LC_CROP_LINEAR
OUT_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}  # LC_CROP_U8 / _F32 / _F16 / _BF16

_FLOATS = ctypes.POINTER(ctypes.c_float)
_SO = _lib.SideLibrary(_build.CROP, {
    "lc_crop_warp_u8": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_void_p] + [c_int] * 5 + [_FLOATS, _FLOATS, c_void_p, c_void_p, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("crops")


def _require(name, t, dtype, what):
    if not isinstance(t, Tensor):
        raise TypeError(f"lc_amd.crops: {name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"lc_amd.crops: {name} is on {t.device}; the HIP path needs tensors on the MI355X "
                           f"(there is no CPU fallback in the product path)")
    if t.dtype != dtype:
        raise TypeError(f"lc_amd.crops: {name} must be {what}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"lc_amd.crops: {name} must be contiguous, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    return t


@torch.no_grad()
def warp_affine(frames, M, out_hw, *, frame_index=None, interp="linear", normalize=None, dtype=torch.float32, out=None, info=None):
    """out (B,C,h,w) of `dtype`: crop b is `cv2.warpAffine(frames[frame_index[b]], M[b], (w, h), flags=interp)` in the fixed-point
    scheme, as bytes (torch.uint8) or as `bytes / 255` (float32 / float16 / bfloat16), with `normalize = (mean[C], std[C])` as
    `(bytes / 255 - mean) / std` -- `transforms.Normalize`'s order, computed in fp32 and rounded once.

    frames (F,H,W,C) uint8 with C in {1, 3}; M (B,2,3) float32, the FORWARD matrix (source -> crop); frame_index (B) int32 or None
    (row b reads frame b).  mean / std are host values (sequences, or tensors that are read back here, once); they travel as kernel
    arguments.  A row whose M has a non-finite entry, or whose frame index lies outside [0, F), is written as all border and gets
    `info[b] = -1` (0 otherwise).  The call returns `out`; pass an `info` tensor to read the rows' states."""
    frames = _require("frames", frames, torch.uint8, "uint8")
    M = _require("M", M, torch.float32, "float32")
    if frames.dim() != 4 or frames.shape[3] not in (1, 3):
        raise ValueError(f"lc_amd.crops: frames must be (F,H,W,C) with C in (1, 3), got {tuple(frames.shape)}")
    if M.dim() != 3 or tuple(M.shape[1:]) != (2, 3):
        raise ValueError(f"lc_amd.crops: M must be (B,2,3), got {tuple(M.shape)}")
    F, H, W, C = (int(s) for s in frames.shape)
    B, h, w = int(M.shape[0]), int(out_hw[0]), int(out_hw[1])
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE and 1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f"lc_amd.crops: frame and crop sizes of 1 to {MAX_SIZE}, got {H} x {W} -> {h} x {w}")
    if interp not in INTERP:
        raise ValueError(f"lc_amd.crops: interp must be one of {sorted(INTERP)}, got {interp!r}")
    if dtype not in OUT_DTYPES:
        raise TypeError(f"lc_amd.crops: dtype must be one of uint8, float32, float16, bfloat16, got {dtype}")
    dev = frames.device
    if frame_index is not None:
        frame_index = _require("frame_index", frame_index, torch.int32, "int32")
        if tuple(frame_index.shape) != (B,):
            raise ValueError(f"lc_amd.crops: frame_index must be ({B},), got {tuple(frame_index.shape)}")
    mean = std = None
    if normalize is not None:
        if dtype == torch.uint8:
            raise TypeError("lc_amd.crops: normalize needs a float dtype")
        mean, std = _A.host_floats("mean", normalize[0], C), _A.host_floats("std", normalize[1], C)
    if out is None:
        out = torch.empty(B, C, h, w, device=dev, dtype=dtype)
    else:
        out = _require("out", out, dtype, str(dtype))
        if tuple(out.shape) != (B, C, h, w):
            raise ValueError(f"lc_amd.crops: out must be {(B, C, h, w)}, got {tuple(out.shape)}")
    if info is None:
        info = torch.empty(B, device=dev, dtype=torch.int32)
    else:
        info = _require("info", info, torch.int32, "int32")
        if tuple(info.shape) != (B,):
            raise ValueError(f"lc_amd.crops: info must be ({B},), got {tuple(info.shape)}")
    _A.same_device(dev, "the frames on {}", M=M, frame_index=frame_index, out=out, info=info)
    lib = load()
    with _lib.on_device(dev):
        rc = lib.lc_crop_warp_u8(_lib.ptr(frames), F, H, W, C, _lib.ptr(frame_index), _lib.ptr(M), B, h, w, INTERP[interp], OUT_DTYPES[dtype],
                                 mean, std, _lib.ptr(out), _lib.ptr(info), _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("crops.warp_affine", rc)
    return out


def affine_from_box(center, scale, rot_rad, out_wh):
    """(M, M_inv) as (2,3) float32: the closed form of the reference's `_get_affine_transform` (`dataset.py:61-108`, shift = 0), in
    fp64 on the host.  Its three point pairs define a similarity: k = dst_w / src_w with src_w = scale[0], a rotation by -rot_rad,
    and the translation that takes `center` to the centre of the output; M_inv is its exact inverse, rounded on its own."""
    cx, cy = (float(v) for v in np.asarray(center, dtype=np.float64).reshape(2))
    src_w = float(np.asarray(scale, dtype=np.float64).reshape(-1)[0])
    if isinstance(out_wh, (int, float)):
        out_wh = (out_wh, out_wh)
    dst_w, dst_h = float(out_wh[0]), float(out_wh[1])
    c, s = math.cos(rot_rad), math.sin(rot_rad)
    k, ki = dst_w / src_w, src_w / dst_w
    dx, dy = dst_w * 0.5, dst_h * 0.5
    M = np.array([[k * c, k * s, dx - (k * c * cx + k * s * cy)],
                  [-k * s, k * c, dy - (-k * s * cx + k * c * cy)]], dtype=np.float64)
    Mi = np.array([[ki * c, -ki * s, cx - (ki * c * dx - ki * s * dy)],
                   [ki * s, ki * c, cy - (ki * s * dx + ki * c * dy)]], dtype=np.float64)
    return M.astype(np.float32), Mi.astype(np.float32)


def _read_rgb(path):
    """(H,W,3) uint8 of an image file, as `imageio.v2.imread(path, pilmode="RGB")` gives it (which decodes with Pillow)."""
    try:
        import imageio.v2 as iio

        return np.asarray(iio.imread(path, as_gray=False, pilmode="RGB"))
    except ImportError:
        from PIL import Image

        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))


def test_item(dataset, index):
    """The non-training branch of the reference's `BOP_Dataset._get_single_item` (`dataset.py:367-491`) restated without OpenCV: the
    same blob, with the same keys, values and dtypes, except that `rgb_full` (H,W,3) uint8 -- the frame as decoded -- and `in_affine`
    (2,3) float32 stand in for `rgb_in`; `finish_blob` cuts the crop on the device.  Only attributes the reference's dataset object
    has are used.  `in_affine` and `out_K` come from the closed form of `affine_from_box`: they equal the reference's bit for bit where
    the box is exact in fp32 and its three-point solve leaves no rounding noise, and lie within the fp32 rounding of its staged points
    (a few ulp) otherwise; every other value is the reference's bit for bit.  `mask_visib` is not decoded (the test branch replaces it by zeros and none of its warps reaches the blob), and no
    random number is drawn, as in the reference's test branch."""
    cfg = dataset.cfg
    im_info, inst_info = dataset.np_annots[index]
    rgb = _read_rgb(im_info["rgb"])
    cam_K = im_info["cam_K"]
    obj_id = inst_info["obj_id"]
    m_info = dataset.model_info[obj_id]
    bbox_xywh = inst_info["bbox_visib"]
    if "bbox_det" in inst_info:
        bbox_xywh = inst_info["bbox_det"]
    else:
        logger.warning("using ground truth bounding box when testing")
    bbox_xyxy = np.concatenate((bbox_xywh[:2], bbox_xywh[:2] + bbox_xywh[2:]), axis=-1)
    bbox_center, scale = (bbox_xyxy[:2] + bbox_xyxy[2:]) * 0.5, float(max(bbox_xywh[2], bbox_xywh[3], 1)) * cfg.dzi_pad_scale
    net_output_wh, net_input_wh = dataset.net_output_wh, dataset.net_input_wh
    # the reference stages the scale and its three points in fp32 (dataset.py:74,95-103): centre and scale are rounded likewise first,
    # which leaves only the fp32 rounding of its second and third point between the two matrices
    box32 = np.asarray(bbox_center, dtype=np.float32), np.float32(scale)
    out_affine, _ = affine_from_box(*box32, 0, net_output_wh)
    in_affine, _ = affine_from_box(*box32, 0, net_input_wh)
    affine33 = np.eye(3, dtype=np.float32)
    affine33[:2] = out_affine
    out_K = affine33 @ cam_K
    noc_scale_xfd, noc_scale_ori, model_transform = itemgetter("noc_scale_xfd", "noc_scale_ori", "xform")(m_info)
    blob = {
        "rgb_full": np.array(rgb, dtype=np.uint8),  # a writable copy: collation turns it into a tensor
        "in_affine": in_affine,
        "noc_scale": noc_scale_xfd,
        "noc_scale_ori": noc_scale_ori,
        "out_pix_scale": scale / net_output_wh[0],
        "out_K": out_K,
        "obj_id": obj_id,
        "im_id": im_info["im_id"],
        "scene_id": im_info["scene_id"],
    }
    if dataset.sparse_cnt > 0:
        blob["pts3d"] = dataset.fps[obj_id][:dataset.sparse_cnt]
    if dataset.transform_model:
        blob["model_transform"] = model_transform
    return blob


test_item.__test__ = False  # a public name that starts with "test_": never a test, wherever a test module imports it

_NET_INPUT_HW = None


def set_net_input_hw(hw):
    """The crop size `finish_blob` cuts when it is not told one: (h, w) of the network's input (the reference's `net_input_wh`, reversed)."""
    global _NET_INPUT_HW
    _NET_INPUT_HW = None if hw is None else (int(hw[0]), int(hw[1]))


def finish_blob(blob, net_input_hw=None):
    """The device half of `test_item`: a batch that holds `rgb_full` (B,H,W,3) uint8 and `in_affine` (B,2,3) float32 on the device
    gets `rgb_in = warp_affine(rgb_full, in_affine, net_input_hw)` -- float32, (B,3,h,w), unnormalised, what the reference's loader
    delivers, so that `test.py:163` goes on normalising it itself -- and loses the two stand-in keys.  Anything else (a batch of the
    reference's own loader, a non-mapping) passes through untouched."""
    if not isinstance(blob, dict) or "rgb_full" not in blob or "in_affine" not in blob:
        return blob
    hw = net_input_hw if net_input_hw is not None else _NET_INPUT_HW
    if hw is None:
        raise RuntimeError("lc_amd.crops: finish_blob needs the size of the network's input (net_input_hw=, or set_net_input_hw)")
    frames, M = blob["rgb_full"], blob["in_affine"]
    if frames.dim() == 3:  # one item, not collated
        frames, M = frames[None], M[None]
    out = dict(blob)
    del out["rgb_full"], out["in_affine"]
    out["rgb_in"] = warp_affine(frames, M.float().contiguous(), hw)
    return out
