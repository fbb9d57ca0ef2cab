"""Training-time background switch and colour augmentation on the device (lc_amd/csrc/augment/lc_augment.hip,
lc_amd/_C/liblc_amd_augment.so; C ABI and the exact definition of every output in include/lc_amd_augment.h): what the reference's loader
does per instance on a host core with the warped crop (`dataset.py:137-148,413-419`: `_switch_bg`, `np.round`, the imgaug chain of
`_gen_color_aug`) and the dynamic zoom-in box draw (`_aug_bbox`, `dataset.py:313-327,402`).

    AugmentConfig(pixel_aug_prob, switch_bg_prob, use_peper_salt, use_motion_blur, use_invert, ...)
    draw(cfg, seed, sample_ids, n_backgrounds, hw=(256, 256)) -> params (B,64) int32, lut (B,3,256) uint8      host numpy, no device
    augment(crops, params, lut, *, msk_in=None, backgrounds=None, seed=0, sample_id=None, dtype=torch.float32, normalize=None,
            pointwise=None) -> (out, info)
    augment_drawn(crops, cfg, *, seed, sample_id, msk_in=None, backgrounds=None, dtype=torch.float32, normalize=None,
                  return_rows=False) -> (out, info[, params, lut])      the same launch with its rows drawn by the kernel
    background_matrices(seed, sample_ids, bg_hw, out_hw) -> (B,2,3) float32 for `crops.warp_affine`
    draw_zoom(cfg, seed, sample_ids, bbox_xyxy, im_hw) -> centre (B,2), scale (B,), rotation (B,) for `crops.affine_from_box`

The host draws the few numbers per sample; ONE launch does everything that touches pixels.  Every random number is
`u(op, i) = (key(op, i) >> 8) / 2**24` with the key of include/lc_amd_augment.h -- a stated integer hash of (seed, sample_id, op, i) in
place of imgaug's and numpy's streams -- so a sample's row is the same in any batch and order.  The filters are Q16 integer 5x5 kernels
with OpenCV's BORDER_REFLECT_101, the point operations one 256-entry table per channel: every output is defined bit for bit
(tests/augment_oracle.py restates it).  What differs from imgaug and OpenCV on purpose is listed in DESIGN.md, section 7.

HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device, needs no
workspace and -- with `params` and `lut` already on the device -- allocates its outputs only and can be captured into a graph.
`augment_drawn` needs no `draw` on the host at all: the kernel forms each sample's row from (cfg, a seed word on the device, sample_id), so
a captured graph draws anew at every replay once that word has changed.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_double, c_int, c_uint64, c_void_p
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

MIN_SIZE = 8        # LC_AUGMENT_MIN_SIZE
MAX_SIZE = 16384    # LC_AUGMENT_MAX_SIZE
WORDS = 64          # LC_AUGMENT_WORDS
OUT_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}  # LC_AUGMENT_U8 / _F32 / _F16 / _BF16
FORMS = {"filtered": 0, "pointwise": 1}  # LC_AUGMENT_FILTERED / _POINTWISE
OP_SNP, OP_SNPV, OP_DROP = 65537, 65538, 65539  # LC_AUGMENT_OP_*: the device's own draws
OP_HOST = 131072    # LC_AUGMENT_OP_HOST: the host's draws start here
# one op code per decision of the host; the index i of u(op, i) tells the draws of one decision apart
OP_SWITCH = OP_HOST + 1     # 0: gate, 1: the background
OP_CHAIN = OP_HOST + 2      # 0: the gate of the whole colour chain
OP_SALT = OP_HOST + 3       # 0: gate
OP_MOTION = OP_HOST + 4     # 0: gate, 1: angle, 2: direction
OP_DROPOUT = OP_HOST + 5    # 0: gate
OP_GAUSS = OP_HOST + 6      # 0: gate, 1: sigma
OP_ADD = OP_HOST + 7        # 0: gate, 1: per channel?, 2..4: the values
OP_INVERT = OP_HOST + 8     # 0: gate, 1..3: the channels
OP_MUL_PC = OP_HOST + 9     # 0: gate, 1: per channel?, 2..4: the factors
OP_MUL = OP_HOST + 10       # 0: gate, 1: the factor
OP_CONTRAST = OP_HOST + 11  # 0: gate, 1: per channel?, 2..4: alpha
OP_BG_REGION = OP_HOST + 12  # 0..3: width, height, left, top
OP_ZOOM = OP_HOST + 13      # 0: scale, 1..2: shift, 3: rotation gate, 4: angle

BIT_SWITCH, BIT_SALT, BIT_MOTION, BIT_DROPOUT, BIT_GAUSS, BIT_LUT = 1, 2, 4, 8, 16, 32
SALT_P = 0.05       # iaa.SaltAndPepper(0.05)
DROPOUT_P = 0.1     # iaa.CoarseDropout(p=0.1, size_percent=0.05)
DROPOUT_PERCENT = 5

_M32 = np.uint64(0xFFFFFFFF)
_FLOATS = ctypes.POINTER(ctypes.c_float)


@dataclass(frozen=True)
class AugmentConfig:
    """What the reference reads from its config (`dataset.py:151-171,321-326,402,413,416`).  The three switches default as
    `_gen_color_aug` reads them (`cfg.get(..., False)`); the probabilities and ratios have no default there and take the values of the
    reference's configs/glmo.yaml."""
    pixel_aug_prob: float = 0.8
    switch_bg_prob: float = 0.5
    use_peper_salt: bool = False
    use_motion_blur: bool = False
    use_invert: bool = False
    dzi_scale_ratio: float = 0.25
    dzi_shift_ratio: float = 0.25
    dzi_pad_scale: float = 1.5
    rotate_prob: float = 1.0


def _fmix32(v):
    v = np.asarray(v, dtype=np.uint64) & _M32
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & _M32
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & _M32
    return v ^ (v >> np.uint64(16))


def key(seed, sample_ids, op, q):
    """key(op, q) of include/lc_amd_augment.h for every sample of `sample_ids` (broadcast against q), as uint64 holding 32 bits."""
    seed = int(seed)
    k = _fmix32(seed & 0xFFFFFFFF)
    k = _fmix32(k ^ np.uint64(seed >> 32))
    k = _fmix32(k ^ (np.asarray(sample_ids, dtype=np.int64).astype(np.uint64) & _M32))
    k = _fmix32(k ^ np.uint64(op))
    return _fmix32(k ^ (np.asarray(q, dtype=np.int64).astype(np.uint64) & _M32))


def u(seed, sample_ids, op, i):
    """The uniform number in [0, 1) behind every host decision: (key(op, i) >> 8) / 2**24, exact in fp64."""
    return (key(seed, sample_ids, op, i) >> np.uint64(8)).astype(np.float64) / float(1 << 24)


def _quantise(g):
    """25 non-negative fp64 weights that sum to 1 -> Q16 integers that sum to exactly 65536 (the remainder goes to the centre)."""
    q = np.floor(np.asarray(g, dtype=np.float64).reshape(25) * 65536.0 + 0.5).astype(np.int64)
    q[12] += 65536 - int(q.sum())
    return q


def gaussian_weights(sigma):
    """The 5x5 Q16 kernel of a Gaussian blur: g_i = exp(-i^2 / 2 sigma^2), i = -2..2, normalised in fp64, the outer product quantised."""
    i = np.arange(-2, 3, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    g = g / g.sum()
    return _quantise(np.outer(g, g))


def motion_weights(angle_deg, direction):
    """The 5x5 Q16 kernel of a motion blur: five line taps at s = -2..2 along (sin t, -cos t) from the centre, weighted linearly from
    (1 - d) / 2 to (1 + d) / 2 along the line, each splatted bilinearly into the grid, normalised in fp64 and quantised."""
    t = math.radians(float(angle_deg))
    d = float(direction)
    grid = np.zeros((5, 5), dtype=np.float64)
    for s in range(-2, 3):
        wgt = (1.0 - d) / 2.0 + (s + 2) / 4.0 * d
        px, py = 2.0 + s * math.sin(t), 2.0 - s * math.cos(t)
        x0, y0 = min(max(int(math.floor(px)), 0), 4), min(max(int(math.floor(py)), 0), 4)
        fx, fy = px - x0, py - y0
        for yy, wy in ((y0, 1.0 - fy), (y0 + 1, fy)):
            for xx, wx in ((x0, 1.0 - fx), (x0 + 1, fx)):
                if yy <= 4 and xx <= 4:
                    grid[yy, xx] += wgt * wy * wx
    return _quantise(grid / grid.sum())


def _step(table, fn):
    return np.clip(np.rint(fn(table.astype(np.float64))), 0, 255).astype(np.int64)


def draw(cfg: AugmentConfig, seed, sample_ids, n_backgrounds, hw=(256, 256)):
    """params (B,64) int32 and lut (B,3,256) uint8 of include/lc_amd_augment.h for the samples `sample_ids`, in host numpy.  The gates
    are nested as in the reference: the switch by `switch_bg_prob` (never without backgrounds), the whole colour chain by
    `pixel_aug_prob`, each augmenter by its own `Sometimes` probability (`dataset.py:153-170`).  A row depends on (cfg, seed, its
    sample id, n_backgrounds, hw) alone.  `hw` sizes the dropout grid (5 % of the crop, at least one cell)."""
    seed = _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    n_backgrounds = _A.whole("n_backgrounds", n_backgrounds, 0, 2 ** 31 - 1, numpy=True)
    h, w = _A.whole("hw", hw[0], MIN_SIZE, MAX_SIZE, numpy=True), _A.whole("hw", hw[1], MIN_SIZE, MAX_SIZE, numpy=True)
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    B = len(ids)
    params = np.zeros((B, WORDS), dtype=np.int32)
    lut = np.tile(np.arange(256, dtype=np.uint8), (B, 3, 1))

    def uu(op, i):
        return u(seed, ids, op, i)

    switch = (uu(OP_SWITCH, 0) < cfg.switch_bg_prob) & (n_backgrounds > 0)
    which = np.minimum((uu(OP_SWITCH, 1) * n_backgrounds).astype(np.int64), max(n_backgrounds - 1, 0))
    chain = uu(OP_CHAIN, 0) < cfg.pixel_aug_prob
    salt = chain & bool(cfg.use_peper_salt) & (uu(OP_SALT, 0) < 0.3)
    motion = chain & bool(cfg.use_motion_blur) & (uu(OP_MOTION, 0) < 0.2)
    dropout = chain & (uu(OP_DROPOUT, 0) < 0.5)
    sigma = 1.2 * uu(OP_GAUSS, 1)
    gauss = chain & (uu(OP_GAUSS, 0) < 0.5) & (sigma >= 1e-3)
    add = chain & (uu(OP_ADD, 0) < 0.5)
    invert = chain & bool(cfg.use_invert) & (uu(OP_INVERT, 0) < 0.4)
    mul_pc = chain & (uu(OP_MUL_PC, 0) < 0.5)
    mul = chain & (uu(OP_MUL, 0) < 0.5)
    contrast = chain & (uu(OP_CONTRAST, 0) < 0.5)
    angle, direction = 360.0 * uu(OP_MOTION, 1), 2.0 * uu(OP_MOTION, 2) - 1.0

    def per_channel(op, prob):
        """(B,3) draws: one per channel where the row's per-channel draw says so, else the first for all three"""
        own = uu(op, 1) < prob
        vals = np.stack([uu(op, 2 + c) for c in range(3)], axis=1)
        return np.where(own[:, None], vals, vals[:, :1])

    add_v = np.minimum(-25 + np.floor(per_channel(OP_ADD, 0.3) * 51.0), 25.0)
    inv_c = np.stack([uu(OP_INVERT, 1 + c) < 0.2 for c in range(3)], axis=1)
    mul_pc_v = 0.6 + 0.8 * per_channel(OP_MUL_PC, 0.5)
    mul_v = 0.6 + 0.8 * uu(OP_MUL, 1)
    alpha = 0.5 + 1.7 * per_channel(OP_CONTRAST, 0.3)

    for b in range(B):
        bits = 0
        if switch[b]:
            bits |= BIT_SWITCH
            params[b, 1] = which[b]
        if salt[b]:
            bits |= BIT_SALT
            params[b, 2] = int(math.floor(SALT_P * 2.0 ** 32))
        if motion[b]:
            bits |= BIT_MOTION
            params[b, 6:31] = motion_weights(angle[b], direction[b])
        if dropout[b]:
            bits |= BIT_DROPOUT
            params[b, 3] = int(math.floor(DROPOUT_P * 2.0 ** 32))
            params[b, 4], params[b, 5] = max(1, h * DROPOUT_PERCENT // 100), max(1, w * DROPOUT_PERCENT // 100)
        if gauss[b]:
            bits |= BIT_GAUSS
            params[b, 31:56] = gaussian_weights(sigma[b])
        if add[b] or invert[b] or mul_pc[b] or mul[b] or contrast[b]:
            bits |= BIT_LUT
            for c in range(3):
                t = np.arange(256, dtype=np.int64)
                if add[b]:
                    t = _step(t, lambda v: v + add_v[b, c])
                if invert[b] and inv_c[b, c]:
                    t = _step(t, lambda v: 255.0 - v)
                if mul_pc[b]:
                    t = _step(t, lambda v: v * mul_pc_v[b, c])
                if mul[b]:
                    t = _step(t, lambda v: v * mul_v[b])
                if contrast[b]:
                    t = _step(t, lambda v: 128.0 + alpha[b, c] * (v - 128.0))
                lut[b, c] = t.astype(np.uint8)
        params[b, 0] = bits
    return params, lut


def background_matrices(seed, sample_ids, bg_hw, out_hw):
    """(B,2,3) float32 forward matrices (background image -> crop) for `crops.warp_affine`: the region of `_switch_bg`
    (`dataset.py:142-146`) drawn from u(OP_BG_REGION, 0..3) -- width, height, left, top, with the slice's right end `l + l + w` as the
    reference writes it, both ends clipped to the image as slicing does -- stretched over the crop in `cv2.resize`'s pixel-centre
    convention (source x = (crop x + 1/2) region_w / W - 1/2 + left).  bg_hw = (Hb, Wb), one pair or one per sample; out_hw = (H, W)."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    hb, wb = (a.astype(np.int64) for a in np.broadcast_to(np.asarray(bg_hw, dtype=np.int64), (len(ids), 2)).T)
    H, W = int(out_hw[0]), int(out_hw[1])
    r = [u(seed, ids, OP_BG_REGION, i) for i in range(4)]
    roi_w = np.maximum(np.trunc(r[0] * wb).astype(np.int64), W)
    roi_h = np.maximum(np.trunc(r[1] * hb).astype(np.int64), H)
    left = np.maximum(np.trunc(r[2] * (wb - roi_w)).astype(np.int64), 0)
    top = np.maximum(np.trunc(r[3] * (hb - roi_h)).astype(np.int64), 0)
    left, top = np.minimum(left, wb), np.minimum(top, hb)
    rw = np.maximum(np.minimum(left + left + roi_w, wb) - left, 1).astype(np.float64)
    rh = np.maximum(np.minimum(top + roi_h, hb) - top, 1).astype(np.float64)
    M = np.zeros((len(ids), 2, 3), dtype=np.float64)
    M[:, 0, 0], M[:, 1, 1] = W / rw, H / rh
    M[:, 0, 2] = (0.5 - left) * (W / rw) - 0.5
    M[:, 1, 2] = (0.5 - top) * (H / rh) - 0.5
    return M.astype(np.float32)


def draw_zoom(cfg: AugmentConfig, seed, sample_ids, bbox_xyxy, im_hw):
    """(centre (B,2), scale (B,), rotation (B,) in radians) in fp64, ready for `crops.affine_from_box`: `_aug_bbox`
    (`dataset.py:313-327`) and the rotation of `dataset.py:402` with u(OP_ZOOM, 0..4) in the place of np.random."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    box = np.asarray(bbox_xyxy, dtype=np.float64).reshape(len(ids), 4)
    x1, y1, x2, y2 = box.T
    im_h, im_w = int(im_hw[0]), int(im_hw[1])
    r = [u(seed, ids, OP_ZOOM, i) for i in range(5)]
    cx, cy, bh, bw = 0.5 * (x1 + x2), 0.5 * (y1 + y2), y2 - y1, x2 - x1
    scale_ratio = 1 + cfg.dzi_scale_ratio * (2 * r[0] - 1)
    centre = np.stack((cx + bw * (cfg.dzi_shift_ratio * (2 * r[1] - 1)), cy + bh * (cfg.dzi_shift_ratio * (2 * r[2] - 1))), axis=1)
    scale = np.maximum(bh, bw) * scale_ratio * cfg.dzi_pad_scale
    scale = np.minimum(scale, max(im_h, im_w)) * 1.0
    rot = np.where(r[3] < cfg.rotate_prob, r[4] * 4 * math.pi, 0.0)
    return centre, scale, rot


class DrawConfig(ctypes.Structure):
    """lc_augment_draw_config, by value: what `draw` reads of an AugmentConfig, and the number of backgrounds a row may name."""
    _fields_ = [("pixel_aug_prob", c_double), ("switch_bg_prob", c_double), ("use_peper_salt", c_int), ("use_motion_blur", c_int),
                ("use_invert", c_int), ("n_backgrounds", c_int)]


_SO = _lib.SideLibrary(_build.AUGMENT, {
    "lc_augment_u8": (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 3 + [c_int] * 3 + [c_uint64, c_void_p, c_int, c_int, _FLOATS, _FLOATS] + [c_void_p] * 3),
    "lc_augment_drawn_u8": (c_int, [c_void_p, c_void_p, c_int, c_void_p, DrawConfig, c_void_p, c_void_p] + [c_int] * 4 + [_FLOATS, _FLOATS] + [c_void_p] * 5),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("augment")  # its whole numbers may be numpy's (`whole(..., numpy=True)`): seeds and sizes come out of arrays here


def check_params(params, h, w, n_backgrounds, has_mask):
    """The row rules of include/lc_amd_augment.h on a HOST (B,64) int32 array: raises ValueError naming the first row the kernel would
    refuse.  -> True where some row uses a 5x5 filter."""
    P = np.asarray(params)
    for b, row in enumerate(P.astype(np.int64)):
        bits = int(row[0])
        if bits & ~63:
            raise ValueError(f"lc_amd.augment: params row {b} sets bits above bit 5 ({bits:#x})")
        if row[56:].any():
            raise ValueError(f"lc_amd.augment: params row {b} has a non-zero reserved word")
        for bit, lo, name in ((BIT_MOTION, 6, "A"), (BIT_GAUSS, 31, "B")):
            wq = row[lo:lo + 25]
            if bits & bit and (wq.min() < 0 or int(wq.sum()) != 65536):
                raise ValueError(f"lc_amd.augment: params row {b}: the weights of filter {name} must be non-negative and sum to 65536, got a sum of {int(wq.sum())} and a minimum of {int(wq.min())}")
        if bits & BIT_DROPOUT and not (1 <= row[4] <= h and 1 <= row[5] <= w):
            raise ValueError(f"lc_amd.augment: params row {b}: a dropout grid of 1 x 1 to {h} x {w}, got {int(row[4])} x {int(row[5])}")
        if bits & BIT_SWITCH:
            if not has_mask or n_backgrounds == 0:
                raise ValueError(f"lc_amd.augment: params row {b} switches the background, which needs msk_in and backgrounds")
            if not (0 <= row[1] < n_backgrounds):
                raise ValueError(f"lc_amd.augment: params row {b} names background {int(row[1])} of {n_backgrounds}")
    return bool(len(P)) and bool((P[:, 0] & (BIT_MOTION | BIT_GAUSS)).any())


@torch.no_grad()
def augment(crops, params, lut, *, msk_in=None, backgrounds=None, seed=0, sample_id=None, dtype=torch.float32, normalize=None, pointwise=None):
    """crops (B,3,h,w) uint8 (what `crops.warp_affine(..., dtype=torch.uint8)` writes); params (B,64) int32 and lut (B,3,256) uint8 as
    `draw` makes them -- host numpy arrays / CPU tensors (checked here against the row rules, then uploaded) or device tensors (judged by
    the kernel: a bad row gets `info = -1` and is written as its unchanged crop); msk_in (B,h,w) float32 = k / 1024 as
    `maskcrop.mask_crops` writes it, or None; backgrounds (G,3,h,w) uint8 or None; seed a whole number below 2^64; sample_id (B,) int32
    or None (row b is sample b).

    -> (out (B,3,h,w) of `dtype`: bytes (torch.uint8), or `bytes / 255` with `normalize = (mean[3], std[3])` as
    `(bytes / 255 - mean) / std`, computed in fp32 and rounded once, exactly as `crops.warp_affine` finishes its crops;
    info (B,) int32: 0, -1 for a refused row).

    `pointwise` selects the compiled form that streams without a halo and refuses rows with a filter bit: None takes it when HOST params
    show no row with a filter (device params are not read back: the filtered form serves every row), True / False say it outright."""
    crops = _A.tensor("crops", crops, (torch.uint8,), "uint8", (None, 3, None, None))
    B, _, h, w = (int(s) for s in crops.shape)
    if not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
        raise ValueError(f"lc_amd.augment: crop sizes of {MIN_SIZE} to {MAX_SIZE}, got {h} x {w}")
    host_params = isinstance(params, np.ndarray) or (isinstance(params, Tensor) and not params.is_cuda)
    if isinstance(params, np.ndarray):
        params = torch.from_numpy(np.ascontiguousarray(params))
    if isinstance(lut, np.ndarray):
        lut = torch.from_numpy(np.ascontiguousarray(lut))
    params = _A.tensor("params", params, (torch.int32,), "int32", (B, WORDS))
    lut = _A.tensor("lut", lut, (torch.uint8,), "uint8", (B, 3, 256))
    if msk_in is not None:
        _A.tensor("msk_in", msk_in, (torch.float32,), "float32", (B, h, w))
    if backgrounds is not None:
        _A.tensor("backgrounds", backgrounds, (torch.uint8,), "uint8", (None, 3, h, w))
    if sample_id is not None:
        _A.tensor("sample_id", sample_id, (torch.int32,), "int32", (B,))
    seed = _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    if dtype not in OUT_DTYPES:
        raise TypeError(f"lc_amd.augment: dtype must be one of uint8, float32, float16, bfloat16, got {dtype}")
    if pointwise is not None and not isinstance(pointwise, bool):
        raise TypeError(f"lc_amd.augment: pointwise must be None, True or False, got {type(pointwise)}")
    mean = std = None
    if normalize is not None:
        if dtype == torch.uint8:
            raise TypeError("lc_amd.augment: normalize needs a float dtype")
        mean, std = _A.host_floats("mean", normalize[0], 3), _A.host_floats("std", normalize[1], 3)
    G = 0 if backgrounds is None else int(backgrounds.shape[0])
    if host_params:
        filtered = check_params(params.numpy(), h, w, G, msk_in is not None)
        if pointwise and filtered:
            raise ValueError("lc_amd.augment: pointwise=True, but a row of params uses a 5x5 filter")
        if pointwise is None:
            pointwise = not filtered
    if not crops.is_cuda:
        raise RuntimeError(f"lc_amd.augment: crops is on {crops.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = crops.device
    if host_params:
        params = params.to(dev)
    if not lut.is_cuda:
        lut = lut.to(dev)
    _A.same_device(dev, "the crops on {}", params=params, lut=lut, msk_in=msk_in, backgrounds=backgrounds, sample_id=sample_id)
    crops, params, lut = crops.contiguous(), params.contiguous(), lut.contiguous()
    msk = None if msk_in is None else msk_in.contiguous()
    bg = None if backgrounds is None or G == 0 else backgrounds.contiguous()
    sid = None if sample_id is None else sample_id.contiguous()
    out = torch.empty(B, 3, h, w, device=dev, dtype=dtype)
    info = torch.empty(B, device=dev, dtype=torch.int32)
    if B:
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_augment_u8(_lib.ptr(crops), _lib.ptr(bg), G if bg is not None else 0, _lib.ptr(msk), _lib.ptr(params), _lib.ptr(lut), B, h, w, seed,
                                   _lib.ptr(sid), OUT_DTYPES[dtype], FORMS["pointwise" if pointwise else "filtered"], mean, std, _lib.ptr(out),
                                   _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("augment.augment", rc)
    return out, info


def _seed_word(seed, dev) -> Tensor:
    """The seed as one 64-bit word on the device.  A whole number is written there by a fill (no host copy, no wait: capturable); a
    tensor is the caller's own word, which the kernel reads at every launch and replay."""
    if isinstance(seed, Tensor):
        if seed.dtype not in (torch.uint64, torch.int64) or seed.numel() != 1:
            raise TypeError(f"lc_amd.augment: a seed tensor holds one uint64 or int64 element, got {seed.dtype} of shape {tuple(seed.shape)}")
        if seed.device != dev:
            raise RuntimeError(f"lc_amd.augment: seed is on {seed.device}, the crops on {dev}")
        return seed
    seed = _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    return torch.full((1,), seed - 2 ** 64 if seed >= 2 ** 63 else seed, dtype=torch.int64, device=dev)  # the same 64 bits


@torch.no_grad()
def augment_drawn(crops, cfg: AugmentConfig, *, seed, sample_id, msk_in=None, backgrounds=None, dtype=torch.float32, normalize=None, return_rows=False):
    """`augment(crops, *draw(cfg, seed, sample_id, G, (h, w)), msk_in=..., backgrounds=..., seed=seed, sample_id=sample_id, ...)` with the
    rows drawn by the kernel (`lc_augment_drawn_u8` of include/lc_amd_augment.h): `params` and `lut` never exist on the host.  G is
    the number of `backgrounds` (0 without them: no row switches).  The bits, the background, the dropout grid and the tables are
    `draw`'s bit for bit; each Q16 filter weight is within 1 of `draw`'s (the device has its own exp, sin and cos), non-negative, and
    each set sums to 65536.

    seed: a whole number below 2^64, or a device tensor of one uint64 / int64 element that the KERNEL reads: a captured graph draws anew
    at every replay once the caller has changed that word (`seed_word.add_(1)`, or a copy into it).  sample_id (B,) int32 is required:
    a drawn row belongs to its sample, not to its place in the batch.  A row that switches the background while `msk_in` is None is
    refused as `augment` refuses it on device params: info = -1, the unchanged crop.

    The launch takes the filtered form unless `cfg.pixel_aug_prob == 0`, which rules both filters out.  Allocates its outputs only
    (and the one word of a by-value seed), never waits for the device, and can be captured into a graph.

    -> (out, info) as `augment`; with `return_rows` also (params (B,64) int32, lut (B,3,256) uint8) on the device: the rows as drawn."""
    crops = _A.tensor("crops", crops, (torch.uint8,), "uint8", (None, 3, None, None))
    B, _, h, w = (int(s) for s in crops.shape)
    if not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
        raise ValueError(f"lc_amd.augment: crop sizes of {MIN_SIZE} to {MAX_SIZE}, got {h} x {w}")
    if not isinstance(cfg, AugmentConfig):
        raise TypeError(f"lc_amd.augment: cfg must be an AugmentConfig, got {type(cfg)}")
    for name in ("pixel_aug_prob", "switch_bg_prob"):
        if not 0.0 <= float(getattr(cfg, name)) <= 1.0:
            raise ValueError(f"lc_amd.augment: {name} must lie in [0, 1], got {getattr(cfg, name)}")
    if sample_id is None:
        raise TypeError("lc_amd.augment: augment_drawn needs sample_id: a drawn row belongs to its sample")
    _A.tensor("sample_id", sample_id, (torch.int32,), "int32", (B,))
    if msk_in is not None:
        _A.tensor("msk_in", msk_in, (torch.float32,), "float32", (B, h, w))
    if backgrounds is not None:
        _A.tensor("backgrounds", backgrounds, (torch.uint8,), "uint8", (None, 3, h, w))
    if dtype not in OUT_DTYPES:
        raise TypeError(f"lc_amd.augment: dtype must be one of uint8, float32, float16, bfloat16, got {dtype}")
    mean = std = None
    if normalize is not None:
        if dtype == torch.uint8:
            raise TypeError("lc_amd.augment: normalize needs a float dtype")
        mean, std = _A.host_floats("mean", normalize[0], 3), _A.host_floats("std", normalize[1], 3)
    if not isinstance(seed, Tensor):
        _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    if not crops.is_cuda:
        raise RuntimeError(f"lc_amd.augment: crops is on {crops.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = crops.device
    _A.same_device(dev, "the crops on {}", msk_in=msk_in, backgrounds=backgrounds, sample_id=sample_id)
    word = _seed_word(seed, dev)
    G = 0 if backgrounds is None else int(backgrounds.shape[0])
    crops, sid = crops.contiguous(), sample_id.contiguous()
    msk = None if msk_in is None else msk_in.contiguous()
    bg = None if G == 0 else backgrounds.contiguous()
    out = torch.empty(B, 3, h, w, device=dev, dtype=dtype)
    info = torch.empty(B, device=dev, dtype=torch.int32)
    params = torch.empty(B, WORDS, device=dev, dtype=torch.int32) if return_rows else None
    lut = torch.empty(B, 3, 256, device=dev, dtype=torch.uint8) if return_rows else None
    if B:
        c = DrawConfig(float(cfg.pixel_aug_prob), float(cfg.switch_bg_prob), int(bool(cfg.use_peper_salt)), int(bool(cfg.use_motion_blur)),
                       int(bool(cfg.use_invert)), G)
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_augment_drawn_u8(_lib.ptr(crops), _lib.ptr(bg), G, _lib.ptr(msk), c, _lib.ptr(word), _lib.ptr(sid), B, h, w, OUT_DTYPES[dtype],
                                         mean, std, _lib.ptr(out), _lib.ptr(info), _lib.ptr(params), _lib.ptr(lut), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("augment.augment_drawn", rc)
    return (out, info, params, lut) if return_rows else (out, info)
