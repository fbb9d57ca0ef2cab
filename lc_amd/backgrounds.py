"""The training loader's backgrounds resident on the device, and the switch that picks, cuts and blends each row's background in place
(lc_amd/csrc/bgstore/lc_bgstore.hip, lc_amd/_C/liblc_amd_bgstore.so; C ABI and the exact definition in include/lc_amd_bgstore.h): what
the reference's loader does per instance on a host core with `_switch_bg(rgb_in, msk_in, np.random.choice(self.bg_list))`
(`dataset.py:137-148,413-415`).

    BackgroundStore.from_images(images, device) -> store        G images of their own sizes in one byte buffer, uploaded once
    pick_backgrounds(store, cfg, *, seed, sample_id) -> (gate, which, bg_hw)
    switch_backgrounds(crops, store, cfg, *, seed, sample_id, msk_in) -> (info, which)      in place in `crops`

No new arithmetic; every number composes contracts the project already states.  With `u = augment.u`:

    gate_b, g_b   bit 0 and P[1] of `augment.draw(cfg, seed, sample_id, G)`: u(OP_SWITCH, 0) < cfg.switch_bg_prob, min(trunc(u(OP_SWITCH, 1) G), G - 1)
    M_b           `augment.background_matrices(seed, id_b, store.hw[g_b], (h, w))`, by `geometry.background_geometry` from the pick's per-row sizes
    bg_b          `crops.warp_affine(image g_b, M_b, (h, w))`, linear, uint8 (include/lc_amd_crop.h)
    crop_b        the blend of bit 0 of include/lc_amd_augment.h with k from `msk_in`: a pixel with k = 1024 keeps its byte

A row whose gate is closed is untouched.  The colour chain's draws do not depend on the number of backgrounds, so
`augment.augment_drawn(switched_crop, cfg, backgrounds=None, ...)` gives the `rgb_in` of a route that hands the same cut to `augment`.

HIP tensors only (anything else raises: there is no CPU fallback).  Three launches on the current stream -- pick, region matrices, switch --
that read the seed from one 64-bit word on the device, never wait for the device and allocate their few per-row outputs only: a captured
graph picks and cuts anew at every replay once the word has changed (`lc_amd.train_inputs.train_inputs(background_store=...)`).
"""
from __future__ import annotations

from ctypes import c_double, c_int, c_void_p

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import augment as _aug
from . import build as _build
from . import geometry as _geometry
from .augment import AugmentConfig

MAX_SIZE = 16384    # LC_BGSTORE_MAX_SIZE = LC_CROP_MAX_SIZE
ALIGN = 4           # every image starts on a multiple of four bytes

_SO = _lib.SideLibrary(_build.BGSTORE, {
    "lc_bgstore_pick": (c_int, [c_double, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lc_bgstore_switch_u8": (c_int, [c_void_p] * 5 + [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("backgrounds")


def layout(sizes):
    """The byte offset of every image of `sizes` = [(Hb, Wb), ...] and the buffer's length: image after image, rows of 3 Wb bytes
    without padding, every start rounded up to a multiple of ALIGN."""
    offsets, end = [], 0
    for hb, wb in sizes:
        start = -(-end // ALIGN) * ALIGN
        offsets.append(start)
        end = start + 3 * int(hb) * int(wb)
    return offsets, end


class BackgroundStore:
    """G background images of their own sizes on the device: `pixels` (N,) uint8, image g as (Hb,Wb,3) bytes from `offsets[g]` on
    (int64 (G,)), `hw` (G,2) int32 = (Hb, Wb).  `sizes` keeps the pairs on the host.  Built once; nothing in it changes afterwards."""

    def __init__(self, pixels: Tensor, offsets: Tensor, hw: Tensor, sizes):
        self.pixels, self.offsets, self.hw, self.sizes = pixels, offsets, hw, tuple(sizes)
        self.G, self.device = len(self.sizes), pixels.device

    def __len__(self):
        return self.G

    @classmethod
    def from_images(cls, images, device) -> "BackgroundStore":
        """images: a sequence of G >= 1 (Hb,Wb,3) uint8 numpy arrays or tensors, sizes of 1 to MAX_SIZE; laid out on the host by
        `layout` and uploaded in one copy."""
        if isinstance(images, (Tensor, np.ndarray)) or not hasattr(images, "__len__"):
            raise TypeError(f"lc_amd.backgrounds: images is a sequence of (Hb,Wb,3) uint8 arrays, got {type(images)}")
        if len(images) < 1:
            raise ValueError("lc_amd.backgrounds: a store holds at least one image")
        arrays = []
        for g, im in enumerate(images):
            a = im.detach().cpu().numpy() if isinstance(im, Tensor) else im
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
                raise TypeError(f"lc_amd.backgrounds: image {g} must be a uint8 array or tensor, got {getattr(a, 'dtype', type(a))}")
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"lc_amd.backgrounds: image {g} has shape {tuple(a.shape)}, expected (Hb,Wb,3)")
            if not (1 <= a.shape[0] <= MAX_SIZE and 1 <= a.shape[1] <= MAX_SIZE):
                raise ValueError(f"lc_amd.backgrounds: image sizes of 1 to {MAX_SIZE}, got {a.shape[0]} x {a.shape[1]} for image {g}")
            arrays.append(a)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"lc_amd.backgrounds: the store lives on the MI355X, got device {device} (there is no CPU fallback in the product path)")
        sizes = [(int(a.shape[0]), int(a.shape[1])) for a in arrays]
        offsets, total = layout(sizes)
        buf = np.zeros(total, dtype=np.uint8)
        for a, o in zip(arrays, offsets):
            buf[o:o + a.size] = a.reshape(-1)
        return cls(torch.from_numpy(buf).to(device), torch.tensor(offsets, dtype=torch.int64).to(device),
                   torch.tensor(sizes, dtype=torch.int32).reshape(-1, 2).to(device), sizes)


def _common(store, cfg, seed, sample_id):
    if not isinstance(store, BackgroundStore):
        raise TypeError(f"lc_amd.backgrounds: store must be a BackgroundStore, got {type(store)}")
    if not isinstance(cfg, AugmentConfig):
        raise TypeError(f"lc_amd.backgrounds: cfg must be an AugmentConfig, got {type(cfg)}")
    prob = float(cfg.switch_bg_prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"lc_amd.backgrounds: switch_bg_prob must lie in [0, 1], got {cfg.switch_bg_prob}")
    sample_id = _A.tensor("sample_id", sample_id, (torch.int32,), "int32", (None,))
    if not isinstance(seed, Tensor):
        _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    elif seed.dtype not in (torch.uint64, torch.int64) or seed.numel() != 1:
        raise TypeError(f"lc_amd.backgrounds: a seed tensor holds one uint64 or int64 element, got {seed.dtype} of shape {tuple(seed.shape)}")
    return prob, sample_id, int(sample_id.shape[0])


def _pick(store, prob, word, sid, B):
    dev = store.device
    gate, which = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    bg_hw = torch.empty((B, 2), device=dev, dtype=torch.int32)
    if B:
        with _lib.on_device(dev):
            rc = load().lc_bgstore_pick(prob, store.G, _lib.ptr(word), _lib.ptr(sid), _lib.ptr(store.hw), B, _lib.ptr(gate), _lib.ptr(which), _lib.ptr(bg_hw),
                                        _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("backgrounds.pick_backgrounds", rc)
    return gate, which, bg_hw


@torch.no_grad()
def pick_backgrounds(store: BackgroundStore, cfg: AugmentConfig, *, seed, sample_id):
    """(gate (B,) int32, which (B,) int32, bg_hw (B,2) int32) on the device, one launch (`lc_bgstore_pick`): bit 0 and P[1] of
    `augment.draw(cfg, seed, sample_id, store.G)` (which = -1 where the gate is closed) and the chosen image's (Hb, Wb), (1, 1) for a closed
    row.  seed: a whole number below 2^64, or a device tensor of one uint64 / int64 element that the KERNEL reads; sample_id (B,) int32."""
    prob, sample_id, B = _common(store, cfg, seed, sample_id)
    _A.same_device(store.device, "the store on {}", sample_id=sample_id, seed=seed if isinstance(seed, Tensor) else None)
    return _pick(store, prob, _aug._seed_word(seed, store.device), sample_id.contiguous(), B)


@torch.no_grad()
def switch_backgrounds(crops, store: BackgroundStore, cfg: AugmentConfig, *, seed, sample_id, msk_in):
    """IN PLACE in crops (B,3,h,w) uint8, contiguous (what `crops.warp_affine(..., dtype=torch.uint8)` writes): every row whose gate is open
    gets its background -- picked from `store`, its region cut and stretched over the crop, blended behind `msk_in` (B,h,w) float32 = k / 1024
    as `maskcrop.mask_crops` writes it -- as the module's head states; a row whose gate is closed keeps its bytes.  seed and sample_id as
    `pick_backgrounds` takes them: the word the rest of the chain reads.

    -> (info (B,) int32: 1 switched, 0 gate closed, -1 refused and untouched; which (B,) int32: the row's image, -1 where the gate is closed).
    Pick, `geometry.background_geometry` and switch: three launches on the current stream, nothing read back, capturable in a graph."""
    crops = _A.tensor("crops", crops, (torch.uint8,), "uint8", (None, 3, None, None))
    B, _, h, w = (int(s) for s in crops.shape)
    prob, sample_id, rows = _common(store, cfg, seed, sample_id)
    if rows != B:
        raise ValueError(f"lc_amd.backgrounds: sample_id has shape {tuple(sample_id.shape)}, expected {(B,)}")
    msk_in = _A.tensor("msk_in", msk_in, (torch.float32,), "float32", (B, h, w))
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f"lc_amd.backgrounds: crop sizes of 1 to {MAX_SIZE}, got {h} x {w}")
    if not crops.is_contiguous():
        raise ValueError(f"lc_amd.backgrounds: crops must be contiguous (the switch works in place), got strides {tuple(crops.stride())} for shape {tuple(crops.shape)}")
    if not crops.is_cuda:
        raise RuntimeError(f"lc_amd.backgrounds: crops is on {crops.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = crops.device
    _A.same_device(dev, "the crops on {}", store=store.pixels, sample_id=sample_id, msk_in=msk_in, seed=seed if isinstance(seed, Tensor) else None)
    word = _aug._seed_word(seed, dev)
    sid, msk = sample_id.contiguous(), msk_in.contiguous()
    _, which, bg_hw = _pick(store, prob, word, sid, B)
    M = _geometry.background_geometry(seed=word, sample_id=sid, bg_hw=bg_hw, out_hw=(h, w))
    info = torch.empty(B, device=dev, dtype=torch.int32)
    if B:
        with _lib.on_device(dev):
            rc = load().lc_bgstore_switch_u8(_lib.ptr(crops), _lib.ptr(msk), _lib.ptr(store.pixels), _lib.ptr(store.offsets), _lib.ptr(store.hw), store.G,
                                             _lib.ptr(which), _lib.ptr(M), h, w, B, _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("backgrounds.switch_backgrounds", rc)
    return info, which
