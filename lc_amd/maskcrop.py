"""Training mask crops on the device (lc_amd/csrc/maskcrop/lc_maskcrop.hip, lc_amd/_C/liblc_amd_maskcrop.so; C ABI and the exact
definition of every output in include/lc_amd_maskcrop.h): what the reference's loader makes per instance from the visible mask on a host
core (`dataset.py:414,425-442`) -- `msk_in`, `msk_vis`, `msk_noc`, `valid_cnt` and the 256 symmetry check points -- from the byte masks
that `lc_amd.gtinfo` leaves on the device.

    mask_crops(masks, M, out_hw, *, mask_index=None, origin=None, vis_interp="linear", valid_th=100, n_check=256, seed=0,
               sample_id=None, want=("msk_vis", "msk_noc", "valid_cnt", "sym_ck_pts2d"), out=None) -> MaskCrops

The warps use OpenCV's fixed-point coordinates (those of `lc_amd.crops`); for a 0/1 source OpenCV's float path is an integer count over
1024, so `msk_vis` is defined bit for bit (k / 1024) and `msk_noc` is the nearest tap.  The check points follow the loader's rounds
(`np.random.choice(valid_cnt, m, replace=False)` until 256 are drawn) with a stated integer hash of (seed, sample_id, round, pixel) in
place of `np.random`: the same sample with the same seed gets the same points in any batch.  tests/maskcrop_oracle.py restates all of it.

HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device, allocates
its outputs only and can be captured into a graph.  The loader's retry on `valid_cnt` is the caller's: the count comes back.
"""
from __future__ import annotations

from ctypes import c_int, c_size_t, c_uint64, c_void_p
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

MAX_SIZE = 16384           # LC_MASKCROP_MAX_SIZE
MAX_ORIGIN = 16777216      # LC_MASKCROP_MAX_ORIGIN
MAX_CHECK = 256            # LC_MASKCROP_MAX_CHECK
MAX_CHECK_PIXELS = 65536   # LC_MASKCROP_MAX_CHECK_PIXELS
INTERP = {"nearest": 0, "linear": 1}               # LC_MASKCROP_NEAREST / _LINEAR
CK_DTYPES = {torch.int32: 0, torch.int64: 1}       # LC_MASKCROP_I32 / _I64
OUTPUTS = ("msk_vis", "msk_noc", "valid_cnt", "sym_ck_pts2d")


class MaskCrops(NamedTuple):
    msk_vis: Optional[Tensor]       # (B,h,w) float32
    msk_noc: Optional[Tensor]       # (B,h,w) bool
    valid_cnt: Optional[Tensor]     # (B,) int32
    sym_ck_pts2d: Optional[Tensor]  # (B,n_check,2) int64 (or int32): (x, y), -1 where the row has too few valid pixels
    info: Tensor                    # (B,) int32: 0, -1 for a refused row


_SO = _lib.SideLibrary(_build.MASKCROP, {
    "lc_mask_crops_workspace_bytes": (c_size_t, [c_int] * 6),
    "lc_mask_crops_u8": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 3 + [c_int] * 6 + [c_uint64, c_void_p, c_int] + [c_void_p] * 6 + [c_size_t, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("maskcrop")  # its whole numbers are Python's own (`whole` without numpy=True)


@torch.no_grad()
def mask_crops(masks, M, out_hw, *, mask_index=None, origin=None, vis_interp="linear", valid_th=100, n_check=256, seed=0, sample_id=None,
               want=OUTPUTS, out=None, ck_dtype=torch.int64) -> MaskCrops:
    """masks (F,Hm,Wm) uint8 or bool (non-zero = set; `GtInfo.mask_visib` as it is); M (B,2,3) float32, the FORWARD matrix frame -> crop
    (`out_affine`, what cv2.warpAffine takes); out_hw = (h, w); mask_index (B,) int32 or None (row b reads mask b); origin (B,2) int32 /
    int64 = (x0, y0) of the (Hm,Wm) window in the frame, `lc_amd.gtinfo`'s `origin_xy`, anywhere, or None for (0,0): frame pixel (X,Y)
    reads window pixel (X - x0, Y - y0) and anything outside the window reads 0.

    -> MaskCrops(msk_vis (B,h,w) float32: `cv2.warpAffine(mask, M, (w,h), flags=vis_interp)` of the float 0/1 mask, k / 1024 (linear) or
    0 / 1 (nearest);  msk_noc (B,h,w) bool: the nearest warp `> 0.5`;  valid_cnt (B,) int32: its set pixels;  sym_ck_pts2d (B,n_check,2)
    of ck_dtype -- int64, which `lc_amd.labels` reads without a copy, or int32 -- (x, y) in crop pixels, all -1 where valid_cnt <
    valid_th or valid_cnt = 0;  info (B,) int32: -1 for a row with a non-finite M, a mask_index outside [0,F) or an origin beyond
    MAX_ORIGIN, which is all zero with valid_cnt 0 and check points -1).

    `want` names the outputs to make (the others are None); `out` may hold tensors to write into under the same names (msk_noc as bool
    or uint8) and `info`.  seed is a whole number below 2^64 and sample_id (B,) int32 or None (row b is sample b): a row's points depend
    on (seed, sample_id, its own valid pixels) alone.  With check points, h w <= MAX_CHECK_PIXELS.

    Called with the in-matrix at the network's INPUT size, n_check=0 and want=("msk_vis",), it yields `msk_in`, the mask the reference's
    background switch blends with (`dataset.py:414`)."""
    masks = _A.tensor("masks", masks, (torch.uint8, torch.bool), "uint8 or bool", (None, None, None))
    M = _A.tensor("M", M, (torch.float32,), "float32", (None, 2, 3))
    h, w = _A.size_pair("out_hw", out_hw, MAX_SIZE)
    F, Hm, Wm = (int(s) for s in masks.shape)
    B = int(M.shape[0])
    if not (1 <= Hm <= MAX_SIZE and 1 <= Wm <= MAX_SIZE):
        raise ValueError(f"lc_amd.maskcrop: mask sizes of 1 to {MAX_SIZE}, got {Hm} x {Wm}")
    if vis_interp not in INTERP:
        raise ValueError(f"lc_amd.maskcrop: vis_interp must be one of {sorted(INTERP)}, got {vis_interp!r}")
    valid_th = _A.whole("valid_th", valid_th, -2 ** 31, 2 ** 31 - 1)
    n_check = _A.whole("n_check", n_check, 0, MAX_CHECK)
    seed = _A.whole("seed", seed, 0, 2 ** 64 - 1)
    if ck_dtype not in CK_DTYPES:
        raise TypeError(f"lc_amd.maskcrop: ck_dtype must be torch.int32 or torch.int64, got {ck_dtype}")
    if isinstance(want, str) or any(name not in OUTPUTS for name in want):
        raise ValueError(f"lc_amd.maskcrop: want holds names out of {OUTPUTS}, got {want!r}")
    want = tuple(want)
    out = dict(out or {})
    if any(name not in OUTPUTS + ("info",) for name in out):
        raise ValueError(f"lc_amd.maskcrop: out holds tensors under names out of {OUTPUTS + ('info',)}, got {sorted(out)}")
    if any(name not in want for name in out if name != "info"):
        raise ValueError("lc_amd.maskcrop: out holds an output that want does not name")
    checks = "sym_ck_pts2d" in want and n_check > 0
    if checks and h * w > MAX_CHECK_PIXELS:
        raise ValueError(f"lc_amd.maskcrop: check points need a crop of at most {MAX_CHECK_PIXELS} pixels, got {h} x {w}")
    if mask_index is not None:
        _A.tensor("mask_index", mask_index, (torch.int32,), "int32", (B,))
    if origin is not None:
        _A.tensor("origin", origin, (torch.int32, torch.int64), "int32 or int64", (B, 2))
    if sample_id is not None:
        _A.tensor("sample_id", sample_id, (torch.int32,), "int32", (B,))
    shapes = dict(msk_vis=((torch.float32,), "float32", (B, h, w)), msk_noc=((torch.bool, torch.uint8), "bool or uint8", (B, h, w)),
                  valid_cnt=((torch.int32,), "int32", (B,)), sym_ck_pts2d=((ck_dtype,), str(ck_dtype), (B, n_check, 2)), info=((torch.int32,), "int32", (B,)))
    for name, t in out.items():
        _A.tensor(f"out[{name!r}]", t, *shapes[name])
        if not t.is_contiguous():
            raise ValueError(f"lc_amd.maskcrop: out[{name!r}] must be contiguous, got strides {tuple(t.stride())}")
    if not masks.is_cuda:
        raise RuntimeError(f"lc_amd.maskcrop: masks is on {masks.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = masks.device
    _A.same_device(dev, "the masks on {}", M=M, mask_index=mask_index, origin=origin, sample_id=sample_id, **{f"out[{k!r}]": v for k, v in out.items()})
    masks = masks.contiguous()
    m8 = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    M = M.contiguous()
    idx = None if mask_index is None else mask_index.contiguous()
    org = None if origin is None else origin.to(torch.int32).contiguous()
    sid = None if sample_id is None else sample_id.contiguous()

    def made(name, dtype, shape):
        if name != "info" and name not in want:
            return None
        return out[name] if name in out else torch.empty(shape, device=dev, dtype=dtype)

    vis = made("msk_vis", torch.float32, (B, h, w))
    noc = made("msk_noc", torch.bool, (B, h, w))
    cnt = made("valid_cnt", torch.int32, (B,))
    ck = made("sym_ck_pts2d", ck_dtype, (B, n_check, 2))
    info = made("info", torch.int32, (B,))
    if B:
        lib = load()
        ws, nbytes = None, 0
        if checks:
            nbytes = int(lib.lc_mask_crops_workspace_bytes(B, h, w, n_check, noc is not None, cnt is not None))
            if nbytes:
                ws = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
        with _lib.on_device(dev):
            rc = lib.lc_mask_crops_u8(_lib.ptr(m8), F, Hm, Wm, _lib.ptr(idx), _lib.ptr(org), _lib.ptr(M), B, h, w, INTERP[vis_interp], valid_th,
                                      n_check if checks else 0, seed, _lib.ptr(sid), CK_DTYPES[ck_dtype], _lib.ptr(vis), _lib.ptr(noc), _lib.ptr(cnt),
                                      _lib.ptr(ck) if checks else None, _lib.ptr(info), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("maskcrop.mask_crops", rc)
    if noc is not None and noc.dtype != torch.bool:
        noc = noc.view(torch.bool)
    return MaskCrops(vis, noc, cnt, ck, info)
