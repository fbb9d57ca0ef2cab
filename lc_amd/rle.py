"""A dataset's COCO run-length masks resident on the device (lc_amd/csrc/rle/lc_rle.hip, lc_amd/_C/liblc_amd_rle.so; C ABI, the format
and the exact definition of every output in include/lc_amd_rle.h): what the reference's loader does per sample on a host core through
pycocotools (`dataset.py:174-182` writes one run-length record per instance, `dataset.py:379` decodes one per sample).

    RleStore.from_counts(list_of_arrays, sizes)            count lists as they are
    RleStore.from_coco(records)                            {'size': [H, W], 'counts': bytes | str | list}, as pycocotools has them
    RleStore.from_masks(masks, sizes=None, origin_xy=None, cap=1024)   byte masks on the device, encoded there
    store.area, store.box, store.valid, store.box_xywh(plus_one=True), store.window_origins(index, (Hm, Wm)), store.to_coco(compress=True)
    decode(store, index=None, origin_xy=None, hw=None) -> (masks (B,Hm,Wm) uint8, info (B,) int32)
    encode(masks, sizes=None, origin_xy=None, cap=1024) -> Encoded(counts (F,cap), n_runs (F,), info (F,))

The store is built once; `decode` then makes no host work per step and takes B integers: its result is what
`maskcrop.mask_crops(masks, ..., mask_index=None, origin=origin_xy)` reads without a copy.  A mask of a frame with H rows and W columns is
a list of counts over the column-major positions p = x H + y, run k having value k & 1; tests/rle_oracle.py restates all of it in numpy.

uint32 arrays (`counts`, `ends`, the encoder's lists) are int32 tensors that hold the same bits: `t.cpu().numpy().view(np.uint32)`.

COCO's compressed string is coded here on the host (`counts_to_string`, `string_to_counts`): it is parsed once per dataset.  Each count x,
from the third on less the count two places before it, goes out in 5-bit groups, low group first: c = x & 0x1f; x >>= 5 (arithmetic);
more = (c & 0x10) ? x != -1 : x != 0; c |= 0x20 if more; the character is c + 48.

HIP tensors only (anything else raises: there is no CPU fallback).  `decode`, `encode` and `store.index()` run on the current stream,
never wait for the device, allocate their outputs only (none with `out=`) and can be captured into a graph.
"""
from __future__ import annotations

from ctypes import c_int, c_int64, c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

MAX_SIZE = 16384           # LC_RLE_MAX_SIZE
MAX_ORIGIN = 16777216      # LC_RLE_MAX_ORIGIN
MAX_COUNTS = 4294967296    # LC_RLE_MAX_COUNTS
DELTA_FROM = 2             # the first count (from 0) that the string holds as a difference to the count two places before it


class Encoded(NamedTuple):
    counts: Tensor   # (F,cap) int32 holding uint32 bits: the canonical list in the first n_runs entries, the rest 0
    n_runs: Tensor   # (F,) int32
    info: Tensor     # (F,) int32: 0, -2 where cap was too small (the row is zero, n_runs the needed number), -1 for a bad size or origin


_SO = _lib.SideLibrary(_build.RLE, {
    "lc_rle_index_u32": (c_int, [c_void_p] * 3 + [c_int64, c_int] + [c_void_p] * 5),
    "lc_rle_decode_u8": (c_int, [c_void_p] * 4 + [c_int64, c_int] + [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 3),
    "lc_rle_encode_u8": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 2 + [c_int] + [c_void_p] * 4),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("rle")  # its whole numbers may be numpy's (`numpy=True`)


# ---- COCO's compressed string, on the host


def counts_to_string(counts) -> bytes:
    """One count list as COCO's compressed string (bytes, as pycocotools' `encode` returns it)."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    out = bytearray()
    for i, x in enumerate(c):
        if i >= DELTA_FROM:
            x -= c[i - 2]
        more = True
        while more:
            g = x & 0x1F
            x >>= 5  # Python's shift of a negative whole number is arithmetic
            more = (x != -1) if (g & 0x10) else (x != 0)
            out.append((g | 0x20 if more else g) + 48)
    return bytes(out)


def string_to_counts(s) -> np.ndarray:
    """The reverse: bytes or str -> uint32 counts.  Raises on a character outside 48..111, a string that ends inside a count, and a
    count outside [0, 2^32)."""
    if isinstance(s, str):
        s = s.encode("ascii")
    if not isinstance(s, (bytes, bytearray)):
        raise TypeError(f"lc_amd.rle: a compressed string is bytes or str, got {type(s)}")
    g = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if g.size == 0:
        return np.zeros(0, dtype=np.uint32)
    if g.min() < 0 or g.max() > 63:
        raise ValueError("lc_amd.rle: a compressed string holds characters '0' (48) to 'o' (111) only")
    last = (g & 0x20) == 0  # the group that ends its count
    if not last[-1]:
        raise ValueError("lc_amd.rle: the compressed string ends inside a count")
    first = np.concatenate(([True], last[:-1]))
    start = np.flatnonzero(first)
    place = np.arange(g.size) - np.repeat(start, np.diff(np.concatenate((start, [g.size]))))  # the group's place inside its count
    if place.max() > 7:  # 35 bits hold every difference of two 32-bit counts
        raise ValueError("lc_amd.rle: a count of the compressed string has more than 8 groups")
    x = np.add.reduceat((g & 0x1F) << (5 * place), start)
    end = np.flatnonzero(last)
    neg = (g[end] & 0x10) != 0  # the sign, from bit 4 of the last group
    x = np.where(neg, x - (np.int64(1) << (5 * (place[end] + 1))), x)
    for par in (0, 1):  # a difference is added to the finished count two places before: a running sum over every other entry
        v = x[par::2]
        plain = max(len(range(par, min(DELTA_FROM, x.size), 2)) - 1, 0)
        v[plain:] = np.cumsum(v[plain:])
    if x.size and (x.min() < 0 or x.max() >= 2 ** 32):
        raise ValueError("lc_amd.rle: the compressed string holds a count outside [0, 2^32)")
    return x.astype(np.uint32)


# ---- argument rules


def _pair(name, hw):
    return _A.size_pair(name, hw, MAX_SIZE, numpy=True)


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else torch.device(device if device is not None else "cpu")
    if dev.type != "cuda":
        raise RuntimeError(f"lc_amd.rle: the store lives on the MI355X, got device {dev} (there is no CPU fallback in the product path)")
    return dev


def _sizes_array(sizes, F):
    a = np.asarray(sizes)
    if a.dtype.kind not in "iu":
        raise TypeError(f"lc_amd.rle: sizes must hold whole numbers, got {a.dtype}")
    if a.shape == (2,):
        a = np.tile(a, (F, 1))
    if a.shape != (F, 2):
        raise ValueError(f"lc_amd.rle: sizes has shape {a.shape}, expected (2,) or ({F}, 2)")
    if F and (a.min() < 1 or a.max() > MAX_SIZE):
        raise ValueError(f"lc_amd.rle: frame sizes of 1 to {MAX_SIZE}, got {int(a.min())} to {int(a.max())}")
    return np.ascontiguousarray(a, dtype=np.int32)


class RleStore:
    """counts (T,) int32 (uint32 bits), offsets (F+1,) int64 and sizes (F,2) int32 = (H, W) on one HIP device, indexed on construction:
    `ends` (T,) int32 (uint32 bits), `area` (F,) int32, `box` (F,4) int32 inclusive (x_min, y_min, x_max, y_max) or four times -1, `valid`
    (F,) int32, 0 or -1.  The arrays are device data: the kernels judge them, and whoever overwrites them in place calls `index()` again."""

    def __init__(self, counts, offsets, sizes, frame_hw=None):
        _A.tensor("counts", counts, (torch.int32,), "int32 (holding uint32 bits)", (None,))
        _A.tensor("offsets", offsets, (torch.int64,), "int64", (None,))
        if offsets.shape[0] < 1:
            raise ValueError("lc_amd.rle: offsets holds F + 1 entries, got none")
        F = int(offsets.shape[0]) - 1
        _A.tensor("sizes", sizes, (torch.int32,), "int32", (F, 2))
        if not counts.is_cuda:
            raise RuntimeError(f"lc_amd.rle: counts is on {counts.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
        _A.same_device(counts.device, "the counts on {}", offsets=offsets, sizes=sizes)
        if counts.shape[0] > MAX_COUNTS:
            raise ValueError(f"lc_amd.rle: at most {MAX_COUNTS} counts, got {counts.shape[0]}")
        self.counts, self.offsets, self.sizes = counts.contiguous(), offsets.contiguous(), sizes.contiguous()
        self.F, self.T, self.device = F, int(counts.shape[0]), counts.device
        self.frame_hw = None if frame_hw is None else _pair("frame_hw", frame_hw)  # the one size of all masks, where the maker knew it
        self.ends = torch.zeros(self.T, device=self.device, dtype=torch.int32)
        self.area = torch.zeros(F, device=self.device, dtype=torch.int32)
        self.box = torch.full((F, 4), -1, device=self.device, dtype=torch.int32)
        self.valid = torch.full((F,), -1, device=self.device, dtype=torch.int32)
        self.index()

    def __len__(self):
        return self.F

    @torch.no_grad()
    def index(self):
        """One launch: `ends`, `area`, `box` and `valid` from the arrays as they are now, in place."""
        if self.F:
            lib = load()
            with _lib.on_device(self.device):
                rc = lib.lc_rle_index_u32(_lib.ptr(self.counts), _lib.ptr(self.offsets), _lib.ptr(self.sizes), self.T, self.F, _lib.ptr(self.ends), _lib.ptr(self.area),
                                          _lib.ptr(self.box), _lib.ptr(self.valid), _lib.stream_ptr(self.device))
            if rc != 0:
                _SO.fail("rle.RleStore.index", rc)
        return self

    @classmethod
    def from_counts(cls, list_of_arrays, sizes, device=None):
        """One array of counts per mask (whole numbers in [0, 2^32)); sizes = (H, W) for all, or (F,2).  Sums are not judged here: `valid` says."""
        if isinstance(list_of_arrays, (np.ndarray, Tensor)) or not hasattr(list_of_arrays, "__len__"):
            raise TypeError(f"lc_amd.rle: from_counts takes a list of arrays, one per mask, got {type(list_of_arrays)}")
        F = len(list_of_arrays)
        rows = []
        for f, c in enumerate(list_of_arrays):
            a = np.asarray(c)
            if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
                raise TypeError(f"lc_amd.rle: the counts of mask {f} must be a list of whole numbers, got {a.dtype} of shape {a.shape}")
            a = a.astype(np.int64) if a.dtype != np.uint64 else a
            if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32):
                raise ValueError(f"lc_amd.rle: the counts of mask {f} must lie in [0, 2^32)")
            rows.append(a.astype(np.uint32))
        s = _sizes_array(sizes, F)
        dev = _device(device)
        offsets = np.zeros(F + 1, dtype=np.int64)
        np.cumsum([r.size for r in rows], out=offsets[1:])
        flat = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint32)
        same = F > 0 and bool((s == s[0]).all())
        return cls(torch.from_numpy(flat.view(np.int32)).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(s).to(dev),
                   frame_hw=(int(s[0, 0]), int(s[0, 1])) if same else None)

    @classmethod
    def from_coco(cls, records, device=None):
        """Records as pycocotools has them, in the caller's order: {'size': [H, W], 'counts': bytes | str (compressed) | list (plain)}."""
        if isinstance(records, dict) or not hasattr(records, "__len__"):
            raise TypeError(f"lc_amd.rle: from_coco takes a list of records, got {type(records)}")
        rows, sizes = [], []
        for f, r in enumerate(records):
            if not isinstance(r, dict) or "size" not in r or "counts" not in r:
                raise ValueError(f"lc_amd.rle: record {f} must be a dict with 'size' and 'counts'")
            c = r["counts"]
            rows.append(string_to_counts(c) if isinstance(c, (bytes, bytearray, str)) else c)
            if len(r["size"]) != 2:
                raise ValueError(f"lc_amd.rle: the size of record {f} is [H, W], got {r['size']!r}")
            sizes.append([int(r["size"][0]), int(r["size"][1])])
        return cls.from_counts(rows, np.asarray(sizes, dtype=np.int64).reshape(len(rows), 2), device)

    @classmethod
    def from_masks(cls, masks, sizes=None, origin_xy=None, cap=1024):
        """Byte masks (F,Hm,Wm) on the device, encoded there (`encode`) and compacted on the host.  Raises when a mask needs more than
        `cap` runs, or has a size or origin out of range."""
        enc = encode(masks, sizes, origin_xy, cap)
        n, info = enc.n_runs.cpu().numpy(), enc.info.cpu().numpy()
        if (info == -2).any():
            f = int(np.flatnonzero(info == -2)[0])
            raise ValueError(f"lc_amd.rle: mask {f} needs {int(n[f])} runs, more than cap = {cap} (the largest need is {int(n.max())})")
        if (info != 0).any():
            raise ValueError(f"lc_amd.rle: mask {int(np.flatnonzero(info != 0)[0])} has a frame size or an origin out of range")
        c = enc.counts.cpu().numpy().view(np.uint32)
        F, Hm, Wm = (int(v) for v in masks.shape)
        s = np.tile(np.asarray([[Hm, Wm]], dtype=np.int32), (F, 1)) if sizes is None else (sizes.cpu().numpy() if isinstance(sizes, Tensor) else sizes)
        return cls.from_counts([c[f, :n[f]] for f in range(F)], s, masks.device)

    def to_coco(self, compress=True):
        """-> [{'size': [H, W], 'counts': bytes (compressed, as pycocotools' `encode` gives) or a list of whole numbers}], read back."""
        c = self.counts.cpu().numpy().view(np.uint32)
        off, s = self.offsets.cpu().numpy(), self.sizes.cpu().numpy()
        out = []
        for f in range(self.F):
            row = c[off[f]:off[f + 1]]
            out.append({"size": [int(s[f, 0]), int(s[f, 1])], "counts": counts_to_string(row) if compress else [int(v) for v in row]})
        return out

    def box_xywh(self, plus_one=True):
        """(F,4) int32 [x_min, y_min, w, h]: w = x_max - x_min + 1 as COCO's `toBbox` has it (plus_one), or x_max - x_min, the convention
        `gtinfo.bop_records` has without `bbox_plus_one`; four times -1 for an empty or invalid mask (pycocotools gives four zeros there)."""
        if not isinstance(plus_one, bool):
            raise TypeError(f"lc_amd.rle: plus_one must be a bool, got {type(plus_one)}")
        b = self.box
        wh = b[:, 2:] - b[:, :2] + (1 if plus_one else 0)
        return torch.where(b[:, :1] < 0, torch.full_like(b, -1), torch.cat((b[:, :2], wh), 1))

    def window_origins(self, index, hw):
        """(B,2) int32 (x0, y0) of (Hm, Wm) windows centred on the boxes of masks `index` ((B,) int32 / int64, or None for all): the box
        centre (x_min + x_max + 1) / 2 less half the window, floored; (0, 0) for an empty mask.  Plain torch on the device."""
        Hm, Wm = _pair("hw", hw)
        b = self.box if index is None else self.box[_A.tensor("index", index, (torch.int32, torch.int64), "int32 or int64", (None,)).long()]
        x0 = torch.div(b[:, 0] + b[:, 2] + 1 - Wm, 2, rounding_mode="floor")
        y0 = torch.div(b[:, 1] + b[:, 3] + 1 - Hm, 2, rounding_mode="floor")
        return torch.where(b[:, :1] < 0, torch.zeros_like(b[:, :2]), torch.stack((x0, y0), 1)).to(torch.int32)


@torch.no_grad()
def decode(store, index=None, origin_xy=None, hw=None, out=None):
    """Row b is mask index[b] ((B,) int32; None: every mask in order) in a (Hm, Wm) window at origin_xy[b] ((B,2) int32 / int64 = (x0, y0),
    anywhere within MAX_ORIGIN; None: (0,0)); hw = (Hm, Wm), or None for the one frame size the store was made with.

    -> (masks (B,Hm,Wm) uint8, bytes 0 / 1, window pixel (i, j) = frame pixel (x0 + j, y0 + i), 0 outside the frame;  info (B,) int32: 0,
    or -1 for an index outside [0,F), an invalid mask or an origin beyond MAX_ORIGIN -- such a row is all zero).  `out` = (masks, info)
    to write into."""
    if not isinstance(store, RleStore):
        raise TypeError(f"lc_amd.rle: decode takes an RleStore, got {type(store)}")
    if hw is None:
        if store.frame_hw is None:
            raise ValueError("lc_amd.rle: the store's masks have no one frame size; say hw=(Hm, Wm)")
        hw = store.frame_hw
    Hm, Wm = _pair("hw", hw)
    if index is not None:
        _A.tensor("index", index, (torch.int32,), "int32", (None,))
    B = store.F if index is None else int(index.shape[0])
    if origin_xy is not None:
        _A.tensor("origin_xy", origin_xy, (torch.int32, torch.int64), "int32 or int64", (B, 2))
    dev = store.device
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("lc_amd.rle: out is the pair (masks, info)")
        _A.tensor("out[0]", out[0], (torch.uint8,), "uint8", (B, Hm, Wm))
        _A.tensor("out[1]", out[1], (torch.int32,), "int32", (B,))
        if not (out[0].is_contiguous() and out[1].is_contiguous()):
            raise ValueError("lc_amd.rle: out must be contiguous")
    _A.same_device(dev, "the store on {}", index=index, origin_xy=origin_xy, **{f"out[{i}]": t for i, t in enumerate(out or ())})
    idx = None if index is None else index.contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    masks, info = out if out is not None else (torch.empty((B, Hm, Wm), device=dev, dtype=torch.uint8), torch.empty((B,), device=dev, dtype=torch.int32))
    if B:
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_rle_decode_u8(_lib.ptr(store.ends), _lib.ptr(store.offsets), _lib.ptr(store.sizes), _lib.ptr(store.valid), store.T, store.F, _lib.ptr(idx),
                                      _lib.ptr(org), B, Hm, Wm, _lib.ptr(masks), _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("rle.decode", rc)
    return masks, info


@torch.no_grad()
def encode(masks, sizes=None, origin_xy=None, cap=1024, out=None) -> Encoded:
    """masks (F,Hm,Wm) uint8 or bool on the device (non-zero = set; `GtInfo.mask_visib` as it is), each a window at origin_xy[f] ((F,2)
    int32 / int64 or None: (0,0)) of a frame of sizes[f] ((F,2) int32 tensor, a pair (H, W) for all, or None: the window is the frame).
    Frame pixels outside the window are 0; window pixels outside the frame are ignored.  -> Encoded: the canonical lists in (F,cap)."""
    masks = _A.tensor("masks", masks, (torch.uint8, torch.bool), "uint8 or bool", (None, None, None))
    F, Hm, Wm = (int(v) for v in masks.shape)
    if not (1 <= Hm <= MAX_SIZE and 1 <= Wm <= MAX_SIZE):
        raise ValueError(f"lc_amd.rle: mask sizes of 1 to {MAX_SIZE}, got {Hm} x {Wm}")
    cap = _A.whole("cap", cap, 1, 2 ** 31 - 1, numpy=True)
    if sizes is not None and not isinstance(sizes, Tensor):
        sizes = torch.from_numpy(np.tile(np.asarray(_pair("sizes", sizes), dtype=np.int32), (F, 1)))
        sizes = sizes.to(masks.device) if masks.is_cuda else sizes
    if sizes is not None:
        _A.tensor("sizes", sizes, (torch.int32,), "int32", (F, 2))
    if origin_xy is not None:
        _A.tensor("origin_xy", origin_xy, (torch.int32, torch.int64), "int32 or int64", (F, 2))
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("lc_amd.rle: out is the triple (counts, n_runs, info)")
        _A.tensor("out[0]", out[0], (torch.int32,), "int32", (F, cap))
        _A.tensor("out[1]", out[1], (torch.int32,), "int32", (F,))
        _A.tensor("out[2]", out[2], (torch.int32,), "int32", (F,))
        if not all(t.is_contiguous() for t in out):
            raise ValueError("lc_amd.rle: out must be contiguous")
    if not masks.is_cuda:
        raise RuntimeError(f"lc_amd.rle: masks is on {masks.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = masks.device
    _A.same_device(dev, "the masks on {}", sizes=sizes, origin_xy=origin_xy, **{f"out[{i}]": t for i, t in enumerate(out or ())})
    masks = masks.contiguous()
    m8 = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    siz = None if sizes is None else sizes.contiguous()
    org = None if origin_xy is None else origin_xy.to(torch.int32).contiguous()
    counts, n_runs, info = out if out is not None else (torch.empty((F, cap), device=dev, dtype=torch.int32), torch.empty((F,), device=dev, dtype=torch.int32),
                                                        torch.empty((F,), device=dev, dtype=torch.int32))
    if F:
        lib = load()
        with _lib.on_device(dev):
            rc = lib.lc_rle_encode_u8(_lib.ptr(m8), F, Hm, Wm, _lib.ptr(siz), _lib.ptr(org), cap, _lib.ptr(counts), _lib.ptr(n_runs), _lib.ptr(info), _lib.stream_ptr(dev))
        if rc != 0:
            _SO.fail("rle.encode", rc)
    return Encoded(counts, n_runs, info)
