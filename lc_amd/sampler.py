"""The rows a training step trains on: their contract in host numpy, and the kernels that draw, judge and gather them on the device
(lc_amd/csrc/sampler/lc_sampler.hip, lc_amd/_C/liblc_amd_sampler.so; C ABI and the exact definitions in include/lc_amd_sampler.h).
What the reference's loader does on the host around `_get_single_item`: the epoch's shuffle and the gather of B records (the sampler and
the collate of its DataLoader), and the retry of `BOP_Dataset.__getitem__` (`dataset.py:332-338`), which draws another random instance
whenever `valid_cnt < valid_pix_cnt_th`.

    permute_host(seed0, epoch, n) -> (n,) int64                                              the epoch's order: a bijection of [0, n)
    draw_rows_host(records, *, seed, seed0, batch, spare) -> Rows                            host numpy; records: an AnnotationTable.host, or n
    select_rows_host(valid_cnt, info, *, batch, valid_th) -> (take (batch,) int32, shortfall)
    AnnotationTable(frame_index, mask_index, mesh_index, obj_id, scene_id, im_id, bbox_xyxy, cam_K, R, t, device=...)   resident records
    draw_rows(table, *, seed, seed0, batch, spare) -> Rows                                   device tensors, one launch
    select_rows(valid_cnt, info, *, batch, valid_th) -> (take (batch,) int32, shortfall (1,) int32)     one launch
    take_rows(take, *tensors) -> tuple                                                       one launch per 16 tensors

A step is `seed - seed0` (the 64-bit word the whole chain reads, less the word the set was made with).  Its `batch` PRIMARY rows walk the
epochs' orders -- every annotation is a primary exactly once per epoch, and an epoch may end inside a batch -- and its `spare` rows are
drawn at random with replacement, as the reference's retry draws.  `select_rows` then lets every primary whose crop is too empty take the
next spare whose crop is not, in row order, and `take_rows` gathers the batch: the expensive stages run on `batch` rows (lc_amd/trainset.py).
The host functions touch no device and are the definition; the three device functions equal them bit for bit, read the seed from the
device, never wait for it and allocate their outputs only, so a captured graph moves on to the next step once the word has changed.
HIP tensors only: there is no CPU fallback."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_uint64, c_void_p
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import augment as _aug
from . import build as _build

MAX_ROWS = 65536            # LC_SAMPLER_MAX_ROWS
MAX_N = 2 ** 31 - 1         # LC_SAMPLER_MAX_N
MAX_STEP_BITS = 40          # LC_SAMPLER_MAX_STEP_BITS
MAX_TENSORS = 16            # LC_SAMPLER_MAX_TENSORS
MAX_ROW_BYTES = 2 ** 30     # LC_SAMPLER_MAX_ROW_BYTES
OP_SPARE = _aug.OP_HOST + 14  # LC_SAMPLER_OP_SPARE
OP_PERM = _aug.OP_HOST + 15   # LC_SAMPLER_OP_PERM
ROUNDS = (0x9E3779B9, 0x3C6EF372, 0xDAA66D2B, 0x78DDE6E4)  # LC_SAMPLER_ROUND_0 .. 3
INT_FIELDS = ("frame_index", "mask_index", "mesh_index", "obj_id", "scene_id", "im_id")
FLOAT_FIELDS = (("bbox_xyxy", (4,)), ("cam_K", (3, 3)), ("R", (3, 3)), ("t", (3,)))
FIELDS = INT_FIELDS + tuple(name for name, _ in FLOAT_FIELDS)  # the table's pointers, in the header's order

_M32 = np.uint64(0xFFFFFFFF)
_NAN32 = np.float32(np.nan)


class Rows(NamedTuple):
    """numpy arrays (`draw_rows_host`) or device tensors (`draw_rows`), one row per drawn instance, primaries first."""
    index: object        # (R,) int32: the annotation, -1 for a refused row
    frame_index: object  # (R,) int32
    mask_index: object   # (R,) int32
    mesh_index: object   # (R,) int32
    obj_id: object       # (R,) int32
    scene_id: object     # (R,) int32
    im_id: object        # (R,) int32
    bbox_xyxy: object    # (R,4) float32
    cam_K: object        # (R,3,3) float32
    R: object            # (R,3,3) float32
    t: object            # (R,3) float32
    info: object         # (R,) int32: 0, or -1 for a refused row (every whole number -1, every float NaN)


def _half_bits(n: int) -> int:
    return max(1, ((n - 1).bit_length() + 1) // 2)


def _epoch_keys(seed0: int, epoch: int):
    """rk_0 .. rk_3 of include/lc_amd_sampler.h as Python ints."""
    f = _aug._fmix32
    es = f(f(seed0 & 0xFFFFFFFF) ^ np.uint64(seed0 >> 32))
    es = f(es ^ np.uint64(epoch & 0xFFFFFFFF))
    es = f(es ^ np.uint64(epoch >> 32))
    es = f(es ^ np.uint64(OP_PERM))
    return [f(es ^ np.uint64(c)) for c in ROUNDS]


def _feistel(x, k: int, rk):
    """One pass of the four-round balanced Feistel network on 2k bits over an array of uint64 values below 2^(2k)."""
    mask = np.uint64((1 << k) - 1)
    L, H = x >> np.uint64(k), x & mask
    for r in range(4):
        L, H = H, L ^ (_aug._fmix32(rk[r] ^ H) & mask)
    return (L << np.uint64(k)) | H


def _whole(name, v, lo, hi) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"lc_amd.sampler: {name} must be a whole number, got {type(v)}")
    v = int(v)
    if not lo <= v <= hi:
        raise ValueError(f"lc_amd.sampler: {name} of {lo} to {hi}, got {v}")
    return v


def permute_host(seed0, epoch, n, q=None):
    """perm(seed0, epoch) of include/lc_amd_sampler.h at the places `q` (default: all of [0, n)), as int64: the definition.  A 4-round
    balanced Feistel network on 2k bits, k = max(1, ceil(bitlength(n - 1) / 2)), whose round function is `fmix32` of the epoch's round key
    and the right half, masked to k bits; a value at or above n goes through the network again until it lies below n (cycle walking,
    which keeps a bijection of [0, 2^(2k)) a bijection of [0, n))."""
    seed0, epoch, n = _whole("seed0", seed0, 0, 2 ** 64 - 1), _whole("epoch", epoch, 0, 2 ** 64 - 1), _whole("n", n, 1, MAX_N)
    x = (np.arange(n, dtype=np.int64) if q is None else np.asarray(q, dtype=np.int64).reshape(-1)).astype(np.uint64)
    if x.size and int(x.max()) >= n:
        raise ValueError(f"lc_amd.sampler: q must lie in [0, {n})")
    k, rk = _half_bits(n), _epoch_keys(seed0, epoch)
    x = _feistel(x, k, rk)
    while True:
        walk = np.flatnonzero(x >= np.uint64(n))
        if not walk.size:
            return x.astype(np.int64)
        x[walk] = _feistel(x[walk], k, rk)


def _records(records):
    """(n, the ten host arrays or None) of what the host functions take as `records`."""
    if isinstance(records, AnnotationTable):
        records = records.host
    if isinstance(records, dict):
        if set(records) != set(FIELDS):
            raise ValueError(f"lc_amd.sampler: records holds the arrays {FIELDS}, got {sorted(records)}")
        return len(records["frame_index"]), records
    return _whole("records", records, -2 ** 31, MAX_N), None


def draw_rows_host(records, *, seed, seed0, batch, spare) -> Rows:
    """The definition of `draw_rows`, in host numpy.  `records`: an AnnotationTable, its `.host` dict, or the whole number n alone (the
    record columns are None then).  seed = the word of this step, seed0 = the word of step 0, both whole numbers below 2^64:
    step = (seed - seed0) mod 2^64.  Primary row j < batch: p = step batch + j, index = perm(seed0, p // n)(p % n).  Spare row
    j >= batch: index = (key(seed, j, OP_SPARE, 0) n) >> 32.  Every row is refused (index and the other whole numbers -1, floats NaN,
    info -1) when step >= 2^40 or n < 1; one row is refused when its record's frame, mask or mesh index is negative."""
    n, rec = _records(records)
    seed, seed0 = _whole("seed", seed, 0, 2 ** 64 - 1), _whole("seed0", seed0, 0, 2 ** 64 - 1)
    B, S = _whole("batch", batch, 1, MAX_ROWS), _whole("spare", spare, 0, MAX_ROWS)
    if B + S > MAX_ROWS:
        raise ValueError(f"lc_amd.sampler: batch + spare of at most {MAX_ROWS}, got {B + S}")
    rows = B + S
    step = (seed - seed0) % 2 ** 64
    index = np.full(rows, -1, dtype=np.int64)
    if n >= 1 and step < 2 ** MAX_STEP_BITS:
        p = [step * B + j for j in range(B)]  # Python's whole numbers: below 2^56
        for e in sorted({v // n for v in p}):
            at = [j for j in range(B) if p[j] // n == e]
            index[at] = permute_host(seed0, e, n, [p[j] % n for j in at])
        if S:
            j = np.arange(B, rows, dtype=np.int64)
            index[B:] = ((_aug.key(seed, j, OP_SPARE, 0) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    bad = index < 0
    cols = {}
    if rec is not None:
        at = np.where(bad, 0, index)
        ints = {name: np.asarray(rec[name], dtype=np.int32)[at] if n >= 1 else np.full(rows, -1, np.int32) for name in INT_FIELDS}
        bad = bad | (ints["frame_index"] < 0) | (ints["mask_index"] < 0) | (ints["mesh_index"] < 0)
        for name in INT_FIELDS:
            cols[name] = np.where(bad, -1, ints[name]).astype(np.int32)
        for name, shape in FLOAT_FIELDS:
            v = np.asarray(rec[name], dtype=np.float32).reshape((-1,) + shape)[at].copy() if n >= 1 else np.empty((rows,) + shape, np.float32)
            v[bad] = _NAN32
            cols[name] = v
    else:
        cols = {name: None for name in FIELDS}
    return Rows(np.where(bad, -1, index).astype(np.int32), *(cols[name] for name in FIELDS), np.where(bad, -1, 0).astype(np.int32))


def select_rows_host(valid_cnt, info, *, batch, valid_th):
    """The definition of `select_rows`, in host numpy: row r is GOOD when info[r] >= 0 and valid_cnt[r] >= valid_th; take[j] = j for a good
    primary (j < batch); the i-th bad primary, in row order, takes the i-th good spare (r >= batch), in row order, and -1 once the good
    spares have run out.  -> (take (batch,) int32, shortfall = the number of -1 entries)."""
    cnt, inf = np.asarray(valid_cnt).reshape(-1), np.asarray(info).reshape(-1)
    if cnt.shape != inf.shape:
        raise ValueError(f"lc_amd.sampler: valid_cnt has {cnt.size} rows and info {inf.size}")
    B = _whole("batch", batch, 1, max(1, min(MAX_ROWS, cnt.size)))
    th = _whole("valid_th", valid_th, -2 ** 31, 2 ** 31 - 1)
    good = (inf >= 0) & (cnt >= th)
    spares = [int(r) for r in np.flatnonzero(good[B:]) + B]
    take = np.arange(B, dtype=np.int32)
    bad = np.flatnonzero(~good[:B])
    for i, j in enumerate(bad):
        take[j] = spares[i] if i < len(spares) else -1
    return take, max(0, len(bad) - len(spares))


# ---- the device --------------------------------------------------------------------------------------------------------------------
_PP = ctypes.POINTER(c_void_p)
_SO = _lib.SideLibrary(_build.SAMPLER, {
    "lc_sampler_rows": (c_int, [c_void_p, c_uint64, c_int, c_int, c_int, _PP, _PP, c_void_p]),
    "lc_sampler_select_i32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "lc_sampler_take_rows": (c_int, [c_void_p, c_int, c_int, c_int, _PP, _PP, ctypes.POINTER(c_uint64), c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("sampler")


def _hip(name, t):
    if not t.is_cuda:
        raise RuntimeError(f"lc_amd.sampler: {name} is on {t.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    return t.device


def _pointers(tensors):
    return (c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


class AnnotationTable:
    """The annotations of a training set as ten resident columns, one row per instance: frame_index, mask_index, mesh_index (which frame,
    visible mask and mesh the instance reads: not negative), obj_id, scene_id, im_id (any int32: carried along) as whole numbers, bbox_xyxy
    (N,4), cam_K (N,3,3) or one (3,3) for all, R (N,3,3), t (N,3) or (N,3,1) as finite floats, rounded to float32.  Host arrays (or lists),
    validated here and uploaded once; `n_frames`, `n_masks`, `n_meshes` bound the three indices where given.  1 <= N <= MAX_N.
    `.host` keeps the validated numpy columns (what `draw_rows_host` reads), `.device` the place of the resident ones."""

    @staticmethod
    def validate(frame_index, mask_index, mesh_index, obj_id, scene_id, im_id, bbox_xyxy, cam_K, R, t, n_frames=None, n_masks=None, n_meshes=None) -> dict:
        """The checks alone, without a device: -> the ten columns as contiguous numpy arrays."""
        given = dict(frame_index=frame_index, mask_index=mask_index, mesh_index=mesh_index, obj_id=obj_id, scene_id=scene_id, im_id=im_id)
        cols, N = {}, None
        for name, v in given.items():
            if isinstance(v, Tensor):
                raise TypeError(f"lc_amd.sampler: {name} is a host array that is uploaded here once, got a torch.Tensor")
            a = np.asarray(v)
            if a.dtype.kind not in "iu" or a.dtype == np.bool_:
                raise TypeError(f"lc_amd.sampler: {name} must hold whole numbers, got {a.dtype}")
            if a.ndim != 1:
                raise ValueError(f"lc_amd.sampler: {name} has shape {a.shape}, expected (N,)")
            N = a.shape[0] if N is None else N
            if a.shape[0] != N:
                raise ValueError(f"lc_amd.sampler: {name} has {a.shape[0]} rows, frame_index has {N}")
            if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1):
                raise ValueError(f"lc_amd.sampler: {name} must fit int32")
            cols[name] = np.ascontiguousarray(a.astype(np.int32))
        if not 1 <= N <= MAX_N:
            raise ValueError(f"lc_amd.sampler: a table of 1 to {MAX_N} annotations, got {N}")
        for name, bound, limit in (("frame_index", "n_frames", n_frames), ("mask_index", "n_masks", n_masks), ("mesh_index", "n_meshes", n_meshes)):
            if limit is not None:
                limit = _whole(bound, limit, 1, 2 ** 31 - 1)
            lo, hi = int(cols[name].min()), int(cols[name].max())
            if lo < 0 or (limit is not None and hi >= limit):
                raise ValueError(f"lc_amd.sampler: {name} must lie in [0, {'2^31' if limit is None else limit}), got {lo} to {hi}")
        floats = dict(bbox_xyxy=bbox_xyxy, cam_K=cam_K, R=R, t=t)
        for name, shape in FLOAT_FIELDS:
            v = floats[name]
            if isinstance(v, Tensor):
                raise TypeError(f"lc_amd.sampler: {name} is a host array that is uploaded here once, got a torch.Tensor")
            a = np.asarray(v)
            if a.dtype.kind not in "fiu" or a.dtype == np.bool_:
                raise TypeError(f"lc_amd.sampler: {name} must hold numbers, got {a.dtype}")
            if name == "cam_K" and a.shape == (3, 3):
                a = np.broadcast_to(a, (N, 3, 3))
            if name == "t" and a.shape == (N, 3, 1):
                a = a.reshape(N, 3)
            if a.shape != (N,) + shape:
                raise ValueError(f"lc_amd.sampler: {name} has shape {a.shape}, expected {(N,) + shape}")
            with np.errstate(over="ignore"):
                a = np.ascontiguousarray(a.astype(np.float32))
            if not np.isfinite(a).all():
                raise ValueError(f"lc_amd.sampler: {name} must be finite (as float32)")
            cols[name] = a
        return cols

    def __init__(self, frame_index, mask_index, mesh_index, obj_id, scene_id, im_id, bbox_xyxy, cam_K, R, t, *, device, n_frames=None, n_masks=None, n_meshes=None):
        self.host = self.validate(frame_index, mask_index, mesh_index, obj_id, scene_id, im_id, bbox_xyxy, cam_K, R, t, n_frames, n_masks, n_meshes)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"lc_amd.sampler: the table lives on a HIP device, got {dev} (there is no CPU fallback in the product path)")
        self.N, self.device = len(self.host["frame_index"]), dev
        self.columns = {name: torch.from_numpy(self.host[name]).to(dev) for name in FIELDS}
        self.device = self.columns["frame_index"].device
        self._table = _pointers([self.columns[name] for name in FIELDS])

    def __len__(self):
        return self.N


def _seed_arg(seed):
    """`augment._seed_word`'s rule on the seed's type, ahead of the device: a whole number below 2^64, or one 64-bit element."""
    if not isinstance(seed, Tensor):
        _A.whole("seed", seed, 0, 2 ** 64 - 1, numpy=True)
    elif seed.dtype not in (torch.uint64, torch.int64) or seed.numel() != 1:
        raise TypeError(f"lc_amd.sampler: a seed tensor holds one uint64 or int64 element, got {seed.dtype} of shape {tuple(seed.shape)}")


@torch.no_grad()
def draw_rows(table: AnnotationTable, *, seed, seed0, batch, spare) -> Rows:
    """`draw_rows_host(table, seed=<the word>, seed0=seed0, batch=batch, spare=spare)` as device tensors, bit for bit, in one launch
    (`lc_sampler_rows`).  seed: a whole number below 2^64, or a device tensor of one uint64 / int64 element that the KERNEL reads (the
    word of the whole chain: `seed.add_(1)` is the next step); seed0: the whole number below 2^64 that the word held at step 0;
    1 <= batch, 0 <= spare, batch + spare <= MAX_ROWS.  A refused row (step >= 2^40; a negative frame, mask or mesh index in the
    resident record) has info = -1; nothing is read back to find out."""
    if not isinstance(table, AnnotationTable):
        raise TypeError(f"lc_amd.sampler: table must be an AnnotationTable, got {type(table)}")
    _seed_arg(seed)
    seed0 = _A.whole("seed0", seed0, 0, 2 ** 64 - 1, numpy=True)
    B, S = _A.whole("batch", batch, 1, MAX_ROWS, numpy=True), _A.whole("spare", spare, 0, MAX_ROWS, numpy=True)
    if B + S > MAX_ROWS:
        raise ValueError(f"lc_amd.sampler: batch + spare of at most {MAX_ROWS}, got {B + S}")
    dev = table.device
    if isinstance(seed, Tensor) and seed.device != dev:
        raise RuntimeError(f"lc_amd.sampler: seed is on {seed.device}, the table on {dev}")
    word = _aug._seed_word(seed, dev)
    rows = B + S

    def made(*shape, dtype=torch.int32):
        return torch.empty((rows,) + shape, device=dev, dtype=dtype)

    out = Rows(made(), *(made() for _ in INT_FIELDS), *(made(*shape, dtype=torch.float32) for _, shape in FLOAT_FIELDS), made())
    with _lib.on_device(dev):
        rc = load().lc_sampler_rows(_lib.ptr(word), seed0, table.N, B, S, table._table, _pointers(list(out)), _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("sampler.draw_rows", rc)
    return out


@torch.no_grad()
def select_rows(valid_cnt, info, *, batch, valid_th):
    """`select_rows_host` on the device, one launch of one workgroup (`lc_sampler_select_i32`): valid_cnt and info (R,) int32 of the R
    drawn rows (1 <= R <= MAX_ROWS), 1 <= batch <= R, valid_th any int32.  -> (take (batch,) int32, shortfall (1,) int32), the same numbers
    at every run: ordered scans, no atomics."""
    valid_cnt = _A.tensor("valid_cnt", valid_cnt, (torch.int32,), "int32", (None,))
    R = int(valid_cnt.shape[0])
    info = _A.tensor("info", info, (torch.int32,), "int32", (R,))
    if not 1 <= R <= MAX_ROWS:
        raise ValueError(f"lc_amd.sampler: 1 to {MAX_ROWS} rows, got {R}")
    B = _A.whole("batch", batch, 1, R, numpy=True)
    th = _A.whole("valid_th", valid_th, -2 ** 31, 2 ** 31 - 1, numpy=True)
    dev = _hip("valid_cnt", valid_cnt)
    _A.same_device(dev, "valid_cnt on {}", info=info)
    cnt, inf = valid_cnt.contiguous(), info.contiguous()
    take, shortfall = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(1, device=dev, dtype=torch.int32)
    with _lib.on_device(dev):
        rc = load().lc_sampler_select_i32(_lib.ptr(cnt), _lib.ptr(inf), th, B, R, _lib.ptr(take), _lib.ptr(shortfall), _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("sampler.select_rows", rc)
    return take, shortfall


@torch.no_grad()
def take_rows(take, *tensors, out=None) -> tuple:
    """tensors[k][take[j]] for every j, for any number of tensors of R rows each (any element type, at least one dimension, contiguous
    rows -- a tensor that is not contiguous is copied into shape first), `lc_sampler_take_rows`: one launch per MAX_TENSORS tensors, their
    pointers and row sizes in the launch's argument.  take (B,) int32; an entry outside [0, R) gives a row of zero bytes (False, 0, 0.0).
    `out`: a tuple of contiguous tensors of B rows to write into (none may share memory with a source).  -> a tuple of (B, ...) tensors."""
    take = _A.tensor("take", take, (torch.int32,), "int32", (None,))
    B = int(take.shape[0])
    if not 1 <= B <= MAX_ROWS:
        raise ValueError(f"lc_amd.sampler: take holds 1 to {MAX_ROWS} rows, got {B}")
    if not tensors:
        raise ValueError("lc_amd.sampler: take_rows needs at least one tensor")
    R = None
    for k, t in enumerate(tensors):
        if not isinstance(t, Tensor):
            raise TypeError(f"lc_amd.sampler: tensors[{k}] must be a torch.Tensor, got {type(t)}")
        if t.dim() < 1:
            raise ValueError(f"lc_amd.sampler: tensors[{k}] has no rows")
        R = int(t.shape[0]) if R is None else R
        if int(t.shape[0]) != R:
            raise ValueError(f"lc_amd.sampler: tensors[{k}] has {int(t.shape[0])} rows, tensors[0] has {R}")
    if not 1 <= R <= MAX_ROWS:
        raise ValueError(f"lc_amd.sampler: tensors of 1 to {MAX_ROWS} rows, got {R}")
    row_bytes = [t[0].numel() * t.element_size() for t in tensors]
    for k, nb in enumerate(row_bytes):
        if not 1 <= nb <= MAX_ROW_BYTES:
            raise ValueError(f"lc_amd.sampler: tensors[{k}] has rows of {nb} bytes, expected 1 to {MAX_ROW_BYTES}")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != len(tensors):
            raise ValueError(f"lc_amd.sampler: out holds one tensor per source, {len(tensors)}")
        for k, (o, t) in enumerate(zip(out, tensors)):
            _A.tensor(f"out[{k}]", o, (t.dtype,), str(t.dtype), (B,) + tuple(t.shape[1:]), str((B,) + tuple(t.shape[1:])))
            if not o.is_contiguous():
                raise ValueError(f"lc_amd.sampler: out[{k}] must be contiguous, got strides {tuple(o.stride())}")
    dev = _hip("take", take)
    _A.same_device(dev, "take on {}", **{f"tensors[{k}]": t for k, t in enumerate(tensors)}, **{f"out[{k}]": o for k, o in enumerate(out or ())})
    take = take.contiguous()
    src = [t.contiguous() for t in tensors]
    dst = list(out) if out is not None else [torch.empty((B,) + tuple(t.shape[1:]), device=dev, dtype=t.dtype) for t in src]
    lib = load()
    with _lib.on_device(dev):
        for a in range(0, len(src), MAX_TENSORS):
            n = min(MAX_TENSORS, len(src) - a)
            rc = lib.lc_sampler_take_rows(_lib.ptr(take), B, R, n, _pointers(src[a:a + n]), _pointers(dst[a:a + n]), (c_uint64 * n)(*row_bytes[a:a + n]),
                                          _lib.stream_ptr(dev))
            if rc != 0:
                _SO.fail("sampler.take_rows", rc)
    return tuple(dst)
