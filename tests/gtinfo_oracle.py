"""fp64 numpy restatement of the annotation record's and the scene composition's contracts (TEST INFRASTRUCTURE ONLY;
include/lc_amd_gtinfo.h states them, lc_amd/csrc/gtinfo/lc_gtinfo.hip holds the kernels).

    record(depth_gt, depth_test, K, delta, origin_xy=None, pixel_center=(0, 0)) -> Ref(info, mask_visib, obj, margin)
    compose(depth_inst, scene_index, frame_hw, n_scenes, origins=None)          -> Composed(depth, instance, info)
    torch_statement(...)                                                         the record as batched float64 torch, for scripts/bench_gtinfo.py

`record` is one instance: depth_gt is its (h,w) window, depth_test the whole (H,W) frame of its scene, origin_xy where the window lies
(None: (0,0), and the window has the frame's size).  delta is rounded to fp32 first (what the C ABI takes) and every operation is a numpy
fp64 operation of its own, in the header's order.  Every output is an integer or a byte: the device must give EQUAL values.  That is a
fair demand wherever no comparison `d_gt n - d_test n <= delta` is decided by the last bits of n, whose division and square root the
kernel may round differently from numpy:

    margin    the smallest relative distance |lhs - delta| / max(|delta|, tiny) of the consulted comparisons at pixels whose ray length
              is not exactly 1.  Where n = 1 exactly (Xk = Yk = 0: the principal-point pixel of a camera whose principal point is whole)
              both products are exact and the difference is one correctly rounded fp64 subtraction on either side, so those pixels may
              sit ON the threshold; tests/test_gtinfo_oracle.py demands 2^-30 of every case elsewhere.  Two more kinds of pixel are
              left out because no rounding of n can decide them: d_gt = d_test bit for bit (the two products are the same number, the
              difference 0: a scene composed from the very renders it is compared with), and a difference that is not finite (an
              infinite depth).  1.0 where nothing is compared.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

TINY = 1e-300
COLUMNS = 12
MAX_ORIGIN = 1 << 24


class Ref(NamedTuple):
    info: np.ndarray        # (12,) int32
    mask_visib: np.ndarray  # (h,w) uint8, window coordinates
    obj: np.ndarray         # (h,w) bool
    margin: float


class Composed(NamedTuple):
    depth: np.ndarray     # (S,H,W) float32
    instance: np.ndarray  # (S,H,W) int32
    info: np.ndarray      # (B,) int32


def ray_length(K, xs, ys, pixel_center=(0.0, 0.0)):
    """Step 1 of the header at the frame columns xs and rows ys (integers): n (len(ys), len(xs)) fp64."""
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    pcx, pcy = (float(np.float32(c)) for c in pixel_center)
    px = np.asarray(xs, dtype=np.int64).astype(np.float64) + pcx
    px = px - K[0, 2]
    py = np.asarray(ys, dtype=np.int64).astype(np.float64) + pcy
    py = py - K[1, 2]
    with np.errstate(all="ignore"):
        Yk = (py / K[1, 1])[:, None]
        kY = K[0, 1] * Yk
        num = px[None, :] - kY
        Xk = num / K[0, 0]
        xx = Xk * Xk
        yy = Yk * Yk
        s = xx + yy
        s = s + 1.0
        return np.sqrt(s)


def _box(m, x0, y0):
    if not m.any():
        return [-1, -1, -1, -1]
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    return [int(xs[0]) + x0, int(ys[0]) + y0, int(xs[-1]) + x0, int(ys[-1]) + y0]


def record(depth_gt, depth_test, K, delta, origin_xy=None, pixel_center=(0.0, 0.0)) -> Ref:
    dg32, dt32 = np.asarray(depth_gt, dtype=np.float32), np.asarray(depth_test, dtype=np.float32)
    h, w = dg32.shape
    H, W = dt32.shape
    if origin_xy is None:
        assert (h, w) == (H, W)
        x0 = y0 = 0
    else:
        x0, y0 = int(origin_xy[0]), int(origin_xy[1])
    delta = float(np.float32(delta))
    with np.errstate(invalid="ignore"):
        obj = dg32 > 0
    # the part of the window that lies in the frame: window rows ya:yb and columns xa:xb
    xa, xb = min(max(-x0, 0), w), max(min(W - x0, w), 0)
    ya, yb = min(max(-y0, 0), h), max(min(H - y0, h), 0)
    visib = np.zeros((h, w), dtype=bool)
    valid = np.zeros((h, w), dtype=bool)
    margin = 1.0
    if xb > xa and yb > ya:
        g = dg32[ya:yb, xa:xb]
        t = dt32[ya + y0:yb + y0, xa + x0:xb + x0]
        n = ray_length(K, np.arange(xa, xb) + x0, np.arange(ya, yb) + y0, pixel_center)
        with np.errstate(all="ignore"):
            o = g > 0
            missing = ~(t > 0)
            dist_g = g.astype(np.float64) * n
            dist_t = t.astype(np.float64) * n
            over = dist_g - dist_t
            vis = o & (missing | (over <= delta))
            consulted = o & ~missing & (n != 1.0) & (g != t) & np.isfinite(over)
            if consulted.any():
                margin = float((np.abs(over[consulted] - delta) / max(abs(delta), TINY)).min())
        visib[ya:yb, xa:xb] = vis
        valid[ya:yb, xa:xb] = o & ~missing
    border = np.zeros((h, w), dtype=bool)
    border[0, :] = border[-1, :] = True
    border[:, 0] = border[:, -1] = True
    info = np.asarray([obj.sum(), valid.sum(), visib.sum(), (obj & border).sum(), *_box(obj, x0, y0), *_box(visib, x0, y0)], dtype=np.int32)
    return Ref(info, visib.astype(np.uint8), obj, margin)


def refused(scene, n_scenes, origin_xy=None) -> bool:
    """The rows the device refuses (the record) or skips (the composition)."""
    if not 0 <= int(scene) < n_scenes:
        return True
    return origin_xy is not None and (abs(int(origin_xy[0])) > MAX_ORIGIN or abs(int(origin_xy[1])) > MAX_ORIGIN)


def records(depth_gt, depth_test, K, delta, scene_index, origins=None, pixel_center=(0.0, 0.0)):
    """A batch: (info (B,12) int32, mask_visib (B,h,w) uint8, smallest margin); a refused row is -1 and a zero mask.  K (3,3) or (B,3,3)."""
    depth_gt, depth_test, K = np.asarray(depth_gt), np.asarray(depth_test), np.asarray(K)
    B, S = len(depth_gt), len(depth_test)
    info, mask, margin = np.full((B, COLUMNS), -1, np.int32), np.zeros(depth_gt.shape, np.uint8), 1.0
    for b in range(B):
        o = None if origins is None else origins[b]
        if refused(scene_index[b], S, o):
            continue
        r = record(depth_gt[b], depth_test[int(scene_index[b])], K if K.ndim == 2 else K[b], delta, o, pixel_center)
        info[b], mask[b], margin = r.info, r.mask_visib, min(margin, r.margin)
    return info, mask, margin


def compose(depth_inst, scene_index, frame_hw, n_scenes, origins=None) -> Composed:
    """The smallest (fp32 bits of z, row) pair per frame pixel, as one uint64 key, exactly as the header states it."""
    d = np.asarray(depth_inst, dtype=np.float32)
    B, h, w = d.shape
    H, W = frame_hw
    keys = np.full((n_scenes, H, W), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    info = np.zeros(B, dtype=np.int32)
    for b in range(B):
        o = None if origins is None else origins[b]
        if refused(scene_index[b], n_scenes, o):
            info[b] = -1
            continue
        x0, y0 = (0, 0) if o is None else (int(o[0]), int(o[1]))
        xa, xb = min(max(-x0, 0), w), max(min(W - x0, w), 0)
        ya, yb = min(max(-y0, 0), h), max(min(H - y0, h), 0)
        if xb <= xa or yb <= ya:
            continue
        z = d[b, ya:yb, xa:xb]
        with np.errstate(invalid="ignore"):
            hit = (z > 0) & (z < np.inf)
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(b)
        view = keys[int(scene_index[b]), ya + y0:yb + y0, xa + x0:xb + x0]
        np.minimum(view, np.where(hit, key, np.uint64(0xFFFFFFFFFFFFFFFF)), out=view)
    hit = keys != np.uint64(0xFFFFFFFFFFFFFFFF)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    instance = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return Composed(depth, instance, info)


def torch_statement(depth_gt, depth_test, K, delta, scene_index, origin_xy=None, pixel_center=(0.0, 0.0)):
    """The record as batched float64 torch on whatever device the tensors live on (scripts/bench_gtinfo.py times it on the GPU next to
    the kernel; tests/test_gtinfo_oracle.py holds it to `records` on the CPU).  -> (info (B,12) int32, mask_visib (B,h,w) uint8).
    Every row must be valid."""
    import torch

    B, h, w = depth_gt.shape
    S, H, W = depth_test.shape
    dev = depth_gt.device
    Kd = K.double()
    x0 = origin_xy[:, 0].long() if origin_xy is not None else torch.zeros(B, dtype=torch.long, device=dev)
    y0 = origin_xy[:, 1].long() if origin_xy is not None else torch.zeros(B, dtype=torch.long, device=dev)
    xs = torch.arange(w, device=dev)[None, :] + x0[:, None]   # (B,w) frame columns
    ys = torch.arange(h, device=dev)[None, :] + y0[:, None]   # (B,h)
    px = xs.double() + float(pixel_center[0])
    px = px - Kd[:, 0, 2, None]
    py = ys.double() + float(pixel_center[1])
    py = py - Kd[:, 1, 2, None]
    Yk = (py / Kd[:, 1, 1, None])[:, :, None]
    kY = Kd[:, 0, 1, None, None] * Yk
    num = px[:, None, :] - kY
    Xk = num / Kd[:, 0, 0, None, None]
    xx = Xk * Xk
    yy = Yk * Yk
    s = xx + yy
    s = s + 1.0
    n = torch.sqrt(s)
    inside = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :]
    dt = depth_test[scene_index.long()[:, None, None], ys.clamp(0, H - 1)[:, :, None], xs.clamp(0, W - 1)[:, None, :]]
    obj = depth_gt > 0
    present = dt > 0
    dl = float(torch.tensor(delta, dtype=torch.float32))
    over = depth_gt.double() * n - dt.double() * n
    valid = obj & inside & present
    visib = obj & inside & (~present | (over <= dl))
    border = torch.zeros(h, w, dtype=torch.bool, device=dev)
    border[0, :] = border[-1, :] = True
    border[:, 0] = border[:, -1] = True
    big = 1 << 30

    def box(m):
        mx, my = m.any(1), m.any(2)  # (B,w), (B,h)
        some = mx.any(1)
        x_lo = torch.where(mx, xs, xs.new_full((), big)).amin(1)
        x_hi = torch.where(mx, xs, xs.new_full((), -big)).amax(1)
        y_lo = torch.where(my, ys, ys.new_full((), big)).amin(1)
        y_hi = torch.where(my, ys, ys.new_full((), -big)).amax(1)
        out = torch.stack((x_lo, y_lo, x_hi, y_hi), -1)
        return torch.where(some[:, None], out, out.new_full((), -1))

    counts = torch.stack((obj.flatten(1).sum(1), valid.flatten(1).sum(1), visib.flatten(1).sum(1), (obj & border).flatten(1).sum(1)), -1)
    return torch.cat((counts, box(obj), box(visib)), 1).to(torch.int32), visib.to(torch.uint8)
