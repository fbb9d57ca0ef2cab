"""fp64 numpy restatement of the VSD score's contract (TEST INFRASTRUCTURE ONLY; include/lc_amd_vsd.h states the contract,
lc_amd/csrc/vsd/lc_vsd.hip is the kernel): BOP's pose_error.vsd with visib_mode='bop19' and cost_type='step'.

    score(depth_est, depth_gt, depth_test, K, delta, taus, diameter=None, window_xy=(0, 0), pixel_center=(0, 0)) -> Ref

One pose per call.  depth_est / depth_gt are (h,w), depth_test the whole (H,W) frame; delta, taus and diameter are rounded to fp32 first
(what the C ABI takes) and every operation is a numpy fp64 operation of its own.  Besides counts and errors the oracle returns

    margin    the smallest relative distance |lhs - rhs| / max(|rhs|, tiny) of any decided comparison of steps 2 to 4 to its threshold:
              dist_gt - dist_test <= delta and dist_est - dist_test <= delta wherever they are consulted, |dist_gt - dist_est| >= tau_k d on
              every pixel of the intersection.  The kernel's square root and division may differ from numpy's in the last fp64 bits; a case
              must keep 2^-30 clear (tests/test_vsd_oracle.py), so that no such difference can decide a pixel.  1.0 where nothing is compared.
    vis_gt, vis_est    the masks, for the tests that reason about single pixels
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

TINY = 1e-300


class Ref(NamedTuple):
    counts: np.ndarray   # (T+3,) int32: union, inter, edge, cost_0 ..
    errors: np.ndarray   # (T,) float32
    margin: float
    vis_gt: np.ndarray   # (h,w) bool
    vis_est: np.ndarray  # (h,w) bool
    decided: np.ndarray  # (h,w,T+2) bool: vis_gt, vis_est and the T cost predicates of every pixel


def ray_length(K, hw, window_xy=(0, 0), pixel_center=(0.0, 0.0)):
    """Step 1: n (h,w) fp64."""
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    h, w = hw
    pcx, pcy = (float(np.float32(c)) for c in pixel_center)
    xs = np.arange(w, dtype=np.int64) + int(window_xy[0])
    ys = np.arange(h, dtype=np.int64) + int(window_xy[1])
    px = xs.astype(np.float64) + pcx
    px = px - K[0, 2]
    py = ys.astype(np.float64) + pcy
    py = py - K[1, 2]
    Y = (py / K[1, 1])[:, None]
    kY = K[0, 1] * Y
    num = px[None, :] - kY
    X = num / K[0, 0]
    xx = X * X
    yy = Y * Y
    s = xx + yy
    s = s + 1.0
    return np.sqrt(s)


def _rel(lhs, rhs):
    return np.abs(lhs - rhs) / np.maximum(np.abs(rhs), TINY)


def score(depth_est, depth_gt, depth_test, K, delta, taus, diameter=None, window_xy=(0, 0), pixel_center=(0.0, 0.0), dist_dtype=np.float64) -> Ref:
    """dist_dtype=np.float32 rounds the three distance images to fp32 before they are subtracted, as BOP's Python does (the first of the
    two deliberate differences of include/lc_amd_vsd.h): `flipped_pixels` counts the pixels that this decides."""
    de32, dg32, dt32 = (np.asarray(a, dtype=np.float32) for a in (depth_est, depth_gt, depth_test))
    h, w = de32.shape
    H, W = dt32.shape
    x0, y0 = int(window_xy[0]), int(window_xy[1])
    assert dg32.shape == (h, w) and 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
    dt32 = dt32[y0:y0 + h, x0:x0 + w]
    delta = float(np.float32(delta))
    taus = np.asarray(taus, dtype=np.float32).astype(np.float64)
    diam = 1.0 if diameter is None else float(np.float32(diameter))
    n = ray_length(K, (h, w), (x0, y0), pixel_center)
    with np.errstate(invalid="ignore"):
        he, hg, missing = de32 > 0, dg32 > 0, ~(dt32 > 0)
        dist_e = (de32.astype(np.float64) * n).astype(dist_dtype).astype(np.float64)
        dist_g = (dg32.astype(np.float64) * n).astype(dist_dtype).astype(np.float64)
        dist_t = (dt32.astype(np.float64) * n).astype(dist_dtype).astype(np.float64)
        over_g = dist_g - dist_t
        over_e = dist_e - dist_t
        vis_g = hg & (missing | (over_g <= delta))
        vis_e = he & (missing | (over_e <= delta) | vis_g)
    union, inter = vis_g | vis_e, vis_g & vis_e
    diff = np.abs(dist_g - dist_e)
    thr = taus * diam
    costly = [inter & (diff >= t) for t in thr]
    cost = [m.sum() for m in costly]
    border = np.zeros((h, w), dtype=bool)
    if x0 > 0:
        border[:, 0] = True
    if x0 + w < W:
        border[:, -1] = True
    if y0 > 0:
        border[0, :] = True
    if y0 + h < H:
        border[-1, :] = True
    edge = (border & (he | hg)).sum()
    counts = np.asarray([union.sum(), inter.sum(), edge, *cost], dtype=np.int32)
    nu, ni = int(counts[0]), int(counts[1])
    errors = np.asarray([1.0 if nu == 0 else np.float64(int(c) + nu - ni) / np.float64(nu) for c in counts[3:]], dtype=np.float64).astype(np.float32)
    margins = [1.0]
    consulted_g = hg & ~missing
    consulted_e = he & ~missing  # (the kernel evaluates it whether or not vis_gt then settles the pixel)
    if consulted_g.any():
        margins.append(float(_rel(over_g[consulted_g], delta).min()))
    if consulted_e.any():
        margins.append(float(_rel(over_e[consulted_e], delta).min()))
    if inter.any():
        margins.append(float(min(_rel(diff[inter], t).min() for t in thr)))
    return Ref(counts, errors, min(margins), vis_g, vis_e, np.stack([vis_g, vis_e, *costly], -1))


def flipped_pixels(*args, **kw) -> int:
    """The number of pixels on which rounding the distance images to fp32 first (BOP's Python) decides vis_gt, vis_est or a cost predicate
    otherwise than the fp64 differences of this project's definition.  Arguments as `score`."""
    a, b = score(*args, **kw), score(*args, dist_dtype=np.float32, **kw)
    return int((a.decided != b.decided).any(-1).sum())


def torch_statement(depth_est, depth_gt, depth_test, K, delta, taus, diameter, scene_index, window_xy, pixel_center=(0.0, 0.0)):
    """The same definition as batched float64 torch on whatever device the tensors live on (scripts/bench_vsd.py times it on the GPU
    next to the kernel; tests/test_vsd_oracle.py holds it to `score` on the CPU).  -> (counts (B,T+3) int32, errors (B,T) float32).
    Every row must be valid."""
    import torch

    B, h, w = depth_est.shape
    dev = depth_est.device
    Kd = K.double()
    x0 = window_xy[:, 0].long() if window_xy is not None else torch.zeros(B, dtype=torch.long, device=dev)
    y0 = window_xy[:, 1].long() if window_xy is not None else torch.zeros(B, dtype=torch.long, device=dev)
    xs = torch.arange(w, device=dev)[None, :] + x0[:, None]
    ys = torch.arange(h, device=dev)[None, :] + y0[:, None]
    px = xs.double() + float(pixel_center[0])
    px = px - Kd[:, 0, 2, None]
    py = ys.double() + float(pixel_center[1])
    py = py - Kd[:, 1, 2, None]
    Y = (py / Kd[:, 1, 1, None])[:, :, None]
    kY = Kd[:, 0, 1, None, None] * Y
    num = px[:, None, :] - kY
    X = num / Kd[:, 0, 0, None, None]
    xx = X * X
    yy = Y * Y
    s = xx + yy
    s = s + 1.0
    n = torch.sqrt(s)
    dt = depth_test[scene_index.long()[:, None, None], ys[:, :, None], xs[:, None, :]]
    he, hg, missing = depth_est > 0, depth_gt > 0, ~(dt > 0)
    dist_e, dist_g, dist_t = depth_est.double() * n, depth_gt.double() * n, dt.double() * n
    dl = float(torch.tensor(delta, dtype=torch.float32))
    vis_g = hg & (missing | (dist_g - dist_t <= dl))
    vis_e = he & (missing | (dist_e - dist_t <= dl) | vis_g)
    union, inter = (vis_g | vis_e).flatten(1).sum(1), vis_g & vis_e
    diff = (dist_g - dist_e).abs()
    d = torch.ones(B, dtype=torch.float64, device=dev) if diameter is None else diameter.double()
    taus = taus if isinstance(taus, torch.Tensor) else torch.tensor(taus, dtype=torch.float32, device=dev)  # (a tensor already on the device: no copy, capturable)
    thr = taus.double()[None, :] * d[:, None]
    cost = (inter[:, None] & (diff[:, None] >= thr[:, :, None, None])).flatten(2).sum(2)
    ni = inter.flatten(1).sum(1)
    err = torch.where(union[:, None] == 0, torch.ones((), dtype=torch.float64, device=dev), (cost + union[:, None] - ni[:, None]).double() / union[:, None].double())
    H, W = depth_test.shape[1:]
    cut_x = ((xs == x0[:, None]) & (x0[:, None] > 0)) | ((xs == x0[:, None] + w - 1) & (x0[:, None] + w < W))   # (B,w)
    cut_y = ((ys == y0[:, None]) & (y0[:, None] > 0)) | ((ys == y0[:, None] + h - 1) & (y0[:, None] + h < H))   # (B,h)
    edge = ((cut_y[:, :, None] | cut_x[:, None, :]) & (he | hg)).flatten(1).sum(1)
    counts = torch.cat((union[:, None], ni[:, None], edge[:, None], cost), 1).to(torch.int32)
    return counts, err.float()
