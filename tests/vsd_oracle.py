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

`pixels` is steps 2 to 4 on maps of any one shape, with each comparison's left side and its margin pixel by pixel (0: a tie) and the three
predicates `<= delta`, `>= tau d` and `d > 0` as arguments: `score` is built on it, tests/test_vsd_oracle.py restates the kernel's launch
shape with it, strip by strip, and plants its mistakes through it.
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


class Pixels(NamedTuple):
    """Steps 2 to 4 pixel by pixel, for the tests that restate the kernel's launch shape or plant a mistake in a comparison."""
    hit: np.ndarray      # est or gt hits: the pixels that edge counts on a cut side
    vis_gt: np.ndarray
    vis_est: np.ndarray
    costly: np.ndarray   # (T,) + shape: the cost predicates, inside the intersection only
    lhs_gt: np.ndarray   # dist_gt - dist_test, dist_est - dist_test and |dist_gt - dist_est|: the left sides of the three comparisons
    lhs_est: np.ndarray
    lhs_cost: np.ndarray
    margin_gt: np.ndarray    # the relative distance of each DECIDED comparison to its threshold, inf where it is not consulted: 0 is a tie
    margin_est: np.ndarray
    margin_cost: np.ndarray  # (T,) + shape


def pixels(de32, dg32, dt32, n, delta, thr, dist_dtype=np.float64, le=np.less_equal, ge=np.greater_equal, hit=lambda d: d > 0) -> Pixels:
    """Steps 2 to 4 on float32 maps of one shape (dt32: the scene's depth under the window) with the ray lengths `n`; delta and thr
    (= tau_k d) are fp64 values of fp32 numbers.  `le`, `ge` and `hit` are the contract's `<= delta`, `>= tau_k d` and `d > 0`: a test
    passes another to state a mistake."""
    with np.errstate(invalid="ignore"):
        he, hg, missing = hit(de32), hit(dg32), ~(dt32 > 0)
        dist_e = (de32.astype(np.float64) * n).astype(dist_dtype).astype(np.float64)
        dist_g = (dg32.astype(np.float64) * n).astype(dist_dtype).astype(np.float64)
        dist_t = (dt32.astype(np.float64) * n).astype(dist_dtype).astype(np.float64)
        over_g = dist_g - dist_t
        over_e = dist_e - dist_t
        vis_g = hg & (missing | le(over_g, delta))
        vis_e = he & (missing | le(over_e, delta) | vis_g)
        inter = vis_g & vis_e
        diff = np.abs(dist_g - dist_e)
        costly = np.stack([inter & ge(diff, t) for t in thr])
        # (the kernel evaluates est's comparison whether or not vis_gt then settles the pixel)
        m_g = np.where(hg & ~missing, _rel(over_g, delta), np.inf)
        m_e = np.where(he & ~missing, _rel(over_e, delta), np.inf)
        m_c = np.stack([np.where(inter, _rel(diff, t), np.inf) for t in thr])
    return Pixels(he | hg, vis_g, vis_e, costly, over_g, over_e, diff, m_g, m_e, m_c)


def cut_sides(hw, frame_hw, window_xy=(0, 0)):
    """The pixels of the window's border on a side that is not the frame's own: where a hit counts as edge."""
    (h, w), (H, W), (x0, y0) = hw, frame_hw, window_xy
    border = np.zeros((h, w), dtype=bool)
    if x0 > 0:
        border[:, 0] = True
    if x0 + w < W:
        border[:, -1] = True
    if y0 > 0:
        border[0, :] = True
    if y0 + h < H:
        border[-1, :] = True
    return border


def errors_of(counts):
    """Step 5: (T,) float32 from one pose's (T+3,) counts."""
    nu, ni = int(counts[0]), int(counts[1])
    return np.asarray([1.0 if nu == 0 else np.float64(int(c) + nu - ni) / np.float64(nu) for c in counts[3:]], dtype=np.float64).astype(np.float32)


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
    p = pixels(de32, dg32, dt32, n, delta, taus * diam, dist_dtype)
    union, inter = p.vis_gt | p.vis_est, p.vis_gt & p.vis_est
    edge = (cut_sides((h, w), (H, W), (x0, y0)) & p.hit).sum()
    counts = np.asarray([union.sum(), inter.sum(), edge, *(m.sum() for m in p.costly)], dtype=np.int32)
    margin = min(1.0, float(p.margin_gt.min()), float(p.margin_est.min()), float(p.margin_cost.min()))
    return Ref(counts, errors_of(counts), margin, p.vis_gt, p.vis_est, np.stack([p.vis_gt, p.vis_est, *p.costly], -1))


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
