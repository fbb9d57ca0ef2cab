#!/usr/bin/env python3
"""Times the zoom-in crops (lc_amd.crops.warp_affine) on the GPU and writes profiles/crops/bench_crops.json.

    python scripts/bench_crops.py [--iters 200] [--warmup 20] [--out profiles/crops/bench_crops.json]

Every variant is captured in a graph after a warm-up and replayed; a time is the median over `--iters` replays timed one by one with
device events (p10 / p90 beside it).  Shapes: 64 crops of 256 x 256 x 3 cut from ONE 480 x 640 frame (64 detections of a frame) and
from 64 frames (one detection each); outputs float32 and bfloat16, each with and without `normalize`.

`written_GBps` is the bytes of the output over the median time, `share_of_8TBps` that rate against the 8 TB/s of HBM (the output is
what has to reach memory; the frames are read through the caches, at most 4 taps x 3 bytes per pixel).  `torch_*` is what a user
of torch can do on the device today: the frames as float32 planes, `affine_grid` + `grid_sample` (bilinear, zero padding), a division
by 255 and the normalisation -- in a graph as well; its result is NOT the fixed-point scheme's (float weights), so only its time
is compared.  `h2d_bytes` counts, from the shapes, what crosses PCIe per batch: the reference's route ships every crop as float32,
this one ships the frames as uint8, the matrices and the frame index.
Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import crops  # noqa: E402
from tests import crops_cases as cc  # noqa: E402

B, HW_OUT, HW_FRAME = 64, (256, 256), (480, 640)
HBM_GBPS = 8000.0


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)))


def boxes(rng, n):
    """n detection boxes inside the frame: (M (n,2,3) forward, float32)."""
    H, W = HW_FRAME
    Ms = []
    for _ in range(n):
        side = rng.uniform(60, 260)
        c = (rng.uniform(side / 2, W - side / 2), rng.uniform(side / 2, H - side / 2))
        Ms.append(crops.affine_from_box(c, side * 1.5, 0.0, (HW_OUT[1], HW_OUT[0]))[0])
    return np.stack(Ms)


def torch_route(planes, theta, idx, mean, std, dtype):
    """affine_grid + grid_sample + divide + normalise: the crop a user of torch gets on the device today."""
    grid = torch.nn.functional.affine_grid(theta, (B, 3) + HW_OUT, align_corners=False)
    src = planes if idx is None else planes[idx]
    out = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False).div(255)
    if mean is not None:
        out = (out - mean) / std
    return out.to(dtype)


def normalised_theta(M):
    """The (B,2,3) theta of affine_grid (output [-1,1]^2 -> input [-1,1]^2, align_corners=False) of forward pixel matrices M."""
    H, W = HW_FRAME
    h, w = HW_OUT
    A = np.concatenate((M.astype(np.float64), np.tile([[[0, 0, 1]]], (len(M), 1, 1))), axis=1)
    Ai = np.linalg.inv(A)  # crop pixel -> source pixel
    to_pix = np.array([[w / 2, 0, (w - 1) / 2], [0, h / 2, (h - 1) / 2], [0, 0, 1]])       # normalised crop -> crop pixel
    to_norm = np.array([[2 / W, 0, 1 / W - 1], [0, 2 / H, 1 / H - 1], [0, 0, 1]])           # source pixel -> normalised source
    return (to_norm @ Ai @ to_pix)[:, :2].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops", "bench_crops.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crops: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    M = boxes(rng, B)
    Md, theta = torch.from_numpy(M).to(dev), torch.from_numpy(normalised_theta(M)).to(dev)
    mean_t, std_t = (torch.tensor(a, device=dev).view(1, 3, 1, 1) for a in cc.NORMALIZE)
    rows = []
    for label, F in (("one_frame", 1), ("64_frames", B)):
        frames = torch.from_numpy(cc.make_frames(3, n=F, hw=HW_FRAME, seed=5)).to(dev)
        planes = frames.permute(0, 3, 1, 2).float().contiguous()
        idx = torch.zeros(B, dtype=torch.int32, device=dev) if F == 1 else None
        idx_long = None if idx is None else idx.long()
        h2d_ours = frames.numel() + M.nbytes + (0 if idx is None else 4 * B)
        h2d_ref = B * 3 * HW_OUT[0] * HW_OUT[1] * 4
        for dtype in (torch.float32, torch.bfloat16):
            for normalize in (None, cc.NORMALIZE):
                out = torch.empty(B, 3, *HW_OUT, device=dev, dtype=dtype)
                info = torch.empty(B, device=dev, dtype=torch.int32)
                ours = timed(lambda: crops.warp_affine(frames, Md, HW_OUT, frame_index=idx, normalize=normalize, dtype=dtype, out=out, info=info),
                             args.iters, args.warmup)
                assert int(info.abs().sum()) == 0
                nm = (mean_t, std_t) if normalize else (None, None)
                ref = timed(lambda: torch_route(planes, theta, idx_long, nm[0], nm[1], dtype), args.iters, args.warmup)
                # the two routes cut the same crops: float weights against 1/32 px weights differ by a few grey levels at most
                diff = (torch_route(planes, theta, idx_long, nm[0], nm[1], torch.float32) -
                        crops.warp_affine(frames, Md, HW_OUT, frame_index=idx, normalize=normalize)).abs()
                scale = 1.0 if normalize is None else 1.0 / min(cc.NORMALIZE[1])
                written = out.numel() * out.element_size()
                rows.append(dict(frames=label, dtype=str(dtype).replace("torch.", ""), normalize=normalize is not None, ours=ours, torch_grid_sample=ref,
                                 speedup_vs_torch=ref["median_us"] / ours["median_us"], bytes_written=written,
                                 written_GBps=written / ours["median_us"] * 1e-3, share_of_8TBps=written / ours["median_us"] * 1e-3 / HBM_GBPS,
                                 h2d_bytes=dict(ours=int(h2d_ours), reference_fp32_crops=int(h2d_ref)),
                                 mean_abs_diff_vs_torch_in_grey_levels=float(diff.mean()) * 255 / scale))
                print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, crops=B, crop_hw=list(HW_OUT), frame_hw=list(HW_FRAME), rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
