#!/usr/bin/env python3
"""The training mask crops on the device (lc_amd.maskcrop) for B = 32 rows: from 480 x 640 masks and from 192 x 192 windows to 128 x 128
and 64 x 64 crops, with 256 check points and without; and the input-size `msk_in` call at 256 x 256 (linear warp alone).  Beside each, a
torch statement of the same result on the device: the four-tap integer blend by gathers for the warps, and for the check points a
sort of the hashed keys of round 0 (the statement is written out here, with the hash of include/lc_amd_maskcrop.h).

Every figure is a replayed graph of PER calls between two device events, divided by PER; SAMPLES such figures give the median and the
10th / 90th percentiles.  Kernel and torch statement are compared on the way: equal bits.

    python scripts/bench_maskcrop.py [--samples 20] [--per 5] [--out profiles/maskcrop/bench_maskcrop.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import maskcrop  # noqa: E402

DEV = torch.device("cuda:0")
B = 32


def graph_samples(fn, samples, per):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / per * 1e3)
    a = np.asarray(out)
    return dict(median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)), p90_us=float(np.percentile(a, 90)), n=len(a))


def fix(v):
    return torch.clamp(torch.round(v), -2.0 ** 30, 2.0 ** 30).to(torch.int64)


def coordinates(M, h, w):
    """(X, Y) (B,h,w) int64 without delta: include/lc_amd_maskcrop.h in float64 torch (torch fuses nothing on its own)."""
    M = M.double()
    D = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    D = torch.where(D != 0, 1.0 / D, torch.zeros_like(D))
    m00, m01, m10, m11 = M[:, 1, 1] * D, -M[:, 0, 1] * D, -M[:, 1, 0] * D, M[:, 0, 0] * D
    b1 = -m00 * M[:, 0, 2] - m01 * M[:, 1, 2]
    b2 = -m10 * M[:, 0, 2] - m11 * M[:, 1, 2]
    ys = torch.arange(h, device=M.device, dtype=torch.float64)[None, :]
    xs = torch.arange(w, device=M.device, dtype=torch.float64)[None, :]
    X0, Y0 = fix((m01[:, None] * ys + b1[:, None]) * 1024.0), fix((m11[:, None] * ys + b2[:, None]) * 1024.0)
    ax, ay = fix(m00[:, None] * xs * 1024.0), fix(m10[:, None] * xs * 1024.0)
    return X0[:, :, None] + ax[:, None, :], Y0[:, :, None] + ay[:, None, :]


def taps(masks, index, origin, sx, sy):
    F, Hm, Wm = masks.shape
    u, v = sx - origin[:, 0, None, None], sy - origin[:, 1, None, None]
    inside = (u >= 0) & (u < Wm) & (v >= 0) & (v < Hm)
    flat = (index[:, None, None].long() * Hm + v.clamp(0, Hm - 1)) * Wm + u.clamp(0, Wm - 1)
    return torch.where(inside, masks.reshape(-1)[flat] != 0, torch.zeros_like(inside)).long()


def torch_warps(masks, index, origin, M, h, w, linear=True, want_noc=True):
    X, Y = coordinates(M, h, w)
    noc = taps(masks, index, origin, (X + 512) >> 10, (Y + 512) >> 10) if want_noc else None
    vis = None
    if linear:
        Xs, Ys = (X + 16) >> 5, (Y + 16) >> 5
        sx, sy, fx, fy = Xs >> 5, Ys >> 5, Xs & 31, Ys & 31
        k = ((32 - fx) * (32 - fy) * taps(masks, index, origin, sx, sy) + fx * (32 - fy) * taps(masks, index, origin, sx + 1, sy) +
             (32 - fx) * fy * taps(masks, index, origin, sx, sy + 1) + fx * fy * taps(masks, index, origin, sx + 1, sy + 1))
        vis = k.float() / 1024.0
    return vis, noc


def fmix32(v):
    v = v & 0xFFFFFFFF
    v = v ^ (v >> 16)
    v = (v * 0x85EBCA6B) & 0xFFFFFFFF
    v = v ^ (v >> 13)
    v = (v * 0xC2B2AE35) & 0xFFFFFFFF
    return v ^ (v >> 16)


def torch_first_round(noc, seed, sample_id, n_check):
    """Round 0 of the check points where valid_cnt >= n_check (what the timed configurations hold): the n_check smallest (key, p) of the
    valid pixels, by one sort per row of the composite, invalid pixels pushed behind."""
    Bn, h, w = noc.shape
    p = torch.arange(h * w, device=noc.device, dtype=torch.int64)[None, :]
    k = fmix32(torch.full((Bn, 1), seed & 0xFFFFFFFF, device=noc.device, dtype=torch.int64))
    k = fmix32(k ^ (seed >> 32))
    k = fmix32(k ^ sample_id[:, None].long())
    k = fmix32(k)  # r = 0
    comp = (fmix32(k ^ p) << 16) | p
    comp = torch.where(noc.reshape(Bn, -1) != 0, comp, torch.full_like(comp, 1 << 62))
    q = torch.sort(comp, dim=1).values[:, :n_check] & 0xFFFF
    return torch.stack((q % w, q // w), -1)


def affine(center, zoom, out_hw, rot):
    c, s = math.cos(rot), math.sin(rot)
    A = np.array([[c, s], [-s, c]]) * zoom
    t = np.array([out_hw[1] * 0.5, out_hw[0] * 0.5]) - A @ np.asarray(center, dtype=np.float64)
    return np.concatenate((A, t[:, None]), 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--per", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskcrop", "bench_maskcrop.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []
    index = torch.arange(B, device=DEV, dtype=torch.int32)
    sid = torch.arange(B, device=DEV, dtype=torch.int32) * 13 + 5
    for src_name, (Hm, Wm) in (("frame_480x640", (480, 640)), ("window_192", (192, 192))):
        # a disc of 60 to 85 px radius per mask, centred in a window, anywhere in a frame
        yy, xx = np.mgrid[:Hm, :Wm]
        cx = rng.uniform(0.4, 0.6, B) * Wm
        cy = rng.uniform(0.4, 0.6, B) * Hm
        rad = rng.uniform(60, 85, B)
        masks_np = ((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2 < rad[:, None, None] ** 2).astype(np.uint8)
        masks = torch.from_numpy(masks_np).to(DEV)
        origin = torch.zeros(B, 2, dtype=torch.int32, device=DEV) if Hm == 480 else torch.from_numpy(rng.integers(-40, 400, (B, 2)).astype(np.int32)).to(DEV)
        org_np = origin.cpu().numpy()
        for out_hw, with_ck in (((128, 128), True), ((128, 128), False), ((64, 64), True), ((64, 64), False), ((256, 256), None)):
            h, w = out_hw
            M = torch.from_numpy(np.stack([affine((cx[b] + org_np[b, 0], cy[b] + org_np[b, 1]), h / (3.0 * rad[b]), out_hw, rng.uniform(0, 2 * math.pi))
                                           for b in range(B)])).to(DEV)
            if with_ck is None:  # msk_in: the linear warp at the input size alone
                kw = dict(mask_index=index, origin=origin, n_check=0, want=("msk_vis",))

                def kernel():
                    return maskcrop.mask_crops(masks, M, out_hw, **kw)

                def plain():
                    return torch_warps(masks, index, origin.long(), M, h, w, linear=True, want_noc=False)

                got, (vis, _) = kernel(), plain()
                torch.cuda.synchronize()
                assert torch.equal(got.msk_vis, vis), (src_name, out_hw)
                name = "msk_in"
            else:
                n_check = 256 if with_ck else 0
                kw = dict(mask_index=index, origin=origin, sample_id=sid, valid_th=100, n_check=n_check, seed=17)

                def kernel():
                    return maskcrop.mask_crops(masks, M, out_hw, **kw)

                def plain():
                    vis, noc = torch_warps(masks, index, origin.long(), M, h, w)
                    cnt = noc.reshape(B, -1).sum(1)
                    return vis, noc, cnt, (torch_first_round(noc, 17, sid, 256) if with_ck else None)

                got, (vis, noc, cnt, ck) = kernel(), plain()
                torch.cuda.synchronize()
                assert torch.equal(got.msk_vis, vis) and torch.equal(got.msk_noc, noc.bool()) and torch.equal(got.valid_cnt.long(), cnt), (src_name, out_hw)
                assert int(cnt.min()) >= 256
                if with_ck:
                    assert torch.equal(got.sym_ck_pts2d, ck), (src_name, out_hw)
                name = "labels_with_check_points" if with_ck else "labels_without_check_points"
            row = dict(source=src_name, config=name, B=B, mask_hw=[Hm, Wm], out_hw=[h, w], mean_valid_cnt=None if with_ck is None else float(cnt.float().mean()),
                       kernel=graph_samples(kernel, a.samples, a.per), torch_statement=graph_samples(plain, a.samples, a.per))
            row["speedup_over_torch"] = row["torch_statement"]["median_us"] / row["kernel"]["median_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(dict(device=torch.cuda.get_device_name(0), samples=a.samples, launches_per_graph=a.per, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
