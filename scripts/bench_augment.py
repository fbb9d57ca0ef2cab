#!/usr/bin/env python3
"""Times the training-time augmentation launch (lc_amd.augment.augment) on the GPU and writes profiles/augment/bench_augment.json.

    python scripts/bench_augment.py [--iters 200] [--warmup 20] [--out profiles/augment/bench_augment.json]

Every variant is captured in a graph after a warm-up and replayed; a time is the median over `--iters` replays timed one by one with
device events (p10 / p90 beside it).  Shapes: 32 and 64 crops of 256 x 256 x 3.  Cases: all six stages on and the four point-wise ones
only (the second compiled form), each with and without the background switch; outputs float32 and bfloat16 with `normalize`.  Every row
of a case has the same stages on and its own weights, table, background and sample id.

`moved_GBps` is the bytes the launch has to move -- the crops, with the switch the backgrounds and the mask, and the output -- over the
median time, `share_of_8TBps` that rate against the 8 TB/s of HBM.  `torch` is the same result stated in torch operations on the device
(integer blend, masks, 25 shifted multiply-adds per filter over a reflected copy, a gather through the table, the float finish), in a
graph as well; the positions hit by salt and dropout are handed to it as ready masks, which the launch derives itself.  Its bytes must
EQUAL the launch's, and the script stops if they do not.
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

from lc_amd import augment  # noqa: E402

H, W, G = 256, 256, 8
HBM_GBPS = 8000.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED = 20240229
CASES = (("all_stages", 63), ("all_but_switch", 62), ("pointwise_with_switch", 1 | 2 | 8 | 32), ("pointwise", 2 | 8 | 32))


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


def make_rows(bits, B, rng):
    """params (B,64) int32 and lut (B,3,256) uint8 with the stages `bits` on in every row."""
    params = np.zeros((B, augment.WORDS), dtype=np.int32)
    params[:, 0] = bits
    params[:, 1] = rng.integers(G, size=B)
    params[:, 2] = int(augment.SALT_P * 2 ** 32)
    params[:, 3] = int(augment.DROPOUT_P * 2 ** 32)
    params[:, 4], params[:, 5] = H * 5 // 100, W * 5 // 100
    for b in range(B):
        params[b, 6:31] = augment.motion_weights(rng.uniform(0, 360), rng.uniform(-1, 1))
        params[b, 31:56] = augment.gaussian_weights(rng.uniform(0.3, 1.2))
    _, lut = augment.draw(augment.AugmentConfig(pixel_aug_prob=1.0, use_invert=True), SEED, np.arange(B), G, hw=(H, W))
    return params, lut


def reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def torch_route(t, bits, dtype):
    """The launch's result in torch operations; `t` holds the device tensors, the hit masks among them."""
    v = t["crops"].int()
    if bits & 1:
        k = t["k"]
        S = k * v + (1024 - k) * t["bg"][t["g"]].int()
        q, rem = S >> 10, S & 1023
        v = q + ((rem > 512) | ((rem == 512) & ((q & 1) == 1))).int()
    if bits & 2:
        v = torch.where(t["hit"], t["salt"], v)
    for bit, name in ((4, "wA"), (8, None), (16, "wB")):
        if not bits & bit:
            continue
        if name is None:
            v = v * t["keep"]
            continue
        pad = v[:, :, t["iy"]][:, :, :, t["ix"]]
        acc = torch.full_like(v, 32768)
        for i in range(25):
            dy, dx = divmod(i, 5)
            acc = acc + t[name][:, i].view(-1, 1, 1, 1) * pad[:, :, dy:dy + H, dx:dx + W]
        v = acc >> 16
    if bits & 32:
        v = torch.gather(t["lut"], 2, v.view(v.shape[0], 3, -1).long()).view_as(v)
    out = (v.float() / 255 - t["mean"]) / t["std"]
    return v, out.to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment", "bench_augment.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    ys, xs = np.mgrid[0:H, 0:W]
    rows = []
    for B in (32, 64):
        crops = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)).to(dev)
        bg = torch.from_numpy(rng.integers(0, 256, (G, 3, H, W), dtype=np.uint8)).to(dev)
        k = rng.choice(np.array([0, 1024, 512, 300]), size=(B, H, W), p=[0.4, 0.4, 0.1, 0.1])
        msk = torch.from_numpy((k / 1024.0).astype(np.float32)).to(dev)
        ids = np.arange(B)
        for label, bits in CASES:
            params, lut = make_rows(bits, B, rng)
            p64 = params.astype(np.int64)
            cell = (ys * p64[0, 4] // H) * p64[0, 5] + (xs * p64[0, 5] // W)
            sid = ids[:, None, None]
            t = dict(crops=crops, bg=bg, g=torch.from_numpy(p64[:, 1]).to(dev), k=torch.from_numpy(k[:, None].astype(np.int32)).to(dev),
                     hit=torch.from_numpy((augment.key(SEED, sid, augment.OP_SNP, (ys * W + xs)[None]) < np.uint64(p64[0, 2] & 0xFFFFFFFF))[:, None]).to(dev),
                     salt=torch.from_numpy(((augment.key(SEED, sid, augment.OP_SNPV, (ys * W + xs)[None]) >> np.uint64(31)) * 255).astype(np.int32)[:, None]).to(dev),
                     keep=torch.from_numpy((augment.key(SEED, sid, augment.OP_DROP, cell[None]) >= np.uint64(p64[0, 3] & 0xFFFFFFFF)).astype(np.int32)[:, None]).to(dev),
                     wA=torch.from_numpy(params[:, 6:31].copy()).to(dev), wB=torch.from_numpy(params[:, 31:56].copy()).to(dev),
                     iy=torch.from_numpy(reflect(np.arange(-2, H + 2), H)).to(dev), ix=torch.from_numpy(reflect(np.arange(-2, W + 2), W)).to(dev),
                     lut=torch.from_numpy(lut.astype(np.int32)).to(dev), mean=torch.tensor(MEAN, device=dev).view(1, 3, 1, 1),
                     std=torch.tensor(STD, device=dev).view(1, 3, 1, 1))
            d_params, d_lut = torch.from_numpy(params).to(dev), torch.from_numpy(lut).to(dev)
            pointwise = not bits & 20
            for dtype in (torch.float32, torch.bfloat16):
                def ours():
                    return augment.augment(crops, d_params, d_lut, msk_in=msk, backgrounds=bg, seed=SEED, dtype=dtype, normalize=(MEAN, STD), pointwise=pointwise)

                got, info = ours()
                got8, _ = augment.augment(crops, d_params, d_lut, msk_in=msk, backgrounds=bg, seed=SEED, dtype=torch.uint8, pointwise=pointwise)
                want8, want = torch_route(t, bits, dtype)
                if int(info.abs().sum()) or not torch.equal(got8.int(), want8):  # the bytes; the float finish is pinned by the tests
                    raise SystemExit(f"bench_augment: {label} B={B}: the launch and the torch statement differ in {int((got8.int() != want8).sum())} bytes")
                close = float((got.float() - want.float()).abs().max())
                mine = timed(ours, args.iters, args.warmup)
                ref = timed(lambda: torch_route(t, bits, dtype), args.iters, args.warmup)
                moved = crops.numel() + (crops.numel() + msk.numel() * 4 if bits & 1 else 0) + got.numel() * got.element_size() + params.nbytes + lut.nbytes
                rows.append(dict(case=label, stages=bits, crops=B, form="pointwise" if pointwise else "filtered", dtype=str(dtype).replace("torch.", ""),
                                 ours=mine, torch=ref, speedup_vs_torch=ref["median_us"] / mine["median_us"], bytes_equal_to_torch=True, max_abs_diff_of_the_float_finish=close, bytes_moved=int(moved),
                                 moved_GBps=moved / mine["median_us"] * 1e-3, share_of_8TBps=moved / mine["median_us"] * 1e-3 / HBM_GBPS))
                print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, crop_hw=[H, W], backgrounds=G, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
