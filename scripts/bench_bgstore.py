#!/usr/bin/env python3
"""Times the resident background store's switch (lc_amd.backgrounds.switch_backgrounds) alone and inside the chained training input
(lc_amd.train_inputs.train_inputs) beside the routes it stands next to, and writes profiles/bgstore/bench_bgstore.json.

    python scripts/bench_bgstore.py [--iters 200] [--warmup 20] [--host-iters 10] [--out profiles/bgstore/bench_bgstore.json]

Shapes: 32 and 64 rows, 256 x 256 crops of four 480 x 640 frames, a store of 64 images of mixed sizes around 375 x 500, the default
AugmentConfig with the three switches on.  Per batch size, device events around replayed graphs (median, p10 / p90 beside it):

  switch3        pick + region matrices + switch on a resident crop and mask: the three launches alone
  switch1        the switch launch alone on a resident pick and resident matrices, with the bytes it has to move counted from the
                 shapes -- for every open row the mask (4 h w), the crop read and written where k < 1024 (2 * 3 bytes per such pixel) and
                 the region of the image it cuts (3 rw rh) -- and their share of 8 TB/s
  chain_store    `seed_word.add_(1)` and `train_inputs(background_store=...)`: every replay picks and cuts anew
  chain_precut   the same chain with `backgrounds` (G,3,256,256) already cut by someone else: the same pixels at every step
  host_route     what a fresh cut per row cost before: host `augment.draw` + `background_matrices` (wall clock), their upload (wall
                 clock, with the wait), one `crops.warp_affine` per open row (its image has its own size; wall clock, with the wait) and
                 a replay of `augment` on the uploaded rows (device events).  `total_us` is their sum.

Before anything is timed the switched crop of the three launches is compared with tests/bgstore_oracle.py's on the first four rows; the
script stops if they differ.  Needs the GPU; there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import _lib, augment, backgrounds, crops, geometry  # noqa: E402
from lc_amd.train_inputs import train_inputs  # noqa: E402

F, H, W, G = 4, 480, 640, 64
IN_HW, OUT_HW = (256, 256), (64, 64)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED = 20240229
PEAK = 8e12


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)))


def graphed(fn, warmup):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    return g, res


def replay_times(g, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgstore", "bench_bgstore.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bgstore: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    cfg = augment.AugmentConfig(use_peper_salt=True, use_motion_blur=True, use_invert=True, rotate_prob=0.5)
    sizes = [(375 + int(rng.integers(-60, 61)), 500 + int(rng.integers(-80, 81))) for _ in range(G)]
    images = [rng.integers(0, 256, (hb, wb, 3), dtype=np.uint8) for hb, wb in sizes]
    store = backgrounds.BackgroundStore.from_images(images, dev)
    frames = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(dev)
    masks_h = np.zeros((F, H, W), dtype=np.uint8)
    for f in range(F):
        masks_h[f, 100 + 20 * f:340 - 10 * f, 150 + 30 * f:470 + 10 * f] = 1
    masks = torch.from_numpy(masks_h).to(dev)
    precut = torch.from_numpy(rng.integers(0, 256, (G, 3) + IN_HW, dtype=np.uint8)).to(dev)
    K = torch.tensor([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], device=dev)
    h, w = IN_HW
    rows = []
    for B in (32, 64):
        ids_h = np.arange(B, dtype=np.int32) * 3 - 7
        sid = torch.from_numpy(ids_h).to(dev)
        x1, y1 = rng.uniform(120, 300, B), rng.uniform(80, 200, B)
        box = torch.from_numpy(np.stack((x1, y1, x1 + rng.uniform(60, 220, B), y1 + rng.uniform(60, 200, B)), axis=1).astype(np.float32)).to(dev)
        fidx = torch.from_numpy((np.arange(B) % F).astype(np.int32)).to(dev)
        crop_h = rng.integers(0, 256, (B, 3, h, w), dtype=np.uint8)
        msk_h = np.zeros((B, h, w), dtype=np.float32)
        msk_h[:, 64:192, 48:208] = 1.0
        msk_h[:, 64:192, 44:48] = 0.5  # a soft edge of one quad
        crop0, msk = torch.from_numpy(crop_h).to(dev), torch.from_numpy(msk_h).to(dev)

        # the outputs first: the three launches against the oracle, on four rows
        from tests import bgstore_oracle

        crop = crop0[:4].clone()
        backgrounds.switch_backgrounds(crop, store, cfg, seed=SEED, sample_id=sid[:4], msk_in=msk[:4])
        want = bgstore_oracle.switch(crop_h[:4], images, cfg, SEED, ids_h[:4], msk_h[:4])[0]
        if not np.array_equal(crop.cpu().numpy(), want):
            raise SystemExit(f"bench_bgstore: B={B}: the switched crop differs from the oracle's")

        word = torch.full((1,), SEED, dtype=torch.int64, device=dev)
        crop = crop0.clone()
        g3, _ = graphed(lambda: backgrounds.switch_backgrounds(crop, store, cfg, seed=word, sample_id=sid, msk_in=msk), args.warmup)
        switch3 = replay_times(g3, args.iters)

        gate, which, bg_hw = backgrounds.pick_backgrounds(store, cfg, seed=word, sample_id=sid)
        M = geometry.background_geometry(seed=word, sample_id=sid, bg_hw=bg_hw, out_hw=IN_HW)
        info = torch.empty(B, dtype=torch.int32, device=dev)
        lib = backgrounds.load()

        def switch1():
            rc = lib.lc_bgstore_switch_u8(_lib.ptr(crop), _lib.ptr(msk), _lib.ptr(store.pixels), _lib.ptr(store.offsets), _lib.ptr(store.hw), store.G, _lib.ptr(which),
                                          _lib.ptr(M), h, w, B, _lib.ptr(info), _lib.stream_ptr(dev))
            assert rc == 0

        g1, _ = graphed(switch1, args.warmup)
        one = replay_times(g1, args.iters)
        open_rows = np.flatnonzero(gate.cpu().numpy())
        Mh = M.cpu().numpy()
        region = sum(3.0 * (w / float(Mh[b, 0, 0])) * (h / float(Mh[b, 1, 1])) for b in open_rows)
        moved = float(len(open_rows) * 4.0 * h * w + 6.0 * float((msk_h[open_rows] < 1.0).sum()) + region)
        one.update(open_rows=int(len(open_rows)), bytes_moved=moved, share_of_8TBs=moved / (one["median_us"] * 1e-6) / PEAK)

        kw = dict(masks=masks, mask_index=fidx, bbox_xyxy=box, cam_K=K, sample_id=sid, cfg=cfg, in_hw=IN_HW, out_hw=OUT_HW, valid_th=100, n_check=256,
                  normalize=(MEAN, STD))

        def chain(**src):
            def fresh():
                word.add_(1)
                return train_inputs(frames, fidx, seed=word, **src, **kw)
            return replay_times(graphed(fresh, args.warmup)[0], args.iters)

        chain_store, chain_precut = chain(background_store=store), chain(backgrounds=precut)

        # the route a fresh cut per row took before: host draw, upload, one warp per open row, augment on the uploaded rows
        params_d = torch.zeros(B, augment.WORDS, dtype=torch.int32, device=dev)
        lut_d = torch.zeros(B, 3, 256, dtype=torch.uint8, device=dev)
        cuts = torch.zeros(B, 3, h, w, dtype=torch.uint8, device=dev)
        image_d = [torch.from_numpy(im[None]).to(dev) for im in images]
        g_aug, _ = graphed(lambda: augment.augment(crop0, params_d, lut_d, msk_in=msk, backgrounds=cuts, seed=SEED, sample_id=sid, normalize=(MEAN, STD)), args.warmup)
        t_draw, t_copy, t_warp, t_replay = [], [], [], []
        for i in range(args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P, lut = augment.draw(cfg, SEED + i, ids_h, G, IN_HW)
            on = np.flatnonzero(P[:, 0] & 1)
            chosen = P[on, 1].copy()
            Mrow = augment.background_matrices(SEED + i, ids_h[on], np.array([sizes[g] for g in chosen]).reshape(-1, 2), IN_HW)
            P[on, 1] = on  # row b's cut is background b of the launch
            t1 = time.perf_counter()
            params_d.copy_(torch.from_numpy(P))
            lut_d.copy_(torch.from_numpy(lut))
            Md = torch.from_numpy(Mrow).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for j, b in enumerate(on):
                crops.warp_affine(image_d[int(chosen[j])], Md[j:j + 1], IN_HW, dtype=torch.uint8, out=cuts[b:b + 1])
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            t_draw.append((t1 - t0) * 1e6)
            t_copy.append((t2 - t1) * 1e6)
            t_warp.append((t3 - t2) * 1e6)
            t_replay.append(replay_times(g_aug, 1)["median_us"])
        host = dict(draw_wall=stats(t_draw), copy_wall=stats(t_copy), warps_wall=stats(t_warp), augment_replay=stats(t_replay))
        host["total_us"] = sum(host[k]["median_us"] for k in ("draw_wall", "copy_wall", "warps_wall", "augment_replay"))
        rows.append(dict(rows=B, switch3=switch3, switch1=one, chain_store=chain_store, chain_precut=chain_precut, host_route=host,
                         switched_crop_equal_to_the_oracle=True))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, host_iters=args.host_iters, frames=[F, H, W], in_hw=list(IN_HW),
               out_hw=list(OUT_HW), store_images=G, store_bytes=int(store.pixels.numel()), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
