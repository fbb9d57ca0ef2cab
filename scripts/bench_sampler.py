#!/usr/bin/env python3
"""Times the device-resident training set (lc_amd.trainset.TrainSet.step_inputs) beside the route it replaces and beside the chain without
over-sampling, and writes profiles/sampler/bench_sampler.json.

    python scripts/bench_sampler.py [--iters 200] [--warmup 20] [--host-iters 50] [--out profiles/sampler/bench_sampler.json]

Shapes: 16 384 annotations over four 480 x 640 frames and as many byte masks, a 256 x 256 input, a 64 x 64 output, 256 check points, eight
backgrounds cut to the input size, float32 output with `normalize`; B = 32 and 64 with S = B / 4 spares.  One annotation in eight has a
mask of a few pixels, so the retry has work to do.  Per case, one fresh step per replay:

  step_inputs  (a) a captured graph of `seed_word.add_(1)` and `TrainSet.step_inputs`: every replay is the next step's batch.  Median over
               `--iters` replays timed one by one with device events (p10 / p90 beside it).
  host_route   (b) what a step cost before: a host shuffle of the epoch (once per epoch, its cost spread over the epoch's steps), the
               gather of B records and their copies into the captured buffers (wall clock, with the wait for them), and a replay of
               `train_inputs` reading those buffers (device events).  `total_us` is their sum.  WITHOUT any retry: rows that are too
               empty stay in the batch.
  resident     (c) a captured graph of `seed_word.add_(1)` and `train_inputs` on B rows that already lie on the device: what the chain
               costs without drawing rows, over-sampling and selection.  (a) - (c) is the price of the resident set, reported as it is.

Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import augment, sampler  # noqa: E402
from lc_amd.train_inputs import train_inputs  # noqa: E402
from lc_amd.trainset import TrainSet  # noqa: E402

N, F, H, W, G = 16384, 4, 480, 640, 8
IN_HW, OUT_HW = (256, 256), (64, 64)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED0 = 20240229
RECORD = ("frame_index", "mask_index", "bbox_xyxy", "cam_K", "index")


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)))


def graphed(fn, warmup):
    for _ in range(warmup):
        fn()
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
    ap.add_argument("--host-iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler", "bench_sampler.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    cfg = augment.AugmentConfig(use_peper_salt=True, use_motion_blur=True, use_invert=True, rotate_prob=0.5)
    frames = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(dev)
    # masks 0 .. F-1 fill a region that every box below lies in; mask F is a blob of 3 x 3 pixels: too empty in any crop
    masks_h = np.zeros((F + 1, H, W), dtype=np.uint8)
    masks_h[:F, 60:420, 100:540] = 1
    masks_h[F, 238:241, 318:321] = 1
    masks = torch.from_numpy(masks_h).to(dev)
    bg = torch.from_numpy(rng.integers(0, 256, (G, 3) + IN_HW, dtype=np.uint8)).to(dev)
    K_h = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)
    x1, y1 = rng.uniform(120, 300, N), rng.uniform(80, 200, N)
    box_h = np.stack((x1, y1, x1 + rng.uniform(60, 220, N), y1 + rng.uniform(60, 200, N)), axis=1).astype(np.float32)
    frame_h = (np.arange(N) % F).astype(np.int32)
    mask_h = np.where(np.arange(N) % 8 == 5, F, frame_h).astype(np.int32)
    cols = dict(frame_index=frame_h, mask_index=mask_h, mesh_index=np.zeros(N, np.int32), obj_id=(np.arange(N) % 30 + 1).astype(np.int32),
                scene_id=(np.arange(N) // 1000).astype(np.int32), im_id=np.arange(N, dtype=np.int32), bbox_xyxy=box_h, cam_K=np.tile(K_h, (N, 1, 1)),
                R=np.tile(np.eye(3, dtype=np.float32), (N, 1, 1)), t=np.tile(np.float32([0, 0, 1]), (N, 1)))
    table = sampler.AnnotationTable(**cols, device=dev, n_frames=F, n_masks=F + 1)
    common = dict(cfg=cfg, in_hw=IN_HW, out_hw=OUT_HW, valid_th=100, n_check=256, backgrounds=bg, normalize=(MEAN, STD))
    cases = []
    for B in (32, 64):
        S = B // 4
        ts = TrainSet(frames, table, masks=masks, seed0=SEED0, batch=B, spare=S, **common)
        word = torch.full((1,), SEED0 - 1, dtype=torch.int64, device=dev)

        def step():
            word.add_(1)
            return ts.step_inputs(word)

        g_a, res_a = graphed(step, args.warmup)
        a = replay_times(g_a, args.iters)
        short, taken_spares = [], []
        for _ in range(20):  # what the retry did, read back outside the timing
            g_a.replay()
            torch.cuda.synchronize()
            short.append(int(res_a["shortfall"][0]))
            taken_spares.append(int((res_a["take"] >= B).sum()))

        # (b) and (c): train_inputs over captured buffers of B records
        bufs = dict(frame_index=torch.zeros(B, dtype=torch.int32, device=dev), mask_index=torch.zeros(B, dtype=torch.int32, device=dev),
                    bbox_xyxy=torch.from_numpy(box_h[:B]).to(dev), cam_K=torch.from_numpy(cols["cam_K"][:B]).to(dev), index=torch.arange(B, dtype=torch.int32, device=dev))
        bufs["frame_index"].copy_(torch.from_numpy(frame_h[:B]))
        bufs["mask_index"].copy_(torch.from_numpy(frame_h[:B]))
        word_b = torch.full((1,), SEED0, dtype=torch.int64, device=dev)

        def chain():
            return train_inputs(frames, bufs["frame_index"], masks=masks, mask_index=bufs["mask_index"], bbox_xyxy=bufs["bbox_xyxy"], cam_K=bufs["cam_K"],
                                sample_id=bufs["index"], seed=word_b, **common)

        def fresh_chain():
            word_b.add_(1)
            return chain()

        g_c, _ = graphed(fresh_chain, args.warmup)
        c = replay_times(g_c, args.iters)

        g_b, _ = graphed(chain, args.warmup)
        steps_per_epoch = -(-N // B)
        t0 = time.perf_counter()
        order = rng.permutation(N)
        shuffle_us = (time.perf_counter() - t0) * 1e6
        host_cols = dict(frame_index=frame_h, mask_index=mask_h, bbox_xyxy=box_h, cam_K=cols["cam_K"], index=np.arange(N, dtype=np.int32))
        t_gather, t_replay = [], []
        for i in range(args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pick = order[i * B:(i + 1) * B]
            for name in RECORD:
                bufs[name].copy_(torch.from_numpy(np.ascontiguousarray(host_cols[name][pick])))
            word_b.fill_(SEED0 + i)
            torch.cuda.synchronize()
            t_gather.append((time.perf_counter() - t0) * 1e6)
            t_replay.append(replay_times(g_b, 1)["median_us"])
        b = dict(shuffle_wall_us_per_epoch=shuffle_us, shuffle_wall_us_per_step=shuffle_us / steps_per_epoch, gather_upload_wall=stats(t_gather), replay=stats(t_replay),
                 retry=False)
        b["total_us"] = b["shuffle_wall_us_per_step"] + b["gather_upload_wall"]["median_us"] + b["replay"]["median_us"]
        cases.append(dict(batch=B, spare=S, step_inputs=a, host_route=b, resident_train_inputs=c, over_sampling_and_selection_us=a["median_us"] - c["median_us"],
                          fresh_step_speedup_vs_host_route=b["total_us"] / a["median_us"], shortfall_over_20_steps=short, spares_taken_over_20_steps=taken_spares))
        print(json.dumps(cases[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, host_iters=args.host_iters, annotations=N, frames=[F, H, W], in_hw=list(IN_HW),
               out_hw=list(OUT_HW), backgrounds=G, n_check=256, empty_annotations="one in eight", cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
