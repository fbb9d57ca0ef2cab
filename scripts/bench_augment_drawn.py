#!/usr/bin/env python3
"""Times the augmentation with its rows drawn by the kernel (lc_amd.augment.augment_drawn) beside the two routes it is measured against,
and writes profiles/augment/bench_augment_drawn.json.

    python scripts/bench_augment_drawn.py [--iters 200] [--warmup 20] [--host-iters 20] [--out profiles/augment/bench_augment_drawn.json]

Shapes: 32 and 64 crops of 256 x 256 x 3 with the background switch and `normalize`, float32 and bfloat16 outputs.  Configurations: the
default probabilities with the three switches on (`training`), and every gate open (`every_gate_open`: each row runs all six stages).
Per case, one fresh draw per step by three routes:

  drawn        a captured graph of `seed_word.add_(1)` and `augment_drawn`: every replay draws anew on the device.  Median over `--iters`
               replays timed one by one with device events (p10 / p90 beside it); `drawn_fixed_seed` is the launch alone.
  host_route   what a step cost before: the host `draw` (wall clock, median of `--host-iters`), the copy of its rows into the captured
               buffers (wall clock, with the wait for it), and the replay of `augment` (device events).  `total_us` is their sum.
  resident     `augment` alone, replayed on the rows the kernel drew, resident on the device: `drawn_fixed_seed - resident` is the price of
               drawing in the kernel.

The drawn launch's output must EQUAL `augment`'s on the rows it returns, and the script stops if it does not.
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

from lc_amd import augment  # noqa: E402

H, W, G = 256, 256, 8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED = 20240229
CONFIGS = (("training", dict(use_peper_salt=True, use_motion_blur=True, use_invert=True)),
           ("every_gate_open", dict(pixel_aug_prob=1.0, switch_bg_prob=1.0, use_peper_salt=True, use_motion_blur=True, use_invert=True)))


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
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment", "bench_augment_drawn.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_drawn: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    rows = []
    for B in (32, 64):
        crops = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)).to(dev)
        bg = torch.from_numpy(rng.integers(0, 256, (G, 3, H, W), dtype=np.uint8)).to(dev)
        k = rng.choice(np.array([0, 1024, 512, 300]), size=(B, H, W), p=[0.4, 0.4, 0.1, 0.1])
        msk = torch.from_numpy((k / 1024.0).astype(np.float32)).to(dev)
        ids = np.arange(B, dtype=np.int32)
        sid = torch.from_numpy(ids).to(dev)
        for label, fields in CONFIGS:
            cfg = augment.AugmentConfig(**fields)
            for dtype in (torch.float32, torch.bfloat16):
                kw = dict(msk_in=msk, backgrounds=bg, dtype=dtype, normalize=(MEAN, STD))
                word = torch.full((1,), SEED, dtype=torch.int64, device=dev)

                # the bytes first: the drawn launch against `augment` on the rows it returns
                out, info, d_params, d_lut = augment.augment_drawn(crops, cfg, seed=word, sample_id=sid, return_rows=True, **kw)
                want, winfo = augment.augment(crops, d_params, d_lut, seed=SEED, sample_id=sid, pointwise=False, **kw)
                if int(info.abs().sum()) or not torch.equal(out, want) or not torch.equal(info, winfo):
                    raise SystemExit(f"bench_augment_drawn: {label} B={B} {dtype}: the drawn launch and augment on its rows differ")
                stages = [int(((d_params[:, 0] & bit) != 0).sum()) for bit in (1, 2, 4, 8, 16, 32)]

                g_fixed, _ = graphed(lambda: augment.augment_drawn(crops, cfg, seed=word, sample_id=sid, **kw), args.warmup)
                fixed = replay_times(g_fixed, args.iters)

                def fresh():
                    word.add_(1)
                    return augment.augment_drawn(crops, cfg, seed=word, sample_id=sid, **kw)

                g_fresh, _ = graphed(fresh, args.warmup)
                drawn = replay_times(g_fresh, args.iters)

                s_params, s_lut = d_params.clone(), d_lut.clone()
                g_res, _ = graphed(lambda: augment.augment(crops, s_params, s_lut, seed=SEED, sample_id=sid, pointwise=False, **kw), args.warmup)
                resident = replay_times(g_res, args.iters)

                t_draw, t_copy, t_replay = [], [], []
                for i in range(args.host_iters):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h_params, h_lut = augment.draw(cfg, SEED + 1 + i, ids, G, hw=(H, W))
                    t1 = time.perf_counter()
                    s_params.copy_(torch.from_numpy(h_params))
                    s_lut.copy_(torch.from_numpy(h_lut))
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    t_draw.append((t1 - t0) * 1e6)
                    t_copy.append((t2 - t1) * 1e6)
                    t_replay.append(replay_times(g_res, 1)["median_us"])
                host = dict(draw_wall=stats(t_draw), copy_wall=stats(t_copy), replay=stats(t_replay))
                host["total_us"] = host["draw_wall"]["median_us"] + host["copy_wall"]["median_us"] + host["replay"]["median_us"]

                rows.append(dict(config=label, crops=B, dtype=str(dtype).replace("torch.", ""), rows_with_stage_bit_0_to_5=stages, drawn=drawn,
                                 drawn_fixed_seed=fixed, resident=resident, host_route=host,
                                 price_of_drawing_us=fixed["median_us"] - resident["median_us"],
                                 fresh_step_speedup_vs_host_route=host["total_us"] / drawn["median_us"], bytes_equal_to_augment_on_the_drawn_rows=True))
                print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, host_iters=args.host_iters, crop_hw=[H, W], backgrounds=G, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
