#!/usr/bin/env python3
"""Test-time pose covariance (lc_amd.posecov.pose_covariance, lc_pose_cov_f32): what it costs next to the chain it rides behind, at the
three shapes of lc_amd.synth.TEST_TIME_CONFIGS' workloads.  One JSON record per shape, all of them written to
profiles/posecov/bench_posecov.json; every time is a device-event timing of replayed graphs unless it says eager.

    zlmo     64 objects, 128 x 128 code maps, stride 1: 16 384 candidates per object, BOTH weighted solvers (one (128,16384,.) covariance launch)
    glmo     64 objects, 64 x 64 continuous maps, stride 2: 1024 candidates, 'weighted'
    gsplmo   64 objects, 16 keypoints with predicted standard deviations (the sparse chain)

    chain_us            GraphedSolvePnP(cfg, out, gt) replayed: `solve_pnp`, whose code this commit does not touch (the parent commit's chain)
    chain_with_cov_us   GraphedSolvePnP(cfg, out, gt, with_cov=True) replayed
    kernel_us           the covariance launch alone, on the rows the chain handed it (20 launches per replayed graph)
    lm_solve_us / lm_iters / lm_us_per_iter   the weighted LM solve alone on the same rows from the RANSAC-free start `pose`, its mean iteration
                        count, and their quotient: what ONE LM evaluation-and-step of the same shape costs (approximate: the quotient includes the
                        solve's set-up)
    torch_oracle_us     tests/posecov_oracle.pose_covariance (a closed-form TORCH RESTATEMENT, float64, not the reference's own code) run eagerly
                        on the same device tensors

    python scripts/bench_posecov.py [--iters 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import inference, synth  # noqa: E402
from lc_amd.config import AttrDict  # noqa: E402
from lc_amd.pnp import pnp_ceres  # noqa: E402
from tests import posecov_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")


def graph_us(fn, iters, per=1):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with inference.quiet_capture(), torch.cuda.graph(g):
        for _ in range(per):
            fn()
    return replay_us(g, iters) / per


def replay_us(g, iters):
    """Median over 5 batches of `iters` replays between two events."""
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters * 1e3)
    return sorted(times)[2]


def eager_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def inputs(name):
    if name == "gsplmo":
        gt, out = synth.sparse_inputs(B=64, N=16, seed=5)
        cfg = dict(solvers=["weighted"])
    else:
        cfg, gt, out = synth.test_time_inputs(name, B=64, seed=5)
        if name == "zlmo":
            cfg["solvers"] = ["weighted", "weighted_filtered"]
    to = lambda d: {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
    return AttrDict(cfg), to(gt), to(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    records = []
    for name in ("zlmo", "glmo", "gsplmo"):
        cfg, gt, out = inputs(name)
        calls = []
        real = inference.pose_covariance
        inference.pose_covariance = lambda *ar, **kw: calls.append((ar, kw)) or real(*ar, **kw)
        try:
            inference.solve_pnp_with_cov(cfg, out, gt)
        finally:
            inference.pose_covariance = real
        (args, kw), = calls
        args = [None if t is None else t.clone() for t in args] + [None] * (6 - len(args))  # (the sparse chain passes no counts)
        B, N = args[1].shape[:2]
        rec = dict(shape=name, objects=64, rows=B, N=N, solvers=list(cfg.solvers), device=torch.cuda.get_device_name(0))
        plain, with_cov = inference.GraphedSolvePnP(cfg, out, gt), inference.GraphedSolvePnP(cfg, out, gt, with_cov=True)
        rec["chain_us"] = round(replay_us(plain.graph, a.iters), 2)
        rec["chain_with_cov_us"] = round(replay_us(with_cov.graph, a.iters), 2)
        rec["kernel_us"] = round(graph_us(lambda: real(*args, **kw), a.iters, per=20), 2)
        K, X, U, W, pose, counts = args
        P = kw.get("shared_poses") or 0
        start = pose[:P] if P else pose
        wkw = dict(weights_are_std=True) if kw.get("weights_are_std") else dict(weights_are_icov=True)
        solve = lambda: pnp_ceres.solve_device(K, X, U, W, start, counts, nan_to_num=True, shared_poses=P, return_iters=True, split=False, **wkw)  # noqa: E731
        iters = solve()[3].float().mean().item()
        rec["lm_solve_us"] = round(graph_us(solve, a.iters, per=4), 2)
        rec["lm_iters"] = round(iters, 2)
        rec["lm_us_per_iter"] = round(rec["lm_solve_us"] / max(iters, 1.0), 2)
        rec["torch_oracle_us"] = round(eager_us(lambda: O.pose_covariance(*args, **kw), 3), 1)
        rec["cov_share_of_chain"] = round((rec["chain_with_cov_us"] - rec["chain_us"]) / rec["chain_us"], 3)
        print(json.dumps(rec), flush=True)
        records.append(rec)
    os.makedirs(os.path.join(ROOT, "profiles", "posecov"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "posecov", "bench_posecov.json"), "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
