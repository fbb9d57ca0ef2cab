#!/usr/bin/env python3
"""BOP's VSD on the device (lc_amd.vsd) for 64 poses of one 480 x 640 frame with a 20 480-face icosphere: the full frame and a 192 x 192
window per pose, each as the whole chain (`compute_vsd`: two renders and the score), the scoring kernel alone on the rendered maps (with its
algorithmic bytes over its time as a share of 8 TB/s), and the two-render part alone.  Beside the scoring kernel, a float64 torch statement
of the same definition on the same device maps (tests/vsd_oracle.torch_statement).

Every figure is a replayed graph of PER calls between two device events, divided by PER; SAMPLES such figures give the median and the
10th / 90th percentiles.  Kernel and torch statement are compared on the way: equal counts (edge included), equal error bits.
"score_kernel" is the public call `vsd_from_depth` under the graph: its three launches (zero, count, finish) and the allocation of its
two outputs from the graph's pool, not the counting kernel's own time; the share of 8 TB/s is the algorithmic bytes over that whole figure.

    python scripts/bench_vsd.py [--samples 20] [--per 5] [--out profiles/vsd/bench_vsd.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import render, vsd  # noqa: E402
from tests import render_cases, vsd_oracle  # noqa: E402

DEV = torch.device("cuda:0")
B, H, W, WIN = 64, 480, 640, 192
NEAR, FAR, DELTA, RADIUS = 0.01, 6.5, 0.015, 0.1
HBM_BYTES_PER_US = 8e6  # 8 TB/s


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


def score_bytes(h, w, T):
    """What the score has to move: both rendered maps of every pose, the part of the one frame the poses look at (at most all of it),
    and the outputs."""
    return 2 * B * h * w * 4 + min(B * h * w, H * W) * 4 + B * (2 * T + 3) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--per", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsd", "bench_vsd.json"))
    a = ap.parse_args()
    v, f = render_cases.icosphere(5, RADIUS)
    assert len(f) == 20480
    ms = render.MeshSet([(v, f)], DEV)
    gen = torch.Generator().manual_seed(0)
    idx = ms.index_of([0] * B)
    K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], device=DEV).expand(B, 3, 3).contiguous()
    tg = torch.cat(((torch.rand(B, 1, generator=gen) - 0.5) * 0.5, (torch.rand(B, 1, generator=gen) - 0.5) * 0.3, 0.7 + 0.3 * torch.rand(B, 1, generator=gen)), -1)
    te = tg + torch.randn(B, 3, generator=gen) * 0.01
    eye = torch.eye(3).expand(B, 3, 3)
    Rg, Re, tg, te = (x.to(DEV).contiguous() for x in (eye, eye, tg, te))
    diam = torch.full((B,), 2 * RADIUS, device=DEV)
    taus = vsd.BOP_TAUS
    taus_dev = torch.tensor(taus, dtype=torch.float32, device=DEV)
    # the frame: every ground-truth object in front of a back plane, a band without measurement
    gt_full = render.render_depth(ms, idx, Rg, tg, K, (H, W), near=NEAR, far=FAR, pixel_center=(0.0, 0.0)).depth
    frame = torch.where(gt_full > 0, gt_full, gt_full.new_full((), 1.5)).amin(0, keepdim=True).contiguous()
    frame[:, 200:230, :] = 0
    zeros = torch.zeros(B, dtype=torch.int32, device=DEV)
    rows = []
    for name, hw in (("full_frame", None), ("window_192", (WIN, WIN))):
        h, w = hw or (H, W)
        win = None if hw is None else vsd.window_origins(te, tg, K, diam, hw, (H, W))
        Kr = K
        if win is not None:
            Kr = K.clone()
            Kr[:, 0, 2] -= win[:, 0].float()
            Kr[:, 1, 2] -= win[:, 1].float()

        def chain():
            return vsd.compute_vsd(ms, idx, Re, te, Rg, tg, K, frame, delta=DELTA, taus=taus, diameter=diam, near=NEAR, far=FAR, window_hw=hw, window_xy=win)

        def renders():
            return render.render_depth(ms, torch.cat((idx, idx)), torch.cat((Re, Rg)), torch.cat((te, tg)), torch.cat((Kr, Kr)), (h, w), near=NEAR,
                                       far=FAR, pixel_center=(0.0, 0.0))

        maps = renders().depth
        d_est, d_gt = maps[:B].contiguous(), maps[B:].contiguous()

        def score():
            return vsd.vsd_from_depth(d_est, d_gt, frame, K, delta=DELTA, taus=taus, diameter=diam, scene_index=zeros, window_xy=win)

        def plain():
            return vsd_oracle.torch_statement(d_est, d_gt, frame, K, DELTA, taus_dev, diam, zeros, win)

        got, whole, (want_c, want_e) = score(), chain(), plain()
        torch.cuda.synchronize()
        assert torch.equal(got.counts, want_c), name
        assert torch.equal(got.errors.view(torch.int32), want_e.view(torch.int32)), name
        assert torch.equal(whole.counts, got.counts) and torch.equal(whole.errors.view(torch.int32), got.errors.view(torch.int32)), name
        nbytes = score_bytes(h, w, len(taus))
        row = dict(config=name, B=B, frame_hw=[H, W], map_hw=[h, w], faces=len(f), T=len(taus),
                   mean_union=float(got.counts[:, 0].float().mean()), mean_error=float(got.errors.mean()), rows_with_edge=int((got.counts[:, 2] > 0).sum()),
                   compute_vsd=graph_samples(chain, a.samples, a.per), score_kernel=graph_samples(score, a.samples, a.per),
                   two_renders=graph_samples(renders, a.samples, a.per), score_torch_float64=graph_samples(plain, a.samples, a.per),
                   score_algorithmic_bytes=nbytes)
        row["score_share_of_8TBps"] = nbytes / row["score_kernel"]["median_us"] / HBM_BYTES_PER_US
        row["score_speedup_over_torch"] = row["score_torch_float64"]["median_us"] / row["score_kernel"]["median_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(dict(device=torch.cuda.get_device_name(0), samples=a.samples, launches_per_graph=a.per,
                       compute_vsd_full_over_window=rows[0]["compute_vsd"]["median_us"] / rows[1]["compute_vsd"]["median_us"], rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
