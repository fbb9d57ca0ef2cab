#!/usr/bin/env python3
"""BOP's ground-truth annotations on the device (lc_amd.gtinfo) for 64 instances of one 480 x 640 frame with a 20 480-face icosphere: the
full frame and a 192 x 192 window per instance, each as the record alone on the rendered maps (`gt_info_from_depth`, with its algorithmic
bytes over its time as a share of 8 TB/s), the composition of the scene's depth from the 64 renders (`compose_scene_depth`), and the whole
chain (`compute_gt_info` with depth_test=None: render, compose, record).  Beside the record, a float64 torch statement of the same
definition on the same device maps (tests/gtinfo_oracle.torch_statement).

Every figure is a replayed graph of PER calls between two device events, divided by PER; SAMPLES such figures give the median and the
10th / 90th percentiles.  Kernel and torch statement are compared on the way: equal records, equal masks.  "record_kernel" is the public
call under the graph: its three launches (identities, reduce, finish) and the allocation of its two outputs from the graph's pool.

    python scripts/bench_gtinfo.py [--samples 20] [--per 5] [--out profiles/gtinfo/bench_gtinfo.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import gtinfo, render, vsd  # noqa: E402
from tests import gtinfo_oracle, render_cases  # noqa: E402

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


def record_bytes(h, w, hits):
    """What the record has to move: every render once, the scene's depth under the groups that hold a hit (counted as the hit pixels),
    the mask and the records."""
    return B * h * w * 4 + hits * 4 + B * h * w + B * 12 * 4


def compose_bytes(h, w, hits):
    """Every render once, one 8-byte key filled, read back and split into two 4-byte maps per frame pixel, one 8-byte atomic per hit."""
    return B * h * w * 4 + H * W * (8 + 8 + 4 + 4) + hits * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--per", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtinfo", "bench_gtinfo.json"))
    a = ap.parse_args()
    v, f = render_cases.icosphere(5, RADIUS)
    assert len(f) == 20480
    ms = render.MeshSet([(v, f)], DEV)
    gen = torch.Generator().manual_seed(0)
    idx = ms.index_of([0] * B)
    K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], device=DEV).expand(B, 3, 3).contiguous()
    t = torch.cat(((torch.rand(B, 1, generator=gen) - 0.5) * 0.5, (torch.rand(B, 1, generator=gen) - 0.5) * 0.3, 0.7 + 0.3 * torch.rand(B, 1, generator=gen)), -1)
    R, t = torch.eye(3).expand(B, 3, 3).contiguous().to(DEV), t.to(DEV).contiguous()
    zeros = torch.zeros(B, dtype=torch.int32, device=DEV)
    rows = []
    for name, hw in (("full_frame", None), ("window_192", (WIN, WIN))):
        h, w = hw or (H, W)
        win = None if hw is None else vsd.window_origins(t, t, K, None, hw, (H, W))
        origin = torch.zeros(B, 2, dtype=torch.int32, device=DEV) if win is None else win
        Kr = K.clone()
        Kr[:, 0, 2] -= origin[:, 0].float()
        Kr[:, 1, 2] -= origin[:, 1].float()
        d_gt = render.render_depth(ms, idx, R, t, Kr, (h, w), near=NEAR, far=FAR, pixel_center=(0.0, 0.0)).depth.contiguous()
        frame = gtinfo.compose_scene_depth(d_gt, zeros, (H, W), 1, origin_xy=origin).depth

        def record():
            return gtinfo.gt_info_from_depth(d_gt, frame, K, delta=DELTA, scene_index=zeros, origin_xy=win)

        def plain():
            return gtinfo_oracle.torch_statement(d_gt, frame, K, DELTA, zeros, win)

        def compose():
            return gtinfo.compose_scene_depth(d_gt, zeros, (H, W), 1, origin_xy=origin, want_instance=True)

        def renders():
            return render.render_depth(ms, idx, R, t, Kr, (h, w), near=NEAR, far=FAR, pixel_center=(0.0, 0.0))

        def chain():
            if hw is None:
                return gtinfo.compute_gt_info(ms, idx, R, t, K, None, frame_hw=(H, W), delta=DELTA, near=NEAR, far=FAR)
            return gtinfo.compute_gt_info(ms, idx, R, t, K, None, frame_hw=(H, W), window_hw=hw, window_xy=win, delta=DELTA, near=NEAR, far=FAR)

        got, whole, (want_i, want_m) = record(), chain(), plain()
        torch.cuda.synchronize()
        assert torch.equal(got.info, want_i), name
        assert torch.equal(got.mask_visib.view(torch.uint8), want_m), name
        assert torch.equal(whole.info, got.info) and torch.equal(whole.mask_visib, got.mask_visib), name
        hits = int(got.info[:, 0].sum())
        nbytes = record_bytes(h, w, hits)
        row = dict(config=name, B=B, frame_hw=[H, W], map_hw=[h, w], faces=len(f), mean_px_count_all=hits / B,
                   mean_visib_fract=float(got.visib_fract().mean()), rows_with_edge=int((got.info[:, 3] > 0).sum()),
                   record_kernel=graph_samples(record, a.samples, a.per), record_torch_float64=graph_samples(plain, a.samples, a.per),
                   compose=graph_samples(compose, a.samples, a.per), render=graph_samples(renders, a.samples, a.per),
                   compute_gt_info=graph_samples(chain, a.samples, a.per), record_algorithmic_bytes=nbytes, compose_algorithmic_bytes=compose_bytes(h, w, hits))
        row["record_share_of_8TBps"] = nbytes / row["record_kernel"]["median_us"] / HBM_BYTES_PER_US
        row["compose_share_of_8TBps"] = row["compose_algorithmic_bytes"] / row["compose"]["median_us"] / HBM_BYTES_PER_US
        row["record_speedup_over_torch"] = row["record_torch_float64"]["median_us"] / row["record_kernel"]["median_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(dict(device=torch.cuda.get_device_name(0), samples=a.samples, launches_per_graph=a.per, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
