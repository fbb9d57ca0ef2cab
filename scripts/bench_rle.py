#!/usr/bin/env python3
"""The device-resident store of run-length masks (lc_amd.rle) at 1 024 and 16 384 instance masks of 480 x 640 frames, every mask the
silhouette of a rendered icosphere: the index of the whole store; the decode of B = 32 rows to full frames and to 192 x 192 windows
around the boxes; decode + mask crops (128 x 128, 256 check points) beside the mask crops alone on resident bytes; the encode of 32
full-frame masks.  Beside the decode, two reference points on the device: a torch statement of it (`repeat_interleave` of k & 1 over the
counts, transposed -- the slow one) and a plain fill of the same output bytes (the fast one).  And the counted bytes per step that no
longer cross the bus: the B byte masks a host would decode and upload, against B indices and origins.

Every figure is a replayed graph of PER calls between two device events, divided by PER; SAMPLES such figures give the median and the
10th / 90th percentiles.  Kernel and torch statement are compared on the way: equal bytes.

    python scripts/bench_rle.py [--samples 20] [--per 5] [--stores 1024 16384] [--out profiles/rle/bench_rle.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import maskcrop, render, rle  # noqa: E402
from tests import render_cases  # noqa: E402

DEV = torch.device("cuda:0")
B, H, W, WIN, CROP = 32, 480, 640, 192, 128
NEAR, FAR, RADIUS, CHUNK, CAP = 0.01, 6.5, 0.1, 256, 2048


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


def silhouettes(ms, n, gen):
    """n rendered icosphere silhouettes (n,H,W) bool in chunks, encoded on the device chunk by chunk: the count lists on the host."""
    K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], device=DEV)
    lists = []
    for lo in range(0, n, CHUNK):
        m = min(CHUNK, n - lo)
        t = torch.cat(((torch.rand(m, 1, generator=gen) - 0.5) * 0.5, (torch.rand(m, 1, generator=gen) - 0.5) * 0.3, 0.75 + 0.25 * torch.rand(m, 1, generator=gen)), -1).to(DEV)
        R = torch.eye(3, device=DEV).expand(m, 3, 3).contiguous()
        d = render.render_depth(ms, ms.index_of([0] * m), R, t.contiguous(), K.expand(m, 3, 3).contiguous(), (H, W), near=NEAR, far=FAR).depth
        enc = rle.encode(d > 0, cap=CAP)
        assert not enc.info.any()
        c, k = enc.counts.cpu().numpy().view(np.uint32), enc.n_runs.cpu().numpy()
        lists += [c[i, :k[i]].copy() for i in range(m)]
    return lists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--per", type=int, default=5)
    ap.add_argument("--stores", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle", "bench_rle.json"))
    a = ap.parse_args()
    v, f = render_cases.icosphere(3, RADIUS)
    ms = render.MeshSet([(v, f)], DEV)
    gen = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    lists, rows = [], []
    for F in a.stores:
        lists += silhouettes(ms, F - len(lists), gen)
        store = rle.RleStore.from_counts(lists[:F], (H, W), device=DEV)
        assert not store.valid.any() and int(store.area.min()) > 0
        index = torch.from_numpy(rng.choice(F, B, replace=False).astype(np.int32)).to(DEV)
        origin = store.window_origins(index, (WIN, WIN))
        frames = (torch.empty((B, H, W), dtype=torch.uint8, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))
        wins = (torch.empty((B, WIN, WIN), dtype=torch.uint8, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))
        # the torch statement's inputs, prepared outside the timed region
        off = store.offsets.cpu().numpy()
        per_row = [store.counts[off[i]:off[i + 1]].long() & 0xFFFFFFFF for i in index.cpu().tolist()]
        values = [(torch.arange(len(c), device=DEV) & 1).to(torch.uint8) for c in per_row]
        plain_out = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)

        def plain():
            for b in range(B):
                plain_out[b] = torch.repeat_interleave(values[b], per_row[b], output_size=H * W).view(W, H).t()

        box = store.box[index.long()].float()
        zoom = CROP / (1.5 * torch.maximum(box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]).clamp(min=8.0))
        cx, cy = (box[:, 0] + box[:, 2]) * 0.5, (box[:, 1] + box[:, 3]) * 0.5
        M = torch.zeros(B, 2, 3, device=DEV)
        M[:, 0, 0] = M[:, 1, 1] = zoom
        M[:, 0, 2], M[:, 1, 2] = CROP * 0.5 - zoom * cx, CROP * 0.5 - zoom * cy
        mk = dict(valid_th=100, n_check=256, seed=17)

        rle.decode(store, index, None, (H, W), out=frames)
        rle.decode(store, index, origin, (WIN, WIN), out=wins)
        plain()
        torch.cuda.synchronize()
        assert torch.equal(frames[0], plain_out) and not frames[1].any() and not wins[1].any()
        a_full = maskcrop.mask_crops(frames[0], M, (CROP, CROP), **mk)
        a_win = maskcrop.mask_crops(wins[0], M, (CROP, CROP), origin=origin, **mk)
        assert all(torch.equal(x, y) for x, y in zip(a_full, a_win)) and int(a_full.valid_cnt.min()) >= 256  # the windows hold every object whole
        enc_in = frames[0].clone()
        enc_out = tuple(torch.empty(s, dtype=torch.int32, device=DEV) for s in ((B, CAP), (B,), (B,)))
        rle.encode(enc_in, cap=CAP, out=enc_out)
        torch.cuda.synchronize()
        assert not enc_out[2].any() and all(np.array_equal(enc_out[0][b, :int(enc_out[1][b])].cpu().numpy(), per_row[b].int().cpu().numpy()) for b in range(B))

        def crops_after_decode():
            rle.decode(store, index, origin, (WIN, WIN), out=wins)
            return maskcrop.mask_crops(wins[0], M, (CROP, CROP), origin=origin, **mk)

        timed = dict(index=store.index,
                     decode_full_frames=lambda: rle.decode(store, index, None, (H, W), out=frames),
                     decode_windows_192=lambda: rle.decode(store, index, origin, (WIN, WIN), out=wins),
                     torch_statement_full_frames=plain,
                     decode_windows_192_then_mask_crops=crops_after_decode,
                     mask_crops_alone_on_resident_windows=lambda: maskcrop.mask_crops(wins[0], M, (CROP, CROP), origin=origin, **mk),
                     encode_full_frames=lambda: rle.encode(enc_in, cap=CAP, out=enc_out),
                     fill_full_frames=lambda: frames[0].zero_(),  # the fills last: they clear what the rows above read
                     fill_windows_192=lambda: wins[0].zero_())
        row = dict(masks=F, counts=store.T, mean_runs=store.T / F, store_bytes=store.T * 8 + (F + 1) * 8 + F * 8 + F * 24, B=B, frame_hw=[H, W],
                   window_hw=[WIN, WIN], crop_hw=[CROP, CROP], n_check=256,
                   bytes_per_step_no_longer_uploaded=dict(full_frames=B * H * W - B * 4, windows_192=B * WIN * WIN - B * 12),
                   timings={k: graph_samples(fn, a.samples, a.per) for k, fn in timed.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(dict(device=torch.cuda.get_device_name(0), samples=a.samples, launches_per_graph=a.per, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
