#!/usr/bin/env python3
"""Label preparation per training step: lc_amd.labels.annots_on_the_fly against its fp32 torch statement (the reference's formulas,
tests/labels_oracle.py on the device), eager and graph-replayed, at three shapes.  One JSON line per shape:

    zlmo_nosym   B = 32, 128 x 128, 21 code planes, no symmetric candidates
    gycbv_3d     B = 32, 64 x 64, continuous head, K = 384 candidates, N = 256 check points (3D branch)
    sym_2d       B = 32, 64 x 64, continuous head, K = 384 candidates, 8 keypoints (2D branch)

`tgt_*`: the streaming launch alone (lc_label_targets_f32, 20 launches per replayed graph), its algorithmic bytes (homo_z and the mask in;
xyz_gt and the targets out) and that traffic / time / 8 TB/s.

    python scripts/bench_labels.py [--iters 50]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import labels  # noqa: E402
from lc_amd.labels import _targets  # noqa: E402
from tests import labels_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")


def batch(kind, gen):
    B = 32
    H = W = 128 if kind == "zlmo_nosym" else 64
    K = torch.tensor([[2.3 * W, 0, W / 2], [0, 2.3 * H, H / 2], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))[0].float()
    t = torch.cat((torch.randn(B, 2, generator=gen) * 5, 600 + torch.rand(B, 1, generator=gen) * 50), -1)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = t[:, 2, None, None] + torch.rand(B, H, W, generator=gen) * 60 - 30
    gt = dict(homo_z_out=torch.stack((u * z, v * z, z), -1), R_no_aug=R, t_no_aug=t, K_no_aug=K, out_K=K,
              msk_noc=(((u - W / 2) ** 2 + (v - H / 2) ** 2) < (0.35 * W) ** 2).expand(B, H, W).contiguous(), noc_scale=torch.full((B, 3), 120.0))
    Rt = torch.cat((R, t[..., None]), -1)
    if kind == "zlmo_nosym":
        gt.update(Rt_candi=[Rt[:, None]], model_transform=torch.eye(4).expand(B, 4, 4).contiguous(), bit_cnt=[7, 7, 7])
        out = dict(xyz_noc_bin=torch.randn(B, 21, H, W, generator=gen))
    else:
        ang = torch.arange(384) * (2 * torch.pi / 384)
        Rz = torch.zeros(384, 3, 3)
        Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = ang.cos(), -ang.sin(), ang.sin(), ang.cos(), 1
        gt["Rt_candi"] = [torch.cat((R[:, None] @ Rz, t[:, None, :, None].expand(B, 384, 3, 1)), -1)]
        out = dict(xyz_noc=torch.randn(B, 3, H, W, generator=gen) * 0.3)
        if kind == "gycbv_3d":
            gt["sym_ck_pts2d"] = torch.randint(16, 48, (B, 256, 2), generator=gen)
        else:
            gt["pts3d"] = torch.randn(B, 8, 3, generator=gen) * 40
            out["pts2d"] = torch.rand(B, 8, 2, generator=gen) * W
    return ({k: ([c.to(DEV) for c in v] if isinstance(v, list) and torch.is_tensor(v[0]) else (v.to(DEV) if torch.is_tensor(v) else v))
             for k, v in gt.items()}, {k: v.to(DEV) for k, v in out.items()})


def torch_annots(gt, out, cfg, step):
    """The reference's label preparation restated in fp32 torch (no host round trip: inv_ex, argmin, gather)."""
    cand = gt["Rt_candi"]
    if len(cand) == 1 and cand[0].shape[1] == 1:
        Rt_best = cand[0][:, 0]
        Rt = torch.cat((gt["R_no_aug"], gt["t_no_aug"][..., None]), -1)
    else:
        c = cand[0]
        if "pts2d" in out:
            e = O.candidate_errors(0, gt["out_K"], gt["pts3d"], out["pts2d"], c)
        else:
            ck = gt["sym_ck_pts2d"]
            B, H, W = gt["homo_z_out"].shape[:3]
            x, y = ck[..., 0] % W, ck[..., 1] % H
            bi = torch.arange(B, device=DEV)[:, None].expand_as(x)
            hz, p = gt["homo_z_out"][bi, y, x], out["xyz_noc"][bi, :, y, x] * gt["noc_scale"][:, None, :]
            R, t = c[..., :3, :3], c[..., :3, 3]
            q = torch.einsum("bij,bnj->bni", torch.linalg.inv_ex(gt["K_no_aug"])[0], hz)
            ref = torch.einsum("bkji,bknj->bkni", R, q[:, None] - t[:, :, None, :])
            e = torch.linalg.vector_norm(p[:, None] - ref, dim=-1).mean(-1)
        Rt_best = c[torch.arange(c.shape[0], device=DEV), torch.argmin(e, -1)]
        Rt = Rt_best
    R, t = Rt[:, :3, :3], Rt[:, :3, 3]
    q = torch.einsum("bij,bhwj->bhwi", torch.linalg.inv_ex(gt["K_no_aug"])[0], gt["homo_z_out"])
    m = gt["msk_noc"].unsqueeze(-1)
    xyz = torch.einsum("bji,bhwj->bhwi", R, q - t[:, None, None, :]) * m
    T, bits = gt.get("model_transform"), gt.get("bit_cnt")
    y = xyz if T is None else (torch.einsum("bij,bhwj->bhwi", T[:, :3, :3], xyz) + T[:, None, None, :3, 3]) * m
    noc = y / gt["noc_scale"][:, None, None, :]
    res = dict(Rt_best=Rt_best, xyz_gt=xyz)
    if bits is None:
        res["xyz_noc_tgt"] = noc.permute(0, 3, 1, 2)
    else:
        mods, raws = [], []
        for a, n in enumerate(bits):
            mx = 2 ** n - 1
            v = torch.clamp((noc[..., a] + 1) * (mx * 0.5), 0, mx).round().to(torch.int32)
            sh = torch.arange(n - 1, -1, -1, device=DEV, dtype=torch.int32)
            raw = ((v.unsqueeze(-1) >> sh) & 1).bool()
            g = raw.clone()
            g[..., 1:] ^= raw[..., :-1]
            g[..., :2] = ~g[..., :2]
            mods.append(g)
            raws.append(raw)
        res["xyz_noc_bin_tgt"] = torch.cat(mods, -1).permute(0, 3, 1, 2)
        res["xyz_noc_bin_raw"] = torch.cat(raws, -1).permute(0, 3, 1, 2)
    gt.update(res)


def eager_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def graph_us(fn, iters, per=1):
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
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters / per * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    cfg = {"sym_aware_start": 0}
    for kind in ("zlmo_nosym", "gycbv_3d", "sym_2d"):
        gt, out = batch(kind, gen)
        g_nat, g_ref = dict(gt), dict(gt)
        nat = lambda: labels.annots_on_the_fly(g_nat, out, cfg, 1)
        ref = lambda: torch_annots(g_ref, out, cfg, 1)
        rec = dict(shape=kind, B=32, H=gt["homo_z_out"].shape[1], W=gt["homo_z_out"].shape[2], K=gt["Rt_candi"][0].shape[1])
        rec["native_eager_us"] = round(eager_us(nat, a.iters), 2)
        rec["torch_eager_us"] = round(eager_us(ref, a.iters), 2)
        rec["native_graph_us"] = round(graph_us(nat, a.iters), 2)
        try:
            rec["torch_graph_us"] = round(graph_us(ref, a.iters), 2)
        except Exception as e:  # noqa: BLE001
            rec["torch_graph_us"] = None
            rec["torch_graph_error"] = str(e)[:120]
        # the streaming launch alone
        bits = gt.get("bit_cnt")
        Rt = torch.cat((gt["R_no_aug"], gt["t_no_aug"][..., None]), -1)
        tgt = lambda: _targets(gt["homo_z_out"], Rt, gt["K_no_aug"], msk=gt["msk_noc"], noc_scale=gt["noc_scale"], xform=gt.get("model_transform"),
                               bit_cnt=bits, want_targets=True)
        us = graph_us(tgt, a.iters, per=20)
        B, H, W = gt["homo_z_out"].shape[:3]
        nbytes = B * H * W * (12 + 1 + 12 + (2 * sum(bits) if bits else 12))
        rec.update(tgt_us=round(us, 2), tgt_bytes=nbytes, tgt_frac_of_8TBps=round(nbytes / (us * 1e-6) / 8e12, 3))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
