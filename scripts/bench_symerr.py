#!/usr/bin/env python3
"""The symmetry-aware pose errors (lc_amd.metrics.compute_sym_pose_errors: mssd, mspd, proj in one call) on 64 poses of 5 000 vertices:
K = 1 symmetry per object, K = 384 (one continuous axis at BOP's step count) and a mixed batch (K in {1, 4, 384, 768}, sixteen poses
each, interleaved).  Beside each, a plain torch statement of the same three errors on the device, float64 like the kernel (one batched
expression per object group: every symmetry of a pose at once).

Every figure is a replayed graph of PER calls between two device events, divided by PER; SAMPLES such figures give the median and the
10th / 90th percentiles.  The two sides are compared on the way (2e-5 relative).

    python scripts/bench_symerr.py [--samples 20] [--per 5]       -> profiles/symerr/bench_symerr.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import metrics, symmetry  # noqa: E402

DEV = torch.device("cuda:0")
B, M = 64, 5000


def symset():
    flip = np.eye(4)
    flip[:3, :3] = np.diag([1.0, -1, -1])
    cont = [{"axis": [0.0, 0.0, 1.0], "offset": [0.0, 0.0, 4.0]}]
    quarter = []
    for q in (1, 2, 3):
        S = np.eye(4)
        S[:3, :3] = symmetry.rodrigues([0, 0, 1.0], q * np.pi / 2)
        quarter.append(S.ravel().tolist())
    info = {1: {}, 4: {"symmetries_discrete": quarter}, 384: {"symmetries_continuous": cont},
            768: {"symmetries_continuous": cont, "symmetries_discrete": [flip.ravel().tolist()]}}
    return symmetry.SymmetrySet.from_models_info(info, device=DEV)


def batch(gen, ss, obj):
    Rg = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))[0]
    Rg = Rg * torch.linalg.det(Rg)[:, None, None]
    w = torch.randn(B, 3, generator=gen, dtype=torch.float64) * 0.03
    Wx = torch.zeros(B, 3, 3, dtype=torch.float64)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    Re = Rg @ torch.linalg.matrix_exp(Wx)
    tg = torch.cat((torch.randn(B, 2, generator=gen, dtype=torch.float64) * 40, 800 + torch.rand(B, 1, generator=gen, dtype=torch.float64) * 200), -1)
    te = tg + torch.randn(B, 3, generator=gen, dtype=torch.float64) * 2
    K = torch.tensor([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])
    d = dict(R_est=Re.float(), t_est=te.float(), R_gt=Rg.float(), t_gt=tg.float(), cam_K=K.expand(B, 3, 3).contiguous(),
             pts=(torch.rand(M, 3, generator=gen) * 2 - 1) * 50)
    d = {k: v.to(DEV).contiguous() for k, v in d.items()}
    d["index"] = ss.index_of(torch.tensor(obj, device=DEV)).contiguous()
    return d


def torch_statement(d, ss, groups):
    """mssd, mspd, proj (B,) float64 with plain torch ops on the device; `groups`: (pose rows, table offset, K) per object, host-known."""
    p = d["pts"].double()
    ph = torch.cat((p, torch.ones_like(p[:, :1])), 1)  # (M,4)
    Re, te, Rg, tg, Kc = (d[k].double() for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K"))
    Pe = Kc @ torch.cat((Re, te[..., None]), -1)                    # (B,3,4)
    he = ph @ Pe.mT                                                  # (B,M,3)
    ue = he[..., :2] / he[..., 2:]
    hg = ph @ (Kc @ torch.cat((Rg, tg[..., None]), -1)).mT
    proj = (ue - hg[..., :2] / hg[..., 2:]).norm(dim=-1).mean(-1)
    mssd, mspd = torch.empty(B, device=DEV, dtype=torch.float64), torch.empty(B, device=DEV, dtype=torch.float64)
    for rows, off, K in groups:
        S = ss.table[off:off + K].reshape(K, 3, 4)
        Rgs = Rg[rows, None] @ S[None, :, :, :3]                     # (b,K,3,3)
        tgs = (Rg[rows, None] @ S[None, :, :, 3:])[..., 0] + tg[rows, None]
        D = Re[rows, None] - Rgs
        d3 = p @ D.mT + (te[rows, None] - tgs)[:, :, None]           # (b,K,M,3)
        mssd[rows] = d3.norm(dim=-1).amax(-1).amin(-1)
        h = ph @ (Kc[rows, None] @ torch.cat((Rgs, tgs[..., None]), -1)).mT
        mspd[rows] = (ue[rows, None] - h[..., :2] / h[..., 2:]).norm(dim=-1).amax(-1).amin(-1)
    return mssd, mspd, proj


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--per", type=int, default=5)
    a = ap.parse_args()
    ss = symset()
    gen = torch.Generator().manual_seed(0)
    rows = []
    for name, obj in (("K1", [1] * B), ("K384", [384] * B), ("mixed_1_4_384_768", [1, 4, 384, 768] * (B // 4))):
        d = batch(gen, ss, obj)
        idx = ss.host_index_of(obj)
        groups = [(torch.tensor(np.nonzero(idx == i)[0], device=DEV), int(ss.obj_off_host[i]), int(ss.obj_k_host[i])) for i in sorted(set(idx.tolist()))]

        def kernel():
            return metrics.compute_sym_pose_errors(d["R_est"], d["t_est"], d["R_gt"], d["t_gt"], d["cam_K"], d["pts"], ss, d["index"])

        def plain():
            return torch_statement(d, ss, groups)

        got, want = kernel(), plain()
        torch.cuda.synchronize()
        for key, w in zip(("mssd", "mspd", "proj"), want):
            rel = ((got[key].double() - w).abs() / w.abs().clamp_min(1)).max().item()
            assert rel <= 2e-5, (name, key, rel)
        pairs = int(sum(ss.obj_k_host[i] for i in idx)) * M
        row = dict(config=name, B=B, M=M, vertex_symmetry_pairs=pairs, kernel=graph_samples(kernel, a.samples, a.per),
                   torch_float64=graph_samples(plain, a.samples, a.per))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = os.path.join(ROOT, "profiles", "symerr")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_symerr.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), samples=a.samples, launches_per_graph=a.per, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
