#!/usr/bin/env python3
"""The symmetry selection with its candidates formed in the launch (lc_sym_select_table_f32) against lc_sym_select_f32 on the same
candidates already resident on the device, and against materialise (lc_sym_candidates_f32) then select.  B = 32, N = 256 check points, 3D
mode through the check pixels (homo_z map + continuous xyz map, 64 x 64).  Three batches: K = 384 in every row, a mixed batch
(K in {1, 4, 384, 768}, eight rows each, grouped by K so that the chunk table can express it), K = 768 in every row.

Every figure is a replayed graph of PER launches between two device events, divided by PER; SAMPLES such figures give the median and the
10th / 90th percentiles.  `pcie_bytes_saved`: the candidate bytes (K x 48 per row) that no longer cross the bus per step, from shapes.

    python scripts/bench_symcand.py [--samples 30] [--per 20]       -> profiles/symcand/bench_symcand.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import _lib, labels, symmetry  # noqa: E402

DEV = torch.device("cuda:0")
B, N, H, W = 32, 256, 64, 64


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
    K = torch.tensor([[2.3 * W, 0, W / 2], [0, 2.3 * H, H / 2], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))[0].float()
    t = torch.cat((torch.randn(B, 2, generator=gen) * 5, 600 + torch.rand(B, 1, generator=gen) * 50), -1)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = t[:, 2, None, None] + torch.rand(B, H, W, generator=gen) * 60 - 30
    d = dict(K=K, base=torch.cat((R, t[..., None]), -1), hz=torch.stack((u * z, v * z, z), -1), xyz=torch.randn(B, 3, H, W, generator=gen) * 0.3,
             sc=torch.full((B, 3), 120.0), ck=torch.randint(16, 48, (B, N, 2), generator=gen))
    d = {k: v.to(DEV).contiguous() for k, v in d.items()}
    d["index"] = ss.index_of(torch.tensor(obj, device=DEV)).contiguous()
    return d


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
    for _ in range(3):
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
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--per", type=int, default=20)
    a = ap.parse_args()
    lib = _lib.load()
    ss = symset()
    gen = torch.Generator().manual_seed(0)
    rows = []
    for name, obj in (("K384", [384] * B), ("mixed_1_4_384_768", [1] * 8 + [4] * 8 + [384] * 8 + [768] * 8), ("K768", [768] * B)):
        d = batch(gen, ss, obj)
        ks = ss.obj_k_host[ss.host_index_of(obj)].astype(np.int64)
        offs = ks.cumsum() - ks
        total = int(ks.sum())
        cand = torch.empty(total, 3, 4, device=DEV)
        row_off = torch.as_tensor(offs, dtype=torch.int32).to(DEV)
        Rt = [torch.empty(B, 3, 4, device=DEV) for _ in range(2)]
        idx = [torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(2)]
        # the chunk table of the grouped batch
        uniq = sorted(set(ks.tolist()))
        chunk_k = (ctypes.c_int * len(uniq))(*uniq)
        chunk_rows = (ctypes.c_int * (len(uniq) + 1))(*([int((ks < k).sum()) for k in uniq] + [B]))
        p = _lib.ptr
        st = lambda: _lib.stream_ptr(DEV)
        rest = lambda o: (1, p(d["K"]), None, None, p(d["xyz"]), 0, 0, p(d["sc"]), p(d["hz"]), p(d["ck"]), B, N, H, W, p(Rt[o]), p(idx[o]), st())

        def table():
            assert lib.lc_sym_select_table_f32(p(d["base"]), p(d["index"]), *labels._table_args(ss), *rest(0)) == 0

        def materialise():
            assert lib.lc_sym_candidates_f32(p(d["base"]), p(d["index"]), *labels._table_args(ss), p(row_off), B, p(cand), total, st()) == 0

        def resident():
            assert lib.lc_sym_select_f32(p(cand), chunk_rows, chunk_k, len(uniq), *rest(1)) == 0

        def pair():
            materialise()
            resident()

        materialise()
        table()
        resident()
        torch.cuda.synchronize()
        assert torch.equal(idx[0], idx[1]) and torch.equal(Rt[0].view(torch.int32), Rt[1].view(torch.int32)), name
        row = dict(config=name, B=B, N=N, candidates=total, pcie_bytes_saved=total * 48,
                   table_launch=graph_samples(table, a.samples, a.per), resident_candidates_launch=graph_samples(resident, a.samples, a.per),
                   materialise_then_select=graph_samples(pair, a.samples, a.per))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = os.path.join(ROOT, "profiles", "symcand")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_symcand.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), samples=a.samples, launches_per_graph=a.per, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
