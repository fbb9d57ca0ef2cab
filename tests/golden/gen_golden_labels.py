"""Writes tests/golden/labels_*.npz: the unmodified reference's `losses.annots_on_the_fly` run on the CPU, in float32 and in float64
on the same synthetic inputs (built here).  Inputs are stored as `in_*` (the ragged candidate list as `in_Rt_candi_<c>`), the float32
outputs as `f32_*`, the float64 ones as `f64_*`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_labels.py /path/to/reference
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(rng, B, H, W):
    """Camera, pose, homogeneous depth of a box-shaped object filling the crop, its mask, noc_scale."""
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = rng.uniform(90, 110, B)
    K[:, 1, 1] = rng.uniform(90, 110, B)
    K[:, 0, 1] = rng.uniform(-1, 1, B)
    K[:, 0, 2] = W / 2 + rng.uniform(-2, 2, B)
    K[:, 1, 2] = H / 2 + rng.uniform(-2, 2, B)
    K[:, 2, 2] = 1
    R = np.stack([rot(rng) for _ in range(B)])
    t = np.stack([rng.uniform(-20, 20, B), rng.uniform(-20, 20, B), rng.uniform(550, 650, B)], -1)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = t[:, 2, None, None] + rng.uniform(-40, 40, (B, H, W))
    homo_z = np.stack([u[None] * z, v[None] * z, z + 0 * u[None]], -1)
    yy, xx = (v - H / 2) / (H / 2), (u - W / 2) / (W / 2)
    msk = (yy[None] ** 2 + xx[None] ** 2 < rng.uniform(0.5, 0.9, (B, 1, 1)))
    noc_scale = rng.uniform(110, 140, (B, 3))
    return K, R, t, homo_z, msk, noc_scale


def check_points(rng, msk, N):
    out = np.zeros((len(msk), N, 2), dtype=np.int64)
    for b, m in enumerate(msk):
        ys, xs = np.nonzero(m)
        i = rng.choice(len(ys), N, replace=len(ys) < N)
        out[b] = np.stack([xs[i], ys[i]], -1)
    return out


def model_transform(rng, B):
    T = np.zeros((B, 4, 4))
    for b in range(B):
        T[b, :3, :3] = rot(rng)
        T[b, :3, 3] = rng.uniform(-5, 5, 3)
    T[:, 3, 3] = 1
    return T


def candidates(symmetry, R, t, info):
    return np.stack([symmetry.symmetry_pose_candidates(R[b], t[b], info) for b in range(len(R))])


def cases(symmetry):
    rng = np.random.default_rng(20261016)
    out = {}
    # 1. no symmetry: one chunk with K = 1, binary head, bit_cnt [7,7,6], model transform
    B, H, W = 3, 16, 24
    K, R, t, hz, msk, sc = scene(rng, B, H, W)
    out["nosym"] = dict(
        Rt_candi=[np.concatenate((R, t[..., None]), -1)[:, None]], homo_z_out=hz, R_no_aug=R, t_no_aug=t, K_no_aug=K, msk_noc=msk, noc_scale=sc,
        model_transform=model_transform(rng, B), bit_cnt=[7, 7, 6], sym_ck_pts2d=check_points(rng, msk, 16),
        out=dict(xyz_noc_bin=rng.normal(size=(B, 20, H, W))), cfg=dict(sym_aware_start=0), step=10)
    # 2. discrete symmetry, 3D branch: chunks {K=1 x2, K=4 x3}, binary-code logits, 64 check points, one sample with only -1 check points
    B, H, W = 5, 32, 32
    K, R, t, hz, msk, sc = scene(rng, B, H, W)
    syms = {"symmetries_discrete": [np.eye(4).reshape(-1).tolist() for _ in range(3)]}
    for i, ax in enumerate(([1, 0, 0], [0, 1, 0], [0, 0, 1])):
        S = np.eye(4)
        S[:3, :3] = np.diag([1.0 if j == i else -1.0 for j in range(3)])
        S[:3, 3] = rng.uniform(-3, 3, 3)
        syms["symmetries_discrete"][i] = S.reshape(-1).tolist()
    c1 = np.concatenate((R[:2], t[:2, :, None]), -1)[:, None]
    c4 = candidates(symmetry, R[2:], t[2:], syms)
    ck = check_points(rng, msk, 64)
    ck[3] = -1
    out["discrete3d"] = dict(
        Rt_candi=[c1, c4], homo_z_out=hz, R_no_aug=R, t_no_aug=t, K_no_aug=K, msk_noc=msk, noc_scale=sc, model_transform=model_transform(rng, B),
        bit_cnt=[7, 7, 6], sym_ck_pts2d=ck, out=dict(xyz_noc_bin=rng.normal(size=(B, 20, H, W))), cfg=dict(sym_aware_start=0), step=0)
    # 3. continuous symmetry, 3D branch: K = 384 from the reference's own candidate generator, continuous xyz_noc head, N = 256
    B, H, W = 4, 32, 32
    K, R, t, hz, msk, sc = scene(rng, B, H, W)
    info = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.0, 0.0, 4.0]}]}
    cand = candidates(symmetry, R, t, info)
    kt = rng.integers(0, 384, B)  # the pose the head "saw"
    q = np.einsum("bij,bhwj->bhwi", np.linalg.inv(K), hz)
    xyz = np.einsum("bji,bhwj->bhwi", cand[np.arange(B), kt, :, :3], q - cand[np.arange(B), kt, None, None, :, 3])
    noc = (xyz / sc[:, None, None]).transpose(0, 3, 1, 2) + rng.normal(scale=0.02, size=(B, 3, H, W))
    out["continuous3d"] = dict(
        Rt_candi=[cand], homo_z_out=hz, R_no_aug=R, t_no_aug=t, K_no_aug=K, msk_noc=msk, noc_scale=sc, sym_ck_pts2d=check_points(rng, msk, 256),
        out=dict(xyz_noc=noc), cfg=dict(sym_aware_start=100), step=100)
    # 4. 2D branch: pts2d in out_dict, K = 384, 8 keypoints
    B, H, W, N = 4, 16, 16, 8
    K, R, t, hz, msk, sc = scene(rng, B, H, W)
    cand = candidates(symmetry, R, t, info)
    pts3d = rng.uniform(-50, 50, (B, N, 3))
    kt = rng.integers(0, 384, B)
    Xc = np.einsum("bij,bnj->bni", cand[np.arange(B), kt, :, :3], pts3d) + cand[np.arange(B), kt, None, :, 3]
    h = np.einsum("bij,bnj->bni", K, Xc)
    uv = h[..., :2] / h[..., 2:] + rng.normal(scale=0.5, size=(B, N, 2))
    out["pts2d"] = dict(
        Rt_candi=[cand], homo_z_out=hz, R_no_aug=R, t_no_aug=t, K_no_aug=K, msk_noc=msk, noc_scale=sc, model_transform=model_transform(rng, B),
        bit_cnt=[6, 6, 6], out_K=K, pts3d=pts3d, out=dict(pts2d=uv), cfg={}, step=0)
    # 5. not yet started: step < sym_aware_start (candidate 0 of every chunk)
    B, H, W = 4, 16, 16
    K, R, t, hz, msk, sc = scene(rng, B, H, W)
    c4 = candidates(symmetry, R[1:], t[1:], syms)
    out["notstarted"] = dict(
        Rt_candi=[np.concatenate((R[:1], t[:1, :, None]), -1)[:, None], c4], homo_z_out=hz, R_no_aug=R, t_no_aug=t, K_no_aug=K, msk_noc=msk,
        noc_scale=sc, model_transform=model_transform(rng, B), bit_cnt=[5, 5, 5], sym_ck_pts2d=check_points(rng, msk, 32),
        out=dict(xyz_noc_bin=rng.normal(size=(B, 15, H, W))), cfg=dict(sym_aware_start=5000), step=4999)
    return out


def run(losses, case, dtype):
    def T(a):
        a = np.asarray(a)
        return torch.from_numpy(a).to(dtype) if a.dtype.kind == "f" else torch.from_numpy(a)

    gt = {k: ([T(c) for c in v] if k == "Rt_candi" else (list(v) if k == "bit_cnt" else T(v))) for k, v in case.items()
          if k not in ("out", "cfg", "step")}
    out = {k: T(v) for k, v in case["out"].items()}
    losses.annots_on_the_fly(gt, out, dict(case["cfg"]), case["step"])
    keys = ["Rt_best", "pose_best", "xyz_gt", "xyz_noc_tgt", "xyz_noc_bin_tgt", "xyz_noc_bin_raw"]
    return {k: gt[k].numpy() for k in keys if k in gt}


def main(ref):
    sys.path.insert(0, ref)
    import losses
    import symmetry

    for name, case in cases(symmetry).items():
        rec = {}
        for k, v in case.items():
            if k == "Rt_candi":
                for i, c in enumerate(v):
                    rec[f"in_Rt_candi_{i}"] = np.asarray(c, np.float32)
            elif k == "out":
                rec.update({f"out_{kk}": np.asarray(vv, np.float32) for kk, vv in v.items()})
            elif k == "cfg":
                rec["sym_aware_start"] = np.int64(v.get("sym_aware_start", 0)) if v else np.int64(-1)
            elif k == "step":
                rec["step"] = np.int64(v)
            elif k == "bit_cnt":
                rec["bit_cnt"] = np.asarray(v, np.int64)
            else:
                a = np.asarray(v)
                rec[f"in_{k}"] = a.astype(np.float32) if a.dtype.kind == "f" else a
        # both runs read the float32 values: the float64 run is the same inputs, exactly up-cast
        case32 = {k: ([c.astype(np.float32) for c in v] if k == "Rt_candi" else
                      ({kk: vv.astype(np.float32) for kk, vv in v.items()} if k == "out" else
                       (np.asarray(v).astype(np.float32) if np.asarray(v).dtype.kind == "f" and k not in ("cfg", "step", "bit_cnt") else v)))
                  for k, v in case.items()}
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            rec.update({f"{tag}_{k}": v for k, v in run(losses, case32, dt).items()})
        path = os.path.join(HERE, f"labels_{name}.npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LC_REFERENCE", ""))
