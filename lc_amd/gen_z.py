"""The offline z_crop tool without OpenGL, mmcv or trimesh: what the reference's `tools/gen_z.py` writes, rendered by lc_amd.render.

    python -m lc_amd.gen_z --data_dir DATA --model_dir MODELS [--xyz_root OUT] [--begin B --end E | --scene S] [--remove_existing]

For every annotated instance of every scene under DATA (`scene_gt.json`, `scene_camera.json`) it renders the 480 x 640 depth of
`MODELS/obj_<id>.ply` (mm, scaled to metres) with near 0.01 m / far 6.5 m (gen_z.py:73-76,141-153) and writes
`OUT/<scene>/<im>_<anno>.pkl.gz`: a gzipped pickle of `z_crop` (uint16, round((z - z_min) / (z_max - z_min + 1e-30) * 65534 + 1) on
hit pixels, cropped to the hit box), `xyxy`, and `z_max`, `z_min` in mm.  An instance that is not visible gets the reference's
record (a full-frame zero z_crop, z_max = z_min = 0).  The encode runs on the device; only the cropped patch comes back.

Instances whose object has no model file in MODELS are skipped, as the reference skips objects outside its class table.
"""
from __future__ import annotations

import argparse
import glob
import gzip
import json
import os
import pickle
import re
import shutil
import sys

import numpy as np

IM_H, IM_W = 480, 640
NEAR, FAR = 0.01, 6.5  # metres

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """(verts (Nv,3) float32, faces (Nf,3) int32) of an ascii or binary_little_endian PLY: `vertex` x y z and `face`
    vertex_indices / vertex_index; every other property and element is skipped by its declared size.  Polygons are fanned."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header")
    if not blob.startswith(b"ply") or end < 0:
        raise ValueError(f"lc_amd.gen_z: {path} is not a PLY file")
    nl = blob.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"lc_amd.gen_z: {path}: truncated header")
    header, pos = blob[:end].decode("ascii", "replace").splitlines(), nl + 1
    fmt, elements = None, []
    for ln in header:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"lc_amd.gen_z: {path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"lc_amd.gen_z: {path}: format {fmt} is not supported (ascii, binary_little_endian)")
    verts = faces = None
    tokens = blob[pos:].split() if fmt == "ascii" else None
    ti = 0
    for name, count, props in elements:
        has_list = any(p[2] is not None for p in props)
        rows = []
        if fmt == "binary_little_endian" and not has_list:
            dt = np.dtype([(p[0], "<" + p[1]) for p in props])
            arr = np.frombuffer(blob, dtype=dt, count=count, offset=pos)
            pos += count * dt.itemsize
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], -1).astype(np.float32)
            continue
        for _ in range(count):
            row = {}
            for pname, t0, t1 in props:
                if fmt == "ascii":
                    if t1 is None:
                        row[pname] = float(tokens[ti])
                        ti += 1
                    else:
                        n = int(tokens[ti])
                        row[pname] = [int(float(x)) for x in tokens[ti + 1:ti + 1 + n]]
                        ti += 1 + n
                else:
                    if t1 is None:
                        d = np.dtype("<" + t0)
                        row[pname] = np.frombuffer(blob, dtype=d, count=1, offset=pos)[0]
                        pos += d.itemsize
                    else:
                        d0, d1 = np.dtype("<" + t0), np.dtype("<" + t1)
                        n = int(np.frombuffer(blob, dtype=d0, count=1, offset=pos)[0])
                        pos += d0.itemsize
                        row[pname] = np.frombuffer(blob, dtype=d1, count=n, offset=pos).tolist()
                        pos += n * d1.itemsize
            rows.append(row)
        if name == "vertex":
            verts = np.asarray([(r["x"], r["y"], r["z"]) for r in rows], dtype=np.float32).reshape(-1, 3)
        elif name == "face":
            tri = []
            for r in rows:
                idx = r.get("vertex_indices", r.get("vertex_index"))
                if idx is None:
                    raise ValueError(f"lc_amd.gen_z: {path}: faces without vertex_indices")
                tri += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
            faces = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    if verts is None or faces is None:
        raise ValueError(f"lc_amd.gen_z: {path}: needs a vertex and a face element")
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"lc_amd.gen_z: {path}: face indices outside [0, {len(verts)})")
    return verts, faces.astype(np.int32)


def load_models(model_dir, device, scale=0.001):
    """The `obj_<id>.ply` files of a BOP models directory as a lc_amd.render.MeshSet with the files' object ids (vertices times `scale`:
    0.001 takes the files' mm to the metres gen_z renders in)."""
    from . import render

    ids, meshes = [], []
    for path in sorted(glob.glob(os.path.join(model_dir, "obj_*.ply"))):
        m = re.fullmatch(r"obj_(\d+)\.ply", os.path.basename(path))
        if not m:
            continue
        v, f = read_ply(path)
        ids.append(int(m.group(1)))
        meshes.append((v * np.float32(scale), f))
    if not meshes:
        raise FileNotFoundError(f"lc_amd.gen_z: no obj_*.ply under {model_dir}")
    return render.MeshSet(meshes, device, obj_ids=ids)


def render_scene(meshes, scene_root, out_root, device):
    """One scene: every instance of every image, one launch per image."""
    import torch

    from . import render

    with open(os.path.join(scene_root, "scene_gt.json")) as f:
        gt = json.load(f)
    with open(os.path.join(scene_root, "scene_camera.json")) as f:
        cam = json.load(f)
    os.makedirs(out_root, exist_ok=True)
    written = 0
    for str_im_id, annos in gt.items():
        keep = [(i, a) for i, a in enumerate(annos) if int(a["obj_id"]) in meshes.obj_ids]
        if not keep:
            continue
        K = np.asarray(cam[str_im_id]["cam_K"], dtype=np.float32).reshape(1, 3, 3).repeat(len(keep), 0)
        R = np.stack([np.asarray(a["cam_R_m2c"], dtype=np.float32).reshape(3, 3) for _, a in keep])
        t = np.stack([np.asarray(a["cam_t_m2c"], dtype=np.float32).reshape(3) / np.float32(1000.0) for _, a in keep])
        idx = meshes.index_of([int(a["obj_id"]) for _, a in keep])
        out = render.render_depth(meshes, idx, torch.from_numpy(R).to(device), torch.from_numpy(t).to(device), torch.from_numpy(K).to(device),
                                  (IM_H, IM_W), near=NEAR, far=FAR)
        for row, (anno_i, a) in enumerate(keep):
            z_info = render.encode_z_info(out.depth[row])
            path = os.path.join(out_root, f"{int(str_im_id):06d}_{anno_i:06d}.pkl.gz")
            if np.asarray(z_info["z_max"]).reshape(-1)[0] == 0:
                print(f"not visible, scene {os.path.basename(scene_root)}, im {int(str_im_id)} obj {a['obj_id']}\n{path}")
            with gzip.open(path, "wb") as f:
                pickle.dump(z_info, f)
            written += 1
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description="gen z_crop (lc_amd.render)")
    ap.add_argument("--scene", type=int)
    ap.add_argument("--dataset", type=str, default=None, help="accepted for compatibility; the models found in --model_dir decide")
    ap.add_argument("--begin", type=int, default=0)
    ap.add_argument("--end", type=int, default=sys.maxsize)
    ap.add_argument("--remove_existing", action="store_true")
    ap.add_argument("--data_dir", type=str, required=True)
    ap.add_argument("--xyz_root", type=str)
    ap.add_argument("--model_dir", type=str)
    args = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lc_amd.gen_z: needs the HIP device (there is no CPU fallback)")
    xyz_root = args.xyz_root or os.path.join(args.data_dir, "z_crop")
    model_dir = args.model_dir or os.path.join(args.data_dir, "../models")
    begin, end = (args.scene, args.scene) if args.scene is not None else (args.begin, args.end)
    device = torch.device("cuda", torch.cuda.current_device())
    meshes = load_models(model_dir, device)
    scenes = sorted(int(s) for s in os.listdir(args.data_dir) if s.isdigit() and os.path.exists(os.path.join(args.data_dir, s, "scene_gt.json")))
    total = 0
    for sid in scenes:
        if sid < begin or sid > end:  # both ends included, as the reference's loop (gen_z.py:115)
            continue
        out = os.path.join(xyz_root, f"{sid:06d}")
        if os.path.isdir(out):
            if not args.remove_existing:
                print(f"{out} already exists, specify --remove_existing if you want to delete them")
                return 0  # as the reference: a message and exit status 0 (gen_z.py:120-122)
            shutil.rmtree(out)
        total += render_scene(meshes, os.path.join(args.data_dir, f"{sid:06d}"), out, device)
    print(f"lc_amd.gen_z: wrote {total} records under {xyz_root}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
