"""The per-object files every path reads, made from a directory of meshes by lc_amd.models (the sibling of `python -m lc_amd.gen_z`):

    python -m lc_amd.prep_models MODELS_DIR [--fps 256] [--scale 1.0] [--info-out PATH] [--fps-out PATH] [--xform [PATH]] [--xform-axis {x,y,z}] [--force]

Reads `MODELS_DIR/obj_<id>.ply` (lc_amd.gen_z.read_ply; vertices times `--scale`) and writes
  * `models_info.json` (default MODELS_DIR/models_info.json): BOP's `{"<id>": {diameter, min_x, min_y, min_z, size_x, size_y, size_z}}`,
    which `model_transform.load_composed_model_info` turns into `noc_scale`, `bbox_3d` and `diameter`;
  * the farthest-point pickle (default MODELS_DIR/fps.pkl; `--fps 0`: none): `{id: (count, 3) float32}`, what `cfg_global.fps` is
    loaded from (dataset.py:232-236; the loader slices `[:sparse_cnt]`, and the first n rows of a result are the n-point result).
  * with `--xform` (off by default; default path MODELS_DIR/models_xform.json), the reference's `models_xform.json`
    (`{"<id>": {"xform": 16 numbers, "xformed_noc_scale": 3 numbers}}`, model_transform.py:21-42): per object the rigid transform after which
    its bounding box is centred and as small as lc_amd.obox's stated grid search finds it, over all orientations or, with `--xform-axis`,
    over the turns about that model axis alone; an existing file is refused before anything is computed.
One line per object is printed.  An existing output is not overwritten without `--force`: an existing pickle is refused before anything
is computed; next to an existing `models_info.json` the stored diameter and extents are printed beside the computed ones and the
file is left as it is.  Needs the HIP device (there is no CPU fallback).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import pickle
import re
import sys

import numpy as np

from . import gen_z, models, obox
from .render import MeshSet

_KEYS = ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z")


def _device():
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lc_amd.prep_models: needs the HIP device (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def read_models(model_dir, scale=1.0):
    """(obj_ids, [(verts, faces)]) of the `obj_<id>.ply` files of a directory, sorted by file name."""
    ids, meshes = [], []
    for path in sorted(glob.glob(os.path.join(model_dir, "obj_*.ply"))):
        m = re.fullmatch(r"obj_(\d+)\.ply", os.path.basename(path))
        if not m:
            continue
        v, f = gen_z.read_ply(path)
        ids.append(int(m.group(1)))
        meshes.append((v * np.float32(scale), f))
    if not meshes:
        raise FileNotFoundError(f"lc_amd.prep_models: no obj_*.ply under {model_dir}")
    return ids, meshes


def _row(d):
    return "diameter {:.6g}  min ({:.6g}, {:.6g}, {:.6g})  size ({:.6g}, {:.6g}, {:.6g})".format(*(d[k] for k in _KEYS))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m lc_amd.prep_models", description="models_info.json and the FPS keypoint pickle of a directory of meshes")
    ap.add_argument("models_dir")
    ap.add_argument("--fps", type=int, default=256, help="farthest points per object (0: no pickle)")
    ap.add_argument("--scale", type=float, default=1.0, help="factor on the files' vertices")
    ap.add_argument("--info-out", default=None)
    ap.add_argument("--fps-out", default=None)
    ap.add_argument("--xform", nargs="?", const="", default=None, metavar="PATH", help="also write models_xform.json (default MODELS_DIR/models_xform.json)")
    ap.add_argument("--xform-axis", choices=("x", "y", "z"), default=None, help="search the turns about this model axis only (needs --xform)")
    ap.add_argument("--force", action="store_true", help="overwrite existing outputs")
    args = ap.parse_args(argv)
    xform_out = None if args.xform is None else (args.xform or os.path.join(args.models_dir, "models_xform.json"))
    if args.xform_axis is not None and xform_out is None:
        print("lc_amd.prep_models: --xform-axis needs --xform", file=sys.stderr)
        return 2
    if xform_out is not None and os.path.exists(xform_out) and not args.force:
        print(f"lc_amd.prep_models: {xform_out} already exists, specify --force to overwrite it", file=sys.stderr)
        return 1
    info_out = args.info_out or os.path.join(args.models_dir, "models_info.json")
    fps_out = args.fps_out or os.path.join(args.models_dir, "fps.pkl")
    if args.fps < 0:
        print("lc_amd.prep_models: --fps must not be negative", file=sys.stderr)
        return 2
    if args.fps and os.path.exists(fps_out) and not args.force:
        print(f"lc_amd.prep_models: {fps_out} already exists, specify --force to overwrite it", file=sys.stderr)
        return 1
    ids, meshes = read_models(args.models_dir, args.scale)
    short = [(i, len(v)) for i, (v, _) in zip(ids, meshes) if len(v) < max(args.fps, 1)]
    if short:
        print(f"lc_amd.prep_models: objects with fewer than {max(args.fps, 1)} vertices (id, vertices): {short}", file=sys.stderr)
        return 1
    mesh_set = MeshSet(meshes, _device(), obj_ids=ids)
    info = models.prepare(mesh_set, args.fps)
    computed = models.to_models_info(info, ids)
    stored = None
    if os.path.exists(info_out) and not args.force:
        with open(info_out) as f:
            stored = {int(k): v for k, v in json.load(f).items()}
    for i, (v, _) in zip(ids, meshes):
        print(f"obj {i}: {len(v)} vertices  {_row(computed[i])}")
        if stored is not None:
            print(f"obj {i}: stored in {os.path.basename(info_out)}:  " + (_row(stored[i]) if i in stored and all(k in stored[i] for k in _KEYS) else "no entry"))
    if stored is not None:
        print(f"lc_amd.prep_models: {info_out} already exists and is left as it is (specify --force to overwrite it)")
    else:
        with open(info_out, "w") as f:
            json.dump({str(i): computed[i] for i in ids}, f, indent=2)
            f.write("\n")
        print(f"lc_amd.prep_models: wrote {info_out}")
    if args.fps:
        with open(fps_out, "wb") as f:
            pickle.dump(models.to_fps_dict(info, ids), f)
        print(f"lc_amd.prep_models: wrote {fps_out} ({args.fps} points per object)")
    if xform_out is not None:
        box = obox.oriented_box(mesh_set, axis=args.xform_axis)
        volume, aabb = box.volume.cpu().numpy(), box.aabb_volume.cpu().numpy()
        for k, i in enumerate(ids):
            print(f"obj {i}: oriented box volume {volume[k]:.6g} (axis-aligned {aabb[k]:.6g})")
        with open(xform_out, "w") as f:
            json.dump(obox.to_models_xform(box, ids), f, indent=2)
            f.write("\n")
        print(f"lc_amd.prep_models: wrote {xform_out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
