"""The per-object files every path reads, made from a directory of meshes by lc_amd.models (the sibling of `python -m lc_amd.gen_z`):

    python -m lc_amd.prep_models MODELS_DIR [--fps 256] [--scale 1.0] [--info-out PATH] [--fps-out PATH] [--xform [PATH]] [--xform-axis {x,y,z}] [--force]
                                 [--symmetries] [--sym-frame {obox,model}] [--sym-max-fold 12] [--sym-queries N] [--sym-eps-abs 15] [--sym-eps-rel 0.1]
    python -m lc_amd.prep_models MODELS_DIR --check-symmetries [MODELS_INFO_JSON] [--sym-queries N] [--sym-eps-abs 15] [--sym-eps-rel 0.1] [--scale 1.0]

Reads `MODELS_DIR/obj_<id>.ply` (lc_amd.gen_z.read_ply; vertices times `--scale`) and writes
  * `models_info.json` (default MODELS_DIR/models_info.json): BOP's `{"<id>": {diameter, min_x, min_y, min_z, size_x, size_y, size_z}}`,
    which `model_transform.load_composed_model_info` turns into `noc_scale`, `bbox_3d` and `diameter`;
  * the farthest-point pickle (default MODELS_DIR/fps.pkl; `--fps 0`: none): `{id: (count, 3) float32}`, what `cfg_global.fps` is
    loaded from (dataset.py:232-236; the loader slices `[:sparse_cnt]`, and the first n rows of a result are the n-point result).
  * with `--xform` (off by default; default path MODELS_DIR/models_xform.json), the reference's `models_xform.json`
    (`{"<id>": {"xform": 16 numbers, "xformed_noc_scale": 3 numbers}}`, model_transform.py:21-42): per object the rigid transform after which
    its bounding box is centred and as small as lc_amd.obox's stated grid search finds it, over all orientations or, with `--xform-axis`,
    over the turns about that model axis alone; an existing file is refused before anything is computed.
  * with `--symmetries` (off by default), the keys `symmetries_discrete` / `symmetries_continuous` in the `models_info.json` it writes (BOP's
    layout, read back by `lc_amd.symmetry.SymmetrySet.from_models_info`) and the sidecar `symmetry_proposal.json` beside it: a STATED SEARCH by
    lc_amd.symfind (`propose_symmetries`), not a proof and not BOP's hand-made annotations -- the rotations about the three axes of one frame
    through its centre (`--sym-frame obox`: the oriented box of lc_amd.obox; `model`: the model axes and the centre of the axis-aligned box),
    the 383 turns of 1/384 and the k/n turns up to `--sym-max-fold`, judged by BOP's rule dev <= eps = max(--sym-eps-abs * scale,
    --sym-eps-rel * diameter) on the first `--sym-queries` farthest points (default 1024; 0: every vertex); it needs a `models_info.json`
    it may write (`--force` over an existing one).
`--check-symmetries [MODELS_INFO_JSON]` (default MODELS_DIR/models_info.json) writes nothing but `symmetry_check.json` beside that file: per
object the diameter (computed, not the file's), eps and per symmetry entry the larger deviation of S and S^-1 over every vertex
(`--sym-queries N` > 0: over the first N farthest points, a lower bound), and exits with 3 if an entry exceeds eps, naming it.
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

from . import gen_z, models, obox, symfind
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


def _queries(mesh_set, meshes, n):
    """Per object the first n farthest points of models.prepare as vertex indices (fewer for a smaller mesh), or None for every vertex."""
    if n <= 0:
        return None
    counts = [min(n, len(v)) for v, _ in meshes]
    index = models.prepare(mesh_set, min(counts), want_diameter=False).fps_index.cpu().numpy()
    if min(counts) == max(counts):
        return [index[k] for k in range(len(meshes))]
    # meshes smaller than n keep all their farthest points: one more selection per distinct count
    out = []
    for k, (v, f) in enumerate(meshes):
        out.append(index[k] if counts[k] == min(counts) else models.prepare(MeshSet([(v, f)], mesh_set.device), counts[k], want_diameter=False).fps_index.cpu().numpy()[0])
    return out


def _check(args):
    info_path = args.check_symmetries or os.path.join(args.models_dir, "models_info.json")
    if not os.path.exists(info_path):
        print(f"lc_amd.prep_models: {info_path} does not exist", file=sys.stderr)
        return 2
    if args.sym_queries is not None and args.sym_queries < 0:
        print("lc_amd.prep_models: --sym-queries must not be negative", file=sys.stderr)
        return 2
    ids, meshes = read_models(args.models_dir, args.scale)
    with open(info_path) as f:
        stored = {int(k): v for k, v in json.load(f).items()}
    missing = [i for i in ids if i not in stored]
    if missing:
        print(f"lc_amd.prep_models: {info_path} has no object {missing}", file=sys.stderr)
        return 2
    mesh_set = MeshSet(meshes, _device(), obj_ids=ids)
    diameters = models.prepare(mesh_set, 0, want_extents=False).diameter.cpu().numpy()
    report = symfind.check_symmetries(symfind.device_scorer(mesh_set), ids, stored, diameters, queries=_queries(mesh_set, meshes, args.sym_queries or 0),
                                      eps_abs=args.sym_eps_abs * args.scale, eps_rel=args.sym_eps_rel)
    for i in ids:
        o = report["objects"][str(i)]
        worst = max([e["dev"] for e in o["symmetries_discrete"] + o["symmetries_continuous"]], default=0.0)
        print(f"obj {i}: diameter {o['diameter']:.6g}  eps {o['eps']:.6g}  {len(o['symmetries_discrete'])} discrete, {len(o['symmetries_continuous'])} continuous, "
              f"largest deviation {worst:.6g}: {'ok' if o['ok'] else 'NOT ok'}")
    out = os.path.join(os.path.dirname(os.path.abspath(info_path)), "symmetry_check.json")
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"lc_amd.prep_models: wrote {out}")
    failed = symfind.failed_entries(report)
    if failed:
        print("lc_amd.prep_models: above eps: " + ", ".join(failed), file=sys.stderr)
        return 3
    return 0


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
    ap.add_argument("--symmetries", action="store_true", help="also propose symmetries_discrete / symmetries_continuous (a stated search) and write symmetry_proposal.json")
    ap.add_argument("--check-symmetries", nargs="?", const="", default=None, metavar="MODELS_INFO_JSON",
                    help="check the symmetries of a models_info.json (default MODELS_DIR/models_info.json) against the meshes, write symmetry_check.json, nothing else")
    ap.add_argument("--sym-frame", choices=("obox", "model"), default="obox", help="the frame whose axes and centre the proposal searches")
    ap.add_argument("--sym-max-fold", type=int, default=12)
    ap.add_argument("--sym-queries", type=int, default=None, help="query the first N farthest points (0: every vertex; default 1024 for --symmetries, 0 for --check-symmetries)")
    ap.add_argument("--sym-eps-abs", type=float, default=15.0, help="BOP's 15 mm, scaled by --scale")
    ap.add_argument("--sym-eps-rel", type=float, default=0.1, help="BOP's 0.1 of the diameter")
    args = ap.parse_args(argv)
    if args.check_symmetries is not None:
        return _check(args)
    if args.symmetries and (args.sym_max_fold < 2 or (args.sym_queries is not None and args.sym_queries < 0)):
        print("lc_amd.prep_models: --sym-max-fold must be at least 2 and --sym-queries not negative", file=sys.stderr)
        return 2
    xform_out = None if args.xform is None else (args.xform or os.path.join(args.models_dir, "models_xform.json"))
    if args.xform_axis is not None and xform_out is None:
        print("lc_amd.prep_models: --xform-axis needs --xform", file=sys.stderr)
        return 2
    if xform_out is not None and os.path.exists(xform_out) and not args.force:
        print(f"lc_amd.prep_models: {xform_out} already exists, specify --force to overwrite it", file=sys.stderr)
        return 1
    info_out = args.info_out or os.path.join(args.models_dir, "models_info.json")
    fps_out = args.fps_out or os.path.join(args.models_dir, "fps.pkl")
    proposal_out = os.path.join(os.path.dirname(os.path.abspath(info_out)), "symmetry_proposal.json")
    if args.symmetries and not args.force and (os.path.exists(info_out) or os.path.exists(proposal_out)):
        print(f"lc_amd.prep_models: --symmetries writes {info_out} and {proposal_out}, one of which already exists, specify --force to overwrite them", file=sys.stderr)
        return 1
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
    if args.symmetries:
        n = 1024 if args.sym_queries is None else args.sym_queries
        queries = _queries(mesh_set, meshes, n)
        if args.sym_frame == "obox":
            frames = [symfind.frame_of_xform(x) for x in obox.oriented_box(mesh_set).xform.cpu().numpy()]
        else:
            frames = [(np.array([computed[i]["min_" + a] + 0.5 * computed[i]["size_" + a] for a in "xyz"]), np.eye(3)) for i in ids]
        proposal, sidecar = symfind.propose_symmetries(symfind.device_scorer(mesh_set), ids, frames, [computed[i]["diameter"] for i in ids], queries=queries,
                                                       eps_abs=args.sym_eps_abs * args.scale, eps_rel=args.sym_eps_rel, max_fold=args.sym_max_fold,
                                                       frame_kind=args.sym_frame)
        for i in ids:
            computed[i].update(proposal[i])
            side = sidecar["objects"][str(i)]
            print(f"obj {i}: proposed {len(proposal[i].get('symmetries_discrete', ()))} discrete, {len(proposal[i].get('symmetries_continuous', ()))} continuous "
                  f"(eps {side['eps']:.6g}, folds {side['folds']}, closed {side['closed']}, truncated {side['truncated']})")
        with open(proposal_out, "w") as f:
            json.dump(sidecar, f, indent=1)
            f.write("\n")
        print(f"lc_amd.prep_models: wrote {proposal_out}")
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
