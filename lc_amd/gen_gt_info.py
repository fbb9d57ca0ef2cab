"""BOP's per-instance visibility annotations without the BOP toolkit or OpenGL: what `calc_gt_masks.py` and `calc_gt_info.py` write for a
scene, made by lc_amd.gtinfo (one render per instance, compared with the scene's depth on the device).

    python -m lc_amd.gen_gt_info SCENE_DIR MODELS_DIR [--depth-dir DIR] [--delta 15] [--margin MX MY] [--frame-hw H W] [--out-dir OUT]
                                                      [--bbox-plus-one] [--rle]

SCENE_DIR holds `scene_gt.json` and `scene_camera.json`; MODELS_DIR the `obj_<id>.ply` files, read as `python -m lc_amd.gen_z` reads them
(mm, scaled to metres; near 0.01 m, far 6.5 m).  It writes, into OUT (default SCENE_DIR),

    scene_gt_info.json          per image the list of its instances' records: bbox_obj, bbox_visib ([x, y, w, h]), px_count_all,
                                px_count_valid, px_count_visib, visib_fract (lc_amd.gtinfo.bop_records)
    mask_npz/<image>.npz        `mask` and `mask_visib`, (N,H,W) bool each: the instances' silhouettes and their visible parts in the frame
    mask_rle.npy                with `--rle`, besides: one dict {'mask': {key: record}, 'mask_visib': {key: record}}, key
                                "<image:06d>_<instance:06d>", record {'size': [H, W], 'counts': COCO's compressed string} as pycocotools
                                writes it -- each inner dict is what the reference keeps in its `*_msk.npy` cache (lc_amd.rle encodes
                                the masks on the device; `np.load(..., allow_pickle=True).item()` reads it back)

The scene's depth: `--depth-dir` holds one `<image>.npy` per image, (H,W) in mm (what a BOP depth image times its depth_scale gives;
decoding the PNGs is left to the caller); without it the depth is composed from the instances' own renders, the synthetic case, and an
instance is hidden only by the scene's other annotated instances.  `--delta` is in mm (BOP: 15).  `--margin MX MY` widens the render on
every side so that px_count_all and bbox_obj measure the whole silhouette of a truncated object; the default is BOP's own, the frame's
width and height (a 3H x 3W render).  `--margin 0 0` is nine times cheaper and cuts those two at the frame.

An instance whose object has no model file keeps its place in the list with a record of -1 throughout, and empty masks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import gen_z


def _rle_records(masks, frame_hw, origin_xy, cap=2048):
    """The frame's part of window masks (N,h,w) as compressed-string records, encoded on the device; a mask with more runs than `cap`
    is encoded again with room for the largest need."""
    from . import rle

    enc = rle.encode(masks, frame_hw, origin_xy, cap)
    n = enc.n_runs.cpu().numpy()
    if len(n) and int(n.max()) > cap:
        enc = rle.encode(masks, frame_hw, origin_xy, int(n.max()))
    if enc.info.cpu().numpy().any():
        raise RuntimeError("lc_amd.gen_gt_info: the run-length encoder refused a mask")
    c = enc.counts.cpu().numpy().view(np.uint32)
    return [{"size": [int(frame_hw[0]), int(frame_hw[1])], "counts": rle.counts_to_string(c[i, :n[i]])} for i in range(len(n))]


def annotate_scene(meshes, scene_dir, out_dir, device, *, depth_dir=None, delta_mm=15.0, margin=None, frame_hw=(gen_z.IM_H, gen_z.IM_W), bbox_plus_one=False,
                   rle=False):
    """One scene, one `compute_gt_info` call per image; returns the number of records written."""
    import torch

    from . import gtinfo

    runs = {"mask": {}, "mask_visib": {}}

    with open(os.path.join(scene_dir, "scene_gt.json")) as f:
        gt = json.load(f)
    with open(os.path.join(scene_dir, "scene_camera.json")) as f:
        cam = json.load(f)
    os.makedirs(os.path.join(out_dir, "mask_npz"), exist_ok=True)
    records, written = {}, 0
    for str_im_id, annos in gt.items():
        if not annos:
            records[str_im_id] = []
            continue
        depth = None
        H, W = int(frame_hw[0]), int(frame_hw[1])
        if depth_dir is not None:
            d = np.load(os.path.join(depth_dir, f"{int(str_im_id):06d}.npy"))
            if d.ndim != 2:
                raise ValueError(f"lc_amd.gen_gt_info: the depth of image {str_im_id} has shape {d.shape}, expected (H, W)")
            H, W = d.shape
            depth = torch.from_numpy((d.astype(np.float32) * np.float32(0.001))[None]).to(device)
        mx, my = (W, H) if margin is None else (int(margin[0]), int(margin[1]))
        n = len(annos)
        K = torch.from_numpy(np.asarray(cam[str_im_id]["cam_K"], dtype=np.float32).reshape(3, 3)).to(device)
        R = np.stack([np.asarray(a["cam_R_m2c"], dtype=np.float32).reshape(3, 3) for a in annos])
        t = np.stack([np.asarray(a["cam_t_m2c"], dtype=np.float32).reshape(3) / np.float32(1000.0) for a in annos])
        idx = meshes.index_of([int(a["obj_id"]) for a in annos])
        out = gtinfo.compute_gt_info(meshes, idx, torch.from_numpy(R).to(device), torch.from_numpy(t).to(device), K, depth, frame_hw=(H, W), margin=(mx, my),
                                     delta=float(delta_mm) * 0.001, near=gen_z.NEAR, far=gen_z.FAR)
        records[str_im_id] = gtinfo.bop_records(out, bbox_plus_one=bbox_plus_one)
        frame = (slice(None), slice(my, my + H), slice(mx, mx + W))  # the window lies at (-mx, -my)
        np.savez_compressed(os.path.join(out_dir, "mask_npz", f"{int(str_im_id):06d}.npz"), mask=(out.depth_gt[frame] > 0).cpu().numpy(),
                            mask_visib=out.mask_visib[frame].cpu().numpy())
        if rle:  # straight from the windows: the encoder cuts them at the frame
            for key, masks in (("mask", out.depth_gt > 0), ("mask_visib", out.mask_visib)):
                for inst, rec in enumerate(_rle_records(masks, (H, W), out.origin_xy)):
                    runs[key][f"{int(str_im_id):06d}_{inst:06d}"] = rec
        written += n
    with open(os.path.join(out_dir, "scene_gt_info.json"), "w") as f:
        json.dump(records, f)
    if rle:
        np.save(os.path.join(out_dir, "mask_rle.npy"), runs, allow_pickle=True)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m lc_amd.gen_gt_info", description="BOP's scene_gt_info.json and visible masks (lc_amd.gtinfo)")
    ap.add_argument("scene_dir")
    ap.add_argument("models_dir")
    ap.add_argument("--depth-dir", default=None, help="<image>.npy per image, (H,W) in mm; default: composed from the instances' renders")
    ap.add_argument("--delta", type=float, default=15.0, help="visibility tolerance in mm")
    ap.add_argument("--margin", type=int, nargs=2, default=None, metavar=("MX", "MY"), help="columns and rows rendered around the frame; default: W H")
    ap.add_argument("--frame-hw", type=int, nargs=2, default=(gen_z.IM_H, gen_z.IM_W), metavar=("H", "W"), help="without --depth-dir")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--bbox-plus-one", action="store_true", help="box widths as pixel counts (x_max - x_min + 1)")
    ap.add_argument("--rle", action="store_true", help="also write mask_rle.npy: the masks as COCO run-length records, encoded on the device")
    args = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lc_amd.gen_gt_info: needs the HIP device (there is no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    meshes = gen_z.load_models(args.models_dir, device)
    out_dir = args.out_dir or args.scene_dir
    n = annotate_scene(meshes, args.scene_dir, out_dir, device, depth_dir=args.depth_dir, delta_mm=args.delta, margin=args.margin, frame_hw=tuple(args.frame_hw),
                       bbox_plus_one=args.bbox_plus_one, rle=args.rle)
    print(f"lc_amd.gen_gt_info: wrote {n} records to {os.path.join(out_dir, 'scene_gt_info.json')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
