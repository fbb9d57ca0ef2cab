"""The two BOP files that say what a synthetic scene holds, with its frames and depth: what no other tool of this project could make.

    python -m lc_amd.gen_scenes MODELS_DIR OUT_DIR --scenes N --objects M [--seed SEED] [--first-id ID] [--cam-K k00 .. k22] [--frame-hw H W]
                                [--z-range ZMIN ZMAX] [--centre-box X0 Y0 X1 Y1] [--gap GAP] [--batch SCENES]

MODELS_DIR holds the `obj_<id>.ply` files, read as `python -m lc_amd.gen_z` reads them (mm, scaled to metres; near 0.01 m, far 6.5 m).
Every image is one scene of lc_amd.synthscene: M slots, slot m of image i holding model (i M + m) modulo the number of models, posed by
`posedraw.draw_scene_poses` from (SEED, image id) with the bounding-sphere radii of `posedraw.mesh_radii`, rendered with the models'
vertices in mid-grey under the default light.  It writes, into OUT_DIR,

    scene_gt.json        per image the list of its PLACED instances: cam_R_m2c (9 numbers, row-major), cam_t_m2c (mm), obj_id
    scene_camera.json    per image cam_K (9 numbers) and depth_scale 1.0
    rgb/<image>.npy      (H,W,3) uint8
    depth/<image>.npy    (H,W) float32 in mm, 0 where nothing is hit: what `python -m lc_amd.gen_gt_info --depth-dir` reads

in BOP's layout, so that `python -m lc_amd.gen_gt_info OUT_DIR MODELS_DIR` and `python -m lc_amd.gen_z` follow without a hand-made file.
The numbers are the float32 poses widened: cam_R_m2c exactly, cam_t_m2c times 1000 in fp64 (dividing by 1000 and rounding to float32
gives the drawn translation back).  Lengths on the command line are metres, pixels are the frame's.  A slot without a good try among
`posedraw.TRIES` is left out of its image; the tool says how many.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import gen_z

LM_K = (572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0)  # BOP's LM / LM-O camera
DELTA = 0.015  # metres: BOP's visibility tolerance, for the chain's own records (not written here)


def slot_models(n_models: int, first_id: int, n_scenes: int, M: int) -> np.ndarray:
    """(n_scenes, M) int32: slot m of image i holds mesh (i M + m) % n_models."""
    i = (np.arange(first_id, first_id + n_scenes, dtype=np.int64)[:, None] * M + np.arange(M, dtype=np.int64)[None]) % n_models
    return i.astype(np.int32)


def write_scenes(meshes, out_dir, device, *, n_scenes, M, seed, first_id=0, cam_K=LM_K, frame_hw=(gen_z.IM_H, gen_z.IM_W), z_range=(0.6, 1.4),
                 centre_box=None, gap=0.0, batch=8):
    """-> (instances written, slots left out)."""
    import torch

    from . import posedraw, shade, synthscene

    H, W = int(frame_hw[0]), int(frame_hw[1])
    box = (0.0, 0.0, float(W), float(H)) if centre_box is None else tuple(float(v) for v in centre_box)
    cfg = posedraw.PoseDrawConfig(z_range=(float(z_range[0]), float(z_range[1])), centre_box=box, gap=float(gap), near=gen_z.NEAR)
    K32 = np.asarray(cam_K, dtype=np.float32).reshape(3, 3)
    K = torch.from_numpy(K32).to(device)
    radius = torch.from_numpy(posedraw.mesh_radii(meshes)).to(device)
    appearance = shade.Appearance(meshes)
    slots = slot_models(meshes.n_meshes, first_id, n_scenes, M)
    os.makedirs(os.path.join(out_dir, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "depth"), exist_ok=True)
    gt, cam, written, left_out = {}, {}, 0, 0
    for lo in range(0, n_scenes, batch):
        ids = np.arange(first_id + lo, first_id + min(lo + batch, n_scenes), dtype=np.int32)
        out = synthscene.synth_scenes(meshes, appearance, radius, cfg, seed=seed, scene_id=torch.from_numpy(ids).to(device),
                                      mesh_index=torch.from_numpy(slots[lo:lo + len(ids)]).to(device), cam_K=K, frame_hw=(H, W), near=gen_z.NEAR, far=gen_z.FAR,
                                      light=shade.DEFAULT_LIGHT, phong=shade.DEFAULT_PHONG, delta=DELTA)
        R, t = out.poses.R.cpu().numpy().reshape(len(ids), M, 9), out.poses.t.cpu().numpy().reshape(len(ids), M, 3)
        which = out.poses.mesh_index_out.cpu().numpy().reshape(len(ids), M)
        frames, depth = out.frames.cpu().numpy(), out.scene.depth.cpu().numpy()
        for s, im_id in enumerate(ids.tolist()):
            gt[str(im_id)] = [dict(cam_R_m2c=[float(v) for v in R[s, m]], cam_t_m2c=[float(v) * 1000.0 for v in t[s, m]], obj_id=int(meshes.obj_ids[which[s, m]]))
                              for m in range(M) if which[s, m] >= 0]
            cam[str(im_id)] = dict(cam_K=[float(v) for v in K32.reshape(-1)], depth_scale=1.0)
            np.save(os.path.join(out_dir, "rgb", f"{im_id:06d}.npy"), frames[s])
            np.save(os.path.join(out_dir, "depth", f"{im_id:06d}.npy"), depth[s] * np.float32(1000.0))
            written += len(gt[str(im_id)])
        left_out += int((out.poses.info.cpu().numpy() == posedraw.NO_ROOM).sum())
    with open(os.path.join(out_dir, "scene_gt.json"), "w") as f:
        json.dump(gt, f)
    with open(os.path.join(out_dir, "scene_camera.json"), "w") as f:
        json.dump(cam, f)
    return written, left_out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m lc_amd.gen_scenes", description="BOP's scene_gt.json and scene_camera.json of synthetic scenes (lc_amd.synthscene)")
    ap.add_argument("models_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--scenes", type=int, required=True, help="the number of images, one scene each")
    ap.add_argument("--objects", type=int, required=True, help="slots per scene, 1 to 64")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--first-id", type=int, default=0, help="the first image id; an image's id is its scene id")
    ap.add_argument("--cam-K", type=float, nargs=9, default=LM_K, metavar="K", help="row-major; default: BOP's LM camera")
    ap.add_argument("--frame-hw", type=int, nargs=2, default=(gen_z.IM_H, gen_z.IM_W), metavar=("H", "W"))
    ap.add_argument("--z-range", type=float, nargs=2, default=(0.6, 1.4), metavar=("ZMIN", "ZMAX"), help="metres")
    ap.add_argument("--centre-box", type=float, nargs=4, default=None, metavar=("X0", "Y0", "X1", "Y1"), help="pixels; default: the frame")
    ap.add_argument("--gap", type=float, default=0.0, help="metres between two bounding spheres")
    ap.add_argument("--batch", type=int, default=8, help="scenes per call")
    args = ap.parse_args(argv)
    if args.scenes < 1 or args.batch < 1 or args.first_id < 0 or args.first_id + args.scenes > 2 ** 31 - 1:
        raise SystemExit("lc_amd.gen_scenes: --scenes and --batch of at least 1, image ids within int32")
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lc_amd.gen_scenes: needs the HIP device (there is no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    meshes = gen_z.load_models(args.models_dir, device)
    written, left_out = write_scenes(meshes, args.out_dir, device, n_scenes=args.scenes, M=args.objects, seed=args.seed, first_id=args.first_id, cam_K=args.cam_K,
                                     frame_hw=tuple(args.frame_hw), z_range=tuple(args.z_range), centre_box=args.centre_box, gap=args.gap, batch=args.batch)
    print(f"lc_amd.gen_scenes: wrote {written} instances of {args.scenes} images to {os.path.join(args.out_dir, 'scene_gt.json')}; {left_out} slots found no room")
    return 0


if __name__ == "__main__":
    sys.exit(main())
