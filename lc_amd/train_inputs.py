"""The training input of one step as one chain of launches on the device: what the reference's loader makes per instance on host cores
(`dataset.py:402-470`), from frames, masks, boxes and cameras that already lie on the device and ONE 64-bit seed word.

    train_inputs(frames, frame_index, *, masks=None, rle_store=None, mask_index=None, bbox_xyxy, cam_K, sample_id, cfg, seed,
                 backgrounds=None, background_store=None, in_hw, out_hw, valid_th=100, n_check=256, vis_interp="linear", dtype=torch.float32,
                 normalize=None, meshes=None, mesh_index=None, R=None, t=None, near=None, far=None, geometry=None) -> dict

Pure Python over the wrappers of the loader's stages, in this order, all on the current stream:

    1. geometry.zoom_geometry          in_affine, out_affine, out_K, out_pix_scale, step_id          drawn from the seed word
    2. rle.decode                      the visible masks as full frames, where an RleStore is given
    3. maskcrop.mask_crops             msk_vis, msk_noc, valid_cnt, sym_ck_pts2d with out_affine; the check points of sample `step_id`
    4. maskcrop.mask_crops             msk_in with in_affine (the mask the background switch blends with)
    5. crops.warp_affine               the uint8 crop of the frame with in_affine
    6. augment.augment_drawn           rgb_in: the background switch and the colour chain, drawn from the same seed word; with a
                                       `backgrounds.BackgroundStore`, backgrounds.switch_backgrounds picks, cuts and blends each row's
                                       background in the uint8 crop first, and the colour chain follows without a switch of its own
    7. render.render_homo_z_out        homo_z_out with the device's out_K, where meshes are given

Nothing is formed on the host and nothing is read back, so the whole call can be captured with `torch.cuda.graph`; the word `seed` names
is read by the kernels of stages 1 and 6 at every replay, and stage 3's check points follow through `step_id`: after `seed.add_(1)` a
replay redraws geometry, check points, colours and, with a store, each row's background and its region.  It adds no kernel of its own."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _args, augment, crops, maskcrop, render, rle
from . import backgrounds as _backgrounds
from . import geometry as _geometry
from .augment import AugmentConfig

_A = _args.Args("train_inputs")


def _batch(**named) -> int:
    """B of the call: the first dimension that every per-row tensor shares."""
    sizes = {name: int(t.shape[0]) for name, t in named.items() if isinstance(t, Tensor) and t.dim() >= 1}
    if "sample_id" not in sizes:
        raise TypeError(f"lc_amd.train_inputs: sample_id must be a (B,) torch.Tensor, got {type(named['sample_id'])}")
    if len(set(sizes.values())) > 1:
        raise ValueError(f"lc_amd.train_inputs: the per-row tensors disagree on B: {', '.join(f'{k} has {v}' for k, v in sizes.items())}")
    return next(iter(sizes.values()))


@torch.no_grad()
def train_inputs(frames, frame_index, *, masks=None, rle_store=None, mask_index=None, bbox_xyxy, cam_K, sample_id, cfg: AugmentConfig, seed,
                 backgrounds=None, background_store=None, in_hw, out_hw, valid_th=100, n_check=256, vis_interp="linear", dtype=torch.float32,
                 normalize=None, meshes=None, mesh_index=None, R=None, t=None, near=None, far=None, geometry=None) -> dict:
    """frames (F,H,W,3) uint8 and frame_index (B,) int32; the visible masks as bytes `masks` (F',H,W) uint8 / bool, or as `rle_store`, an
    `rle.RleStore` of masks of the frames' size that is decoded to full frames -- one of the two -- with mask_index (B,) int32 (None: row b
    reads mask b); bbox_xyxy (B,4) float32, cam_K (B,3,3) or (3,3) float32, sample_id (B,) int32; cfg an AugmentConfig; seed a device
    tensor of one uint64 / int64 element (or a whole number, which fixes the draw); backgrounds (G,3,h,w) uint8 already cut to the
    input size, or background_store, a `backgrounds.BackgroundStore` of images of their own sizes from which every row's background is
    picked and cut anew at every step -- at most one of the two; in_hw and out_hw = (h, w) of the network's input and output; valid_th, n_check, vis_interp as `mask_crops`
    takes them, dtype and normalize as `augment_drawn` does; meshes a `render.MeshSet` with mesh_index (B,) int32, R (B,3,3), t (B,3) and
    near, far -- all of them or none.  `geometry`: a `geometry.ZoomGeometry` of device tensors to use in the place of stage 1 (what a host
    draw uploads: the route this chain replaces, kept for measuring it); its step_id feeds the check points as ever.

    -> dict of device tensors under the reference's blob names: rgb_in (B,3,h,w) of `dtype`, msk_vis (B,ho,wo) float32, msk_noc (B,ho,wo)
    bool, sym_ck_pts2d (B,n_check,2) int64, valid_cnt (B,) int32, out_K (B,3,3) float32, out_pix_scale (B,) float32, homo_z_out
    (B,ho,wo,3) float32 with meshes; and in_affine (B,2,3) float32 and info (B,) int32, the least of the stages' infos: -1 for a row that
    any stage refused (a refused geometry gives NaN matrices, which every later stage refuses in turn)."""
    if (masks is None) == (rle_store is None):
        raise ValueError("lc_amd.train_inputs: the visible masks come as bytes (masks) or as an RleStore (rle_store): one of the two")
    if backgrounds is not None and background_store is not None:
        raise ValueError("lc_amd.train_inputs: the backgrounds come cut to the input size (backgrounds) or as a BackgroundStore (background_store): at most one of the two")
    if background_store is not None and not isinstance(background_store, _backgrounds.BackgroundStore):
        raise TypeError(f"lc_amd.train_inputs: background_store must be a BackgroundStore, got {type(background_store)}")
    if rle_store is not None and not isinstance(rle_store, rle.RleStore):
        raise TypeError(f"lc_amd.train_inputs: rle_store must be an RleStore, got {type(rle_store)}")
    with_meshes = meshes is not None
    poses = dict(mesh_index=mesh_index, R=R, t=t, near=near, far=far)
    if with_meshes and any(v is None for v in poses.values()):
        raise ValueError(f"lc_amd.train_inputs: meshes need mesh_index, R, t, near and far; {', '.join(k for k, v in poses.items() if v is None)} missing")
    if not with_meshes and any(v is not None for v in poses.values()):
        raise ValueError(f"lc_amd.train_inputs: {', '.join(k for k, v in poses.items() if v is not None)} given without meshes")
    if not isinstance(cfg, AugmentConfig):
        raise TypeError(f"lc_amd.train_inputs: cfg must be an AugmentConfig, got {type(cfg)}")
    frames = _A.tensor("frames", frames, (torch.uint8,), "uint8", (None, None, None, 3))
    H, W = int(frames.shape[1]), int(frames.shape[2])
    in_h, in_w = _A.size_pair("in_hw", in_hw, crops.MAX_SIZE)
    out_h, out_w = _A.size_pair("out_hw", out_hw, crops.MAX_SIZE)
    B = _batch(sample_id=sample_id, frame_index=frame_index, bbox_xyxy=bbox_xyxy, mask_index=mask_index, cam_K=cam_K if isinstance(cam_K, Tensor) and cam_K.dim() == 3 else None,
               mesh_index=mesh_index, R=R, t=t)
    if masks is not None:
        masks = _A.tensor("masks", masks, (torch.uint8, torch.bool), "uint8 or bool", (None, H, W))
    elif rle_store.frame_hw != (H, W):
        raise ValueError(f"lc_amd.train_inputs: the store's masks are decoded to full frames of {H} x {W}, but the store was made with {rle_store.frame_hw}")
    if not frames.is_cuda:
        raise RuntimeError(f"lc_amd.train_inputs: frames is on {frames.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
    dev = frames.device
    _A.same_device(dev, "the frames on {}", sample_id=sample_id if isinstance(sample_id, Tensor) else None)

    word = augment._seed_word(seed, dev)
    if geometry is not None and not isinstance(geometry, _geometry.ZoomGeometry):
        raise TypeError(f"lc_amd.train_inputs: geometry must be a ZoomGeometry of device tensors, got {type(geometry)}")
    g = geometry if geometry is not None else _geometry.zoom_geometry(cfg, seed=word, sample_id=sample_id, bbox_xyxy=bbox_xyxy, im_hw=(H, W), cam_K=cam_K, in_wh=(in_w, in_h),
                                                                        out_wh=(out_w, out_h))
    infos = [g.info]
    if rle_store is not None:
        masks, dinfo = rle.decode(rle_store, index=mask_index, hw=(H, W))
        mask_index = None  # row b of the decoded frames is row b's mask
        if int(masks.shape[0]) != B:
            raise ValueError(f"lc_amd.train_inputs: the store gives {int(masks.shape[0])} masks for {B} rows; say mask_index")
        infos.append(dinfo)
    mc = maskcrop.mask_crops(masks, g.out_affine, (out_h, out_w), mask_index=mask_index, vis_interp=vis_interp, valid_th=valid_th, n_check=n_check,
                             sample_id=g.step_id)
    mi = maskcrop.mask_crops(masks, g.in_affine, (in_h, in_w), mask_index=mask_index, n_check=0, want=("msk_vis",))
    winfo = torch.empty(B, device=dev, dtype=torch.int32)
    crop = crops.warp_affine(frames, g.in_affine, (in_h, in_w), frame_index=frame_index, dtype=torch.uint8, info=winfo)
    infos += [mc.info, mi.info, winfo]
    if background_store is not None:
        sinfo, _ = _backgrounds.switch_backgrounds(crop, background_store, cfg, seed=word, sample_id=sample_id, msk_in=mi.msk_vis)
        infos.append(sinfo)  # (1 on a switched row: above the 0 of the other stages, so only a refusal shows)
    rgb_in, ainfo = augment.augment_drawn(crop, cfg, seed=word, sample_id=sample_id, msk_in=mi.msk_vis, backgrounds=backgrounds, dtype=dtype, normalize=normalize)
    infos.append(ainfo)
    out = dict(rgb_in=rgb_in, msk_vis=mc.msk_vis, msk_noc=mc.msk_noc, sym_ck_pts2d=mc.sym_ck_pts2d, valid_cnt=mc.valid_cnt, out_K=g.out_K,
               out_pix_scale=g.out_pix_scale, in_affine=g.in_affine)
    if with_meshes:
        K_no_aug = cam_K.expand(B, 3, 3) if tuple(cam_K.shape) == (3, 3) else cam_K
        out["homo_z_out"], _ = render.render_homo_z_out(meshes, mesh_index, R, t, K_no_aug, g.out_K, (out_h, out_w), near=near, far=far)
    info = infos[0]
    for i in infos[1:]:
        info = torch.minimum(info, i)
    out["info"] = info
    return out
