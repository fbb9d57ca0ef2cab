"""A training set that lives on the device: frames, masks and the annotation table are resident, and one 64-bit seed word decides which
instances a step trains on and everything that is drawn for them.

    TrainSet(frames, table, *, masks=None, rle_store=None, cfg, seed0, batch, spare, in_hw, out_hw, valid_th=100, n_check=256,
             backgrounds=None, background_store=None, meshes=None, near=None, far=None, dtype=torch.float32, normalize=None,
             vis_interp="linear")
    TrainSet.step_inputs(seed) -> dict

`lc_amd.train_inputs.train_inputs` chains the loader's stages for B rows that the caller has chosen, gathered and uploaded.  This chain
puts the two host pieces that were left in front of it on the device (lc_amd/sampler.py): which rows a step trains on -- the epoch's
shuffle and the gather of their records -- and the retry of `BOP_Dataset.__getitem__` (`dataset.py:332-338`), which draws another random
instance whenever `valid_cnt < valid_pix_cnt_th`.  R = batch + spare rows are drawn; the cheap stages run on all R; the rows whose crop is
too empty are replaced by spares whose crop is not; the expensive stages run on exactly `batch` rows:

    1. sampler.draw_rows               R rows: the step's primaries in the epoch's order, spares at random; their records
    2. geometry.zoom_geometry          R rows
    3. rle.decode                      R rows, where an RleStore is given
    4. maskcrop.mask_crops             R rows with out_affine: msk_vis, msk_noc, valid_cnt, sym_ck_pts2d
    5. sampler.select_rows             take (batch,), shortfall (1,)
    6. sampler.take_rows               the geometry, the records and stage 4's outputs of the taken rows
    7. on the taken rows only, with the taken geometry: maskcrop.mask_crops for msk_in, crops.warp_affine,
       backgrounds.switch_backgrounds / augment.augment_drawn, and render.render_homo_z_out where meshes are given

Nothing is formed on the host and nothing is read back: the call can be captured with `torch.cuda.graph`, and after `seed.add_(1)` one
replay gives the next step's batch of the epoch.  `train_inputs` is not involved and not changed."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _args, augment, crops, maskcrop, render, rle
from . import backgrounds as _backgrounds
from . import geometry as _geometry
from . import sampler as _sampler
from .augment import AugmentConfig

_A = _args.Args("trainset")


class TrainSet:
    """frames (F,H,W,3) uint8 on the device; table a `sampler.AnnotationTable` on the same device; the visible masks as bytes `masks`
    (F',H,W) uint8 / bool or as `rle_store`, an `rle.RleStore` of masks of the frames' size -- one of the two; cfg an AugmentConfig; seed0 the
    whole number below 2^64 that the seed word holds at step 0; batch >= 1 rows a step trains on and spare >= 0 rows drawn beside them,
    batch + spare <= sampler.MAX_ROWS; in_hw and out_hw = (h, w) of the network's input and output; valid_th, n_check, vis_interp as
    `mask_crops` takes them; backgrounds / background_store, dtype and normalize as `train_inputs` takes them; meshes a `render.MeshSet` with
    near and far -- all three or none (the table's mesh_index, R and t are the poses)."""

    def __init__(self, frames, table, *, masks=None, rle_store=None, cfg: AugmentConfig, seed0, batch, spare, in_hw, out_hw, valid_th=100, n_check=256,
                 backgrounds=None, background_store=None, meshes=None, near=None, far=None, dtype=torch.float32, normalize=None, vis_interp="linear"):
        if (masks is None) == (rle_store is None):
            raise ValueError("lc_amd.trainset: the visible masks come as bytes (masks) or as an RleStore (rle_store): one of the two")
        if backgrounds is not None and background_store is not None:
            raise ValueError("lc_amd.trainset: the backgrounds come cut to the input size (backgrounds) or as a BackgroundStore (background_store): at most one of the two")
        if background_store is not None and not isinstance(background_store, _backgrounds.BackgroundStore):
            raise TypeError(f"lc_amd.trainset: background_store must be a BackgroundStore, got {type(background_store)}")
        if rle_store is not None and not isinstance(rle_store, rle.RleStore):
            raise TypeError(f"lc_amd.trainset: rle_store must be an RleStore, got {type(rle_store)}")
        if not isinstance(table, _sampler.AnnotationTable):
            raise TypeError(f"lc_amd.trainset: table must be an AnnotationTable, got {type(table)}")
        if not isinstance(cfg, AugmentConfig):
            raise TypeError(f"lc_amd.trainset: cfg must be an AugmentConfig, got {type(cfg)}")
        if meshes is not None and not isinstance(meshes, render.MeshSet):
            raise TypeError(f"lc_amd.trainset: meshes must be a MeshSet, got {type(meshes)}")
        planes = dict(near=near, far=far)
        if meshes is not None and any(v is None for v in planes.values()):
            raise ValueError(f"lc_amd.trainset: meshes need near and far; {', '.join(k for k, v in planes.items() if v is None)} missing")
        if meshes is None and any(v is not None for v in planes.values()):
            raise ValueError(f"lc_amd.trainset: {', '.join(k for k, v in planes.items() if v is not None)} given without meshes")
        frames = _A.tensor("frames", frames, (torch.uint8,), "uint8", (None, None, None, 3))
        H, W = int(frames.shape[1]), int(frames.shape[2])
        self.in_hw = _A.size_pair("in_hw", in_hw, crops.MAX_SIZE)
        self.out_hw = _A.size_pair("out_hw", out_hw, crops.MAX_SIZE)
        self.seed0 = _A.whole("seed0", seed0, 0, 2 ** 64 - 1, numpy=True)
        self.batch = _A.whole("batch", batch, 1, _sampler.MAX_ROWS, numpy=True)
        self.spare = _A.whole("spare", spare, 0, _sampler.MAX_ROWS, numpy=True)
        if self.batch + self.spare > _sampler.MAX_ROWS:
            raise ValueError(f"lc_amd.trainset: batch + spare of at most {_sampler.MAX_ROWS}, got {self.batch + self.spare}")
        self.valid_th = _A.whole("valid_th", valid_th, -2 ** 31, 2 ** 31 - 1)
        self.n_check = _A.whole("n_check", n_check, 0, maskcrop.MAX_CHECK)
        if vis_interp not in maskcrop.INTERP:
            raise ValueError(f"lc_amd.trainset: vis_interp must be one of {sorted(maskcrop.INTERP)}, got {vis_interp!r}")
        if dtype not in augment.OUT_DTYPES:
            raise TypeError(f"lc_amd.trainset: dtype must be one of uint8, float32, float16, bfloat16, got {dtype}")
        if masks is not None:
            masks = _A.tensor("masks", masks, (torch.uint8, torch.bool), "uint8 or bool", (None, H, W))
        elif rle_store.frame_hw != (H, W):
            raise ValueError(f"lc_amd.trainset: the store's masks are decoded to full frames of {H} x {W}, but the store was made with {rle_store.frame_hw}")
        if not frames.is_cuda:
            raise RuntimeError(f"lc_amd.trainset: frames is on {frames.device}; the HIP path needs tensors on the MI355X (there is no CPU fallback in the product path)")
        dev = frames.device
        _A.same_device(dev, "the frames on {}", table=table.columns["frame_index"], masks=masks, backgrounds=backgrounds if isinstance(backgrounds, Tensor) else None)
        self.frames, self.table, self.masks, self.rle_store, self.cfg, self.device, self.im_hw = frames, table, masks, rle_store, cfg, dev, (H, W)
        self.backgrounds, self.background_store, self.meshes, self.near, self.far = backgrounds, background_store, meshes, near, far
        self.dtype, self.normalize, self.vis_interp = dtype, normalize, vis_interp

    @torch.no_grad()
    def step_inputs(self, seed) -> dict:
        """The training input of the step `seed - seed0`.  seed: a device tensor of one uint64 / int64 element that the kernels read (or a
        whole number, which fixes the step).

        -> dict of device tensors of `batch` rows: `train_inputs`' keys -- rgb_in, msk_vis, msk_noc, sym_ck_pts2d, valid_cnt, out_K,
        out_pix_scale, in_affine, info, and homo_z_out with meshes -- which hold, byte for byte, what `train_inputs` makes of the taken rows'
        records with `sample_id = index` and `geometry=` the taken geometry; plus index (the row's annotation), frame_index, mask_index,
        mesh_index, obj_id, scene_id, im_id, bbox_xyxy, K_no_aug, R_no_aug, t_no_aug (its record), geometry (the taken `ZoomGeometry`),
        take (batch,) int32 (the drawn row behind each row of the batch) and shortfall (1,) int32.

        `sample_id` of every stage is the annotation `index`: an instance drawn twice in a step -- as a primary and as a spare, or by two
        spares -- is the same sample twice, with the same geometry, colours and background.  A row with take = -1 (its primary was too
        empty and no good spare was left: `shortfall` counts them) has info = -1, zeros in its record, geometry, masks, count and check
        points, an all-border crop behind rgb_in (which is that crop's augmentation: read `info`), and nothing rendered."""
        dev = self.device
        word = augment._seed_word(seed, dev)
        (in_h, in_w), (out_h, out_w) = self.in_hw, self.out_hw
        rows = _sampler.draw_rows(self.table, seed=word, seed0=self.seed0, batch=self.batch, spare=self.spare)
        g = _geometry.zoom_geometry(self.cfg, seed=word, sample_id=rows.index, bbox_xyxy=rows.bbox_xyxy, im_hw=self.im_hw, cam_K=rows.cam_K, in_wh=(in_w, in_h),
                                    out_wh=(out_w, out_h))
        infos = [rows.info, g.info]
        masks, mask_index = self.masks, rows.mask_index
        if self.rle_store is not None:
            masks, dinfo = rle.decode(self.rle_store, index=rows.mask_index, hw=self.im_hw)
            mask_index = None  # row r of the decoded frames is row r's mask
            infos.append(dinfo)
        mc = maskcrop.mask_crops(masks, g.out_affine, (out_h, out_w), mask_index=mask_index, vis_interp=self.vis_interp, valid_th=self.valid_th, n_check=self.n_check,
                                 sample_id=g.step_id)
        infos.append(mc.info)
        row_info = infos[0]
        for i in infos[1:]:
            row_info = torch.minimum(row_info, i)
        take, shortfall = _sampler.select_rows(mc.valid_cnt, row_info, batch=self.batch, valid_th=self.valid_th)
        (in_affine, out_affine, out_K, pix, step_id, g_info, index, frame_index, mask_index_t, mesh_index, obj_id, scene_id, im_id, bbox, K, R, t, msk_vis, msk_noc, ck,
         valid_cnt, info) = _sampler.take_rows(take, g.in_affine, g.out_affine, g.out_K, g.out_pix_scale, g.step_id, g.info, rows.index, rows.frame_index, rows.mask_index,
                                               rows.mesh_index, rows.obj_id, rows.scene_id, rows.im_id, rows.bbox_xyxy, rows.cam_K, rows.R, rows.t, mc.msk_vis, mc.msk_noc,
                                               mc.sym_ck_pts2d, mc.valid_cnt, row_info)
        taken = _geometry.ZoomGeometry(in_affine, out_affine, out_K, pix, step_id, g_info, None, None, None, None)
        ok = torch.clamp(take, max=0)  # 0, or -1 for a row that took nothing: its frame and mask index below leave [0, F), and every stage refuses it
        if self.rle_store is not None:
            mi = maskcrop.mask_crops(masks, in_affine, (in_h, in_w), mask_index=take, n_check=0, want=("msk_vis",))
        else:
            mi = maskcrop.mask_crops(masks, in_affine, (in_h, in_w), mask_index=mask_index_t + ok, n_check=0, want=("msk_vis",))
        winfo = torch.empty(self.batch, device=dev, dtype=torch.int32)
        crop = crops.warp_affine(self.frames, in_affine, (in_h, in_w), frame_index=frame_index + ok, dtype=torch.uint8, info=winfo)
        infos = [info, ok, mi.info, winfo]
        if self.background_store is not None:
            sinfo, _ = _backgrounds.switch_backgrounds(crop, self.background_store, self.cfg, seed=word, sample_id=index, msk_in=mi.msk_vis)
            infos.append(sinfo)
        rgb_in, ainfo = augment.augment_drawn(crop, self.cfg, seed=word, sample_id=index, msk_in=mi.msk_vis, backgrounds=self.backgrounds, dtype=self.dtype,
                                              normalize=self.normalize)
        infos.append(ainfo)
        out = dict(rgb_in=rgb_in, msk_vis=msk_vis, msk_noc=msk_noc, sym_ck_pts2d=ck, valid_cnt=valid_cnt, out_K=out_K, out_pix_scale=pix, in_affine=in_affine)
        if self.meshes is not None:
            out["homo_z_out"], _ = render.render_homo_z_out(self.meshes, mesh_index + ok, R, t, K, out_K, (out_h, out_w), near=self.near, far=self.far)
        info = infos[0]
        for i in infos[1:]:
            info = torch.minimum(info, i)
        out.update(info=info, index=index, frame_index=frame_index, mask_index=mask_index_t, mesh_index=mesh_index, obj_id=obj_id, scene_id=scene_id, im_id=im_id,
                   bbox_xyxy=bbox, K_no_aug=K, R_no_aug=R, t_no_aug=t, geometry=taken, take=take, shortfall=shortfall)
        return out
