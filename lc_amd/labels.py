"""Label preparation of a training step on the device: `losses.annots_on_the_fly` and what it calls (`losses.py:68-139,187-193`,
`symmetry.py:8-56`), same names, arguments, dict keys and return values.

    xyz_from_homo_z(homo_z, R, t, K)                 -> (B,H,W,3)        lc_label_targets_f32 (xyz only)
    select_pose_2d / select_pose_3d(..., pose_candi) -> (B,3,4)          lc_sym_select_f32, one chunk
    selete_best_pose(gt_dict, out_dict, started)     -> Rt_best, pose_best, xyz_gt
    annots_on_the_fly(gt_dict, out_dict, cfg, step)  -> gt_dict updated with Rt_best, pose_best, xyz_gt and the network targets

A step takes two launches of lc_labels.hip -- the candidate selection of every chunk at once (skipped when there is nothing to
choose), then one streaming pass that writes xyz_gt and the targets -- plus the code decode at the check pixels for a binary-code head
and the small torch ops of the quaternion.  Nothing reads a value back to the host (no .item(), no data-dependent shapes): the call can
be captured in a graph.  HIP tensors only; `lc_amd.dropin.install(native_labels=True)` puts these names in place of the reference's.

Opt-in depth source (`set_depth_source(meshes, near, far)`, `clear_depth_source()`; `lc_amd.dropin --native-depth MODELS_DIR`): a
gt_dict WITHOUT the key `homo_z_out` gets it rendered on the device (lc_amd.render.render_homo_z_out from R_no_aug, t_no_aug, K_no_aug,
out_K and obj_id; `msk_noc` too where it is absent).  With the key present nothing changes.

Opt-in symmetry source (`set_symmetry_source(symset)`, `clear_symmetry_source()`; `lc_amd.dropin --native-sym MODELS_INFO_JSON`): the
candidate poses are formed on the device from the base pose (R_no_aug, t_no_aug), `obj_id` and the per-object table of a
lc_amd.symmetry.SymmetrySet, inside the selection launch (lc_sym_select_table_f32).  `Rt_candi` is IGNORED while a source is set (it need
not be in gt_dict), every row takes its own candidate count from the table, and the step does not depend on the batch's mix of objects: one
captured graph serves every batch.  A row whose obj_id the set lacks gets a NaN `Rt_best` (nothing is read back to refuse it on the host).

    symmetry_pose_candidates(base_R, base_t, symset, obj_id)      -> (B,K,3,4)         lc_sym_candidates_f32 (the reference's `Rt_candi`)
    symmetry_pose_candidates_list(base_R, base_t, symset, obj_id) -> [(K_b,3,4)] * B   the same for rows of different K
"""
from __future__ import annotations

import ctypes
from operator import itemgetter

import torch
from torch import Tensor

from . import _lib, floatbits
from . import transforms as xforms


_DEPTH_SOURCE = None  # (MeshSet, near, far, size_hw or None)


def set_depth_source(meshes, near, far, size_hw=None):
    """From now on `annots_on_the_fly` renders `homo_z_out` for a gt_dict that has none: `meshes` is a lc_amd.render.MeshSet whose
    obj_ids are the dataset's, `near` / `far` are in the unit of t_no_aug and of the meshes.  The map size is `size_hw` if given, else
    that of `msk_noc`, else that of the network's output maps."""
    global _DEPTH_SOURCE
    from . import render

    if not isinstance(meshes, render.MeshSet):
        raise TypeError(f"lc_amd.labels: set_depth_source takes a lc_amd.render.MeshSet, got {type(meshes)}")
    if not float(near) < float(far):
        raise ValueError("lc_amd.labels: set_depth_source needs near < far")
    _DEPTH_SOURCE = (meshes, float(near), float(far), None if size_hw is None else (int(size_hw[0]), int(size_hw[1])))


def clear_depth_source():
    global _DEPTH_SOURCE
    _DEPTH_SOURCE = None


def _render_missing_depth(gt_dict, out_dict):
    """gt_dict['homo_z_out'] (and 'msk_noc' if absent) from the depth source: dataset.py:293-311 + :444 on the fly."""
    from . import render

    meshes, near, far, size_hw = _DEPTH_SOURCE
    if size_hw is None:
        if 'msk_noc' in gt_dict:
            size_hw = tuple(gt_dict['msk_noc'].shape[-2:])
        else:
            maps = [v for v in out_dict.values() if isinstance(v, Tensor) and v.dim() == 4]
            if not maps:
                raise RuntimeError("lc_amd.labels: the depth source needs a map size (set_depth_source(..., size_hw=), msk_noc or an output map)")
            size_hw = tuple(maps[0].shape[-2:])
    dev = meshes.device
    hz, msk = render.render_homo_z_out(meshes, meshes.index_of(gt_dict['obj_id']), _f32("R_no_aug", gt_dict['R_no_aug'].to(dev)),
                                       _f32("t_no_aug", gt_dict['t_no_aug'].to(dev)), _f32("K_no_aug", gt_dict['K_no_aug'].to(dev)),
                                       _f32("out_K", gt_dict['out_K'].to(dev)), size_hw, near=near, far=far)
    gt_dict['homo_z_out'] = hz
    if 'msk_noc' not in gt_dict:
        gt_dict['msk_noc'] = msk


_SYM_SOURCE = None  # lc_amd.symmetry.SymmetrySet


def set_symmetry_source(symset):
    """From now on `annots_on_the_fly` / `selete_best_pose` form the symmetric pose candidates on the device from R_no_aug, t_no_aug,
    obj_id and `symset` (a lc_amd.symmetry.SymmetrySet whose obj_ids are the dataset's); gt_dict['Rt_candi'] is ignored."""
    global _SYM_SOURCE
    from . import symmetry

    if not isinstance(symset, symmetry.SymmetrySet):
        raise TypeError(f"lc_amd.labels: set_symmetry_source takes a lc_amd.symmetry.SymmetrySet, got {type(symset)}")
    _SYM_SOURCE = symset


def clear_symmetry_source():
    global _SYM_SOURCE
    _SYM_SOURCE = None


def _table_args(symset):
    return _lib.ptr(symset.table), _lib.ptr(symset.obj_off), _lib.ptr(symset.obj_k), symset.n_obj, symset.total


def _base_pose(symset, base_R, base_t):
    R, t = base_R.reshape(-1, 3, 3), base_t.reshape(-1, 3, 1)
    return _f32("base pose", torch.cat((R, t), -1).to(symset.device))


def _candidates(base_R, base_t, symset, obj_id):
    """(flat (Ktot,3,4) float32, first row and candidate count of every batch row (host arrays))."""
    index = symset.host_index_of(obj_id)
    base = _base_pose(symset, base_R, base_t)
    B = int(base.shape[0])
    if len(index) != B:
        raise ValueError(f"lc_amd.labels: {B} base poses and {len(index)} obj_ids")
    ks = symset.obj_k_host[index].astype("int64")
    offs = ks.cumsum() - ks
    total = int(ks.sum())
    dev = symset.device
    out = torch.empty(total, 3, 4, device=dev, dtype=torch.float32)
    if B:
        idx = torch.as_tensor(index, dtype=torch.int32).to(dev)
        row_off = torch.as_tensor(offs, dtype=torch.int32).to(dev)
        with _lib.on_device(dev):
            rc = _lib.load().lc_sym_candidates_f32(_lib.ptr(base), _lib.ptr(idx), *_table_args(symset), _lib.ptr(row_off), B,
                                                   _lib.ptr(out), total, _lib.stream_ptr(dev))
        _lib.check(rc, "lc_sym_candidates_f32")
    return out, offs, ks


@torch.no_grad()
def symmetry_pose_candidates_list(base_R: Tensor, base_t: Tensor, symset, obj_id):
    """`symmetry.py:58-93` for a batch, from the table: row b's (K_b,3,4) float32 candidates [R_b R_s | R_b t_s + t_b] (views of one
    buffer).  Reads obj_id on the host for the shapes (one synchronising copy when it is a device tensor): not for the hot path, which
    needs no materialised candidates.  An obj_id the set lacks raises."""
    out, offs, ks = _candidates(base_R, base_t, symset, obj_id)
    return [out[int(o):int(o + k)] for o, k in zip(offs, ks)]


@torch.no_grad()
def symmetry_pose_candidates(base_R: Tensor, base_t: Tensor, symset, obj_id) -> Tensor:
    """(B,K,3,4): the candidates of a batch whose rows share one candidate count K (the reference's `Rt_candi` of one chunk)."""
    out, offs, ks = _candidates(base_R, base_t, symset, obj_id)
    if len(set(ks.tolist())) > 1:
        raise ValueError(f"lc_amd.labels: the rows have different candidate counts {sorted(set(ks.tolist()))}, so there is no (B,K,3,4) "
                         f"array of them; use symmetry_pose_candidates_list")
    return out.view(len(ks), int(ks[0]) if len(ks) else 1, 3, 4)


def _f32(name, t):
    """A contiguous float32 HIP tensor (16-bit and float64 inputs are converted; the labels take no gradient)."""
    return _lib.require_hip_f32(name, t.detach().float() if t.dtype == torch.float64 else t.detach())


def chunk_table(candis):
    """Host side of the ragged candidate list, from shapes only: (chunk_rows, chunk_k, chunk_off, B, Ktot).  Chunk c covers batch rows
    [chunk_rows[c], chunk_rows[c+1]) with chunk_k[c] candidates each; its candidates start at row chunk_off[c] of the concatenated
    (Ktot,3,4) array."""
    rows, ks, offs = [0], [], []
    r = o = 0
    for c in candis:
        if c.dim() != 4 or tuple(c.shape[-2:]) != (3, 4):
            raise ValueError(f"lc_amd.labels: candidate chunks are (B_c,K,3,4), got {tuple(c.shape)}")
        bc, k = int(c.shape[0]), int(c.shape[1])
        ks.append(k)
        offs.append(o)
        r += bc
        o += bc * k
        rows.append(r)
    return rows, ks, offs, r, o


def _select(mode, candis, cam_K, N, *, pts_a=None, pts_b=None, xyz_map=None, noc_scale=None, homo_z=None, ck=None, table=None):
    """One launch over every chunk: (Rt_best (B,3,4) f32, index within the row's candidates (B,) int32).  `table` = (SymmetrySet, base
    poses (B,3,4) f32, obj_index (B,) int32) instead of `candis`: the candidates are formed in the launch."""
    dev = cam_K.device
    if table is None:
        rows, ks, _, B, _ = chunk_table(candis)
        cand = _f32("Rt_candi", torch.cat([c.reshape(-1, 3, 4) for c in candis], 0))
    else:
        symset, base, obj_index = table
        B = int(base.shape[0])
        if tuple(obj_index.shape) != (B,) or obj_index.dtype != torch.int32 or obj_index.device != base.device or base.device != symset.device:
            raise ValueError(f"lc_amd.labels: obj_index must be ({B},) int32 on {symset.device}, like the base poses")
        obj_index = obj_index.contiguous()
    K = _f32("cam_K", cam_K.reshape(B, 3, 3))
    Rt = torch.empty(B, 3, 4, device=dev, dtype=torch.float32)
    idx = torch.empty(B, device=dev, dtype=torch.int32)
    code, bs, H, W = 0, 0, 0, 0
    if homo_z is not None:
        H, W = int(homo_z.shape[1]), int(homo_z.shape[2])
        homo_z = _f32("homo_z_out", homo_z)
    for name, t, w in (("points", pts_a, 3), ("points", pts_b, 2 if mode == 0 else 3), ("sym_ck_pts2d", ck, 2)):
        if t is not None and tuple(t.shape) != (B, N, w):
            raise ValueError(f"lc_amd.labels: {name} must be ({B},{N},{w}), got {tuple(t.shape)}")
    if homo_z is not None and (homo_z.dim() != 4 or homo_z.shape[0] != B or homo_z.shape[3] != 3):
        raise ValueError(f"lc_amd.labels: homo_z_out must be ({B},H,W,3), got {tuple(homo_z.shape)}")
    if xyz_map is not None and (xyz_map.dim() != 4 or tuple(xyz_map.shape) != (B, 3, H, W)):
        raise ValueError(f"lc_amd.labels: xyz_noc must be ({B},3,{H},{W}), got {tuple(xyz_map.shape)}")
    if xyz_map is not None:
        (xyz_map,), (bs,), code = _lib.hip_maps(xyz_noc=xyz_map.detach())
    if ck is not None:
        if not ck.is_cuda:
            raise RuntimeError("lc_amd.labels: sym_ck_pts2d must be on the HIP device")
        ck = ck.to(torch.int64).contiguous()
    lib = _lib.load()
    rest = (mode, _lib.ptr(K), _lib.ptr(pts_a), _lib.ptr(pts_b), _lib.ptr(xyz_map), code, bs, _lib.ptr(noc_scale), _lib.ptr(homo_z), _lib.ptr(ck), B, N, H, W,
            _lib.ptr(Rt), _lib.ptr(idx), _lib.stream_ptr(dev))
    with _lib.on_device(dev):
        if table is None:
            rc = lib.lc_sym_select_f32(_lib.ptr(cand), _ints(rows), _ints(ks), len(ks), *rest)
        else:
            rc = lib.lc_sym_select_table_f32(_lib.ptr(base), _lib.ptr(obj_index), *_table_args(symset), *rest)
    _lib.check(rc, "lc_sym_select_f32" if table is None else "lc_sym_select_table_f32")
    return Rt, idx


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _targets(homo_z, Rt, cam_K, *, msk=None, noc_scale=None, xform=None, bit_cnt=None, want_xyz=True, want_targets=False):
    """The streaming launch: xyz_gt (B,H,W,3) and, with want_targets, the continuous target (B,3,H,W) or the code planes (B,C,H,W) bool."""
    B, H, W = int(homo_z.shape[0]), int(homo_z.shape[1]), int(homo_z.shape[2])
    dev = homo_z.device
    hz = _f32("homo_z", homo_z.reshape(B, H, W, 3))
    Rt = _f32("Rt", Rt.reshape(B, 3, 4))
    K = _f32("cam_K", cam_K.reshape(B, 3, 3))
    m8 = mf = None
    if msk is not None:
        if not msk.is_cuda:
            raise RuntimeError("lc_amd.labels: msk_noc must be on the HIP device")
        msk = msk.reshape(B, H, W)
        if msk.dtype == torch.bool:
            m8 = msk.contiguous().view(torch.uint8)
        elif msk.dtype == torch.uint8:
            m8 = msk.contiguous()
        else:
            mf = msk.contiguous().float()
    sc = xf = None
    if want_targets:
        sc = _f32("noc_scale", noc_scale.reshape(B, 3))
        xf = None if xform is None else _f32("model_transform", xform.reshape(B, 4, 4))
    xyz = torch.empty(B, H, W, 3, device=dev, dtype=torch.float32) if want_xyz else None
    noc = tgt = raw = None
    bits = [0, 0, 0]
    if want_targets and bit_cnt is None:
        noc = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
    elif want_targets:
        bits = [int(b) for b in bit_cnt] if isinstance(bit_cnt, (list, tuple)) else [int(bit_cnt)] * 3
        C = sum(bits)
        tgt = torch.empty(B, C, H, W, device=dev, dtype=torch.bool)
        raw = torch.empty(B, C, H, W, device=dev, dtype=torch.bool)
    lib = _lib.load()
    with _lib.on_device(dev):
        rc = lib.lc_label_targets_f32(_lib.ptr(hz), _lib.ptr(m8), _lib.ptr(mf), _lib.ptr(Rt), _lib.ptr(K), _lib.ptr(sc), _lib.ptr(xf), B, H, W,
                                      *bits, int(floatbits._black_background), _lib.ptr(xyz), _lib.ptr(noc), _lib.ptr(tgt), _lib.ptr(raw),
                                      _lib.stream_ptr(dev))
    _lib.check(rc, "lc_label_targets_f32")
    return xyz, noc, tgt, raw


@torch.no_grad()
def xyz_from_homo_z(homo_z: Tensor, pose_R: Tensor, pose_t: Tensor, cam_K: Tensor) -> Tensor:
    """`losses.py:187-193`: (B,H,W,3) homogeneous depth -> object coordinates R^T (K^-1 h - t)."""
    Rt = torch.cat((pose_R.reshape(-1, 3, 3), pose_t.reshape(-1, 3, 1)), -1)
    return _targets(homo_z, Rt, cam_K)[0]


@torch.no_grad()
def select_pose_2d(cam_K: Tensor, pts3d: Tensor, pts2d: Tensor, pose_candi: Tensor) -> Tensor:
    """`symmetry.py:8-31`: the candidate (B,K,3,4) whose projection of pts3d (B,N,3) lies closest to pts2d (B,N,2) on average."""
    if pose_candi.shape[-3] == 1:
        return pose_candi.squeeze(-3)
    N = int(pts3d.shape[-2])
    Rt, _ = _select(0, [pose_candi], cam_K, N, pts_a=_f32("pts3d", pts3d), pts_b=_f32("pts2d", pts2d))
    return Rt.to(pose_candi.dtype)


@torch.no_grad()
def select_pose_3d(cam_K: Tensor, pts3d_out: Tensor, homo_z: Tensor, pose_candi: Tensor) -> Tensor:
    """`symmetry.py:33-56`: the candidate (B,K,3,4) whose back-projection of homo_z (B,N,3) lies closest to pts3d_out (B,N,3) on average."""
    if pose_candi.shape[-3] == 1:
        return pose_candi.squeeze(-3)
    N = int(pts3d_out.shape[-2])
    Rt, _ = _select(1, [pose_candi], cam_K, N, pts_a=_f32("pts3d_out", pts3d_out), pts_b=_f32("homo_z", homo_z))
    return Rt.to(pose_candi.dtype)


def _best(gt_dict, out_dict, sym_aware_started):
    """(Rt_best, the pose xyz_gt is computed with (B,3,4)) of `losses.py:68-118`."""
    homo_z, R_no_aug, t_no_aug, K_no_aug = itemgetter('homo_z_out', 'R_no_aug', 't_no_aug', 'K_no_aug')(gt_dict)
    table = None
    if _SYM_SOURCE is not None:
        # candidate 0 of every row is its base pose, and a row with one candidate keeps it: the reference's three paths (every row K = 1:
        # xyz_gt from the un-augmented pose; not started: candidate 0; else the selection) need no knowledge of the batch's objects
        Rt_base = torch.cat((R_no_aug.reshape(-1, 3, 3), t_no_aug.reshape(-1, 3, 1)), -1)
        if not sym_aware_started or _SYM_SOURCE.max_k == 1:
            return Rt_base, Rt_base
        table = (_SYM_SOURCE, _base_pose(_SYM_SOURCE, R_no_aug, t_no_aug), _SYM_SOURCE.index_of(gt_dict['obj_id']))
        candis, cand_dtype = None, R_no_aug.dtype
    else:
        candis = gt_dict['Rt_candi']
        cand_dtype = candis[0].dtype
    if table is None and len(candis) == 1 and candis[0].shape[-3] == 1:  # no symmetric candidates: xyz_gt from the un-augmented pose (losses.py:72-76)
        Rt_best = candis[0].squeeze(-3)
        return Rt_best, torch.cat((R_no_aug.reshape(-1, 3, 3), t_no_aug.reshape(-1, 3, 1)), -1)
    if table is None and not sym_aware_started:
        Rt_best = torch.cat([c[..., 0, :, :] for c in candis], 0)
        return Rt_best, Rt_best
    if 'pts2d' not in out_dict:
        ck = gt_dict['sym_ck_pts2d']
        B, N = int(ck.shape[0]), int(ck.shape[1])
        if 'xyz_noc' in out_dict:
            Rt, _ = _select(1, candis, K_no_aug, N, xyz_map=out_dict['xyz_noc'], noc_scale=_f32("noc_scale", gt_dict['noc_scale'].reshape(B, 3)),
                            homo_z=homo_z, ck=ck, table=table)
        elif 'xyz_noc_bin' in out_dict:
            logits = out_dict['xyz_noc_bin'].detach()
            H, W = int(logits.shape[-2]), int(logits.shape[-1])
            index = ((ck[..., 1] % H) * W + ck[..., 0] % W).to(torch.int32).contiguous()
            counts = torch.full((B,), N, device=logits.device, dtype=torch.int32)
            pts = torch.empty(B, N, 3, device=logits.device, dtype=torch.float32)
            floatbits.decode_selected_rows(logits, gt_dict.get('bit_cnt', None), index, counts, pts, noc_scale=gt_dict['noc_scale'],
                                           model_transform=gt_dict.get('model_transform', None))
            Rt, _ = _select(1, candis, K_no_aug, N, pts_a=pts, homo_z=homo_z, ck=ck, table=table)
        else:
            raise RuntimeError('False branch')
    else:
        pts2d = out_dict['pts2d']
        Rt, _ = _select(0, candis, gt_dict['out_K'], int(pts2d.shape[-2]), pts_a=_f32("pts3d", gt_dict['pts3d']), pts_b=_f32("pts2d", pts2d), table=table)
    return Rt.to(cand_dtype), Rt


def _pose_rep(Rt_best):
    return xforms.RT_to_quaternion_rep(Rt_best[..., :3, :3], Rt_best[..., :, 3])


@torch.no_grad()
def selete_best_pose(gt_dict, out_dict, sym_aware_started):
    """`losses.py:68-118`: (Rt_best (B,3,4), pose_best (B,7), xyz_gt (B,H,W,3))."""
    Rt_best, Rt_xyz = _best(gt_dict, out_dict, sym_aware_started)
    xyz_gt = _targets(gt_dict['homo_z_out'], Rt_xyz, gt_dict['K_no_aug'], msk=gt_dict['msk_noc'])[0]
    return Rt_best, _pose_rep(Rt_best), xyz_gt


@torch.no_grad()
def annots_on_the_fly(gt_dict, out_dict, cfg_global, step):
    """`losses.py:121-139`: the symmetry-aware pose and the network targets of this step, written into gt_dict."""
    if _DEPTH_SOURCE is not None and 'homo_z_out' not in gt_dict:
        _render_missing_depth(gt_dict, out_dict)
    sym_aware_started = step >= cfg_global.get('sym_aware_start', 0)
    Rt_best, Rt_xyz = _best(gt_dict, out_dict, sym_aware_started)
    T, bit_cnt = gt_dict.get('model_transform', None), gt_dict.get('bit_cnt', None)
    if bit_cnt is None:
        assert T is None, 'coordinate transform not implemented for continuous xyz output'
    xyz_gt, noc, tgt, raw = _targets(gt_dict['homo_z_out'], Rt_xyz, gt_dict['K_no_aug'], msk=gt_dict['msk_noc'], noc_scale=gt_dict['noc_scale'],
                                     xform=T, bit_cnt=bit_cnt, want_targets=True)
    annot_dict = dict(Rt_best=Rt_best, pose_best=_pose_rep(Rt_best), xyz_gt=xyz_gt)
    if bit_cnt is None:
        annot_dict['xyz_noc_tgt'] = noc
    else:
        annot_dict['xyz_noc_bin_tgt'] = tgt
        annot_dict['xyz_noc_bin_raw'] = raw
    gt_dict.update(annot_dict)
