"""Per-object symmetry tables on the device: what `symmetry.symmetry_pose_candidates` (`symmetry.py:58-93`) builds per SAMPLE in the
loader's workers, built once per OBJECT from `models_info.json`.  The candidates of a training step are a pure function of the base pose
(12 numbers the device already holds) and of this table; lc_labels.hip forms them where they are used (lc_amd.labels).

    SymmetrySet.from_models_info(info_or_path, obj_ids=None, continuous_steps=384, device=...)
    SymmetrySet.index_of(obj_id_tensor) -> int32 device tensor, -1 for an id the set lacks (no host read)

numpy only (the reference's scipy `Rotation.from_rotvec` is the Rodrigues formula, written out here)."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch
from torch import Tensor


def rodrigues(axis, angle):
    """Rotation by `angle` about the unit vector `axis`, float64: I + sin(a) [n]x + (1 - cos(a)) [n]x^2."""
    n = np.asarray(axis, dtype=np.float64)
    Kx = np.array([[0.0, -n[2], n[1]], [n[2], 0.0, -n[0]], [-n[1], n[0], 0.0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def symmetry_transforms(model_info, continuous_steps=384):
    """The transforms (R_s (K,3,3), t_s (K,3)) of one object, float64.  Indexing as the reference where the reference defines it:
      no symmetry  K = 1, the identity;
      discrete     the identity, then `symmetries_discrete` in file order (R_s = sym[:3,:3], t_s = sym[:3,3]);
      continuous   exactly one entry; for c = 0..C-1 the rotation by 2 pi c / C about `axis` (normalised here; BOP files hold unit axes,
                   for which the reference's rotation vector angle * axis is the same rotation), t_s = -R_s offset + offset;
      both         K = D C, index k = d C + c with d = 0 the identity: R_s = R_c R_d, t_s = R_c t_d + t_c (the order of the BOP
                   toolkit's get_symmetry_transformations).  The reference has NO such case: it raises NotImplementedError.
    Entry 0 is the exact identity (R_s = I, t_s = 0 bit for bit), so candidate 0 is the base pose itself."""
    C = int(continuous_steps)
    if C < 1:
        raise ValueError(f"lc_amd.symmetry: continuous_steps must be at least 1, got {continuous_steps}")
    disc = [(np.eye(3), np.zeros(3))]
    for i, sym in enumerate(model_info.get("symmetries_discrete", ()) or ()):
        m = np.asarray(sym, dtype=np.float64)
        if m.size != 16:
            raise ValueError(f"lc_amd.symmetry: symmetries_discrete[{i}] must hold 16 numbers, got {m.size}")
        m = m.reshape(4, 4)
        if not np.isfinite(m).all():
            raise ValueError(f"lc_amd.symmetry: symmetries_discrete[{i}] has a non-finite entry")
        disc.append((m[:3, :3].copy(), m[:3, 3].copy()))
    cont = [(np.eye(3), np.zeros(3))]
    cs = model_info.get("symmetries_continuous", ()) or ()
    if len(cs) > 1:
        raise ValueError(f"lc_amd.symmetry: exactly one continuous symmetry per object is supported (as in the reference), got {len(cs)}")
    if len(cs) == 1:
        axis = np.asarray(cs[0]["axis"], dtype=np.float64).reshape(-1)
        offset = np.asarray(cs[0].get("offset", (0.0, 0.0, 0.0)), dtype=np.float64).reshape(-1)
        if axis.size != 3 or offset.size != 3:
            raise ValueError("lc_amd.symmetry: symmetries_continuous needs an axis and an offset of 3 numbers each")
        if not (np.isfinite(axis).all() and np.isfinite(offset).all()):
            raise ValueError("lc_amd.symmetry: symmetries_continuous has a non-finite entry")
        norm = float(np.linalg.norm(axis))
        if norm == 0.0:
            raise ValueError("lc_amd.symmetry: the axis of a continuous symmetry has zero length")
        for c in range(1, C):
            R = rodrigues(axis / norm, 2.0 * math.pi * c / C)
            cont.append((R, -(R @ offset) + offset))
    Rs, ts = [], []
    for Rd, td in disc:
        for Rc, tc in cont:
            first = not Rs
            Rs.append(np.eye(3) if first else Rc @ Rd)
            ts.append(np.zeros(3) if first else Rc @ td + tc)
    return np.stack(Rs), np.stack(ts)


def host_table(transforms, obj_ids):
    """(sorted obj_ids, table (Ktot,12) float64, obj_off, obj_k int32) of per-object (R_s (K,3,3), t_s (K,3)) lists: host arrays only."""
    obj_ids = [int(o) for o in obj_ids]
    if not obj_ids or len(set(obj_ids)) != len(obj_ids) or min(obj_ids) < 0 or len(transforms) != len(obj_ids):
        raise ValueError("lc_amd.symmetry: obj_ids must name every object once, with non-negative ids")
    order = np.argsort(obj_ids)
    rows, offs, ks = [], [], []
    for i in order:
        R, t = transforms[i]
        R, t = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
        if len(R) < 1 or len(R) != len(t) or not (np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError(f"lc_amd.symmetry: object {obj_ids[i]}: transforms must be finite (K,3,3) and (K,3) with K >= 1")
        if not np.array_equal(R[0], np.eye(3)) or t[0].any():
            raise ValueError(f"lc_amd.symmetry: object {obj_ids[i]}: transform 0 must be the exact identity")
        offs.append(sum(ks))
        ks.append(len(R))
        rows.append(np.concatenate((R, t[..., None]), -1).reshape(-1, 12))
    if sum(ks) >= 2 ** 31 // 12:
        raise ValueError("lc_amd.symmetry: symmetry table of 2^31 elements or more")
    return [obj_ids[i] for i in order], np.ascontiguousarray(np.concatenate(rows, 0)), np.asarray(offs, np.int32), np.asarray(ks, np.int32)


def models_info_transforms(info, obj_ids=None, continuous_steps=384):
    """(obj_ids, [symmetry_transforms of each]) of a BOP `models_info.json` dict (keys: object ids as strings or ints) or a path to one."""
    if isinstance(info, (str, os.PathLike)):
        with open(info) as f:
            info = json.load(f)
    by_id = {int(k): v for k, v in info.items()}
    ids = sorted(by_id) if obj_ids is None else [int(o) for o in obj_ids]
    missing = [o for o in ids if o not in by_id]
    if missing:
        raise KeyError(f"lc_amd.symmetry: models_info has no object {missing}")
    transforms = []
    for o in ids:
        try:
            transforms.append(symmetry_transforms(by_id[o], continuous_steps))
        except ValueError as e:
            raise ValueError(f"{e} (object {o})") from None
    return ids, transforms


class SymmetrySet:
    """The symmetry transforms of a set of objects as ONE device table.  `table` (Ktot,12) float64: a transform [R_s | t_s] per row as a
    row-major 3 x 4; object i (in the order of the sorted `obj_ids`) owns rows [obj_off[i], obj_off[i] + obj_k[i]).  Host copies:
    `table_host`, `obj_off_host`, `obj_k_host`; `max_k`."""

    def __init__(self, transforms, obj_ids, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"lc_amd.symmetry: SymmetrySet lives on the HIP device, got {device} (there is no CPU fallback in the product path)")
        self.obj_ids, self.table_host, self.obj_off_host, self.obj_k_host = host_table(transforms, obj_ids)
        self.n_obj, self.total, self.max_k = len(self.obj_ids), int(self.obj_k_host.sum()), int(self.obj_k_host.max())
        self.table = torch.from_numpy(self.table_host).to(device)
        self.obj_off = torch.from_numpy(self.obj_off_host).to(device)
        self.obj_k = torch.from_numpy(self.obj_k_host).to(device)
        self.device = self.table.device
        lut = np.full(max(self.obj_ids) + 2, -1, dtype=np.int32)  # last entry: every unknown id
        lut[np.asarray(self.obj_ids, dtype=np.int64)] = np.arange(self.n_obj, dtype=np.int32)
        self._lut_host = lut
        self._lut = torch.from_numpy(lut).to(device)

    @classmethod
    def from_models_info(cls, info, obj_ids=None, continuous_steps=384, device="cuda"):
        """`info`: the dict of a BOP `models_info.json` (keys: object ids as strings or ints) or a path to the file.  `obj_ids`: the
        objects to keep (default: all); one that the file lacks is refused."""
        ids, transforms = models_info_transforms(info, obj_ids, continuous_steps)
        return cls(transforms, ids, device)

    def index_of(self, obj_ids) -> Tensor:
        """Device int32 table index of each object id (a tensor on the device stays there: nothing is read back).  An id the set lacks
        gives -1: the kernels refuse such a row on the device -- its Rt_best is NaN and its index -1, nothing is read for it -- exactly as
        lc_amd.render.MeshSet.index_of refuses a mesh; ids known on the host are refused there (`host_index_of`)."""
        ids = obj_ids if isinstance(obj_ids, Tensor) else torch.as_tensor(np.asarray(obj_ids, dtype=np.int64))
        ids = ids.to(self.device).long().reshape(-1)
        n = self._lut.numel() - 1
        ids = torch.where((ids >= 0) & (ids < n), ids, torch.full_like(ids, n))
        return self._lut[ids]

    def host_index_of(self, obj_ids) -> np.ndarray:
        """The same on the host (a device tensor is read back: not for the hot path); an id the set lacks raises."""
        ids = obj_ids.detach().cpu().numpy() if isinstance(obj_ids, Tensor) else np.asarray(obj_ids)
        ids = ids.astype(np.int64).reshape(-1)
        n = len(self._lut_host) - 1
        idx = self._lut_host[np.where((ids >= 0) & (ids < n), ids, n)]
        if (idx < 0).any():
            raise KeyError(f"lc_amd.symmetry: the set has no object {sorted(set(ids[idx < 0].tolist()))} (it holds {self.obj_ids})")
        return idx
