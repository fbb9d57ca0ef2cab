"""Depth maps rendered on the device from mesh, pose and K (lc_amd/csrc/render/lc_render.hip, lc_amd/_C/liblc_amd_render.so, C ABI
and the exact definition of the result in include/lc_amd_render.h).

    MeshSet(meshes, device, obj_ids=None)                  the meshes of a dataset on the device, validated on the host
    render_depth(meshes, mesh_index, R, t, K, size_hw, *, near, far, pixel_center=(0.5, 0.5), want_face=False, want_homo=False,
                 pix2k=None) -> Rendered(depth, mask, face, homo_z, info)
    render_homo_z_out(meshes, mesh_index, R, t, K_no_aug, out_K, size_hw, *, near, far) -> (homo_z_out, msk_noc)

What the reference renders offline with an EGL/OpenGL renderer (`tools/gen_z.py`) and reads back in its loader (`dataset.py:287-311`):
`depth[b,y,x]` is the camera-space z of the nearest surface point on the ray through K-coordinates `(x + cx, y + cy)` with
`near < z < far`, 0 where nothing is hit.  No back-face culling.  THERE IS NO NEAR-PLANE CLIPPING: a face with any vertex at
`z <= near` is dropped whole and counted in `info[b]` (BOP objects never straddle the near plane).  Coverage is exact on a 2^-8 px
grid and the winner of a pixel is the smallest (fp32 bits of z, face index) pair, so every call gives the same bits.

`render_homo_z_out` is the on-the-fly form of `dataset.py:293-311` followed by the warp of `dataset.py:444`: output pixel (x,y) of the
crop `out_K = A K_no_aug` is rendered directly at the full-frame position A^-1 (x,y) + 0.5.  Two deliberate differences from the
stored-file route: there is no nearest-neighbour snap to full-frame pixels (the stored route samples at most half a source pixel
away from here), and there is no 16-bit quantisation of z (step (z_max - z_min) / 65534 in the files).

float32 HIP tensors only (anything else raises: there is no CPU fallback).  Runs on the current stream, never waits for the device,
can be captured into a graph.
"""
from __future__ import annotations

from ctypes import c_float, c_int, c_size_t, c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from . import build as _build

MAX_SIZE = 16384   # LC_RENDER_MAX_SIZE
RECORD_BYTES = 64  # LC_RENDER_RECORD_BYTES


class Rendered(NamedTuple):
    depth: Tensor             # (B,H,W) float32, 0 where nothing is hit
    mask: Tensor              # (B,H,W) bool
    face: Optional[Tensor]    # (B,H,W) int32 index of the winning face within its mesh, -1 where nothing is hit (want_face)
    homo_z: Optional[Tensor]  # (B,H,W,3) float32 (p_x, p_y, 1) z (want_homo)
    info: Tensor              # (B,) int32: faces dropped at the near plane; -1 = mesh_index outside the set


_SO = _lib.SideLibrary(_build.RENDER, {
    "lc_render_workspace_bytes": (c_size_t, [c_int, c_int]),
    "lc_render_depth_f32": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 4 + [c_int] * 3 + [c_float] * 4 + [c_void_p] * 6 + [c_size_t, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load
_A = _args.Args("render")


class MeshSet:
    """Triangle meshes on the device: `meshes` is a list of (verts (Nv,3) float, faces (Nf,3) int) arrays or tensors, `obj_ids` the
    object id of each (default 0, 1, ...).  Everything a launch could fault on is checked HERE, on the host, before the upload: every
    face index lies in [0, Nv) of its own mesh and every vertex is finite.  Keeps the concatenated arrays, the per-mesh table
    (vert_off, n_vert, face_off, n_face) and `max_faces`."""

    def __init__(self, meshes, device, obj_ids=None):
        meshes = list(meshes)
        if not meshes:
            raise ValueError("lc_amd.render: MeshSet needs at least one mesh")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"lc_amd.render: MeshSet lives on the HIP device, got {device} (there is no CPU fallback in the product path)")
        obj_ids = list(range(len(meshes))) if obj_ids is None else [int(o) for o in obj_ids]
        if len(obj_ids) != len(meshes) or len(set(obj_ids)) != len(obj_ids) or min(obj_ids) < 0:
            raise ValueError("lc_amd.render: obj_ids must name every mesh once, with non-negative ids")
        vs, fs, table = [], [], []
        vo = fo = 0
        for k, (v, f) in enumerate(meshes):
            v = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, Tensor) else v)
            f = np.ascontiguousarray(f.detach().cpu().numpy() if isinstance(f, Tensor) else f)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
                raise ValueError(f"lc_amd.render: mesh {k}: verts must be (Nv,3) and faces (Nf,3), got {v.shape} and {f.shape}")
            if not np.issubdtype(f.dtype, np.integer):
                raise TypeError(f"lc_amd.render: mesh {k}: faces must hold integers, got {f.dtype}")
            v = v.astype(np.float32)
            if not np.isfinite(v).all():
                raise ValueError(f"lc_amd.render: mesh {k}: vertices must be finite")
            if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
                raise ValueError(f"lc_amd.render: mesh {k}: face indices must lie in [0, {v.shape[0]}), got [{f.min()}, {f.max()}]")
            vs.append(v)
            fs.append(f.astype(np.int32))
            table.append((vo, v.shape[0], fo, f.shape[0]))
            vo += v.shape[0]
            fo += f.shape[0]
        if vo >= 2 ** 31 or fo >= 2 ** 31:
            raise ValueError("lc_amd.render: more than 2^31 vertices or faces")
        self.obj_ids = obj_ids
        self.n_meshes, self.total_verts, self.total_faces = len(meshes), vo, fo
        self.max_faces = max(e[3] for e in table)
        self.table_host = np.asarray(table, dtype=np.int32)
        self.verts = torch.from_numpy(np.concatenate(vs, 0) if vo else np.zeros((0, 3), np.float32)).to(device)
        self.faces = torch.from_numpy(np.concatenate(fs, 0) if fo else np.zeros((0, 3), np.int32)).to(device)
        self.table = torch.from_numpy(self.table_host).to(device)
        self.device = self.verts.device  # with its index: "cuda" means the current device, and tensors report "cuda:N"
        lut = np.full(max(obj_ids) + 2 if obj_ids else 1, -1, dtype=np.int32)  # last entry: every unknown id
        lut[np.asarray(obj_ids, dtype=np.int64)] = np.arange(len(obj_ids), dtype=np.int32)
        self._lut = torch.from_numpy(lut).to(device)

    def index_of(self, obj_ids) -> Tensor:
        """Device int32 mesh index of each object id (a tensor on the device stays there: nothing is read back); an id that is not in the
        set gives -1, which renders nothing and sets info = -1."""
        ids = obj_ids if isinstance(obj_ids, Tensor) else torch.as_tensor(np.asarray(obj_ids, dtype=np.int64))
        ids = ids.to(self.device).long().reshape(-1)
        n = self._lut.numel() - 1
        ids = torch.where((ids >= 0) & (ids < n), ids, torch.full_like(ids, n))
        return self._lut[ids]


@torch.no_grad()
def render_depth(meshes: MeshSet, mesh_index, R, t, K, size_hw, *, near, far, pixel_center=(0.5, 0.5), want_face=False, want_homo=False,
                 pix2k=None) -> Rendered:
    if not isinstance(meshes, MeshSet):
        raise TypeError(f"lc_amd.render: meshes must be a MeshSet, got {type(meshes)}")
    R = _lib.require_hip_f32("R", R)
    t = _lib.require_hip_f32("t", t)
    K = _lib.require_hip_f32("K", K)
    M = None if pix2k is None else _lib.require_hip_f32("pix2k", pix2k)
    if not isinstance(mesh_index, Tensor) or not mesh_index.is_cuda or mesh_index.dtype != torch.int32:
        raise TypeError("lc_amd.render: mesh_index must be an int32 tensor on the GPU (MeshSet.index_of)")
    B = int(mesh_index.shape[0])
    H, W = int(size_hw[0]), int(size_hw[1])
    _A.rows("mesh_index", mesh_index, (B,))
    R, t = R.reshape(-1, 3, 3), t.reshape(-1, 3)
    _A.rows("R", R, (B, 3, 3))
    _A.rows("t", t, (B, 3))
    _A.rows("K", K, (B, 3, 3))
    if M is not None:
        _A.rows("pix2k", M, (B, 2, 3))
        want_homo = True
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f"lc_amd.render: map sizes of 1 to {MAX_SIZE}, got {H} x {W}")
    dev = meshes.device
    _A.same_device(dev, "the meshes on {}", mesh_index=mesh_index, R=R, t=t, K=K, pix2k=M)
    mesh_index = mesh_index.contiguous()
    lib = load()
    depth = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    mask = torch.empty(B, H, W, device=dev, dtype=torch.bool)
    face = torch.empty(B, H, W, device=dev, dtype=torch.int32) if want_face else None
    homo = torch.empty(B, H, W, 3, device=dev, dtype=torch.float32) if want_homo else None
    info = torch.empty(B, device=dev, dtype=torch.int32)
    nbytes = int(lib.lc_render_workspace_bytes(B, meshes.max_faces))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    with _lib.on_device(dev):
        rc = lib.lc_render_depth_f32(_lib.ptr(meshes.verts), _lib.ptr(meshes.faces), _lib.ptr(meshes.table), _lib.ptr(mesh_index), meshes.n_meshes,
                                     meshes.total_verts, meshes.total_faces, meshes.max_faces, _lib.ptr(R), _lib.ptr(t), _lib.ptr(K), _lib.ptr(M),
                                     B, H, W, float(near), float(far), float(pixel_center[0]), float(pixel_center[1]), _lib.ptr(depth),
                                     _lib.ptr(face), _lib.ptr(mask), _lib.ptr(homo), _lib.ptr(info), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("render.render_depth", rc)
    return Rendered(depth, mask, face, homo, info)


def _affine_inv(M: Tensor) -> Tensor:
    """Inverse of (B,3,3) matrices whose last row is (0,0,1), in closed form (elementwise: no solver call, nothing read back)."""
    a, b, c, d, e, f = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 0], M[:, 1, 1], M[:, 1, 2]
    det = a * e - b * d
    ia, ib, id_, ie = e / det, -b / det, -d / det, a / det
    z, o = torch.zeros_like(a), torch.ones_like(a)
    return torch.stack((ia, ib, -(ia * c + ib * f), id_, ie, -(id_ * c + ie * f), z, z, o), -1).reshape(-1, 3, 3)


def crop_matrices(K_no_aug: Tensor, out_K: Tensor):
    """(K_render (B,3,3), pix2k (B,2,3)) of `render_homo_z_out`: with A = out_K K_no_aug^-1 (dataset.py:421-423), output pixel (x,y)
    samples at K_no_aug-coordinates A^-1 (x,y) + 0.5, i.e. K_render = A T(-0.5) K_no_aug at sample offset 0 and pix2k = A^-1 + 0.5.
    Formed in fp64 on the device and rounded to fp32 once."""
    Kn, Ko = K_no_aug.reshape(-1, 3, 3).double(), out_K.reshape(-1, 3, 3).double()
    A = Ko @ _affine_inv(Kn)
    Tm = torch.eye(3, dtype=torch.float64, device=Kn.device)
    Tm[0, 2] = Tm[1, 2] = -0.5
    Kr = A @ Tm @ Kn
    Kr[:, 2, 0] = 0.0
    Kr[:, 2, 1] = 0.0
    Kr[:, 2, 2] = 1.0
    Ai = _affine_inv(A)[:, :2, :].clone()
    Ai[:, :, 2] += 0.5
    return Kr.float().contiguous(), Ai.float().contiguous()


@torch.no_grad()
def render_homo_z_out(meshes: MeshSet, mesh_index, R, t, K_no_aug, out_K, size_hw, *, near, far):
    """(homo_z_out (B,H,W,3), msk_noc (B,H,W) bool): `dataset.py:293-311` + `:444` on the fly (see the module docstring for the two
    deliberate differences from the stored-file route)."""
    K_no_aug = _lib.require_hip_f32("K_no_aug", K_no_aug)
    out_K = _lib.require_hip_f32("out_K", out_K)
    Kr, pix2k = crop_matrices(K_no_aug, out_K)
    out = render_depth(meshes, mesh_index, R, t, Kr, size_hw, near=near, far=far, pixel_center=(0.0, 0.0), pix2k=pix2k)
    return out.homo_z, out.mask


@torch.no_grad()
def encode_z_info(depth: Tensor):
    """The record `tools/gen_z.py:154-182` stores for one (H,W) depth map in metres, encoded on the device; only the cropped uint16 patch
    (and four box coordinates and two scalars) come back: dict(z_crop, xyxy, z_max, z_min) with z in mm.  A map without a hit gives the
    reference's not-visible record."""
    if depth.dim() != 2:
        raise ValueError(f"lc_amd.render: encode_z_info takes one (H,W) map, got {tuple(depth.shape)}")
    H, W = depth.shape
    msk = depth > 0
    ys, xs = msk.any(1).nonzero().flatten(), msk.any(0).nonzero().flatten()
    if ys.numel() == 0:
        return dict(z_crop=np.zeros((H, W), dtype=np.uint16), xyxy=[0, 0, W - 1, H - 1], z_max=np.zeros(1, dtype=np.float32),
                    z_min=np.zeros(1, dtype=np.float32))
    big = torch.finfo(torch.float32).max
    z_min, z_max = torch.where(msk, depth, depth.new_full((), big)).min(), depth.max()
    code = torch.where(msk, (depth - z_min) / (z_max - z_min + 1e-30) * 65534 + 1, depth.new_zeros(()))
    box = torch.stack((xs[0], ys[0], xs[-1], ys[-1])).cpu().tolist()
    x1, y1, x2, y2 = box
    q = code[y1:y2 + 1, x1:x2 + 1].round().to(torch.int32)
    q = torch.where(q > 32767, q - 65536, q).to(torch.int16)  # the uint16 bit pattern, narrowed on the device: 2 bytes per pixel come back
    crop = q.contiguous().cpu().numpy().view(np.uint16)
    return dict(z_crop=crop, xyxy=[x1, y1, x2, y2], z_max=np.float32(z_max.item() * 1000), z_min=np.float32(z_min.item() * 1000))


def decode_z_info(z_info, size_hw):
    """Host restatement of what the loader makes of a record (`dataset.py:293-311` without the hole filling): (depth (H,W) float32 in
    the record's unit, mask (H,W) bool)."""
    x1, y1, x2, y2 = z_info["xyxy"]
    zc = np.asarray(z_info["z_crop"])
    z_max, z_min = np.float32(np.asarray(z_info["z_max"]).reshape(-1)[0]), np.float32(np.asarray(z_info["z_min"]).reshape(-1)[0])
    depth = np.zeros(size_hw, dtype=np.float32)
    mask = np.zeros(size_hw, dtype=bool)
    m = zc != 0
    z = (zc.astype(np.float32) - 1) * ((z_max - z_min) / 65534) + z_min
    depth[y1:y2 + 1, x1:x2 + 1] = np.where(m, z, 0).astype(np.float32)
    mask[y1:y2 + 1, x1:x2 + 1] = m
    return depth, mask
