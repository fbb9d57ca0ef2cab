"""The argument rules of the side-library bindings, each written once.  A binding module holds `_A = _args.Args("<module>")` and every
refusal starts with `lc_amd.<module>: `.  Where the modules word or decide a rule differently, the difference is an argument here and
nothing is unified.  Nothing touches the device, synchronises or allocates -- but `scene_index`, which makes the one index tensor the
kernels need -- so every caller stays capturable in a graph."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
from torch import Tensor


MESHES_ON = "the meshes are on {} (there is no CPU fallback in the product path)"  # `first` of same_device where a MeshSet leads the call


def _stars(shape) -> str:
    return f"({', '.join('*' if d is None else str(d) for d in shape)})"


class Args:
    def __init__(self, module: str):
        self.p = f"lc_amd.{module}"

    def tensor(self, name, t, dtypes, what, shape, expected=None) -> Tensor:
        """Type, element type (`what` names `dtypes` in the message) and shape (None: any size; `expected`: how the message writes it)."""
        if not isinstance(t, Tensor):
            raise TypeError(f"{self.p}: {name} must be a torch.Tensor, got {type(t)}")
        if t.dtype not in dtypes:
            raise TypeError(f"{self.p}: {name} must be {what}, got {t.dtype}")
        if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
            raise ValueError(f"{self.p}: {name} has shape {tuple(t.shape)}, expected {expected or _stars(shape)}")
        return t

    def f32(self, name, t, shape) -> Tensor:
        return self.tensor(name, t, (torch.float32,), "float32", shape)

    def i32(self, name, t, shape) -> Tensor:
        """An index tensor of a fixed shape, int32 or int64 (the caller converts); the message writes the shape as a tuple."""
        return self.tensor(name, t, (torch.int32, torch.int64), "int32 or int64", shape, str(tuple(shape)))

    def rows(self, name, t, shape):
        """The shape alone, of a tensor that `_lib.require_hip_f32` has passed."""
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{self.p}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")

    def whole(self, name, v, lo, hi, numpy=False) -> int:
        """A whole number of lo to hi, never a bool; numpy: numpy's integer scalars count as whole numbers too."""
        if isinstance(v, bool) or not isinstance(v, (int, np.integer) if numpy else int):
            raise TypeError(f"{self.p}: {name} must be a whole number, got {type(v)}")
        v = int(v)
        if not (lo <= v <= hi):
            raise ValueError(f"{self.p}: {name} of {lo} to {hi}, got {v}")
        return v

    def pair(self, name, v):
        if isinstance(v, (Tensor, str)) or not hasattr(v, "__len__") or len(v) != 2:
            raise ValueError(f"{self.p}: {name} is a pair, got {v!r}")
        return v[0], v[1]

    def size_pair(self, name, hw, limit, numpy=False):
        """(h, w), each a whole number of 1 to limit."""
        h, w = self.pair(name, hw)
        return self.whole(name, h, 1, limit, numpy), self.whole(name, w, 1, limit, numpy)

    def center(self, pixel_center, cx_cy=False):
        """pixel_center as two floats.  cx_cy: the older wording of lc_amd.vsd, which names the members and lets any two-element object through."""
        if not cx_cy:
            cx, cy = self.pair("pixel_center", pixel_center)
            return float(cx), float(cy)
        if not hasattr(pixel_center, "__len__") or len(pixel_center) != 2:
            raise ValueError(f"{self.p}: pixel_center is a pair (cx, cy), got {pixel_center!r}")
        return float(pixel_center[0]), float(pixel_center[1])

    def delta(self, delta) -> float:
        if isinstance(delta, bool) or not isinstance(delta, (int, float)):
            raise TypeError(f"{self.p}: delta must be a number, got {type(delta)}")
        if not math.isfinite(delta) or delta < 0:
            raise ValueError(f"{self.p}: delta must be finite and not negative, got {delta}")
        return float(delta)

    def host_floats(self, name, x, n):
        """normalize's mean or std as n C floats of a kernel argument; a tensor is read back here, once."""
        vals = [float(v) for v in (x.detach().cpu().reshape(-1).tolist() if isinstance(x, Tensor) else np.asarray(x, dtype=np.float64).reshape(-1))]
        if len(vals) != n:
            raise ValueError(f"{self.p}: normalize {name} must hold one value per channel ({n}), got {len(vals)}")
        return (ctypes.c_float * n)(*vals)

    def same_device(self, dev, first, **named):
        """Every tensor of `named` (None entries pass) is on `dev`; `first` words where the call's first tensor is, `{}` standing for `dev`."""
        for name, t in named.items():
            if t is not None and t.device != dev:
                raise RuntimeError(f"{self.p}: {name} is on {t.device}, {first.format(dev)}")

    def scenes(self, depth_test, scene_index, B: int, noun: str):
        """depth_test as (S,H,W) and the rule for a missing scene_index: one scene serves every pose (`noun`: what the module calls a
        row), B scenes serve one each.  -> (depth_test, S)"""
        if isinstance(depth_test, Tensor) and depth_test.dim() == 2:
            depth_test = depth_test[None]
        Dt = self.f32("depth_test", depth_test, (None, None, None))
        S = int(Dt.shape[0])
        if scene_index is None:
            if S not in (1, B):
                raise ValueError(f"{self.p}: scene_index is needed to tell which of the {S} scenes each of the {B} {noun} belongs to")
        else:
            self.i32("scene_index", scene_index, (B,))
        return Dt, S

    @staticmethod
    def scene_index(scene_index, S: int, B: int, dev) -> Tensor:
        if scene_index is None:
            return torch.zeros(B, device=dev, dtype=torch.int32) if S == 1 else torch.arange(B, device=dev, dtype=torch.int32)
        return scene_index.to(torch.int32).contiguous()

    def cam_K(self, name, K, B: int, f32=None) -> Tensor:
        """K (B,3,3), or (3,3) for every row: expanded as a view, made contiguous by the caller on the device."""
        if isinstance(K, Tensor) and tuple(K.shape) == (3, 3):
            K = K.expand(B, 3, 3)
        return (f32 or self.f32)(name, K, (B, 3, 3))

    def pose_batch(self, mesh_index, R: dict, t: dict, K, K_name="K", f32=None):
        """The rules of B poses, in this order: mesh_index, where there is one, is an int32 (B,) tensor and sets B (else the first R does);
        every R of `R` (name -> tensor) is (B,3,3); every t of `t` is (B,3) or (B,3,1) and comes back as (B,3); K as `cam_K`.  `f32` is the
        check of the float tensors (default: `self.f32`).  -> (B, [R ...], [t ...], K)"""
        f32 = f32 or self.f32
        B = None
        if mesh_index is not None:
            if not isinstance(mesh_index, Tensor) or mesh_index.dtype != torch.int32:
                raise TypeError(f"{self.p}: mesh_index must be an int32 tensor on the GPU (MeshSet.index_of)")
            if mesh_index.dim() != 1:
                raise ValueError(f"{self.p}: mesh_index has shape {tuple(mesh_index.shape)}, expected (B,)")
            B = int(mesh_index.shape[0])
        Rs = []
        for name, x in R.items():
            Rs.append(f32(name, x, (B, 3, 3)))
            B = int(Rs[0].shape[0])
        for name, x in t.items():
            if isinstance(x, Tensor) and tuple(x.shape) not in ((B, 3), (B, 3, 1)):
                raise ValueError(f"{self.p}: {name} has shape {tuple(x.shape)}, expected {(B, 3)} or {(B, 3, 1)}")
        ts = [f32(name, x.reshape(B, 3) if isinstance(x, Tensor) else x, (B, 3)) for name, x in t.items()]
        return B, Rs, ts, self.cam_K(K_name, K, B, f32)
