#!/usr/bin/env python3
"""Pin the reader of the z_crop records: a record written by THIS project's encoder (lc_amd.render.encode_z_info) from an
oracle-rendered 48 x 64 depth map is fed to the UNMODIFIED reference's loader, `dataset.BOP_Dataset._get_homo_with_depth(annot,
size_hw, fill_hole=False)` (dataset.py:287-311), and its `homo_z`, `msk_full` are stored with the inputs.

Run in the build container only (`python tests/golden/gen_golden_render.py`); the GPU box never sees the reference.  The loader's
module imports cv2, imgaug, pycocotools, imageio and a few modules of the reference that need more; none is used by the method, so
they are stubbed HERE only.  Output: render_reader_48x64.npz (data only).
"""
import gzip
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("LC_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from lc_amd.render import encode_z_info  # noqa: E402
from tests import render_cases as rc  # noqa: E402
from tests import render_oracle as ro  # noqa: E402

CASE = dict(mesh="torus", size_hw=(48, 64))


def _stub(name, **attrs):
    if name in sys.modules:
        return sys.modules[name]
    try:
        __import__(name)
        return sys.modules[name]
    except Exception:  # noqa: BLE001
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        parent, _, child = name.rpartition(".")
        if parent:
            setattr(_stub(parent), child, m)
        return m


def main():
    _stub("cv2", setNumThreads=lambda n: None, INTER_LINEAR=1, INTER_NEAREST=0)
    for name in ("imgaug", "imgaug.augmenters", "pycocotools", "pycocotools.mask", "imageio", "imageio.v2", "lib.bop", "symmetry", "floatbits"):
        _stub(name)
    _stub("model_transform", load_composed_model_info=None)
    import dataset  # the unmodified reference

    v, f = rc.MESHES[CASE["mesh"]]
    pose, size = rc.POSES[CASE["mesh"]], CASE["size_hw"]
    K = rc.camera(size)
    ref = ro.render(v, f, pose.R, pose.t, K, size, rc.NEAR, rc.FAR)
    z_info = encode_z_info(torch.from_numpy(ref.depth))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "000000_000000.pkl.gz")
        with gzip.open(path, "wb") as fh:
            pickle.dump(z_info, fh)
        homo_z, msk_full = dataset.BOP_Dataset._get_homo_with_depth(None, ({}, {"z_path": path}), size, fill_hole=False)
    out = os.path.join(HERE, "render_reader_48x64.npz")
    np.savez_compressed(out, verts=v, faces=f, R=pose.R, t=pose.t, K=K, size_hw=np.asarray(size), near=rc.NEAR, far=rc.FAR,
                        z_crop=z_info["z_crop"], xyxy=np.asarray(z_info["xyxy"]), z_max=np.float32(z_info["z_max"]), z_min=np.float32(z_info["z_min"]),
                        ref_homo_z=homo_z, ref_msk_full=msk_full)
    print(out, os.path.getsize(out), "bytes; hits", int(msk_full.sum()))


if __name__ == "__main__":
    main()
