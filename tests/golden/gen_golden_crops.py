#!/usr/bin/env python3
"""Pin `lc_amd.crops.test_item` against the UNMODIFIED reference loader: `dataset._get_affine_transform` and the non-training branch of
`dataset.BOP_Dataset._get_single_item` (dataset.py:61-108, 367-491) run on objects built by hand with `object.__new__` from
tests/crops_cases.loader_fixture() -- one 37 x 53 frame, two instances, one with `bbox_det` -- and their blobs are stored with every
`cv2.warpAffine` call they made.

Run in the build container only (`python tests/golden/gen_golden_crops.py`); the GPU box never sees the reference.  The modules the
loader imports and that are absent are stubbed HERE only: `cv2.getAffineTransform` is the fp64 three-point solve,
`cv2.warpAffine` records (M, dsize, flags) and returns the oracle's bytes for a uint8 source (zeros for the float masks, whose
warps never reach the test blob), `imageio.v2.imread` returns the frame, `pycocotools.mask.decode` an empty mask.
Output: crops_item.npz (data only).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("LC_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from tests import crops_cases as cc  # noqa: E402
from tests import crops_oracle as co  # noqa: E402

FRAME = cc.FRAMES[3][0]
CALLS = []
INTER_NEAREST, INTER_LINEAR = 0, 1


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


def _warp_affine(src, M, dsize, flags=INTER_LINEAR):
    CALLS.append(dict(M=np.array(M), dsize=tuple(dsize), flags=int(flags), dtype=str(src.dtype), shape=tuple(src.shape)))
    w, h = dsize
    if src.dtype == np.uint8:
        return co.warp_one(src, M, (h, w), co.LINEAR if flags == INTER_LINEAR else co.NEAREST)
    return np.zeros((h, w) + tuple(src.shape[2:]), dtype=src.dtype)


def main():
    _stub("cv2", setNumThreads=lambda n: None, INTER_LINEAR=INTER_LINEAR, INTER_NEAREST=INTER_NEAREST,
          getAffineTransform=lambda src, dst: co.three_point_solve(src, dst), warpAffine=_warp_affine)
    for name in ("imgaug", "imgaug.augmenters", "pycocotools", "lib.bop", "symmetry", "floatbits", "imageio"):
        _stub(name)
    _stub("pycocotools.mask", decode=lambda rle: np.zeros(FRAME.shape[:2], dtype=np.uint8))
    _stub("imageio.v2", imread=lambda path, **kw: FRAME)
    _stub("model_transform", load_composed_model_info=None)
    import dataset  # the unmodified reference

    fx = cc.loader_fixture()
    ds = object.__new__(dataset.BOP_Dataset)
    ds.__dict__.update(fx)
    store = dict(frame=FRAME, n_items=len(fx["np_annots"]), net_input_wh=np.asarray(fx["net_input_wh"]), net_output_wh=np.asarray(fx["net_output_wh"]))
    for i in range(len(fx["np_annots"])):
        del CALLS[:]
        blob = ds[i]  # __getitem__ -> _get_single_item, the non-training branch
        store[f"item{i}_keys"] = np.asarray(list(blob))
        for k, v in blob.items():
            store[f"item{i}_{k}"] = v.numpy() if hasattr(v, "numpy") else np.asarray(v)
        rgb_call = [c for c in CALLS if c["dtype"] == "uint8"]
        assert len(rgb_call) == 1 and rgb_call[0]["dsize"] == tuple(fx["net_input_wh"]) and rgb_call[0]["flags"] == INTER_LINEAR
        store[f"call{i}_in_M"] = rgb_call[0]["M"]
        store[f"call{i}_n_calls"] = len(CALLS)
        # the reference's own helper, once more on its own, for both sizes
        inst = fx["np_annots"][i][1]
        box = inst.get("bbox_det", inst["bbox_visib"])
        center, scale = (box[:2] + box[:2] + box[2:]) * 0.5, float(max(box[2], box[3], 1)) * cc.DZI_PAD_SCALE
        for tag, wh in (("in", fx["net_input_wh"]), ("out", fx["net_output_wh"])):
            A, Ai = dataset._get_affine_transform(center, scale, 0, wh)
            store[f"affine{i}_{tag}"], store[f"affine{i}_{tag}_inv"] = A, Ai
    out = os.path.join(HERE, "crops_item.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes;", {k: (v.dtype, v.shape) for k, v in store.items() if k.startswith("item0_")})


if __name__ == "__main__":
    main()
