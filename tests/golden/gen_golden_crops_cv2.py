#!/usr/bin/env python3
"""Pin the zoom-in crops to the REAL cv2.warpAffine (dataset.py:411,425-426; OpenCV 4.6.0.66 is pinned in the reference's
scripts/req_0.txt).

This cannot run in the build container (no OpenCV: `import cv2` fails), which is why bit parity at this boundary is "unpinned": the
contract of include/lc_amd_crop.h is OpenCV's published fixed-point scheme for 8-bit images, but newer OpenCV builds take float or IPP
paths for some shapes.  On ANY machine with `opencv-python`, one run of

    python tests/golden/gen_golden_crops_cv2.py

stores, for every case of tests/crops_cases.py (both channel counts, every output size, both interpolations), the bytes of
`cv2.warpAffine(src, M, dsize, flags=flags)` in tests/golden/crops_cv2.npz with OpenCV's version string, after which
tests/test_crops_cv2_golden.py stops skipping and demands equality with them.  Rows whose matrix is not finite are left out (the
reference never builds one; what OpenCV makes of it is not part of the contract).  The inputs are generated from fixed seeds, so they
are bit-identical wherever the generator runs.  Data only is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import crops_cases as cc  # noqa: E402


def keys():
    """[(key, C, frame, name, M, (h, w), interp)] of every stored crop."""
    out = []
    for C in (3, 1):
        for hw in cc.OUT_SIZES:
            for interp in ("linear", "nearest"):
                for k, (name, M) in enumerate(cc.CASES):
                    if np.isfinite(M).all():
                        f = int(cc.FRAME_INDEX[k % cc.B])
                        out.append((f"c{C}_{hw[0]}x{hw[1]}_{interp}_{name}", C, f, name, M, hw, interp))
    return out


def main(out_dir=HERE):
    try:
        import cv2
    except Exception as e:  # noqa: BLE001
        raise SystemExit(f"gen_golden_crops_cv2: OpenCV is needed ({e}); run this where `import cv2` works")
    cv2.setNumThreads(0)
    store = dict(cv2_version=np.asarray(cv2.__version__))
    for key, C, f, name, M, (h, w), interp in keys():
        src = cc.FRAMES[C][f] if C == 3 else cc.FRAMES[C][f][..., 0]
        dst = cv2.warpAffine(src, M, (w, h), flags=cv2.INTER_LINEAR if interp == "linear" else cv2.INTER_NEAREST)
        store[key] = dst.reshape(h, w, C)
    path = os.path.join(out_dir, "crops_cv2.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes,", len(store) - 1, "crops, OpenCV", cv2.__version__)


if __name__ == "__main__":
    main()
