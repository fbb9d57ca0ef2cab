#!/usr/bin/env python3
"""Pin the run-length mask store to the REAL pycocotools (dataset.py:180,379; pycocotools 2.0.6 is pinned in the reference's
scripts/req_0.txt).

This cannot run in the build container (`import pycocotools` fails), which is why that boundary is "unpinned": the contract of
include/lc_amd_rle.h and lc_amd/rle.py is this project's statement of COCO's format and of its compressed string.  On ANY machine with
pycocotools, one run of

    python tests/golden/gen_golden_rle_coco.py

stores, for every valid mask of tests/rle_cases.py (three frame sizes), pycocotools' own `encode(np.asfortranarray(mask))['counts']`,
`area` and `toBbox` in tests/golden/rle_coco.json with the package's version, after which tests/test_rle_coco_golden.py stops skipping
and demands equality with them.  The masks are made from fixed lists and seeds, so they are bit-identical wherever the generator runs.
Data only is stored.  `main(out_dir, stand_in=True)` writes the same file from the project's own oracle: the test uses it to prove that
the check works and refuses a spoilt copy.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import rle_cases as cases, rle_oracle as oracle  # noqa: E402

NAME = "rle_coco.json"


def keys():
    """[(key, (H, W), mask (H,W) uint8)] of every stored record."""
    return [(f"{H}x{W}-{name}", (H, W), oracle.decode(c, H, W)) for H, W in cases.FRAMES for name, c in cases.valid_lists(H, W)]


def main(out_dir=HERE, stand_in=False):
    store = {}
    if stand_in:
        version = "stand-in: tests/rle_oracle.py"
        for key, (H, W), m in keys():
            area, (x0, y0, x1, y1) = oracle.area_box(m)
            store[key] = dict(counts=oracle.to_string(oracle.encode(m)), area=area, bbox=[x0, y0, x1 - x0 + 1, y1 - y0 + 1] if area else [0, 0, 0, 0])
    else:
        try:
            import pycocotools
            import pycocotools.mask as cocomask
        except Exception as e:  # noqa: BLE001
            raise SystemExit(f"gen_golden_rle_coco: pycocotools is needed ({e}); run this where `import pycocotools.mask` works")
        version = str(getattr(pycocotools, "__version__", "unknown"))
        for key, (H, W), m in keys():
            r = cocomask.encode(np.asfortranarray(m))
            assert list(r["size"]) == [H, W] and np.array_equal(cocomask.decode(r), m)
            store[key] = dict(counts=r["counts"].decode("ascii"), area=int(cocomask.area(r)), bbox=[int(v) for v in cocomask.toBbox(r)])
    path = os.path.join(out_dir, NAME)
    with open(path, "w") as f:
        json.dump(dict(pycocotools_version=version, records=store), f, indent=0)
    print(path, os.path.getsize(path), "bytes,", len(store), "records, pycocotools", version)
    return path


if __name__ == "__main__":
    main()
