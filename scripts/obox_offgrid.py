#!/usr/bin/env python3
"""How far the stated grid search of lc_amd.obox ends above the true minimum on boxes turned by rotations that lie on no grid point:
writes profiles/obox/offgrid_ratio.json.

    python scripts/obox_offgrid.py [--out profiles/obox/offgrid_ratio.json]

The case list is tests/obox_cases.OFF_GRID (the eight corners of a box, half-extents BOX_HALF, turned by each rotation vector and rounded to
fp32); the figures are the numpy oracle's (tests/obox_oracle.py), to which tests/test_gpu_obox.py holds the kernels bit for bit, so no GPU is
needed.  Per case and mode: `volume_over_true` = the recovered volume over the box's own 8 hx hy hz, `aabb_over_true` the same for the box
under the identity, and the path.  About one axis only the last case (a turn about z) can be undone; the others are listed for what they are.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import obox_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obox", "offgrid_ratio.json"))
    args = ap.parse_args()
    true = float(np.prod(np.asarray(cases.BOX_HALF, np.float64) * 2))
    rows = []
    for i, rv in enumerate(cases.OFF_GRID):
        r, z = cases.reference(f"offgrid:{i}"), cases.reference(f"offgrid:{i}", 2)
        rows.append(dict(rotvec_deg=list(rv), volume_over_true=float(r.volume[0]) / true, aabb_over_true=float(r.aabb_volume[0]) / true,
                         path=r.path[0].tolist(), about_z_volume_over_true=float(z.volume[0]) / true, about_z_path=z.path[0].tolist()))
        print(json.dumps(rows[-1]))
    res = dict(source="tests/obox_oracle.py (numpy, fp32 scores)", box_half=list(cases.BOX_HALF), levels=6, step0_deg=9, rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
