#!/usr/bin/env python3
"""Pin lc_amd.vsd to BOP's own toolkit (bop_toolkit_lib.pose_error.vsd, visib_mode 'bop19', cost_type 'step').

This cannot run in the build container (`import bop_toolkit_lib` fails, and its renderer needs an OpenGL context), which is why the BOP
boundary of include/lc_amd_vsd.h is "unpinned": the contract is this project's restatement.  On ANY machine with the toolkit, one run of

    python tests/golden/gen_golden_vsd_bop.py

stores in tests/golden/vsd_bop.npz, for every valid row of tests/vsd_cases.py seen through its camera WITHOUT the skew (the toolkit's
renderer and its depth-to-distance conversion take fx, fy, cx, cy only), what the toolkit itself produced: its two rendered depth maps,
the scene depth made of its renders, K, delta, the taus, the diameter and its errors.  tests/test_vsd_bop_golden.py then stops skipping: it
feeds those maps to `vsd_from_depth` and demands equal errors, except on records where the one numerical difference of the definitions
(BOP rounds the distance images to fp32 before it subtracts, here the differences stay fp64) decides a pixel; it counts those pixels and
caps them at 1 in 10^4.  The toolkit path below has never been run by this project (nothing to run it with); the file format and the
checks have, through

    python tests/golden/gen_golden_vsd_bop.py --stand-in [--out DIR]

which writes the same file from tests/render_oracle.py and tests/vsd_oracle.py (`source` says which of the two made a file).  Data only is
stored.  Unit: metres.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import render_cases as rc  # noqa: E402
from tests import vsd_cases as C  # noqa: E402
from tests import vsd_oracle  # noqa: E402

FILE = "vsd_bop.npz"
FIELDS = ("depth_est", "depth_gt", "depth_test", "K", "taus", "diameter", "errors")  # diameter: NaN = the taus are absolute


def records():
    """[(key, case with the skew-free camera, row)] of every stored record: the valid rows of the case list."""
    out = []
    for c in C.CASES:
        K = c.K.copy()
        K[0, 1] = 0
        c0 = c._replace(K=K)
        out += [(f"{c.name}/{i}", c0, r) for i, r in enumerate(c.rows) if 0 <= r.scene < len(c.scenes)]
    return out


def _pack(store, key, est, gt, test, c, row, errors):
    vals = (est, gt, test, c.K, np.asarray(c.taus, np.float32), np.float32(C.DIAMETER[row.mesh] if c.normalised else np.nan), np.asarray(errors, np.float64))
    for name, v in zip(FIELDS, vals):
        store[f"{key}/{name}"] = v


def stand_in():
    """The records as the render oracle and the score oracle make them."""
    store = dict(source=np.asarray("stand-in: tests/render_oracle.py + tests/vsd_oracle.py"), delta=np.float32(C.DELTA))
    for key, c, row in records():
        est, gt = C.render(c, row.mesh, row.est).depth, C.render(c, row.mesh, row.gt).depth
        test = C.scene_depth(c, c.scenes[row.scene])
        ref = vsd_oracle.score(est, gt, test, c.K, C.DELTA, c.taus, C.DIAMETER[row.mesh] if c.normalised else None)
        _pack(store, key, est, gt, test, c, row, ref.errors.astype(np.float64))
    return store


def from_toolkit():
    try:
        import bop_toolkit_lib
        from bop_toolkit_lib import inout, pose_error, renderer
    except Exception as e:  # noqa: BLE001
        raise SystemExit(f"gen_golden_vsd_bop: BOP's toolkit is needed ({e}); run this where `import bop_toolkit_lib` works, or pass --stand-in")
    store = dict(source=np.asarray(f"bop_toolkit_lib {getattr(bop_toolkit_lib, '__version__', 'unknown version')}"), delta=np.float32(C.DELTA))
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for i, m in enumerate(C.MESH_NAMES):
            v, f = rc.MESHES[m]
            paths[m] = os.path.join(tmp, f"obj_{i + 1:06d}.ply")
            inout.save_ply(paths[m], dict(pts=v.astype(np.float64), faces=f.astype(np.int64)))
        rens = {}

        def ren_of(size_hw):
            if size_hw not in rens:
                rens[size_hw] = renderer.create_renderer(size_hw[1], size_hw[0], renderer_type="vispy", mode="depth")
                for i, m in enumerate(C.MESH_NAMES):
                    rens[size_hw].add_object(i + 1, paths[m])
            return rens[size_hw]

        def depth(c, mesh, p):
            K = c.K.astype(np.float64)
            out = ren_of(c.size_hw).render_object(C.MESH_NAMES.index(mesh) + 1, p.R.astype(np.float64), p.t.astype(np.float64).reshape(3, 1),
                                                  K[0, 0], K[1, 1], K[0, 2], K[1, 2])
            return np.asarray(out["depth"], dtype=np.float32)

        for key, c, row in records():
            s = c.scenes[row.scene]
            test = np.full(c.size_hw, np.float32(s.plane), dtype=np.float32)
            for mesh, p in s.objects:
                d = depth(c, mesh, p)
                test = np.where((d > 0) & (d < test), d, test)
            if s.patch is not None:
                y0, y1, x0, x1 = s.patch
                test[y0:y1, x0:x1] = 0
            est, gt = depth(c, row.mesh, row.est), depth(c, row.mesh, row.gt)
            errors = pose_error.vsd(row.est.R.astype(np.float64), row.est.t.astype(np.float64).reshape(3, 1), row.gt.R.astype(np.float64),
                                    row.gt.t.astype(np.float64).reshape(3, 1), test, c.K.astype(np.float64), float(np.float32(C.DELTA)),
                                    [float(np.float32(t)) for t in c.taus], bool(c.normalised), float(np.float32(C.DIAMETER[row.mesh])),
                                    ren_of(c.size_hw), C.MESH_NAMES.index(row.mesh) + 1, "step")
            _pack(store, key, est, gt, test.astype(np.float32), c, row, errors)
    return store


def main(out_dir=HERE, use_stand_in=False):
    store = stand_in() if use_stand_in else from_toolkit()
    path = os.path.join(out_dir, FILE)
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes,", len(records()), "records,", str(store["source"]))
    return path


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stand-in", action="store_true", help="write the file from the project's own oracles (exercises format and checks)")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    main(a.out, a.stand_in)
