"""Writes tests/golden/sym_err_b12_m700.npz: the unmodified reference's `lib/utils/error6d.py` mssd, mspd and proj, run in float64 on
inputs that were rounded to float32 first (what the device holds).  12 poses, 700 vertices, objects with K = 1, 2, 4 and 36 transforms
(the last a continuous axis with an offset, 36 steps); the transforms come from lc_amd.symmetry.symmetry_transforms and are handed to the
reference as its [{'R', 't'}] list.  The symmetry behind each minimum is found with the reference too: its mssd / mspd of one symmetry
at a time.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_symerr.py /path/to/reference

Stored: R_est, R_gt (12,3,3), t_est, t_gt (12,3), cam_K (12,3,3), pts (700,3) float32; obj_index (12,) int32; models_info (the four model
infos as JSON), steps; mssd, mspd, proj (12,) float64; mssd_sym, mspd_sym (12,) int64."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import symerr_cases as C  # noqa: E402


def main(ref):
    sys.path.insert(0, os.path.join(ref, "lib", "utils"))
    import error6d

    case, infos = C.golden_inputs()
    B = len(case["obj_index"])
    out = {k: [] for k in ("mssd", "mspd", "proj", "mssd_sym", "mspd_sym")}
    for b in range(B):
        Re, te, Rg, tg, K, pts, R_s, t_s = C.pose_args(case, b)
        te, tg = te.reshape(3, 1), tg.reshape(3, 1)
        syms = [{"R": R, "t": t.reshape(3, 1)} for R, t in zip(R_s, t_s)]
        out["mssd"].append(error6d.mssd(Re, te, Rg, tg, pts, syms))
        out["mspd"].append(error6d.mspd(Re, te, Rg, tg, K, pts, syms))
        out["proj"].append(error6d.proj(Re, te, Rg, tg, K, pts))
        e3 = [error6d.mssd(Re, te, Rg, tg, pts, [s]) for s in syms]
        e2 = [error6d.mspd(Re, te, Rg, tg, K, pts, [s]) for s in syms]
        assert min(e3) == out["mssd"][-1] and min(e2) == out["mspd"][-1]
        out["mssd_sym"].append(int(np.argmin(e3)))
        out["mspd_sym"].append(int(np.argmin(e2)))
    rec = {k: case[k] for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K", "pts", "obj_index")}
    rec.update(models_info=np.asarray(json.dumps(infos)), steps=np.int64(36))
    rec.update({k: np.asarray(v, np.float64) for k, v in out.items() if not k.endswith("_sym")})
    rec.update({k: np.asarray(v, np.int64) for k, v in out.items() if k.endswith("_sym")})
    path = os.path.join(HERE, "sym_err_b12_m700.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), out["mssd_sym"], out["mspd_sym"])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LC_REFERENCE", ""))
