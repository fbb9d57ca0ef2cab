"""Writes tests/golden/symcand_*.npz: the unmodified reference's `symmetry.symmetry_pose_candidates` (scipy's Rotation inside) run in
float64 on base poses that were rounded to float32 first (what the device holds), its result rounded once to float32 -- and
tests/golden/symcand_labels_info.json: the `models_info` entries that gen_golden_labels.py drew for the labels_*.npz cases (recorded by
running its `cases` with the reference's function wrapped), with the object of every batch row of those files.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_symcand.py /path/to/reference

Per file: base_R (B,3,3), base_t (B,3) float64 (|t| up to ~1500, mm); steps; sym_discrete (D-1,16) and / or axis, offset (3,);
cand (B,K,3,4) float32."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden_labels import cases as label_cases, rot  # noqa: E402


def poses(rng, B):
    R = np.stack([rot(rng) for _ in range(B)])
    t = np.stack([rng.uniform(-400, 400, B), rng.uniform(-400, 400, B), rng.uniform(300, 1500, B)], -1)
    return R, t


def discrete(rng, D):
    syms = []
    for _ in range(D - 1):
        S = np.eye(4)
        S[:3, :3] = rot(rng)
        S[:3, 3] = rng.uniform(-30, 30, 3)
        syms.append(S.reshape(-1).tolist())
    return {"symmetries_discrete": syms}


def continuous(rng):
    axis = np.zeros(3)
    while np.abs(axis).min() < 0.2:  # far from every coordinate axis
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
    return {"symmetries_continuous": [{"axis": axis.tolist(), "offset": rng.uniform(-20, 20, 3).tolist()}]}


def main(ref):
    sys.path.insert(0, ref)
    import symmetry

    rng = np.random.default_rng(20261019)
    todo = {"discrete2": (discrete(rng, 2), 384, 8), "discrete4": (discrete(rng, 4), 384, 8), "continuous384": (continuous(rng), 384, 6),
            "continuous7": (continuous(rng), 7, 8)}
    for name, (info, steps, B) in todo.items():
        R, t = poses(rng, B)
        R32, t32 = R.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
        cand = np.stack([symmetry.symmetry_pose_candidates(R32[b], t32[b], info, continuous_steps=steps) for b in range(B)])
        rec = dict(base_R=R, base_t=t, steps=np.int64(steps), cand=cand.astype(np.float32))
        if "symmetries_discrete" in info:
            rec["sym_discrete"] = np.asarray(info["symmetries_discrete"], np.float64)
        else:
            rec["axis"] = np.asarray(info["symmetries_continuous"][0]["axis"], np.float64)
            rec["offset"] = np.asarray(info["symmetries_continuous"][0]["offset"], np.float64)
        path = os.path.join(HERE, f"symcand_{name}.npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), cand.shape)

    # the models_info behind the labels_*.npz cases: object 1 has no symmetry, 2 the discrete one, 3 the continuous one
    seen = []

    class Recording:
        @staticmethod
        def symmetry_pose_candidates(R, t, info, continuous_steps=384):
            if not any(info is s for s in seen):
                seen.append(info)
            return symmetry.symmetry_pose_candidates(R, t, info, continuous_steps)

    label_cases(Recording)
    disc = next(s for s in seen if "symmetries_discrete" in s)
    cont = next(s for s in seen if "symmetries_continuous" in s)
    assert len(seen) == 2
    rec = {"models_info": {"1": {}, "2": disc, "3": cont},
           "obj_id": {"nosym": [1, 1, 1], "discrete3d": [1, 1, 2, 2, 2], "continuous3d": [3] * 4, "pts2d": [3] * 4, "notstarted": [1, 2, 2, 2]}}
    path = os.path.join(HERE, "symcand_labels_info.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LC_REFERENCE", ""))
