"""numpy restatement of the candidate composition of lc_labels.hip (sym_candidate), bit for bit: the fp32 base pose widened to fp64,
every product and sum a numpy ufunc of its own (each rounded once, no fma), in the kernel's order, one rounding to fp32 at the end;
candidate 0 is the base pose copied.  Plus the bound within which two such fp64 evaluations rounded to fp32 may differ."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _terms(base, R_s, t_s):
    """base (B,3,4) float32, R_s (K,3,3), t_s (K,3) float64 -> the three products of every entry, (3,B,K,3,4) float64, and t_b (B,1,3)."""
    b = np.asarray(base, np.float32).astype(np.float64)
    S = np.concatenate((np.asarray(R_s, np.float64), np.asarray(t_s, np.float64)[..., None]), -1)  # (K,3,4)
    prods = np.stack([b[:, None, :, m, None] * S[None, :, None, m, :] for m in range(3)])  # b[i][m] * S[m][j]
    return prods, b[:, None, :, 3]


def compose(base, R_s, t_s):
    """(B,K,3,4) float32: candidate k of row b."""
    p, tb = _terms(base, R_s, t_s)
    v = (p[0] + p[1]) + p[2]
    v[..., 3] = v[..., 3] + tb
    out = v.astype(np.float32)
    out[:, 0] = np.asarray(base, np.float32)
    return out


def bound(base, R_s, t_s):
    """(B,K,3,4) float32: one fp32 spacing at the magnitude of the largest term of each entry."""
    p, tb = _terms(base, R_s, t_s)
    big = np.abs(p).max(0)
    big[..., 3] = np.maximum(big[..., 3], np.abs(tb))
    return np.spacing(big.astype(np.float32))


def batch_candidates(base, transforms, rows):
    """The ragged batch: row b takes the transforms of object rows[b] -> list of (K_b,3,4) float32."""
    return [compose(base[b:b + 1], *transforms[o])[0] for b, o in enumerate(rows)]


def model_info_of(z):
    """The models_info entry a symcand_*.npz was made from."""
    if "sym_discrete" in z.files:
        return {"symmetries_discrete": z["sym_discrete"].tolist()}
    return {"symmetries_continuous": [{"axis": z["axis"].tolist(), "offset": z["offset"].tolist()}]}


def labels_info():
    """(models_info, {case: obj_id of every row}) behind tests/golden/labels_*.npz."""
    with open(os.path.join(GOLDEN, "symcand_labels_info.json")) as f:
        rec = json.load(f)
    return rec["models_info"], rec["obj_id"]
