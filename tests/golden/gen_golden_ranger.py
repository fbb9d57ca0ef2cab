"""Writes tests/golden/ranger_golden.npz and ranger_state_dict.json: the unmodified reference's `lib.optim.ranger.Ranger` run on the CPU in
float32 on the golden case of tests/ranger_oracle.py (its tensors, three param groups, per-step learning rates, seeded gradients, a tensor
without a gradient on steps 3-4).  After each snapshot step t it stores, per tensor i, `s{t}_t{i}_{p,grad,exp_avg,exp_avg_sq,slow_buffer}`
(grad: the centred gradient the reference leaves in p.grad) and `s{t}_t{i}_step`; the JSON records the layout of the reference's
`state_dict()` at the end (param_groups keys and values, state keys, types and shapes).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ranger.py /path/to/reference
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ranger_oracle as ro  # noqa: E402


def main(ref):
    sys.path.insert(0, ref)
    from lib.optim.ranger import Ranger

    params = [p.clone() for p in ro.initial_params()]
    groups = []
    for spec in ro.GROUPS:
        g = dict(params=[params[i] for i in spec["idx"]], lr=spec["lr"], weight_decay=spec["weight_decay"])
        if "betas" in spec:
            g["betas"] = spec["betas"]
        groups.append(g)
    with contextlib.redirect_stdout(io.StringIO()):
        opt = Ranger(groups)
    out = {}
    for t in range(1, ro.STEPS + 1):
        for grp, spec in zip(opt.param_groups, ro.GROUPS):
            grp["lr"] = ro.lr_at(spec, t)
        for i, p in enumerate(params):
            p.grad = ro.grad_at(i, t)
        opt.step()
        if t in ro.SNAPSHOTS:
            for i, p in enumerate(params):
                st = opt.state[p]
                out[f"s{t}_t{i}_p"] = p.numpy().copy()
                out[f"s{t}_t{i}_grad"] = (p.grad if p.grad is not None else torch.full_like(p, float("nan"))).numpy().copy()
                out[f"s{t}_t{i}_step"] = np.int64(st["step"])
                for k in ro.STATE_KEYS:
                    out[f"s{t}_t{i}_{k}"] = st[k].numpy().copy()
    np.savez_compressed(os.path.join(HERE, "ranger_golden.npz"), **out)
    sd = opt.state_dict()
    layout = {"param_groups": [{k: (v if k != "params" else list(v)) for k, v in g.items()} for g in sd["param_groups"]],
              "state": {str(i): {k: ({"type": "tensor", "dtype": str(v.dtype), "shape": list(v.shape)} if torch.is_tensor(v) else
                                     {"type": type(v).__name__, "value": v}) for k, v in st.items()} for i, st in sd["state"].items()}}
    with open(os.path.join(HERE, "ranger_state_dict.json"), "w") as f:
        json.dump(layout, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LC_REFERENCE", ""))
