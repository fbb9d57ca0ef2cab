"""A restatement of the Ranger step (RAdam + Lookahead + gradient centralisation) written from its formulas, in any float dtype: float64 on
the CPU is the oracle, float32 the reference's own rounding (one rounding per torch op, in the order the reference issues them).  Also the
golden case of tests/golden/gen_golden_ranger.py: its tensors, groups, per-step learning rates and seeded gradients.

The step scalars follow the reference's host logic: N_sma and step_size from the tensor's own step count, cached in ten slots keyed by
`step % 10` alone (shared by all groups: a group with other betas reuses another group's entry for the same step), the RAdam branch
when N_sma > threshold, weight decay only when it is non-zero, the Lookahead sync when the tensor's step is a multiple of k."""
import math

import torch

SHAPES = [(32, 16, 3, 3), (16, 8, 4, 4), (1, 64), (16,), (3, 7, 5)]
GROUPS = [dict(idx=[0, 1], lr=2e-4, weight_decay=1e-4), dict(idx=[2, 3], lr=1e-3, weight_decay=0),
          dict(idx=[4], lr=5e-4, weight_decay=1e-3, betas=(0.9, 0.99))]
STEPS = 13
SNAPSHOTS = (5, 6, 12, 13)
NO_GRAD = {3: (3, 4)}  # tensor 3 has no gradient on steps 3 and 4
STATE_KEYS = ("exp_avg", "exp_avg_sq", "slow_buffer")


def lr_at(group, t):
    return group["lr"] * (1 + 0.1 * t)


def initial_params(dtype=torch.float32):
    g = torch.Generator().manual_seed(1234)
    return [torch.randn(s, generator=g, dtype=torch.float64).float().to(dtype) for s in SHAPES]


def grad_at(i, t, dtype=torch.float32):
    """Gradient of tensor i on step t (1-based), None where the golden case has none; every row gets an offset so centralisation matters."""
    if t in NO_GRAD.get(i, ()):
        return None
    g = torch.Generator().manual_seed(100000 + 1000 * t + i)
    x = torch.randn(SHAPES[i], generator=g, dtype=torch.float64) * 0.1
    if x.dim() > 1:
        x = x + torch.randn((SHAPES[i][0],) + (1,) * (x.dim() - 1), generator=g, dtype=torch.float64) * 0.05
    return x.float().to(dtype)  # the float32 inputs, whatever dtype runs on them


class Oracle:
    """Ranger in the dtype of the tensors it is handed.  groups: list of dicts with 'params' (tensors updated in place), 'lr', 'betas',
    'eps', 'weight_decay', 'k'; state[i] is the per-tensor dict (step, exp_avg, exp_avg_sq, slow_buffer)."""

    def __init__(self, groups, alpha=0.5, N_sma_threshhold=5, gc_gradient_threshold=1):
        self.groups = groups
        self.alpha, self.thr, self.gc = alpha, N_sma_threshhold, gc_gradient_threshold
        self.cache = [[None, None, None] for _ in range(10)]
        self.state = {}

    def scalars(self, step, beta1, beta2):
        c = self.cache[int(step % 10)]
        if c[0] != step:
            b2t = beta2 ** step
            n_max = 2 / (1 - beta2) - 1
            n_sma = n_max - 2 * step * b2t / (1 - b2t)
            if n_sma > self.thr:
                size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** step)
            else:
                size = 1.0 / (1 - beta1 ** step)
            c[:] = [step, n_sma, size]
        return c[1], c[2]

    def step(self, grads):
        """grads: one list per group (None = no gradient); the centred gradients are written back into the given tensors."""
        for group, gl in zip(self.groups, grads):
            beta1, beta2 = group["betas"]
            for p, g in zip(group["params"], gl):
                if g is None:
                    continue
                st = self.state.setdefault(id(p), {})
                if not st:
                    st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), slow_buffer=p.clone())
                if g.dim() > self.gc and g.numel():
                    g.add_(-g.mean(dim=tuple(range(1, g.dim())), keepdim=True))
                st["step"] += 1
                m, v, s = st["exp_avg"], st["exp_avg_sq"], st["slow_buffer"]
                v.mul_(beta2).add_((g * (1 - beta2)) * g)
                m.mul_(beta1).add_(g * (1 - beta1))
                n_sma, size = self.scalars(st["step"], beta1, beta2)
                lr, wd = group["lr"], group["weight_decay"]
                if wd != 0:
                    p.add_(p * (-wd * lr))
                if n_sma > self.thr:
                    p.add_((m / (v.sqrt() + group["eps"])) * (-size * lr))
                else:
                    p.add_(m * (-size * lr))
                if st["step"] % group["k"] == 0:
                    s.add_((p - s) * self.alpha)
                    p.copy_(s)


def golden_groups(params):
    """The golden case's param groups over `params` (constructor defaults: betas (0.95, 0.999), eps 1e-5, k 6)."""
    out = []
    for spec in GROUPS:
        out.append(dict(params=[params[i] for i in spec["idx"]], lr=spec["lr"], weight_decay=spec["weight_decay"],
                        betas=spec.get("betas", (0.95, 0.999)), eps=1e-5, k=6))
    return out


def run_golden(dtype, upto=STEPS, on_snapshot=None, device="cpu"):
    """The golden trajectory with the oracle: calls on_snapshot(t, params, grads, oracle) after each snapshot step."""
    params = [p.to(dtype).to(device) for p in initial_params()]
    groups = golden_groups(params)
    o = Oracle(groups)
    for t in range(1, upto + 1):
        for grp, spec in zip(groups, GROUPS):
            grp["lr"] = lr_at(spec, t)
        grads = [grad_at(i, t, dtype) for i in range(len(SHAPES))]
        grads = [None if g is None else g.to(device) for g in grads]
        o.step([[grads[i] for i in spec["idx"]] for spec in GROUPS])
        if on_snapshot and t in SNAPSHOTS:
            on_snapshot(t, params, grads, o)
    return params, o
