#!/usr/bin/env python3
"""One JSON line: the fused Ranger step (lc_amd.optim.Ranger) on the parameter sets of the example models (examples/train_dense_ddp.py,
--trunk cdpn and --trunk os8 at --width 64, channels_last as the examples lay them out), next to a per-tensor loop of torch ops.

The per-tensor loop (`per_tensor_loop_*`) is NOT the reference's code, which this script does not run: it is a restatement of Ranger's
step with the reference's op structure per tensor (mean / neg / add_ for the centralisation, mul_ + addcmul_, mul_ + add_ with alpha,
add_ with alpha for the weight decay, sqrt + add_ + addcdiv_ or add_ with alpha for the update, sub + add_ with alpha + copy_ for
Lookahead), run tensor by tensor on the device.

Per set: the fused kernel's device time per step (torch.profiler, averaged over k = 6 consecutive steps, one of them a Lookahead step)
and the algorithmic bytes (per element read p, grad, exp_avg, exp_avg_sq and write them back, the gradient only where it is centralised;
slow_buffer read and written on the Lookahead step) -> GB/s and the fraction of 8 TB/s; the same with the gradients as views into one
flat buffer packed like a DDP gradient bucket (`bucket_*`: arrays out of 16-byte phase with their parameter take 4-byte accesses);
device-event time per back-to-back step() of each form; launches per step; and the host time of step() in a loop that frees and
reallocates the gradients every step (zero_grad(set_to_none=True), as the reference's train.py does) with the number of table builds.
--train adds the median example training step (glmo shape, bf16, B = 32) with each optimizer.

    python scripts/bench_optim.py [--steps 60] [--train]
"""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples")]

PEAK = 8.0e12


def model_params(trunk, width):
    import train_dense_ddp as ex

    torch.manual_seed(0)
    m = ex.DenseNet(3, width, trunk).cuda().to(memory_format=torch.channels_last)
    return [p.detach().clone() for p in m.parameters()]


def with_grads(params, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in params:
        p.grad = torch.empty_like(p).normal_(generator=g).mul_(1e-3)
    return params


def algorithmic_bytes(params, k=6):
    per = 0
    for p in params:
        centred = p.dim() > 1
        per += p.numel() * 4 * ((8 if centred else 7) + 2 / k)
    return per


def timed(step, n):
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e-3


def launches(step):
    from torch.profiler import ProfilerActivity, profile

    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "Memcpy" not in e.name
               and not e.name.startswith("Optimizer.step"))


class PerTensorLoop:
    """Ranger's step tensor by tensor in torch ops, with the reference's op structure (see the module docstring)."""

    def __init__(self, params, lr, wd, betas=(0.95, 0.999), eps=1e-5, k=6, alpha=0.5, thr=5):
        self.params, self.lr, self.wd, self.betas, self.eps, self.k, self.alpha, self.thr = params, lr, wd, betas, eps, k, alpha, thr
        self.state = [dict(step=0, m=torch.zeros_like(p), v=torch.zeros_like(p), s=p.clone()) for p in params]

    @torch.no_grad()
    def step(self):
        b1, b2 = self.betas
        for p, st in zip(self.params, self.state):
            g = p.grad
            if g.dim() > 1:
                g.add_(-(g.mean(dim=tuple(range(1, g.dim())), keepdim=True)))
            st["step"] += 1
            t = st["step"]
            st["v"].mul_(b2).addcmul_(g, g, value=1 - b2)
            st["m"].mul_(b1).add_(g, alpha=1 - b1)
            b2t = b2 ** t
            n_max = 2 / (1 - b2) - 1
            n_sma = n_max - 2 * t * b2t / (1 - b2t)
            if self.wd != 0:
                p.add_(p, alpha=-self.wd * self.lr)
            if n_sma > self.thr:
                size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t)
                p.addcdiv_(st["m"], st["v"].sqrt().add_(self.eps), value=-size * self.lr)
            else:
                p.add_(st["m"], alpha=-(1.0 / (1 - b1 ** t)) * self.lr)
            if t % self.k == 0:
                st["s"].add_(p - st["s"], alpha=self.alpha)
                p.copy_(st["s"])


def kernel_us(step, n):
    """Mean device time per step of the lc_ranger kernels over n steps (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile

    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            step()
        torch.cuda.synchronize()
    return sum(e.time_range.elapsed_us() for e in prof.events() if "lc_ranger" in e.name) / n


def bucket_grads(params, seed, offset=0):
    """The gradients as views into one flat buffer packed back to back in parameter order (DDP's gradient_as_bucket_view layout),
    starting `offset` floats in (offset 1: every gradient whose predecessors' sizes are multiples of 4 out of phase)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat = torch.empty(offset + sum(p.numel() for p in params), device="cuda").normal_(generator=g).mul_(1e-3)
    at = offset
    for p in params:
        p.grad = flat[at:at + p.numel()].as_strided(p.shape, p.stride())
        at += p.numel()
    return params


def set_to_none_host_us(params, steps):
    """Host time of step() when every step's gradients are new tensors (the previous ones freed), and the number of table builds."""
    from lc_amd.optim import Ranger

    opt = Ranger(params, lr=2e-4, weight_decay=1e-4)
    host = []
    for i in range(steps):
        for p in params:
            p.grad = torch.empty_like(p).fill_(1e-3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.step()
        host.append(time.perf_counter() - t0)
        opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    host.sort()
    return round(host[len(host) // 2] * 1e6, 1), opt._rebuilds


def bench_set(trunk, width, steps):
    from lc_amd.optim import Ranger

    fused_params = with_grads(model_params(trunk, width), 1)
    opt = Ranger(fused_params, lr=2e-4, weight_decay=1e-4)
    t_fused = timed(opt.step, steps)
    n_fused = launches(opt.step)
    k_fused = kernel_us(opt.step, 12)
    bucket_params = bucket_grads(model_params(trunk, width), 1)
    out_of_phase = sum(1 for p in bucket_params if (p.grad.data_ptr() - p.data_ptr()) % 16)
    bopt = Ranger(bucket_params, lr=2e-4, weight_decay=1e-4)
    t_bucket = timed(bopt.step, steps)
    k_bucket = kernel_us(bopt.step, 12)
    skew_params = bucket_grads(model_params(trunk, width), 1, offset=1)
    skew_out = sum(1 for p in skew_params if (p.grad.data_ptr() - p.data_ptr()) % 16)
    k_skew = kernel_us(Ranger(skew_params, lr=2e-4, weight_decay=1e-4).step, 12)
    loop = PerTensorLoop(with_grads(model_params(trunk, width), 1), 2e-4, 1e-4)
    t_loop = timed(loop.step, max(6, steps // 4))
    n_loop = launches(loop.step)
    host_us, rebuilds = set_to_none_host_us(model_params(trunk, width), 12)
    nbytes = algorithmic_bytes(fused_params)
    return {"trunk": trunk, "width": width, "tensors": len(fused_params), "params": sum(p.numel() for p in fused_params),
            "bytes_per_step": int(nbytes), "fused_kernel_us": round(k_fused, 1), "fused_GBps": round(nbytes / k_fused / 1e3, 1),
            "fused_frac_of_8TBps": round(nbytes / k_fused / 1e-6 / PEAK, 3), "fused_launches": n_fused,
            "fused_step_ms_back_to_back": round(t_fused * 1e3, 4),
            "bucket_grads_out_of_phase": out_of_phase, "bucket_kernel_us": round(k_bucket, 1),
            "bucket_frac_of_8TBps": round(nbytes / k_bucket / 1e-6 / PEAK, 3),
            "skewed_grads_out_of_phase": skew_out, "skewed_kernel_us": round(k_skew, 1), "skewed_frac_of_8TBps": round(nbytes / k_skew / 1e-6 / PEAK, 3), "bucket_step_ms_back_to_back": round(t_bucket * 1e3, 4),
            "set_to_none_host_us_per_step": host_us, "set_to_none_table_builds": rebuilds,
            "per_tensor_loop_ms": round(t_loop * 1e3, 4), "per_tensor_loop_launches": n_loop,
            "per_tensor_loop_over_fused_step": round(t_loop / t_fused, 2)}


def train_median(optim, steps):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_dense_ddp.py"), "--steps", str(steps), "--batch", "32", "--width", "64",
           "--dtype", "bf16", "--optim", optim]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
    return float(re.search(r"median step ([0-9.]+) ms", out).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-steps", type=int, default=40)
    args = ap.parse_args()
    res = {"metric": "ranger_step", "sets": [bench_set(t, 64, args.steps) for t in ("cdpn", "os8")]}
    if args.train:
        res["train_step_median_ms"] = {o: train_median(o, args.train_steps) for o in ("adam", "ranger")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
