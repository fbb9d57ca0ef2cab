"""The Ranger optimizer (`lib/optim/ranger.py` of the reference: RAdam + Lookahead + gradient centralisation) with its whole step in one
HIP launch (lc_amd/csrc/optim/lc_ranger.hip, lc_amd/_C/liblc_amd_optim.so, C ABI in include/lc_amd_optim.h).

    Ranger(params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
           gc_conv_only=False)

Same constructor, defaults, `param_groups` keys and `state` keys (`step` a Python int, `exp_avg`, `exp_avg_sq`, `slow_buffer`) as the
reference, so checkpoints load in both directions.  The step scalars (N_sma, step_size, the RAdam branch, the Lookahead step) are
computed on the host in Python floats exactly as the reference computes them, including its `radam_buffer` cache keyed by `step % 10`
alone across groups.  A step uploads them in one small host-to-device copy and issues one launch (two when a centralised tensor has
rows longer than LC_RANGER_ONE_PASS_ROW); it never waits for the device.  The device table of tensor pointers is rebuilt only when the
set of tensors with a gradient, or their storage, changes.

float32 parameters on a HIP device only; anything else raises (there is no CPU fallback).  `lc_amd.dropin.install(native_optim=True)`
puts this class in place of the reference's.
"""
from __future__ import annotations

import math
from ctypes import c_int, c_void_p

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import _lib
from . import build as _build

BLOCK_ELEMS = 8192  # include/lc_amd_optim.h: LC_RANGER_BLOCK_ELEMS
ONE_PASS_ROW = 8192  # LC_RANGER_ONE_PASS_ROW
BLOCK_ROWS = 1024  # LC_RANGER_BLOCK_ROWS
WEIGHT_DECAY, ADAPTIVE, LOOKAHEAD, GRAD_IN_PHASE = 1, 2, 4, 8

SCALARS = np.dtype([("beta1", "<f4"), ("one_minus_beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta2", "<f4"), ("neg_wd_lr", "<f4"),
                    ("neg_step_lr", "<f4"), ("eps", "<f4"), ("alpha", "<f4"), ("flags", "<i4"), ("pad", "<i4"), ("grad", "<u8")])
TENSOR = np.dtype([("p", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("slow", "<u8"), ("numel", "<i8"), ("row", "<i4"),
                   ("mean_off", "<i4"), ("phase", "<i4"), ("pad", "<i4")])
BLOCK = np.dtype([("tensor", "<i4"), ("n", "<i4"), ("e0", "<i8")])
assert SCALARS.itemsize == 48 and TENSOR.itemsize == 56 and BLOCK.itemsize == 16

_SO = _lib.SideLibrary(_build.OPTIM, {"lc_ranger_step_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p])})
_SIGNATURES, load = _SO.signatures, _SO.load


def _dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense: the elements fill [data_ptr, data_ptr + numel) exactly, in some order of the dimensions."""
    expect = 1
    for stride, size in sorted((s, z) for s, z in zip(t.stride(), t.shape) if z != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def _same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and all(x == y for x, y, z in zip(a.stride(), b.stride(), a.shape) if z != 1)


class Ranger(Optimizer):
    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
                 gc_conv_only=False):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.radam_buffer = [[None, None, None] for _ in range(10)]
        self.use_gc = use_gc
        self.gc_gradient_threshold = 3 if gc_conv_only else 1
        self._key = None  # what the device table was built for

    def _active(self):
        """(param, state, group, where) of every parameter with a gradient, in the reference's order; states initialised as the
        reference initialises them."""
        out = []
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                where = f"param_groups[{gi}]['params'][{pi}] (shape {tuple(p.shape)})"
                if g.is_sparse:
                    raise RuntimeError(f"lc_amd.optim.Ranger: {where} has a sparse gradient; Ranger does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p.data)
                    state["exp_avg_sq"] = torch.zeros_like(p.data)
                    state["slow_buffer"] = torch.empty_like(p.data)
                    state["slow_buffer"].copy_(p.data)
                out.append((p, state, group, where))
        return out

    def _scalars(self, active, staged=None):
        """Advance every active tensor's step and compute its step scalars as lib/optim/ranger.py:143-196 does, radam_buffer included;
        with each row this step's gradient pointer.  A gradient whose strides differ from its parameter's is copied into the parameter's
        layout first and listed in `staged` as (gradient, copy) (the centred copy goes back after the launch)."""
        rows = []
        for p, state, group, _ in active:
            state["step"] += 1
            step = state["step"]
            beta1, beta2 = group["betas"]
            buffered = self.radam_buffer[int(step % 10)]
            if step == buffered[0]:
                N_sma, step_size = buffered[1], buffered[2]
            else:
                buffered[0] = step
                beta2_t = beta2 ** step
                N_sma_max = 2 / (1 - beta2) - 1
                N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
                buffered[1] = N_sma
                if N_sma > self.N_sma_threshhold:
                    step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (
                        1 - beta1 ** step)
                else:
                    step_size = 1.0 / (1 - beta1 ** step)
                buffered[2] = step_size
            wd, lr = group["weight_decay"], group["lr"]
            flags = (WEIGHT_DECAY if wd != 0 else 0) | (ADAPTIVE if N_sma > self.N_sma_threshhold else 0) | (LOOKAHEAD if step % group["k"] == 0 else 0)
            if p.numel():
                g = p.grad
                if g.stride() != p.stride() and not _same_layout(g, p):
                    tmp = torch.empty_like(p.data).copy_(g)
                    if staged is not None:
                        staged.append((g, tmp))
                    g = tmp
                gp = g.data_ptr()
                flags |= GRAD_IN_PHASE if (gp - p.data_ptr()) % 16 == 0 else 0
                rows.append((beta1, 1 - beta1, beta2, 1 - beta2, -wd * lr, -step_size * lr, group["eps"], self.alpha, flags, 0, gp))
        return np.array(rows, dtype=SCALARS)

    def _layout_key(self, active):
        """What the static part of the table depends on: the parameters with a gradient and their state tensors (not the gradients,
        whose pointers go with the per-step scalars: a loop that frees its gradients every step keeps the table)."""
        key = [self.gc_gradient_threshold]
        for p, state, _, _ in active:
            if p.numel():
                key += (p.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), state["slow_buffer"].data_ptr())
        return tuple(key)

    def _rebuild(self, active):
        """Check every tensor, re-lay state tensors whose strides differ from their parameter's, and build the static part of the table."""
        device = None
        descs, blocks, rowsum = [], [], []
        n_means = 0
        held = []
        for p, state, group, where in active:
            g = p.grad
            if not p.is_cuda:
                raise RuntimeError(f"lc_amd.optim.Ranger: {where} is on {p.device}; the fused step needs parameters on the MI355X "
                                   f"(there is no CPU fallback)")
            if p.dtype != torch.float32 or g.dtype != torch.float32:
                raise TypeError(f"lc_amd.optim.Ranger: {where} must be float32 with a float32 gradient, got {p.dtype} / {g.dtype}")
            if device is None:
                device = p.device
            elif p.device != device:
                raise RuntimeError(f"lc_amd.optim.Ranger: {where} is on {p.device}, other parameters on {device}; one device per optimizer")
            if g.device != p.device:
                raise RuntimeError(f"lc_amd.optim.Ranger: the gradient of {where} is on {g.device}, the parameter on {p.device}")
            if p.numel() == 0:
                continue
            if not _dense(p):
                raise RuntimeError(f"lc_amd.optim.Ranger: {where} is not dense in memory (strides {p.stride()})")
            if p.data_ptr() % 4:
                raise RuntimeError(f"lc_amd.optim.Ranger: {where} is not 4-byte aligned")
            # State tensors of another layout (a contiguous checkpoint over channels_last parameters) are re-laid here, once; a
            # gradient of another layout than its parameter's is copied into it for each step and the centred copy written back.
            for name in ("exp_avg", "exp_avg_sq", "slow_buffer"):
                t = state[name]
                if t.device != p.device or t.dtype != p.dtype or not _same_layout(t, p):
                    state[name] = torch.empty_like(p.data).copy_(t)  # the parameter's strides; same values
            m, v, s = state["exp_avg"], state["exp_avg_sq"], state["slow_buffer"]
            numel = p.numel()
            row = numel // p.shape[0] if g.dim() > self.gc_gradient_threshold else 0
            if row and p.shape[0] > 1 and p.stride(0) != row:
                raise RuntimeError(f"lc_amd.optim.Ranger: the dim-0 rows of {where} are not contiguous (strides {p.stride()})")
            ti = len(descs)
            ptrs = [t.data_ptr() for t in (p, m, v, s)]
            phase = sum(bit for bit, a in zip((1, 2, 4), ptrs[1:]) if (a - ptrs[0]) % 16 == 0)
            mean_off = -1
            if row > ONE_PASS_ROW:
                mean_off = n_means
                nrows = numel // row
                rowsum.append(np.stack([np.full(nrows, ti), np.full(nrows, row), np.arange(nrows)], 1))
                n_means += nrows
            descs.append((*ptrs, numel, row, mean_off, phase, 0))
            if row and row <= ONE_PASS_ROW:
                per = min(BLOCK_ELEMS // row, BLOCK_ROWS)
                r0 = np.arange(0, numel // row, per)
                blocks.append(np.stack([np.full(len(r0), ti), np.minimum(per, numel // row - r0) * row, r0 * row], 1))
            else:
                e0 = np.arange(0, numel, BLOCK_ELEMS)
                blocks.append(np.stack([np.full(len(e0), ti), np.minimum(BLOCK_ELEMS, numel - e0), e0], 1))
            held += [p, m, v, s]
        table_blocks = np.concatenate(rowsum + blocks) if blocks else np.zeros((0, 3), np.int64)
        blk = np.zeros(len(table_blocks), dtype=BLOCK)
        if len(table_blocks):
            blk["tensor"], blk["n"], blk["e0"] = table_blocks[:, 0], table_blocks[:, 1], table_blocks[:, 2]
        self._ntensors = len(descs)
        self._nrowsum = sum(len(r) for r in rowsum)
        self._nupdate = len(blk) - self._nrowsum
        self._static = np.array(descs, dtype=TENSOR).tobytes() + blk.tobytes()
        self._device = device
        self._held = held  # parameters and state tensors only: gradients are not kept alive past the step
        self._rebuilds = getattr(self, "_rebuilds", 0) + 1
        if self._ntensors:
            self._table = torch.empty(self._ntensors * SCALARS.itemsize + len(self._static), dtype=torch.uint8, device=device)
            self._means = torch.empty(max(n_means, 1), dtype=torch.float32, device=device)
        self._key = self._layout_key(active)

    @torch.no_grad()
    def step(self, closure=None):
        active = self._active()
        if not active:
            return None
        rebuild = self._layout_key(active) != getattr(self, "_key", None)
        if rebuild:
            self._rebuild(active)  # raises before any step advances
        lib = load()
        staged = []
        scal = self._scalars(active, staged)
        if not self._ntensors:
            return None
        payload = scal.tobytes() + self._static if rebuild else scal.tobytes()
        host = torch.frombuffer(bytearray(payload), dtype=torch.uint8).pin_memory()
        with _lib.on_device(self._device):
            self._table[:len(payload)].copy_(host, non_blocking=True)
            rc = lib.lc_ranger_step_f32(c_void_p(self._table.data_ptr()), self._ntensors, self._nrowsum, self._nupdate,
                                        c_void_p(self._means.data_ptr()), _lib.stream_ptr(self._device))
            if rc != 0:
                _SO.fail("optim.Ranger.step", rc)
            for g, tmp in staged:
                g.copy_(tmp)
        return None
