"""The fused Ranger step (lc_amd.optim.Ranger, lc_amd/csrc/optim/lc_ranger.hip) on the device against the float64 restatement of
tests/ranger_oracle.py and the unmodified reference's own float32 trajectory (tests/golden/ranger_golden.npz).

Accuracy bound everywhere: a state tensor's max error against float64 is at most twice the reference's own float32 error (or, where the
reference did not run, the float32 restatement's), plus 2 units in the last place of the tensor's largest value."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests.ranger_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ranger_golden.npz")
KEYS = ("p", "grad") + ro.STATE_KEYS
EPS32 = torch.finfo(torch.float32).eps
DEV = "cuda"


def _within(ours, exact, ref32, what):
    exact = exact.double().cpu()
    err = (ours.double().cpu() - exact).abs().max().item() if exact.numel() else 0.0
    ref_err = (ref32.double().cpu() - exact).abs().max().item() if exact.numel() else 0.0
    bound = 2 * ref_err + 2 * EPS32 * (exact.abs().max().item() if exact.numel() else 0.0)
    assert err <= bound, (what, err, ref_err)


def _golden_oracle():
    snaps = {}

    def keep(t, params, grads, o):
        for i, p in enumerate(params):
            st = o.state[id(p)]
            snaps[t, i] = dict(p=p.clone(), grad=grads[i].clone(), step=st["step"], **{k: st[k].clone() for k in ro.STATE_KEYS})

    ro.run_golden(torch.float64, on_snapshot=keep)
    return snaps


def _golden_groups(params):
    groups = []
    for spec in ro.GROUPS:
        g = dict(params=[params[i] for i in spec["idx"]], lr=spec["lr"], weight_decay=spec["weight_decay"])
        if "betas" in spec:
            g["betas"] = spec["betas"]
        groups.append(g)
    return groups


def _golden_step(opt, params, t):
    for grp, spec in zip(opt.param_groups, ro.GROUPS):
        grp["lr"] = ro.lr_at(spec, t)
    for i, p in enumerate(params):
        g = ro.grad_at(i, t)
        if g is not None:
            g = g.to(DEV)
            g = g.contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g
        p.grad = g


def test_golden_trajectory_within_twice_the_references_error():
    from lc_amd.optim import Ranger

    gold, exact = dict(np.load(GOLDEN)), _golden_oracle()
    params = [p.to(DEV) for p in ro.initial_params()]
    params = [p.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else p for p in params]
    opt = Ranger(_golden_groups(params))
    for t in range(1, ro.STEPS + 1):
        _golden_step(opt, params, t)
        opt.step()
        if t in ro.SNAPSHOTS:
            torch.cuda.synchronize()
            for i, p in enumerate(params):
                st = opt.state[p]
                assert st["step"] == int(gold[f"s{t}_t{i}_step"]) == exact[t, i]["step"]
                ours = dict(p=p, grad=p.grad, **{k: st[k] for k in ro.STATE_KEYS})
                for k in KEYS:
                    _within(ours[k], exact[t, i][k], torch.from_numpy(gold[f"s{t}_t{i}_{k}"]), (t, i, k))


def _sweep_shapes():
    """About 150 tensors: the example models' parameter shapes (ResNet-34 trunk + CDPN decoder at width 64), empty and odd sizes, and
    rows longer than the one-pass limit (8192)."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    for cin, cout, n in ((64, 64, 3), (64, 128, 4), (128, 256, 6), (256, 512, 3)):
        for b in range(n):
            c_in = cin if b == 0 else cout
            shapes += [(cout, c_in, 3, 3), (cout,), (cout,), (cout, cout, 3, 3), (cout,), (cout,)]
            if b == 0 and cin != cout:
                shapes += [(cout, cin, 1, 1), (cout,), (cout,)]
    shapes += [(512, 256, 4, 4), (256,), (256,), (256, 256, 3, 3), (256,), (256,), (5, 256, 1, 1), (5,)]
    for _ in range(8):  # the decoder's upsampling stages
        shapes += [(64, 64, 3, 3), (64,), (64,)]
    shapes += [(0,), (4, 0, 3), (3, 7, 5), (7,), (1, 64), (3, 1), (2, 9000), (3, 2, 4800), (1, 20000), (5, 3), (1,)]
    return shapes


def _sweep_run(steps, seed=0, exact=False, wd=1e-4):
    """(fused params/states/grads, float64 oracle, float32 oracle) after `steps` steps with the example's lr and weight decay."""
    from lc_amd.optim import Ranger

    gen = torch.Generator().manual_seed(seed)
    shapes = _sweep_shapes()
    init = [torch.randn(s, generator=gen) for s in shapes]
    dev = [x.to(DEV) for x in init]
    dev = [x.contiguous(memory_format=torch.channels_last) if x.dim() == 4 else x for x in dev]
    opt = Ranger(dev, lr=2e-4, weight_decay=wd)
    oracles = {}
    if exact:
        for dt in (torch.float64, torch.float32):
            ps = [x.to(dt) for x in init]
            oracles[dt] = (ps, ro.Oracle([dict(params=ps, lr=2e-4, weight_decay=wd, betas=(0.95, 0.999), eps=1e-5, k=6)]))
    grads = None
    for t in range(1, steps + 1):
        grads = [torch.randn(s, generator=gen) * 0.1 + 0.02 for s in shapes]
        for p, g in zip(dev, grads):
            p.grad = g.to(DEV).contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g.to(DEV)
        opt.step()
        for dt, (ps, o) in oracles.items():
            o.step([[g.to(dt) for g in grads]])
    torch.cuda.synchronize()
    return dev, opt, oracles


def test_sweep_of_model_shapes_against_the_oracle():
    from lc_amd import optim

    dev, opt, oracles = _sweep_run(7, exact=True)
    assert len(dev) >= 140
    assert opt._nrowsum > 0  # the two-launch form ran (rows of 9000, 9600 and 20000)
    (p64, o64), (p32, o32) = oracles[torch.float64], oracles[torch.float32]
    for i, p in enumerate(dev):
        st, s64, s32 = opt.state[p], o64.state[id(p64[i])], o32.state[id(p32[i])]
        assert st["step"] == s64["step"] == 7
        _within(p, p64[i], p32[i], (i, tuple(p.shape), "p"))
        for k in ro.STATE_KEYS:
            _within(st[k], s64[k], s32[k], (i, tuple(p.shape), k))
        if p.dim() == 4:
            assert all(st[k].is_contiguous(memory_format=torch.channels_last) for k in ro.STATE_KEYS)
    assert optim.ONE_PASS_ROW == 8192


def test_two_runs_are_bitwise_identical():
    a, oa, _ = _sweep_run(7, seed=3)
    b, ob, _ = _sweep_run(7, seed=3)
    for p, q in zip(a, b):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad)
        for k in ro.STATE_KEYS:
            assert torch.equal(oa.state[p][k], ob.state[q][k])


def _packed(shapes, offset, gap, layouts_like):
    """Views into ONE flat buffer, `offset` floats in and `gap` floats apart (a DDP gradient bucket's packing at odd offsets), each
    with the strides of the matching tensor of `layouts_like`."""
    sizes = [int(np.prod(s)) for s in shapes]
    buf = torch.zeros(offset + sum(sizes) + gap * len(sizes) + 4, device=DEV)
    out, at = [], offset
    for s, n, like in zip(shapes, sizes, layouts_like):
        out.append(buf[at:at + n].as_strided(s, like.stride()))
        at += n + gap
    return out


def test_out_of_phase_views_give_the_same_bits():
    """Parameters and gradients as views into flat buffers at odd float offsets (arrays out of 16-byte phase with each other, and p
    itself unaligned) take the 4-byte access path for the arrays out of phase; the results equal the run on separate allocations bit
    for bit (the row sums do not depend on where a row lies)."""
    from lc_amd.optim import Ranger

    ref, oref, _ = _sweep_run(7, seed=5)
    shapes = _sweep_shapes()
    for p_off, g_off in ((0, 3), (1, 2), (3, 3)):
        gen = torch.Generator().manual_seed(5)
        init = [torch.randn(s, generator=gen) for s in shapes]
        dev = _packed(shapes, p_off, 1, ref)
        for d, x in zip(dev, init):
            d.copy_(x.to(DEV))
        opt = Ranger(dev, lr=2e-4, weight_decay=1e-4)
        gbuf = _packed(shapes, g_off, 2, ref)  # gaps of 1 and 2 floats: the relative phase changes from tensor to tensor
        for t in range(1, 8):
            grads = [torch.randn(s, generator=gen) * 0.1 + 0.02 for s in shapes]
            for p, g, gb in zip(dev, grads, gbuf):
                gb.copy_(g.to(DEV))
                p.grad = gb
            opt.step()
        torch.cuda.synchronize()
        phases = {(p.data_ptr() - p.grad.data_ptr()) % 16 for p in dev if p.numel()}
        assert 0 in phases and len(phases) > 1  # gradients in and out of phase with their parameters
        for p, q in zip(dev, ref):
            assert torch.equal(p, q) and torch.equal(p.grad, q.grad), (p_off, g_off, tuple(p.shape))
            for k in ro.STATE_KEYS:
                assert torch.equal(opt.state[p][k], oref.state[q][k]), (p_off, g_off, tuple(p.shape), k)


def test_a_gradient_laid_out_unlike_its_parameter_is_centred_in_place():
    """A contiguous gradient on a channels_last parameter (the reference accepts it): the same bits as a channels_last gradient, and the
    centred gradient ends up in that same p.grad tensor."""
    from lc_amd.optim import Ranger

    gen = torch.Generator().manual_seed(7)
    x, gs = torch.randn(32, 16, 3, 3, generator=gen), [torch.randn(32, 16, 3, 3, generator=gen) + 0.1 for _ in range(7)]
    runs = []
    for fmt in (torch.channels_last, torch.contiguous_format):
        p = x.to(DEV).contiguous(memory_format=torch.channels_last)
        opt = Ranger([p], lr=2e-4, weight_decay=1e-4)
        for g in gs:
            grad = g.to(DEV).contiguous(memory_format=fmt)
            p.grad = grad
            opt.step()
            assert p.grad is grad
        torch.cuda.synchronize()
        runs.append((p, grad, opt.state[p]))
    (p1, g1, s1), (p2, g2, s2) = runs
    assert g2.is_contiguous() and torch.equal(p1, p2) and torch.equal(g1, g2)
    assert g2.mean(dim=(1, 2, 3)).abs().max().item() < 1e-6
    assert all(torch.equal(s1[k], s2[k]) for k in ro.STATE_KEYS)


def test_a_set_to_none_loop_keeps_its_table_and_frees_old_gradients():
    """The reference's train.py frees the gradients every step (zero_grad(set_to_none=True)): backward then allocates new ones wherever it
    can.  The table is built once, and no gradient outlives its step."""
    import weakref

    from lc_amd.optim import Ranger

    shapes = _sweep_shapes()
    params = [torch.randn(s, device=DEV) for s in shapes]
    opt = Ranger(params, lr=2e-4, weight_decay=1e-4)
    keep = []  # the previous step's gradients stay alive here, so the new ones cannot reuse their addresses
    for _ in range(8):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
        refs = [weakref.ref(p.grad) for p in params]
        keep = [p.grad for p in params]
        opt.zero_grad(set_to_none=True)
        assert all(r() is not None for r in refs)
    del keep
    assert all(r() is None for r in refs)
    assert opt._rebuilds == 1


def test_resume_from_a_reference_layout_checkpoint():
    """The reference's float32 state after step 6 (contiguous tensors, as a reference checkpoint holds them) loaded into the fused class
    over channels_last parameters; six more steps stay within the bound at step 12 and the state tensors take the parameters' layout."""
    from lc_amd.optim import Ranger

    gold, exact = dict(np.load(GOLDEN)), _golden_oracle()
    params = [torch.from_numpy(gold[f"s6_t{i}_p"]).to(DEV) for i in range(len(ro.SHAPES))]
    params = [p.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else p for p in params]
    opt = Ranger(_golden_groups(params))
    sd = opt.state_dict()
    sd["state"] = {i: dict(step=int(gold[f"s6_t{i}_step"]), **{k: torch.from_numpy(gold[f"s6_t{i}_{k}"]) for k in ro.STATE_KEYS})
                   for i in range(len(ro.SHAPES))}
    opt.load_state_dict(sd)
    for t in range(7, 13):
        _golden_step(opt, params, t)
        opt.step()
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        st = opt.state[p]
        assert st["step"] == exact[12, i]["step"] and isinstance(st["step"], int)
        ours = dict(p=p, grad=p.grad, **{k: st[k] for k in ro.STATE_KEYS})
        for k in KEYS:
            _within(ours[k], exact[12, i][k], torch.from_numpy(gold[f"s12_t{i}_{k}"]), ("resumed", i, k))
        if p.dim() == 4:
            assert st["exp_avg"].is_contiguous(memory_format=torch.channels_last)


def test_a_step_is_at_most_two_launches_and_never_synchronises():
    from torch.profiler import ProfilerActivity, profile

    from lc_amd.optim import Ranger

    shapes = _sweep_shapes()
    params = [torch.randn(s, device=DEV) for s in shapes]
    for p in params:
        p.grad = torch.randn_like(p)
    opt = Ranger(params, lr=2e-4, weight_decay=1e-4)
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "lc_ranger" in e.name]
    assert 1 <= len(kernels) <= 2, kernels
    assert not [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "lc_ranger" not in e.name
                and "emcpy" not in e.name and "Memcpy" not in e.name and not e.name.startswith("Optimizer.step")], names
    syncs = [n for n in names if ("Synchronize" in n or n in ("hipMemcpy", "hipMemcpyWithStream", "hipStreamWaitEvent"))
             and n not in ("cudaDeviceSynchronize", "hipDeviceSynchronize")]
    assert not syncs, syncs


def test_unsupported_parameters_raise_naming_the_parameter():
    from lc_amd.optim import Ranger

    p = torch.zeros(4, 4, device=DEV, dtype=torch.float64)
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match=r"param_groups\[0\]\['params'\]\[0\]"):
        Ranger([p]).step()
    q = torch.zeros(8, 4, device=DEV)[:, :2]
    q.grad = torch.zeros(8, 2, device=DEV)
    with pytest.raises(RuntimeError, match="dense"):
        Ranger([q]).step()


def _run_example(tmp, ranks, extra=()):
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dump = str(tmp / f"r{ranks}")
    common = [os.path.join(ROOT, "examples", "train_dense_ddp.py"), "--steps", "7", "--batch", "4", "--width", "16", "--bn-eval",
              "--dtype", "fp32", "--np-seed", "3", "--optim", "ranger", "--dump", dump, *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    if ranks > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
               "--master-port", str(port), *common, "--backend", "gloo", "--share-gpu"]
    else:
        cmd = [sys.executable, *common]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    return [torch.load(f"{dump}.rank{r}.pt") for r in range(ranks)]


def test_example_trains_with_ranger_and_ranks_stay_equal(tmp_path):
    r0, r1 = _run_example(tmp_path, 2)
    for d in (r0, r1):
        assert len(d["losses"]) == 7 and all(v == v and abs(v) < 1e9 for v in d["losses"])
    assert torch.equal(r0["params"], r1["params"])
    assert not torch.equal(r0["params"], r0["params_at_start"])
