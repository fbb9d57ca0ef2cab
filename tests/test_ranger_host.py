"""The fused Ranger without a GPU: the host-side step scalars and Lookahead timing against the reference's golden trajectory, the
state_dict layout against the reference's, the argument checks of lc_ranger_step_f32, the drop-in's opt-in rebinding, and a registry of
the kernels in liblc_amd_optim.so (each one named by a GPU test that launches it; none uses scratch memory)."""
import ast
import json
import os
import sys

import numpy as np
import pytest
import torch

import tests.ranger_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# kernel symbol fragment -> tests of tests/test_gpu_ranger.py that launch it
KERNELS = {
    "lc_ranger_update_kernel": ["test_golden_trajectory_within_twice_the_references_error", "test_sweep_of_model_shapes_against_the_oracle"],
    "lc_ranger_row_mean_kernel": ["test_sweep_of_model_shapes_against_the_oracle"],
}


def _golden_opt():
    from lc_amd.optim import Ranger

    params = ro.initial_params()
    groups = []
    for spec in ro.GROUPS:
        g = dict(params=[params[i] for i in spec["idx"]], lr=spec["lr"], weight_decay=spec["weight_decay"])
        if "betas" in spec:
            g["betas"] = spec["betas"]
        groups.append(g)
    return params, Ranger(groups)


def test_step_scalars_and_lookahead_follow_the_golden_trajectory():
    """The host half of a step (_scalars) on the golden case: per-tensor step counts and the Lookahead flags match where the reference
    synced (p == slow_buffer right after a sync), and the scalars equal the float64 restatement's (radam_buffer quirk included)."""
    gold = dict(np.load(os.path.join(GOLDEN, "ranger_golden.npz")))
    params, opt = _golden_opt()
    o = ro.Oracle(ro.golden_groups(params))
    for t in range(1, ro.STEPS + 1):
        for grp, spec in zip(opt.param_groups, ro.GROUPS):
            grp["lr"] = ro.lr_at(spec, t)
        for i, p in enumerate(params):
            p.grad = ro.grad_at(i, t)
        active = opt._active()
        rows = opt._scalars(active)
        assert len(rows) == len(active)
        for row, (p, state, group, _) in zip(rows, active):
            beta1, beta2 = group["betas"]
            n_sma, size = o.scalars(state["step"], beta1, beta2)
            assert row["neg_step_lr"] == np.float32(-size * group["lr"])
            assert bool(row["flags"] & 2) == (n_sma > 5)
            assert bool(row["flags"] & 1) == (group["weight_decay"] != 0)
            assert bool(row["flags"] & 4) == (state["step"] % 6 == 0)
            assert row["one_minus_beta2"] == np.float32(1 - beta2) and row["alpha"] == np.float32(0.5)
        if t in ro.SNAPSHOTS:
            for i, p in enumerate(params):
                st = opt.state[p]
                assert st["step"] == int(gold[f"s{t}_t{i}_step"])
                synced = st["step"] % 6 == 0
                assert synced == np.array_equal(gold[f"s{t}_t{i}_p"], gold[f"s{t}_t{i}_slow_buffer"]), (t, i)


def test_radam_cache_is_shared_across_groups_by_step_alone():
    params, opt = _golden_opt()
    for i, p in enumerate(params):
        p.grad = ro.grad_at(i, 1)
    rows = opt._scalars(opt._active())
    # tensor 4 (other betas) reuses the entry tensor 0 wrote for step 1: same step size per unit lr
    assert rows[4]["neg_step_lr"] / np.float32(-ro.lr_at(ro.GROUPS[2], 0)) == pytest.approx(1 / (1 - 0.95), rel=1e-6)


def test_state_dict_layout_matches_the_reference():
    layout = json.load(open(os.path.join(GOLDEN, "ranger_state_dict.json")))
    params, opt = _golden_opt()
    for t in range(1, ro.STEPS + 1):
        for grp, spec in zip(opt.param_groups, ro.GROUPS):
            grp["lr"] = ro.lr_at(spec, t)
        for i, p in enumerate(params):
            p.grad = ro.grad_at(i, t)
        opt._scalars(opt._active())  # the host half of every step (the device half needs the GPU)
    sd = opt.state_dict()
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in layout["param_groups"]]
    for ours, ref in zip(sd["param_groups"], layout["param_groups"]):
        for k, v in ref.items():
            assert (list(ours[k]) if isinstance(ours[k], tuple) else ours[k]) == pytest.approx(v), k
    assert sorted(sd["state"]) == sorted(int(i) for i in layout["state"])
    for i, st in sd["state"].items():
        ref = layout["state"][str(i)]
        assert sorted(st) == sorted(ref)
        assert type(st["step"]).__name__ == ref["step"]["type"] == "int" and st["step"] == ref["step"]["value"]
        for k in ro.STATE_KEYS:
            assert ref[k]["type"] == "tensor" and list(st[k].shape) == ref[k]["shape"] and str(st[k].dtype) == ref[k]["dtype"]


def test_constructor_matches_the_reference():
    from lc_amd.optim import Ranger

    p = torch.zeros(2, 2, requires_grad=True)
    opt = Ranger([p])
    assert opt.defaults == dict(lr=1e-3, alpha=0.5, k=6, step_counter=0, betas=(0.95, 0.999), N_sma_threshhold=5, eps=1e-5, weight_decay=0)
    assert (opt.alpha, opt.k, opt.N_sma_threshhold, opt.gc_gradient_threshold, opt.use_gc) == (0.5, 6, 5, 1, True)
    assert Ranger([p], gc_conv_only=True).gc_gradient_threshold == 3
    for bad in (dict(alpha=1.5), dict(k=0), dict(lr=0), dict(eps=0)):
        with pytest.raises(ValueError):
            Ranger([p], **bad)


def test_cpu_parameters_raise_and_nothing_advances():
    from lc_amd.optim import Ranger

    p = torch.zeros(3, 4, requires_grad=True)
    p.grad = torch.ones(3, 4)
    opt = Ranger([p])
    with pytest.raises(RuntimeError, match=r"param_groups\[0\]\['params'\]\[0\].*no CPU fallback"):
        opt.step()
    assert opt.state[p]["step"] == 0
    p.grad = p.grad.to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()


def test_step_entry_point_checks_its_arguments():
    from lc_amd import optim

    lib = optim.load()
    assert lib.lc_ranger_step_f32(None, 1, 0, 0, None, None) == 0  # nothing to update: no launch
    assert lib.lc_ranger_step_f32(None, 1, 0, 3, None, None) != 0 and b"table" in lib.lc_amd_optim_last_error()
    buf = torch.zeros(256, dtype=torch.uint8)
    assert lib.lc_ranger_step_f32(buf.data_ptr(), 1, 2, 3, None, None) != 0 and b"row_means" in lib.lc_amd_optim_last_error()
    assert lib.lc_ranger_step_f32(buf.data_ptr(), 1, -1, 3, None, None) != 0
    assert lib.lc_amd_optim_source_hash().decode() == __import__("lc_amd.build", fromlist=["x"]).source_hash(optim._build.OPTIM)


def test_main_library_is_untouched_by_the_optim_sources():
    from lc_amd import build

    assert not any("optim" in s for s in build.sources()) and build.sources(build.OPTIM) == [os.path.join(build.CSRC, "optim", "lc_ranger.hip")]
    assert build.source_hash() != build.source_hash(build.OPTIM)


@pytest.fixture
def stand_in_reference(monkeypatch, tmp_path):
    """The two modules of a reference checkout the rebinding touches: lib/optim/ranger.py defining Ranger, utils.py importing the name."""
    (tmp_path / "lib" / "optim").mkdir(parents=True)
    (tmp_path / "lib" / "optim" / "ranger.py").write_text("class Ranger:\n    pass\n")
    (tmp_path / "utils.py").write_text("from lib.optim.ranger import Ranger\n")
    monkeypatch.setattr(sys, "path", [str(tmp_path)] + list(sys.path))
    for name in ("utils", "lib", "lib.optim", "lib.optim.ranger"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    before = dict(sys.modules)
    yield tmp_path
    for name in set(sys.modules) - set(before):  # install() registers modules under the reference's names: none of them outlive the test
        del sys.modules[name]
    sys.modules.update(before)


def test_dropin_rebinds_the_references_ranger_on_request(stand_in_reference):
    import importlib

    from lc_amd import dropin, optim

    utils = importlib.import_module("utils")
    ref = importlib.import_module("lib.optim.ranger")
    orig = ref.Ranger
    done = dropin.install(patch_ptnet=False, gpu_initialiser=False)
    assert "optim" not in done and ref.Ranger is orig and utils.Ranger is orig
    done = dropin.install(patch_ptnet=False, gpu_initialiser=False, native_optim=True)
    assert done["optim"] is True and ref.Ranger is optim.Ranger and utils.Ranger is optim.Ranger


def test_dropin_flags_in_either_order(monkeypatch, tmp_path):
    from lc_amd import dropin

    seen = []
    monkeypatch.setattr(dropin, "install", lambda **kw: seen.append(kw) or {})
    monkeypatch.setattr(dropin.runpy, "run_path", lambda *a, **k: None)
    script = str(tmp_path / "train.py")
    for argv in (["--native-optim", "--native-labels", script], ["--native-labels", "--native-optim", script], ["--native-optim", script], [script]):
        monkeypatch.setattr(sys, "argv", list(sys.argv))
        dropin.main(argv)
    assert seen == [dict(native_labels=True, native_optim=True)] * 2 + [dict(native_labels=False, native_optim=True), dict(native_labels=False)]


def test_every_optim_kernel_is_launched_by_a_named_gpu_test_and_none_spills():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import optim

    optim.load()
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_ranger.py")).read())
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    res = kernel_resources(optim._build.OPTIM.so_path)
    assert res
    for name, d in res.items():
        hits = [frag for frag in KERNELS if frag in name]
        assert len(hits) == 1, name
        assert all(t in tests for t in KERNELS[hits[0]]), hits
        assert d.get("private_segment_fixed_size", 0) == 0, (name, "scratch")
