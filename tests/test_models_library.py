"""What the main library's registries check, for liblc_amd_models.so (no GPU needed): every compiled kernel form is named in
tests/launch_forms_models.py with the GPU tests that launch it and every entry still names a form and existing tests
(tests/test_launch_forms.py does this for liblc_amd.so only); the kernels' registers, LDS and scratch (tests/test_kernel_resources.py);
and the shared loader's refusals for this target (tests/test_host_logic.py runs them over every name of `build.TARGETS`)."""
import ast
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from tests.launch_forms_models import FORMS  # noqa: E402


@pytest.fixture(scope="module")
def res():
    from kernel_resources import kernel_resources
    from lc_amd import build, models

    models.load()  # builds the library if the sources changed
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    return kernel_resources(build.MODELS.so_path)


def test_every_kernel_form_has_exactly_one_entry_and_every_entry_a_form(res):
    symbols = sorted(res)
    assert len(symbols) == 4, symbols  # a new kernel or template instance changes this count and needs its entry below
    for s in symbols:
        assert len([rx for rx, _ in FORMS if re.search(rx + r"(?:E|I)", s)]) == 1, s
    for rx, tests in FORMS:
        assert tests and any(re.search(rx + r"(?:E|I)", s) for s in symbols), rx


def test_every_named_test_exists():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_models.py")).read())
    defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for rx, tests in FORMS:
        for t in tests:
            mod, _, fn = t.partition("::")
            assert mod == "test_gpu_models" and fn in defined, (rx, t)


def test_kernels_do_not_spill_and_fit_their_workgroups(res):
    def find(part):
        hits = [d for n, d in res.items() if part in n]
        assert hits, part
        return hits

    # 1024-thread workgroups: four waves per SIMD share its 512 registers, so 128 per thread is the limit of a launch at all
    for d in find("lc_model_points_kernel"):
        assert d.get("private_segment_fixed_size", 0) == 0 and d["vgpr_count"] <= 128 and d.get("agpr_count", 0) == 0, d
        assert d.get("group_segment_fixed_size", 0) <= 1024 and d["max_flat_workgroup_size"] == 1024, d
    # the pair walk is VALU-bound: many resident waves, a 4 KB tile per workgroup
    for d in find("lc_model_diameter_kernel"):
        assert d.get("private_segment_fixed_size", 0) == 0 and d["waves_per_simd_by_registers"] >= 8 and d.get("group_segment_fixed_size", 0) <= 8 * 1024, d
    for d in find("lc_model_diameter_reduce_kernel"):
        assert d.get("private_segment_fixed_size", 0) == 0 and d["waves_per_simd_by_registers"] >= 8, d


def test_shared_loader_refuses_what_it_cannot_rebuild(tmp_path, monkeypatch):
    from lc_amd import _lib, build

    target = build.MODELS._replace(so_path=str(tmp_path / "lib_models.so"))
    monkeypatch.setattr(build, "hipcc_available", lambda: False)
    monkeypatch.setattr(build, "build", lambda *a, **k: pytest.fail("the loader must not try to build here"))
    monkeypatch.delenv("LC_AMD_ALLOW_STALE", raising=False)
    with pytest.raises(RuntimeError) as e:
        _lib.load_target(target, {}, build_if_missing=False)
    assert str(e.value) == f"lc_amd: {target.so_path} is missing or stale; run `python __graft_entry__.py build`"
    open(target.so_path, "wb").write(b"\x7fELF no marker in here")
    for build_if_missing in (True, False):
        with pytest.raises(RuntimeError) as e:
            _lib.load_target(target, {}, build_if_missing=build_if_missing)
        msg = str(e.value)
        assert msg.startswith(f"lc_amd: {target.so_path} was built from other sources than the ones next to it (embedded hash None, "
                              f"sources {build.source_hash(build.MODELS)}) and hipcc is not available")
    assert not any(build.source_hash(t) in msg for t in build.TARGETS if t is not build.MODELS)


def test_source_hash_covers_the_shared_cross_lane_header():
    from lc_amd import build

    deps = build._deps(build.MODELS)
    assert build.SHARED_H in deps and os.path.join(ROOT, "include", "lc_amd_models.h") in deps
