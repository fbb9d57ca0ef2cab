"""The label-preparation kernels (lc_labels.hip) use no scratch memory (read from the code object with scripts/kernel_resources.py; no GPU
needed): a spill to scratch would make the streaming pass several times slower without any functional test noticing."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_label_kernels_do_not_spill():
    from lc_amd import _lib
    from kernel_resources import kernel_resources

    _lib.load()
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    res = kernel_resources()
    for part, count in (("lc_sym_select_kernel", 5), ("lc_label_targets_kernel", 3)):
        hits = [d for n, d in res.items() if part in n]
        assert len(hits) == count, (part, len(hits))
        for d in hits:
            assert d.get("private_segment_fixed_size", 0) == 0, (d["name"], "scratch")
            assert d["vgpr_count"] <= 512, d["name"]
