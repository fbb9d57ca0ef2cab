"""Every compiled kernel form of liblc_amd.so is named in tests/launch_forms.py, either with the GPU tests that launch it or with the reason
no test can; every entry of that table still names a form of the library and every test it names exists (no GPU needed: the symbols are
read from the code object, as scripts/kernel_resources.py reads them).  A new template instance cannot land without a test that names it."""
import ast
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from tests.launch_forms import FORMS, UNREACHABLE  # noqa: E402


@pytest.fixture(scope="module")
def symbols():
    from lc_amd import _lib
    from kernel_resources import kernel_resources

    _lib.load()  # builds the library if the sources changed
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    return sorted(kernel_resources())


def _entries():
    return [(rx, tuple(tests)) for rx, tests in FORMS] + [(rx, None) for rx in UNREACHABLE]


def test_every_kernel_symbol_has_an_entry(symbols):
    loose = [s for s in symbols if not any(re.search(rx, s) for rx, _ in _entries())]
    assert not loose, "kernel forms without a test in tests/launch_forms.py:\n  " + "\n  ".join(loose)


def test_every_entry_names_a_kernel_symbol(symbols):
    stale = [rx for rx, _ in _entries() if not any(re.search(rx, s) for s in symbols)]
    assert not stale, f"entries of tests/launch_forms.py that match no kernel of the library: {stale}"


def test_unreachable_forms_are_not_also_claimed_by_a_test(symbols):
    for rx in UNREACHABLE:
        assert UNREACHABLE[rx].strip(), rx
        claimed = [(s, t) for s in symbols if re.search(rx, s) for frx, t in FORMS if re.search(frx, s)]
        assert not claimed, (rx, claimed)


def test_every_named_test_exists():
    defined = {}
    for path in glob.glob(os.path.join(ROOT, "tests", "test_*.py")):
        mod = os.path.basename(path)[:-3]
        tree = ast.parse(open(path).read())
        defined[mod] = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    missing = []
    for rx, tests in FORMS:
        assert tests, rx
        for t in tests:
            mod, _, fn = t.partition("::")
            if fn not in defined.get(mod, ()):
                missing.append((rx, t))
    assert not missing, missing
