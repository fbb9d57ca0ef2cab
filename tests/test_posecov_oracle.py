"""tests/posecov_oracle.py (the closed-form fp64 statement the GPU tests check the kernel against) against the unmodified reference's own
results stored in tests/golden/posecov_*.npz: cov, var, perr to fp64 round-off, the zero / non-zero pattern of info exactly."""
import os

import numpy as np
import pytest
import torch

from tests import posecov_oracle as po
from tests.golden import gen_golden_posecov as gen


@pytest.mark.parametrize("name", po.CASES)
def test_oracle_reproduces_the_references_float64_results(name):
    d = po.load_fixture(name)
    args, kw = po.fixture_call(d)
    got = po.pose_covariance(*args, **kw)
    rows = torch.from_numpy(d["well_posed"] | (d["f64_info"] != 0))  # (rank-deficient rows: the SPD verdict is a rounding accident)
    assert torch.equal(got.info[rows] != 0, torch.from_numpy(d["f64_info"] != 0)[rows])
    # 1e-12: both sides are fp64 evaluations of the same sums in different orders, through a 6x6 inverse of condition ~1e6
    for key, g in (("cov", got.cov), ("var", got.var), ("perr", got.pred_err[:, None])):
        ref = torch.from_numpy(d[f"f64_{key}"]).reshape(g.shape)
        assert float(po.row_error(g, ref)[rows].max()) < 1e-12, key
    fallback = got.info != 0
    assert torch.equal(got.cov[fallback], torch.eye(6, dtype=torch.float64).expand(int(fallback.sum()), 6, 6))


@pytest.mark.parametrize("name", po.CASES)
def test_float32_evaluation_is_as_close_as_the_references_own(name):
    """The oracle's fp32 evaluation stands in for the reference's fp32 run at sizes without a fixture: where a fixture exists, its distance
    from the fp64 results is of the size of the reference's own (within a factor 4 either way, or below the 4 x 2^-24 floor)."""
    d = po.load_fixture(name)
    args, kw = po.fixture_call(d)
    got = po.pose_covariance(*args, **kw, dtype=torch.float32)
    rows = torch.from_numpy(d["well_posed"] & (d["f32_info"] == 0))
    assert not got.info[rows].any()
    ours = po.row_error(got.cov, torch.from_numpy(d["f64_cov"]))[rows]
    theirs = po.row_error(torch.from_numpy(d["f32_cov"]), torch.from_numpy(d["f64_cov"]))[rows]
    assert bool((ours <= (4 * theirs).clamp_min(po.FLOOR)).all()), (ours, theirs)


def test_fixture_inputs_are_the_generators_seeded_cases():
    """The committed inputs, options and well-posed marks are the generator's own (seeded) cases, bit for bit."""
    for name, (c, opts, well) in gen.cases().items():
        d = po.load_fixture(name)
        for k, v in c.items():
            assert (v is None and f"in_{k}" not in d) or np.array_equal(d[f"in_{k}"], v.numpy(), equal_nan=True), (name, k)
        assert {k[4:]: bool(v) for k, v in d.items() if k.startswith("opt_")} == opts and d["well_posed"].tolist() == [bool(w) for w in well]
        assert d["f64_cov"].dtype == np.float64 and d["f32_cov"].dtype == np.float32


def test_generator_reproduces_the_stored_results_from_a_reference_checkout():
    """With a reference checkout at LC_REFERENCE the generator's evaluation of the unmodified reference is run again and compared with what
    the fixtures store (skipped where there is none)."""
    ref = os.environ.get("LC_REFERENCE", "")
    if not (ref and os.path.isdir(os.path.join(ref, "lib", "nll"))):
        pytest.skip("no reference checkout at LC_REFERENCE")
    for name, d in gen.generate(ref).items():
        stored = po.load_fixture(name)
        for k, v in d.items():
            if k.startswith("f64_"):
                np.testing.assert_allclose(stored[k], v, rtol=1e-9, atol=0, equal_nan=True)
