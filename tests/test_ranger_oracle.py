"""The Ranger restatement of tests/ranger_oracle.py against the unmodified reference's own trajectory (tests/golden/ranger_golden.npz):
in float32 it follows the reference to a few units in the last place, and in float64 it stays within the reference's float32 round-off."""
import os

import numpy as np
import pytest
import torch

import tests.ranger_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ranger_golden.npz")
KEYS = ("p", "grad") + ro.STATE_KEYS


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _snapshots(dtype):
    snaps = {}

    def keep(t, params, grads, o):
        for i, p in enumerate(params):
            st = o.state[id(p)]
            snaps[t, i] = dict(p=p.clone(), grad=grads[i].clone(), step=st["step"], **{k: st[k].clone() for k in ro.STATE_KEYS})

    ro.run_golden(dtype, on_snapshot=keep)
    return snaps


def test_float32_restatement_follows_the_reference(golden):
    for (t, i), s in _snapshots(torch.float32).items():
        assert int(golden[f"s{t}_t{i}_step"]) == s["step"]
        for k in KEYS:
            ref = torch.from_numpy(golden[f"s{t}_t{i}_{k}"])
            ulp = torch.finfo(torch.float32).eps * ref.abs().max().item()
            assert (s[k] - ref).abs().max().item() <= 4 * ulp, (t, i, k)


def test_float64_oracle_within_the_references_round_off(golden):
    for (t, i), s in _snapshots(torch.float64).items():
        assert int(golden[f"s{t}_t{i}_step"]) == s["step"]
        for k in KEYS:
            ref = torch.from_numpy(golden[f"s{t}_t{i}_{k}"]).double()
            assert (s[k] - ref).abs().max().item() <= 1e-5 * max(ref.abs().max().item(), 1e-6), (t, i, k)


def test_the_case_crosses_both_branches_and_two_lookahead_syncs(golden):
    o = ro.Oracle(ro.golden_groups(ro.initial_params()))
    assert o.scalars(5, 0.95, 0.999)[0] <= 5 < o.scalars(6, 0.95, 0.999)[0]
    # tensor 3 missed two steps: its count lags, so its Lookahead syncs fall on other steps than the others'
    assert int(golden["s13_t0_step"]) == 13 and int(golden["s13_t3_step"]) == 11
    assert np.array_equal(golden["s12_t0_p"], golden["s12_t0_slow_buffer"]) and not np.array_equal(golden["s12_t3_p"], golden["s12_t3_slow_buffer"])
