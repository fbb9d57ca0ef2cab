"""The run-length mask store against pycocotools' own strings, areas and boxes, when tests/golden/rle_coco.json exists
(tests/golden/gen_golden_rle_coco.py; SKIPS until someone with pycocotools runs it): the string codec and the oracle on the host, the store
on the GPU.  The same checks run once against a stand-in written by the project's oracle, and must refuse a spoilt copy of it."""
import json
import os

import numpy as np
import pytest

from tests import rle_oracle as oracle
from tests.golden.gen_golden_rle_coco import NAME, keys, main as write_golden

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", NAME)
REASON = f"no tests/golden/{NAME} (pycocotools not in the build image): parity with pycocotools' strings, area and toBbox unpinned"


def host_mismatches(path):
    """Keys whose stored string, area or box the host side does not reproduce -- or whose string it does not read back to the mask."""
    from lc_amd import rle

    z = json.load(open(path))["records"]
    bad = []
    for key, (H, W), m in keys():
        r = z[key]
        canon = oracle.encode(m)
        area, (x0, y0, x1, y1) = oracle.area_box(m)
        box = [x0, y0, x1 - x0 + 1, y1 - y0 + 1] if area else [0, 0, 0, 0]  # pycocotools: four zeros for an empty mask
        ok = rle.counts_to_string(canon) == r["counts"].encode() == oracle.to_string(canon).encode()
        try:
            back = rle.string_to_counts(r["counts"])
            ok = ok and oracle.is_valid(back, H, W) and np.array_equal(oracle.decode(back, H, W), m)
        except ValueError:
            ok = False
        if not (ok and r["area"] == area and r["bbox"] == box):
            bad.append(key)
    return bad


def device_mismatches(path):
    import torch

    from lc_amd import rle

    z = json.load(open(path))["records"]
    ks = keys()
    store = rle.RleStore.from_coco([dict(size=list(hw), counts=z[key]["counts"]) for key, hw, _ in ks], device=torch.device("cuda:0"))
    xywh, area, valid = store.box_xywh(plus_one=True).cpu().tolist(), store.area.cpu().tolist(), store.valid.cpu().tolist()
    bad = []
    for f, (key, hw, m) in enumerate(ks):
        got, info = rle.decode(store, torch.tensor([f], dtype=torch.int32, device=store.device), hw=hw)
        want_box = z[key]["bbox"] if z[key]["area"] else [-1] * 4  # this project's rule for an empty mask
        if valid[f] != 0 or int(info[0]) != 0 or not np.array_equal(got[0].cpu().numpy(), m) or area[f] != z[key]["area"] or xywh[f] != want_box:
            bad.append(key)
    return bad


@pytest.mark.skipif(not os.path.exists(PATH), reason=REASON)
def test_host_side_equals_pycocotools():
    assert not host_mismatches(PATH), json.load(open(PATH))["pycocotools_version"]


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(PATH), reason=REASON)
def test_store_equals_pycocotools():
    assert not device_mismatches(PATH), json.load(open(PATH))["pycocotools_version"]


def _spoil(path, key, field):
    z = json.load(open(path))
    r = z["records"][key]
    if field == "counts":
        r["counts"] = r["counts"][:-1] + chr(ord(r["counts"][-1]) ^ 1)  # the last count one off: the sum no longer fits
    else:
        r[field] = r[field] + 1 if field == "area" else [r[field][0], r[field][1], r[field][2] + 1, r[field][3]]
    json.dump(z, open(path, "w"))


def test_the_check_passes_a_stand_in_and_refuses_a_spoilt_copy(tmp_path):
    path = write_golden(str(tmp_path), stand_in=True)
    assert len(json.load(open(path))["records"]) == len(keys()) == 39
    assert host_mismatches(path) == []
    for key, field in (("64x64-blob", "counts"), ("37x53-corner-br", "area"), ("130x67-long-run", "bbox")):
        write_golden(str(tmp_path), stand_in=True)
        _spoil(path, key, field)
        assert host_mismatches(path) == [key], (key, field)


@pytest.mark.gpu
def test_the_device_check_passes_a_stand_in_and_refuses_a_spoilt_copy(tmp_path):
    path = write_golden(str(tmp_path), stand_in=True)
    assert device_mismatches(path) == []
    for key, field in (("64x64-blob", "counts"), ("37x53-corner-br", "area"), ("130x67-long-run", "bbox")):
        write_golden(str(tmp_path), stand_in=True)
        _spoil(path, key, field)
        assert device_mismatches(path) == [key], (key, field)
