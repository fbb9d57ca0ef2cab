"""The zoom-in crops against bytes of the real cv2.warpAffine, when tests/golden/crops_cv2.npz exists
(tests/golden/gen_golden_crops_cv2.py; SKIPS until someone with OpenCV runs it): the oracle on the host, the kernel on the GPU."""
import os

import numpy as np
import pytest

from tests import crops_cases as cc
from tests import crops_oracle as co
from tests.golden.gen_golden_crops_cv2 import keys

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crops_cv2.npz")
REASON = "no tests/golden/crops_cv2.npz (OpenCV not in the build image): bit parity with cv2.warpAffine unpinned"


@pytest.mark.skipif(not os.path.exists(PATH), reason=REASON)
def test_oracle_equals_cv2_bytes():
    z = np.load(PATH)
    bad = [key for key, C, f, name, M, hw, interp in keys() if not np.array_equal(co.warp_one(cc.FRAMES[C][f], M, hw, interp), z[key])]
    assert not bad, (str(z["cv2_version"]), bad)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(PATH), reason=REASON)
def test_kernel_equals_cv2_bytes():
    import torch

    from lc_amd.crops import warp_affine

    z = np.load(PATH)
    bad = []
    for key, C, f, name, M, hw, interp in keys():
        got = warp_affine(torch.from_numpy(cc.FRAMES[C][f:f + 1]).cuda(), torch.from_numpy(M[None]).cuda(), hw, interp=interp, dtype=torch.uint8)
        if not np.array_equal(got[0].permute(1, 2, 0).cpu().numpy(), z[key]):
            bad.append(key)
    assert not bad, (str(z["cv2_version"]), bad)
