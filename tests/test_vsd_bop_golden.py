"""lc_amd.vsd against BOP's own toolkit, when tests/golden/vsd_bop.npz exists (tests/golden/gen_golden_vsd_bop.py; SKIPS until someone with
bop_toolkit_lib runs it): the toolkit's two rendered depth maps and scene depth go to the score -- the oracle on the host, `vsd_from_depth`
on the GPU -- and its errors are demanded back.

The one numerical difference of the definitions is allowed for and counted: BOP rounds the distance images to fp32 before it subtracts,
here the differences stay fp64.  tests/vsd_oracle.flipped_pixels says on how many pixels of a record that decides a visibility or a cost
predicate.  A record without such a pixel must give the stored errors, rounded to fp32, bit for bit.  A record with f of them is an
exception: a flipped pixel moves the numerator cost_k + union - inter and the denominator union by at most one each, so
|e - e_bop| <= 2 f / union is what is demanded of it (union the smaller of the two, at least 1).  Over the whole file the flipped pixels
are capped at 1 in 10^4 of the pixels.

So that none of this can rot while the toolkit is absent, the same check runs here against a stand-in: the generator writing the same file
format from the project's own oracles into a temporary directory -- and against a spoilt copy of it, which the check must refuse."""
import os

import numpy as np
import pytest

from tests import vsd_oracle as orc
from tests.golden import gen_golden_vsd_bop as gen

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", gen.FILE)
REASON = f"no tests/golden/{gen.FILE} (bop_toolkit_lib not in the build image): parity with BOP's pose_error.vsd unpinned"
CAP = 1e-4  # flipped pixels per pixel, over the file


def _record(z, key):
    r = {name: z[f"{key}/{name}"] for name in gen.FIELDS}
    r["diameter"] = None if np.isnan(r["diameter"]) else np.float32(r["diameter"])
    return r


def _oracle(r, delta):
    return orc.score(r["depth_est"], r["depth_gt"], r["depth_test"], r["K"], delta, r["taus"], r["diameter"]).errors


def _kernel(r, delta):
    import torch

    from lc_amd import vsd

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = vsd.vsd_from_depth(t(r["depth_est"][None]), t(r["depth_gt"][None]), t(r["depth_test"]), t(r["K"]), delta=delta, taus=[float(x) for x in r["taus"]],
                             diameter=None if r["diameter"] is None else t(np.asarray([r["diameter"]], np.float32)))
    return out.errors[0].cpu().numpy()


def check(path, scorer):
    """-> (records, exceptions, flipped pixels, pixels).  Raises AssertionError on a record that misses what the module docstring demands."""
    z = np.load(path)
    delta = float(z["delta"])
    keys = [key for key, _, _ in gen.records()]
    assert all(f"{key}/{name}" in z for key in keys for name in gen.FIELDS), "the file does not hold the case list's records"
    exceptions = flipped = pixels = 0
    for key in keys:
        r = _record(z, key)
        got = scorer(r, delta)
        want = r["errors"]
        assert got.dtype == np.float32 and got.shape == want.shape == r["taus"].shape, key
        f = orc.flipped_pixels(r["depth_est"], r["depth_gt"], r["depth_test"], r["K"], delta, r["taus"], r["diameter"])
        pixels += r["depth_est"].size
        flipped += f
        if f == 0:
            assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32)), (str(z["source"]), key, got.tolist(), want.tolist())
        else:
            exceptions += 1
            ours = orc.score(r["depth_est"], r["depth_gt"], r["depth_test"], r["K"], delta, r["taus"], r["diameter"])
            theirs = orc.score(r["depth_est"], r["depth_gt"], r["depth_test"], r["K"], delta, r["taus"], r["diameter"], dist_dtype=np.float32)
            union = max(1, min(int(ours.counts[0]), int(theirs.counts[0])))
            assert (np.abs(got.astype(np.float64) - want) <= 2.0 * f / union + 2.0 ** -24).all(), (str(z["source"]), key, f, union, got.tolist(), want.tolist())
    print(f"{z['source']}: {len(keys)} records, {exceptions} exceptions, {flipped} flipped pixels of {pixels}")
    assert flipped <= CAP * pixels, (flipped, pixels)
    return len(keys), exceptions, flipped, pixels


@pytest.mark.skipif(not os.path.exists(PATH), reason=REASON)
def test_oracle_equals_bop_errors():
    check(PATH, _oracle)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(PATH), reason=REASON)
def test_kernel_equals_bop_errors():
    check(PATH, _kernel)


@pytest.fixture(scope="module")
def stand_in(tmp_path_factory):
    return gen.main(str(tmp_path_factory.mktemp("vsd_bop")), use_stand_in=True)


def test_the_check_against_a_stand_in(stand_in, tmp_path):
    """File format, record list, the exception count and the cap, with the oracle in the kernel's place; a spoilt file is refused."""
    z = np.load(stand_in)
    assert str(z["source"]).startswith("stand-in") and os.path.getsize(stand_in) < 1 << 20
    n, exceptions, flipped, pixels = check(stand_in, _oracle)
    assert n == len(gen.records()) >= 15 and pixels >= 15 * 20 * 45 and exceptions <= n
    assert any(np.isnan(z[f"{key}/diameter"]) for key, _, _ in gen.records()) and all(c.K[0, 1] == 0 for _, c, _ in gen.records())
    # one error of one graded record moved by a single pixel of its union: refused
    store = dict(z)
    key = next(k for k, c, r in gen.records() if r.expect is None)
    ref = _record(z, key)
    union = int(orc.score(ref["depth_est"], ref["depth_gt"], ref["depth_test"], ref["K"], float(z["delta"]), ref["taus"], ref["diameter"]).counts[0])
    store[f"{key}/errors"] = ref["errors"] + np.eye(1, len(ref["errors"]), 0)[0] / union
    spoilt = os.path.join(tmp_path, gen.FILE)
    np.savez_compressed(spoilt, **store)
    with pytest.raises(AssertionError):
        check(spoilt, _oracle)


def test_fp32_rounding_of_the_distances_can_decide_a_pixel():
    """The counter counts.  A 1 x 64 map, the scene at depth 1, the estimate at fp32(1 + delta / n) -- delta behind the scene along each
    pixel's ray to within the rounding of its own depth.  The fp64 differences fall on either side of delta by some 1e-8; the distances
    rounded to fp32 first (steps of 1.2e-7) settle many of these pixels the other way."""
    K = np.array([[100, 0, 0], [0, 100, 0], [0, 0, 1]], dtype=np.float32)
    n = orc.ray_length(K, (1, 64))
    test, gt, delta = np.ones((1, 64), np.float32), np.zeros((1, 64), np.float32), np.float32(0.25)
    est = (1 + 0.25 / n).astype(np.float32)
    a = orc.score(est, gt, test, K, delta, (0.1,))
    b = orc.score(est, gt, test, K, delta, (0.1,), dist_dtype=np.float32)
    f = orc.flipped_pixels(est, gt, test, K, delta, (0.1,))
    assert f == int((a.vis_est != b.vis_est).sum()) and 8 <= f <= 56
    assert 0 < int(a.vis_est.sum()) < 64  # the fp64 definition itself tells these pixels apart
    assert orc.flipped_pixels(est + np.float32(0.01), gt, test, K, delta, (0.1,)) == 0  # a centimetre clear of delta: nothing to decide


@pytest.mark.gpu
def test_the_kernel_against_a_stand_in(stand_in):
    n, exceptions, flipped, pixels = check(stand_in, _kernel)
    assert n == len(gen.records())
