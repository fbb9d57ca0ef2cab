"""tests/render_oracle.py (the fp64 statement the GPU tests check the rasteriser against) against analytic answers, its invariance under
the order of the faces, and, for every case the GPU tests use, the two conditions they rely on.  No GPU needed."""
import numpy as np
import pytest

from tests import render_cases as rc
from tests import render_oracle as ro

EYE = np.eye(3, dtype=np.float32)


def test_sphere_depth_at_the_centre_pixel():
    """The ray through the centre of pixel (32,32) is the optical axis: it meets a sphere of radius r at distance d in z = d - r; a
    3-subdivision icosphere's faces lie inside the sphere by at most r (1 - cos(half the largest face angle)) < 0.6 % of r."""
    v, f = rc.icosphere(3, 0.1)
    K = np.array([[100, 0, 32.5], [0, 100, 32.5], [0, 0, 1]], dtype=np.float32)
    ref = ro.render(v, f, rc.rot((1, 2, 3), 11.0), np.array([0, 0, 0.5], dtype=np.float32), K, (65, 65), rc.NEAR, rc.FAR)
    assert ref.mask[32, 32] and 0.4 <= ref.z64[32, 32] <= 0.4 + 0.006 * 0.1
    assert ref.depth[32, 32] == np.float32(ref.z64[32, 32])
    # the silhouette is the circle of radius f r / sqrt(d^2 - r^2) = 20.41 px: its area within the polygon's 1 % and a pixel ring
    assert abs(ref.mask.sum() - np.pi * 20.41 ** 2) <= 0.01 * np.pi * 20.41 ** 2 + 2 * np.pi * 20.41


def test_fronto_parallel_quad_constant_z_and_exact_count():
    """A quad at z = 0.5 whose corners project to (10.25, 8.25) and (40.25, 30.25): the samples x + 0.5 in [10.25, 40.25] are x = 10..39,
    y + 0.5 in [8.25, 30.25] are y = 8..29 -- 30 x 22 pixels, all at the plane's z, the diagonal's pixels hit once."""
    K = np.array([[128, 0, 0], [0, 128, 0], [0, 0, 1]], dtype=np.float32)
    u = np.array([[10.25, 8.25], [40.25, 8.25], [40.25, 30.25], [10.25, 30.25]])
    v = np.concatenate((u / 128 * 0.5, np.full((4, 1), 0.5)), -1).astype(np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    ref = ro.render(v, f, EYE, np.zeros(3, dtype=np.float32), K, (48, 64), rc.NEAR, rc.FAR)
    assert ref.mask.sum() == 30 * 22 and ref.mask[8:30, 10:40].all()
    assert (ref.depth[ref.mask] == np.float32(0.5)).all() and (ref.z64[ref.mask] == 0.5).all()
    assert ref.info == 0 and set(np.unique(ref.face)) == {-1, 0, 1}
    # a sample exactly on an edge is covered: corners on sample points, the quad then spans x = 10..40 inclusive
    v2 = np.concatenate((np.array([[10.5, 8.5], [40.5, 8.5], [40.5, 30.5], [10.5, 30.5]]) / 128 * 0.5, np.full((4, 1), 0.5)), -1).astype(np.float32)
    assert ro.render(v2, f, EYE, np.zeros(3, dtype=np.float32), K, (48, 64), rc.NEAR, rc.FAR).mask.sum() == 31 * 23
    # zero-area faces cover nothing; faces behind the near plane are dropped whole and counted
    assert ro.render(v2, np.array([[0, 1, 1], [0, 0, 0]]), EYE, np.zeros(3, dtype=np.float32), K, (48, 64), rc.NEAR, rc.FAR).mask.sum() == 0
    v3 = v2.copy()
    v3[3, 2] = 0.005
    r3 = ro.render(v3, f, EYE, np.zeros(3, dtype=np.float32), K, (48, 64), rc.NEAR, rc.FAR)
    assert r3.info == 1 and set(np.unique(r3.face)) == {-1, 0}
    # far: nothing beyond it
    assert ro.render(v2, f, EYE, np.zeros(3, dtype=np.float32), K, (48, 64), rc.NEAR, 0.4).mask.sum() == 0


@pytest.mark.parametrize("mesh", ["torus", "ico", "fan", "near"])
def test_invariant_under_a_permutation_of_the_faces(mesh):
    c = next(c for c in rc.CASES if c.name == f"{mesh}-64x64")
    v, f = rc.MESHES[mesh]
    perm = np.random.default_rng(5).permutation(len(f))
    a = rc.reference(c.name)
    b = ro.render(v, f[perm], c.pose.R, c.pose.t, c.K, c.size_hw, rc.NEAR, rc.FAR)
    assert np.array_equal(a.depth.view(np.uint32), b.depth.view(np.uint32)) and np.array_equal(a.mask, b.mask) and a.info == b.info
    exact_tie = a.mask & (a.second.astype(np.float32) == a.depth)
    back = np.where(b.face >= 0, perm[np.maximum(b.face, 0)], -1)
    assert np.array_equal(back[~exact_tie], a.face[~exact_tie])


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_cases_meet_the_conditions_of_the_gpu_test(name):
    """(a) no projected vertex coordinate within 2^-30 px of a snapping boundary (the kernel's fp64 may differ from numpy's in the last
    bits: contracted multiply-adds); (b) at most 5 % of an image's covered pixels are tie pixels."""
    ref = rc.reference(name)
    assert ref.margin >= 2.0 ** -30
    n = int(ref.mask.sum())
    ties = int(ro.tie_pixels(ref, ro.z_tolerance(ref)).sum())
    assert ties <= 0.05 * n
    if "out-of-view" in name:
        assert n == 0 and ref.info == 0
    else:
        assert n >= 15
    if name.startswith("near-"):
        assert ref.info == 3
    if name.startswith("box-"):  # the large faces: tiles in which one face alone wins more than 64 samples (the whole-wave path)
        H, W = ref.mask.shape
        big = sum(int(np.bincount(ref.face[y:y + 32, x:x + 32][ref.mask[y:y + 32, x:x + 32]], minlength=1).max(initial=0) > 64)
                  for y in range(0, H, 32) for x in range(0, W, 32))
        assert big >= 2


def test_reader_pin_against_the_reference_loader():
    """tests/golden/render_reader_48x64.npz (gen_golden_render.py): a record this project's encoder wrote, as the unmodified reference's
    `_get_homo_with_depth(..., fill_hole=False)` read it.  The oracle + encode reproduces the record, and decode reproduces the loader's
    homo_z and mask: z to the quantisation step against the oracle, (u + 0.5, v + 0.5, 1) z bit for bit against the loader."""
    import os

    import torch

    from lc_amd.render import decode_z_info, encode_z_info

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_reader_48x64.npz"))
    size = tuple(int(x) for x in g["size_hw"])
    ref = ro.render(g["verts"], g["faces"], g["R"], g["t"], g["K"], size, float(g["near"]), float(g["far"]))
    z_info = encode_z_info(torch.from_numpy(ref.depth))
    assert np.array_equal(z_info["z_crop"], g["z_crop"]) and list(z_info["xyxy"]) == g["xyxy"].tolist()
    assert np.float32(z_info["z_max"]) == g["z_max"] and np.float32(z_info["z_min"]) == g["z_min"]
    depth, mask = decode_z_info(z_info, size)
    assert np.array_equal(mask, g["ref_msk_full"] > 0) and np.array_equal(mask, ref.mask)
    assert np.array_equal(depth, g["ref_homo_z"][..., 2])
    xs, ys = np.meshgrid(np.arange(size[1]) + 0.5, np.arange(size[0]) + 0.5)
    homo = (np.stack((xs, ys, np.ones_like(xs)), -1) * depth[..., None]).astype(np.float32)  # dataset.py:307: fp64 product, stored as fp32
    assert np.array_equal(homo, g["ref_homo_z"])
    step = (float(g["z_max"]) - float(g["z_min"])) / 65534
    assert np.abs(depth.astype(np.float64) - 1000 * ref.z64)[mask].max() <= 0.5 * step + 1000 * ref.z64.max() * 8 * 2.0 ** -24
