"""tests/texshade_oracle.py without a GPU: against bytes written by hand on the exact quads, the mip rule on odd sizes restated with plain
loops, and against tests/shade_oracle.py where the two must agree (no texture; a constant texture)."""
import numpy as np
import pytest

from tests import shade_cases, shade_oracle
from tests import texshade_cases as cases
from tests import texshade_oracle as oracle


def _halve(level):
    """The level behind an even-sized one, written as block sums."""
    H, W = level.shape[:2]
    return ((level.astype(np.int64).reshape(H // 2, 2, W // 2, 2, 3).sum((1, 3)) + 2) >> 2).astype(np.uint8)


@pytest.mark.parametrize("name,level", [("quad8", 0), ("quad4", 1), ("quad2", 2)])
def test_the_exact_quads_give_the_bytes_written_by_hand(name, level):
    # a unit quad at z = 1 on n x n pixels: the sample of pixel (i, j) has U = (i + 1/2) / n and V = (j + 1/2) / n, exactly; with an 8 x 8
    # texture rho2 = (8 / n)^2 = 1, 4, 16, above 2^(2L-1) for L <= 0, 1, 2; at that level tx = i and ty = n - 1 - j: texel (i, n-1-j) itself
    want = cases.TEX8
    for _ in range(level):
        want = _halve(want)
    want = want[::-1]  # v = 0 is the last row of the stored image
    for flip in (False, True):
        ref, lev = cases.reference(name, flip)
        assert ref.hit.all() and (lev == level).all() and ref.info.tolist() == [0]
        assert np.array_equal(ref.out[0], want) and np.array_equal(ref.pre[0], want.astype(np.float64)), name
    flat, lev = cases.reference(name, False, False)
    assert (lev == 0).all() and (level == 0) == np.array_equal(flat.out[0], want)
    if level == 1:  # lod off on 4 x 4 pixels: tx = 2 i + 1/2, the mean of two texels in each direction -- level 1 before its rounding
        T = cases.TEX8.astype(np.float64).reshape(4, 2, 4, 2, 3).sum((1, 3)) / 4.0
        assert np.array_equal(flat.pre[0], T[::-1])


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (7, 1)])
def test_the_mip_rule_on_small_and_odd_images(hw):
    im = cases.image(hw, 100 * hw[0] + hw[1])
    chain = oracle.mip_chain(im)
    assert len(chain) == {(1, 1): 1, (2, 2): 2, (3, 5): 3, (7, 1): 3}[hw] and np.array_equal(chain[0], im) and chain[-1].shape == (1, 1, 3)
    assert [c.shape[:2] for c in chain] == oracle.level_sizes(*hw, len(chain))
    for L in range(1, len(chain)):
        src = chain[L - 1].astype(int)
        Hs, Ws = src.shape[:2]
        assert chain[L].shape[:2] == (max(1, Hs // 2), max(1, Ws // 2))
        for y in range(chain[L].shape[0]):
            for x in range(chain[L].shape[1]):
                x0, x1, y0, y1 = min(2 * x, Ws - 1), min(2 * x + 1, Ws - 1), min(2 * y, Hs - 1), min(2 * y + 1, Hs - 1)
                assert chain[L][y, x].tolist() == ((src[y0, x0] + src[y0, x1] + src[y1, x0] + src[y1, x1] + 2) >> 2).tolist(), (L, y, x)
    assert len(oracle.mip_chain(im, 1)) == 1 and len(oracle.mip_chain(im, 2)) == min(2, len(chain))
    texels, table = oracle.store([im, im[:1]])
    n = sum(h * w for h, w in oracle.level_sizes(*hw, len(chain)))
    assert table.tolist() == [[0, hw[0], hw[1], len(chain)], [n, 1, hw[1], hw[1].bit_length()]] and not texels[:, 3].any()
    assert np.array_equal(texels[:hw[0] * hw[1], :3], im.reshape(-1, 3)) and np.array_equal(texels[n - 1, :3], chain[-1][0, 0])
    assert oracle.entry_ok(table[1], len(texels)) and not oracle.entry_ok(table[1], len(texels) - 1) and not oracle.entry_ok((0, hw[0], hw[1], 16), 10 ** 9)


@pytest.mark.parametrize("name", ["b3-40x48", "scene"])
def test_without_a_texture_and_with_a_constant_one_the_bytes_are_shade_oracle_s(name):
    c = cases.build(name)
    b = c.base
    plain = c.tm._replace(tex_index=np.full(len(b.meshes), -1, np.int32))
    want = shade_cases.shade(b)
    for flip in (False, True):
        got, level = cases.shade(c, flip, tm=plain)
        assert np.array_equal(got.out, want.out) and np.array_equal(got.info, want.info) and np.array_equal(got.pre[got.hit], want.pre[want.hit]) and (level == -1).all()
    tints = [(201, 17, 96), (3, 250, 128), (77, 77, 78)][:len(b.meshes)]
    meshes = [(m[0], m[1], m[2], np.full((len(m[0]), 3), t, np.uint8)) for m, t in zip(b.meshes, tints)]
    want = shade_cases.shade(b._replace(meshes=tuple(meshes)))
    texels, table = oracle.store([np.full((5, 9, 3), t, np.uint8) for t in tints])
    const = c.tm._replace(base=shade_oracle.concat(meshes), tex_index=np.arange(len(meshes), dtype=np.int32), texels=texels, tex_table=table)
    for flip in (False, True):
        for lod in (True, False):
            got, level = cases.shade(c, flip, lod, tm=const)
            assert np.array_equal(got.out, want.out) and np.array_equal(got.hit, want.hit) and (level[got.hit] >= 0).all(), (flip, lod)
            assert np.abs(got.pre[got.hit] - want.pre[want.hit]).max() <= 2.0 ** -40  # the weights sum to 1 within 2^-50
    if b.scene is not None:
        sc = b.scene
        want = shade_cases.shade_scene(b)
        got = oracle.shade_scene(plain, cases.sentinel((sc.S, *sc.frame_hw, 3)), sc.instance, b.face, b.mesh_index, sc.scene_index, b.R, b.t, b.K, b.light, b.phong,
                                 c.wrap, True, sc.origin_xy)
        assert np.array_equal(got.out, want.out) and np.array_equal(got.info, want.info)


def test_the_refusals_of_the_oracle():
    ref, _ = cases.reference("bad-uv")
    c = cases.build("bad-uv")
    seen = np.unique(c.base.face[c.base.face >= 0])
    refused = (c.base.face != -1) & ~ref.hit
    assert ref.info.tolist() == [1] and set(np.unique(c.base.face[refused])) == {seen[0], seen[1], seen[-1]}
    assert np.array_equal(ref.out[refused], cases.sentinel(ref.out.shape)[refused])
    tm = cases.build("b3-40x48").tm
    assert oracle.row_ok(tm, 0, 0) and oracle.row_ok(tm, 2, 1) and not oracle.row_ok(tm, 0, 2) and not oracle.row_ok(tm, 3, 0) and not oracle.row_ok(tm, -1, 0)
    assert not oracle.row_ok(tm._replace(tex_index=np.array([2, 1, -1])), 0, 0) and not oracle.row_ok(tm._replace(tex_index=np.array([-2, 1, -1])), 0, 0)
    assert not oracle.row_ok(tm._replace(texels=tm.texels[:-1]), 1, 0) and oracle.row_ok(tm._replace(texels=tm.texels[:-1]), 0, 0)
