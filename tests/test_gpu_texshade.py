"""The textured shading pass (`lc_amd.texture`) on the device against tests/texshade_oracle.py on the cases of tests/texshade_cases.py: with
the ORACLE's face and instance maps uploaded the bytes and `info` are EQUAL -- no tolerance, no excluded pixel -- and misses and refused
pixels keep the sentinel; the device's mip chains equal the oracle's; meshes without a texture and constant textures equal `lc_amd.shade`
on the device; batch order and single-row calls change nothing; `render_color` is captured in one graph without parallel branches and
replayed under another pose and light."""
import functools

import numpy as np
import pytest
import torch

from tests import texshade_cases as cases
from tests import texshade_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


def _appearance(c, images=None, tex_index=None, colors=None, levels=None, uvs=None):
    from lc_amd import render, texture

    b = c.base
    ms = render.MeshSet([(v, f) for v, f, _, _ in b.meshes], DEV)
    store = texture.TextureStore.from_images(list(c.images if images is None else images), DEV, levels=levels)
    ap = texture.TexturedAppearance(ms, list(c.uvs if uvs is None else uvs), c.tex_index if tex_index is None else tex_index, store,
                                    [m[3] for m in b.meshes] if colors is None else colors, [m[2] for m in b.meshes])
    return ms, ap


@functools.lru_cache(maxsize=None)
def _set(name):
    return _appearance(cases.build(name))


def _rows(c, rows=None):
    b, rows = c.base, slice(None) if rows is None else rows
    return dict(mesh_index=_dev(b.mesh_index[rows]), R=_dev(b.R[rows]), t=_dev(b.t[rows]), K=_dev(b.K[rows])), dict(light=_dev(b.light[rows]), phong=_dev(b.phong[rows]))


def _shade(name, flip=False, lod=True, rows=None, objects=None, wrap=None):
    from lc_amd import texture

    c = cases.build(name)
    b = c.base
    ms, ap = _set(name) if objects is None else objects
    sel = slice(None) if rows is None else rows
    pose, lit = _rows(c, rows)
    out = _dev(cases.sentinel((len(b.face), *b.size_hw, 3))[sel])
    info = torch.full((out.shape[0],), 77, dtype=torch.int32, device=DEV)
    wrap = _dev(cases._wrap(c, flip)[sel] if wrap is None else wrap, torch.int32)
    got = texture.shade(ms, ap, _dev(b.face[sel]), pose["mesh_index"], pose["R"], pose["t"], pose["K"], **lit, wrap=wrap, lod=lod, out=out, info=info)
    assert got is out
    return out.cpu().numpy(), info.cpu().numpy()


def _shade_scene(name, flip=False, lod=True):
    from lc_amd import texture

    c = cases.build(name)
    b, sc = c.base, c.base.scene
    ms, ap = _set(name)
    pose, lit = _rows(c)
    frames = _dev(cases.sentinel((sc.S, *sc.frame_hw, 3)))
    info = torch.full((len(b.face),), 77, dtype=torch.int32, device=DEV)
    got = texture.shade_scene(ms, ap, frames, _dev(sc.instance), _dev(b.face), pose["mesh_index"], _dev(sc.scene_index), pose["R"], pose["t"], pose["K"], **lit,
                              wrap=_dev(cases._wrap(c, flip), torch.int32), lod=lod, origin_xy=None if sc.origin_xy is None else _dev(sc.origin_xy), info=info)
    assert got is frames
    return frames.cpu().numpy(), info.cpu().numpy()


def _equal(name, out, info, ref):
    diff = np.nonzero((out != ref.out).any(-1))
    print(f"\n{name}: {int(ref.hit.sum())} hit pixels, {len(diff[0])} differ, info {info.tolist()}", end="")
    assert np.array_equal(out, ref.out), (name, [(i, out[i].tolist(), ref.out[i].tolist(), ref.pre[i].tolist()) for i in zip(*(d[:5] for d in diff))])
    assert np.array_equal(out[~ref.hit], cases.sentinel(out.shape)[~ref.hit]) and np.array_equal(info, ref.info), (name, info, ref.info)


@pytest.mark.parametrize("name,level", [("quad8", 0), ("quad4", 1), ("quad2", 2)])
def test_the_hand_written_quads_show_the_texture_s_levels_with_v_flipped(name, level):
    out, info = _shade(name)
    assert np.array_equal(out[0], oracle.mip_chain(cases.TEX8)[level][::-1]) and info.tolist() == [0]
    if level:  # without lod the 8 x 8 level is sampled between its texels: not the smaller level's bytes
        flat, _ = _shade(name, lod=False)
        _equal(name, flat, info, cases.reference(name, False, False)[0])
        assert not np.array_equal(flat, out)


@pytest.mark.parametrize("lod", [True, False])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_bytes_the_misses_and_info_equal_the_oracle_s(name, flip, lod):
    ref, _ = cases.reference(name, flip, lod)
    _equal(name, *_shade(name, flip, lod), ref)
    if cases.build(name).base.scene is not None:
        _equal(name + " (scene form)", *_shade_scene(name, flip, lod), cases.scene_reference(name, flip, lod))


def test_the_cases_reach_three_levels_both_wraps_a_seam_and_coordinates_outside_the_unit_square():
    _, level = cases.reference("levels")
    assert len(np.unique(level[level >= 0])) >= 3  # rho2 crosses several thresholds inside one image
    c = cases.build("b3-40x48")
    _, level = cases.reference("b3-40x48")
    assert len(np.unique(level[level >= 0])) >= 3 and (level == -1).any()
    uv = c.uvs[1]
    assert uv.min() < -1.4 and uv.max() > 2.4 and set(c.wrap.tolist()) == {0, 1}
    faces = c.base.meshes[1][1]
    by_vertex = {}
    for f in range(len(faces)):
        for k in range(3):
            by_vertex.setdefault(int(faces[f, k]), set()).add(tuple(uv[f, k]))
    assert all(len(s) > 1 for s in by_vertex.values())  # every shared vertex carries different coordinates in its faces: seams
    a, b = cases.reference("b3-40x48", False)[0], cases.reference("b3-40x48", True)[0]
    assert not np.array_equal(a.out[0], b.out[0]) and not np.array_equal(a.out[1], b.out[1]) and np.array_equal(a.out[2], b.out[2])  # wrap matters, but to a texture
    assert {(1, 1), (5, 67), (40, 48)} <= set(cases.SIZES) and any(h > 16 and w > 16 and h % 16 and w % 16 for h, w in cases.SIZES)  # several 16 x 16 tiles, none whole


@pytest.mark.parametrize("name", ["b3-40x48", "quad8", "levels"])
def test_the_device_s_mip_chain_equals_the_oracle_s(name):
    c = cases.build(name)
    _, ap = _set(name)
    texels, table = oracle.store(c.images)
    assert np.array_equal(ap.textures.table.cpu().numpy(), table) and np.array_equal(ap.textures.table_host, table)
    assert np.array_equal(ap.textures.texels.cpu().numpy(), texels)
    for k, im in enumerate(c.images):
        chain = oracle.mip_chain(im)
        assert int(table[k, 3]) == len(chain) and chain[-1].shape[:2] == (1, 1)
        for L, lev in enumerate(chain):
            assert np.array_equal(ap.textures.level(k, L).cpu().numpy(), lev), (k, L)


def test_odd_sizes_a_capped_chain_and_a_large_texture_build_the_oracle_s_levels():
    from lc_amd import texture

    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (2, 2), (3, 5), (7, 1), (301, 517))]  # the last: more than one workgroup per level
    for levels in (None, 1, 3):
        store = texture.TextureStore.from_images(images, DEV, levels=levels)
        texels, table = oracle.store(images, levels)
        assert np.array_equal(store.table_host, table) and np.array_equal(store.texels.cpu().numpy(), texels), levels
    assert table[:, 3].tolist() == [1, 2, 3, 3, 3] and oracle.store(images)[1][:, 3].tolist() == [1, 2, 3, 3, 10]


def test_every_refused_row_keeps_the_background_and_says_minus_one():
    c = cases.build("b3-40x48")
    ref, _ = cases.reference("b3-40x48")
    bg = cases.sentinel(ref.out.shape)
    assert bg.min() > 0  # a non-zero background

    def run(edit, wrap=None):
        objects = _appearance(c)
        edit(objects[1])
        return _shade("b3-40x48", objects=objects, wrap=wrap)

    def rows_refused(out, info, refused):
        for b in range(3):
            assert np.array_equal(out[b], bg[b] if b in refused else ref.out[b]) and info[b] == (-1 if b in refused else ref.info[b]), b

    # tex_index outside [-1, n_tex): 2 = n_tex for the box, -2 for the icosphere
    rows_refused(*run(lambda ap: ap.tex_index.copy_(_dev([2, 1, -1], torch.int32))), {0})
    rows_refused(*run(lambda ap: ap.tex_index.copy_(_dev([0, -2, -1], torch.int32))), {1})
    # a table entry that reaches outside the buffer: one level too many for the last texture, an offset behind the end, a negative one, a size of 0
    n = int(_set("b3-40x48")[1].textures.total_texels)
    for entry in ((n - 64 * 32, 64, 32, 7), (n, 64, 32, 1), (-1, 64, 32, 1), (0, 0, 32, 1), (0, 64, 32, 0), (0, 64, 32, 16), (0, 16385, 1, 1)):
        def edit(ap, entry=entry):
            ap.textures.table[1] = _dev(entry, torch.int64)
        rows_refused(*run(edit), {1})
    rows_refused(*run(lambda ap: None, wrap=[0, 2, -1]), {1, 2})  # wrap is 0 or 1, also for a mesh without a texture
    # an unknown mesh, as lc_amd.shade refuses it
    from lc_amd import texture

    ms, ap = _set("b3-40x48")
    pose, lit = _rows(c)
    out, info = _dev(bg), torch.zeros(3, dtype=torch.int32, device=DEV)
    texture.shade(ms, ap, _dev(c.base.face), _dev([0, 3, -1], torch.int32), pose["R"], pose["t"], pose["K"], **lit, wrap=_dev(c.wrap, torch.int32), out=out, info=info)
    rows_refused(out.cpu().numpy(), info.cpu().numpy(), {1, 2})


def test_every_refused_pixel_keeps_the_background_and_says_one():
    for name in ("bad-uv", "planted-face"):
        c = cases.build(name)
        ref, _ = cases.reference(name)
        refused = (c.base.face != -1) & ~ref.hit
        out, info = _shade(name)
        assert refused.sum() >= 3 and ref.info.tolist() == [1] and info.tolist() == [1], name
        assert np.array_equal(out[refused], cases.sentinel(out.shape)[refused]) and cases.sentinel(out.shape)[refused].min() > 0 and np.array_equal(out, ref.out), name
    ref = cases.scene_reference("scene-planted")
    frames, info = _shade_scene("scene-planted")
    assert ref.info.tolist() == [1, 1, 0, 0] and info.tolist() == [1, 1, 0, 0] and np.array_equal(frames, ref.out)  # a window pixel off the maps, a row of the other scene
    planted = [(1, 47, 63), (0, 47, 0), (0, 0, 0), (0, 0, 1)]
    assert all(np.array_equal(frames[p], cases.sentinel(frames.shape)[p]) for p in planted)


@pytest.mark.parametrize("name", ["b3-40x48", "scene"])
def test_without_textures_and_with_constant_textures_the_bytes_are_lc_amd_shade_s(name):
    from lc_amd import shade

    c = cases.build(name)
    b = c.base
    pose, lit = _rows(c)
    bg = _dev(cases.sentinel((len(b.face), *b.size_hw, 3)))
    ms, plain = _appearance(c, tex_index=np.full(len(b.meshes), -1, np.int32))
    vertex = shade.Appearance(ms, [m[3] for m in b.meshes], [m[2] for m in b.meshes])
    want = shade.shade(ms, vertex, _dev(b.face), pose["mesh_index"], pose["R"], pose["t"], pose["K"], **lit, out=bg.clone())
    got, info = _shade(name, objects=(ms, plain))
    assert np.array_equal(got, want.cpu().numpy()) and not info.any()
    # one colour per mesh, on every vertex and in its whole texture: any coordinates, either wrap, any level give that colour
    tints = [(201, 17, 96), (3, 250, 128), (77, 77, 78)][:len(b.meshes)]
    ms, const = _appearance(c, images=[np.full((5, 9, 3), t, np.uint8) for t in tints], tex_index=np.arange(len(b.meshes), dtype=np.int32),
                            colors=[np.full((len(m[0]), 3), t, np.uint8) for m, t in zip(b.meshes, tints)],
                            uvs=[cases.corner_uvs(len(m[1]), 7) if u is None else u for m, u in zip(b.meshes, c.uvs)])
    vertex = shade.Appearance(ms, [np.full((len(m[0]), 3), t, np.uint8) for m, t in zip(b.meshes, tints)], [m[2] for m in b.meshes])
    want = shade.shade(ms, vertex, _dev(b.face), pose["mesh_index"], pose["R"], pose["t"], pose["K"], **lit, out=bg.clone()).cpu().numpy()
    for flip in (False, True):
        for lod in (True, False):
            got, info = _shade(name, flip, lod, objects=(ms, const))
            assert np.array_equal(got, want) and not info.any(), (flip, lod)


def test_batch_order_and_single_row_calls_give_the_same_bytes():
    whole, info = _shade("b3-40x48")
    order = [2, 1, 0]
    out, oinfo = _shade("b3-40x48", rows=order)
    assert np.array_equal(out, whole[order]) and np.array_equal(oinfo, info[order])  # (every row over its own sentinel)
    for b in range(len(whole)):
        one, i1 = _shade("b3-40x48", rows=[b])
        assert np.array_equal(one[0], whole[b]) and i1.tolist() == [int(info[b])], b


def _graph_shape(graph):
    """(edges as (from, to) node handles, node count) of a captured graph that was kept (`CUDAGraph(keep_graph=True)`), from the HIP runtime."""
    import ctypes

    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)  # the runtime torch has loaded
    hip = ctypes.CDLL(path)
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    g, n, nodes = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(n)) == 0 and hip.hipGraphGetNodes(g, None, ctypes.byref(nodes)) == 0
    src, dst = (ctypes.c_void_p * n.value)(), (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(n)) == 0
    return list(zip(src, dst)), nodes.value


def test_render_color_in_one_captured_graph_follows_its_pose_and_light_tensors():
    from lc_amd import texture

    c = cases.build("b3-40x48")
    b = c.base
    ms, ap = _set("b3-40x48")
    pose, lit = _rows(c)
    R, t, light, wrap = pose["R"].clone(), pose["t"].clone(), lit["light"].clone(), _dev(c.wrap, torch.int32)
    bg = _dev(cases.sentinel((3, *b.size_hw, 3)))
    kw = dict(near=b.near, far=b.far, phong=lit["phong"], wrap=wrap, background=bg)

    def run():
        return texture.render_color(ms, ap, pose["mesh_index"], R, t, pose["K"], b.size_hw, light=light, **kw)[0]

    first = run().clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph(keep_graph=True)  # kept, so that its nodes and edges can be read below
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = run()
    newR = _dev(np.stack([cases.render_cases.rot((0.2, 1, 0.4), 20.0 + 30 * k) @ b.R[k] for k in range(3)]).astype(np.float32))
    newt, newl = pose["t"] + torch.tensor([0.01, -0.005, 0.03], device=DEV), torch.tensor([[-0.2, 0.3, 0.05]], device=DEV).expand(3, 3).contiguous()
    R.copy_(newR), t.copy_(newt), light.copy_(newl)
    graph.replay()
    torch.cuda.synchronize()
    eager = texture.render_color(ms, ap, pose["mesh_index"], newR, newt, pose["K"], b.size_hw, light=newl, **kw)[0]
    assert torch.equal(out, eager) and not torch.equal(out, first) and (out != bg).any()
    # the graph is a chain: no node has two successors or two predecessors, and one edge fewer than nodes
    edges, nodes = _graph_shape(graph)
    assert nodes >= 4 and len(edges) == nodes - 1, (nodes, edges)  # the rasteriser's nodes, the canvas, info's memset, the shading launch
    for side in (0, 1):
        ends = [e[side] for e in edges]
        assert len(set(ends)) == len(ends), ("a fork" if side == 0 else "a join", edges)
    # end to end off the rasteriser's tie pixels: the oracle on the oracle's own face map
    first = first.cpu().numpy()
    ref, _ = cases.reference("b3-40x48")
    ties = cases.shade_cases.tie_masks(b)
    assert ties.sum() < 0.1 * ref.hit.sum() and np.array_equal(first[~ties], ref.out[~ties])


def test_render_scene_equals_the_oracle_off_the_tie_pixels_and_b_zero_launches_nothing():
    from lc_amd import texture

    full = cases.shade_cases.build("scene-full")
    c = cases.build("scene")._replace(base=full)
    sc = full.scene
    ms, ap = _appearance(c)
    pose, lit = _rows(c)
    frames, scene = texture.render_scene(ms, ap, pose["mesh_index"], _dev(sc.scene_index), pose["R"], pose["t"], _dev(cases.shade_cases.FRAME_K), sc.frame_hw, sc.S,
                                         near=full.near, far=full.far, **lit, wrap=_dev(c.wrap, torch.int32), lod=True)
    ref = cases.shade_scene(c)
    want = ref.out.copy()
    want[~ref.hit] = 0  # over zeros, not over the sentinel
    ties = cases.shade_cases.scene_tie_mask(full)
    assert np.array_equal(frames.cpu().numpy()[~ties], want[~ties]) and np.array_equal(scene.instance.cpu().numpy()[~ties], sc.instance[~ties])
    e = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    out = texture.shade(ms, ap, torch.zeros(0, 16, 16, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), e(0, 3, 3), e(0, 3), e(0, 3, 3),
                        light=texture.DEFAULT_LIGHT, phong=texture.DEFAULT_PHONG)
    assert tuple(out.shape) == (0, 16, 16, 3)
