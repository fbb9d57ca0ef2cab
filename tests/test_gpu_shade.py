"""The shading pass (`lc_amd.shade`) on the device against tests/shade_oracle.py on the cases of tests/shade_cases.py: with the ORACLE's face
and instance maps uploaded the bytes are EQUAL, misses keep the sentinel and `info` is equal; the scene form equals the instance form
pasted by the instance map; batch order and single-row calls change nothing; a captured graph relights with its light tensor; end to end,
`render_color` and `render_scene` equal the two oracles off the rasteriser's tie pixels; and the frames go into `warp_affine` as they come."""
import functools

import numpy as np
import pytest
import torch

from tests import shade_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _set(name):
    from lc_amd import render, shade

    c = cases.build(name)
    ms = render.MeshSet([(v, f) for v, f, _, _ in c.meshes], DEV)
    return ms, shade.Appearance(ms, [m[3] for m in c.meshes], [m[2] for m in c.meshes])


def _rows(c, rows=None):
    rows = slice(None) if rows is None else rows
    return dict(mesh_index=_dev(c.mesh_index[rows]), R=_dev(c.R[rows]), t=_dev(c.t[rows]), K=_dev(c.K[rows])), dict(light=_dev(c.light[rows]), phong=_dev(c.phong[rows]))


def _shade(name, rows=None):
    from lc_amd import shade

    c = cases.build(name)
    ms, ap = _set(name)
    sel = slice(None) if rows is None else rows
    pose, lit = _rows(c, rows)
    out = _dev(cases.sentinel((len(c.face), *c.size_hw, 3))[sel])
    info = torch.full((out.shape[0],), 77, dtype=torch.int32, device=DEV)
    got = shade.shade(ms, ap, _dev(c.face[sel]), pose["mesh_index"], pose["R"], pose["t"], pose["K"], **lit, out=out, info=info)
    assert got is out
    return out.cpu().numpy(), info.cpu().numpy()


def _shade_scene(name):
    from lc_amd import shade

    c = cases.build(name)
    sc = c.scene
    ms, ap = _set(name)
    pose, lit = _rows(c)
    frames = _dev(cases.sentinel((sc.S, *sc.frame_hw, 3)))
    info = torch.full((len(c.face),), 77, dtype=torch.int32, device=DEV)
    got = shade.shade_scene(ms, ap, frames, _dev(sc.instance), _dev(c.face), pose["mesh_index"], _dev(sc.scene_index), pose["R"], pose["t"], pose["K"], **lit,
                            origin_xy=None if sc.origin_xy is None else _dev(sc.origin_xy), info=info)
    assert got is frames
    return frames.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_bytes_the_misses_and_info_equal_the_oracle_s(name):
    ref = cases.reference(name)
    out, info = _shade(name)
    diff = np.nonzero((out != ref.out).any(-1))
    print(f"\n{name}: {int(ref.hit.sum())} hit pixels, {len(diff[0])} differ, info {info.tolist()}", end="")
    assert np.array_equal(out, ref.out), (name, [(i, out[i].tolist(), ref.out[i].tolist(), ref.pre[i].tolist()) for i in zip(*(d[:5] for d in diff))])
    assert np.array_equal(out[~ref.hit], cases.sentinel(out.shape)[~ref.hit]) and np.array_equal(info, ref.info)
    if cases.build(name).scene is not None:
        ref = cases.scene_reference(name)
        frames, info = _shade_scene(name)
        assert np.array_equal(frames, ref.out), (name, int((frames != ref.out).any(-1).sum()))
        assert np.array_equal(frames[~ref.hit], cases.sentinel(frames.shape)[~ref.hit]) and np.array_equal(info, ref.info)


@pytest.mark.parametrize("name", ["scene", "scene-full"])
def test_the_scene_form_is_the_instance_form_pasted_by_the_instance_map(name):
    sc = cases.build(name).scene
    rows, _ = _shade(name)
    frames, _ = _shade_scene(name)
    want = cases.sentinel(frames.shape)
    s, Y, X = np.nonzero(sc.instance >= 0)
    b = sc.instance[s, Y, X]
    org = np.zeros((len(rows), 2), np.int64) if sc.origin_xy is None else sc.origin_xy
    want[s, Y, X] = rows[b, Y - org[b, 1], X - org[b, 0]]
    assert np.array_equal(frames, want)


def test_batch_order_and_single_row_calls_give_the_same_bytes():
    whole, info = _shade("batch")
    order = [3, 1, 0, 2]
    out, oinfo = _shade("batch", order)
    assert np.array_equal(out, whole[order]) and np.array_equal(oinfo, info[order])  # (every row over its own sentinel)
    for b in range(len(whole)):
        one, i1 = _shade("batch", [b])
        assert np.array_equal(one[0], whole[b]) and i1.tolist() == [int(info[b])], b


def test_a_captured_graph_relights_with_its_light_tensor():
    from lc_amd import shade

    c = cases.build("ico20")
    ms, ap = _set("ico20")
    pose, lit = _rows(c)
    face, light = _dev(c.face), lit["light"].clone()
    out = torch.zeros(1, *c.size_hw, 3, dtype=torch.uint8, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run():
        shade.shade(ms, ap, face, pose["mesh_index"], pose["R"], pose["t"], pose["K"], light=light, phong=lit["phong"], out=out, info=info)

    run()
    first = out.clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            run()
    new = torch.tensor([[-0.2, 0.3, 0.05]], device=DEV)
    light.copy_(new)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = shade.shade(ms, ap, face, pose["mesh_index"], pose["R"], pose["t"], pose["K"], light=new, phong=lit["phong"])
    want = cases.shade(c._replace(light=new.cpu().numpy()), out=np.zeros((1, *c.size_hw, 3), np.uint8)).out
    assert torch.equal(out, eager) and not torch.equal(out, first) and np.array_equal(out.cpu().numpy(), want) and int(info[0]) == 0


def test_render_color_equals_the_two_oracles_off_the_tie_pixels():
    from lc_amd import shade

    c = cases.build("ico20")
    ms, ap = _set("ico20")
    pose, lit = _rows(c)
    bg = _dev(cases.sentinel((1, *c.size_hw, 3)))
    keep = bg.clone()
    frames, rendered = shade.render_color(ms, ap, pose["mesh_index"], pose["R"], pose["t"], pose["K"], c.size_hw, near=c.near, far=c.far, **lit, background=bg)
    ref, ties = cases.reference("ico20"), cases.tie_masks(c)
    got = frames.cpu().numpy()
    assert torch.equal(bg, keep) and frames.dtype == torch.uint8 and tuple(frames.shape) == (1, *c.size_hw, 3) and frames.is_contiguous()
    assert np.array_equal(got[~ties], ref.out[~ties]) and np.array_equal(rendered.face.cpu().numpy()[~ties], c.face[~ties])
    black, _ = shade.render_color(ms, ap, pose["mesh_index"], pose["R"], pose["t"], pose["K"], c.size_hw, near=c.near, far=c.far, **lit)
    assert np.array_equal(black.cpu().numpy()[ref.hit & ~ties], ref.out[ref.hit & ~ties]) and not black.cpu().numpy()[~ref.hit & ~ties].any()


def test_render_scene_equals_the_oracles_and_feeds_the_crops_and_the_annotations():
    from lc_amd import crops, gtinfo, shade
    from tests import crops_oracle

    c = cases.build("scene-full")
    sc = c.scene
    ms, ap = _set("scene-full")
    pose, lit = _rows(c)
    frames, scene = shade.render_scene(ms, ap, pose["mesh_index"], _dev(sc.scene_index), pose["R"], pose["t"], _dev(cases.FRAME_K), sc.frame_hw, sc.S,
                                       near=c.near, far=c.far, **lit)
    ties = cases.scene_tie_mask(c)
    want = cases.shade_scene(c).out
    want[~cases.scene_reference("scene-full").hit] = 0  # over zeros, not over the sentinel
    got = frames.cpu().numpy()
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (sc.S, *sc.frame_hw, 3) and frames.is_contiguous()
    assert np.array_equal(got[~ties], want[~ties]) and np.array_equal(scene.instance.cpu().numpy()[~ties], sc.instance[~ties])
    assert np.array_equal(scene.depth.cpu().numpy()[~ties] > 0, sc.depth[~ties] > 0) and scene.info.tolist() == [0, 0, 0, 0]
    # the frames are what the zoom-in crops read: one 32 x 32 crop of scene 1 against the crops' oracle on the ORACLE's frame
    M = np.array([[[0.75, 0.1, -3.0], [-0.1, 0.75, 2.5]]], np.float32)
    crop = crops.warp_affine(frames, _dev(M), (32, 32), frame_index=_dev([1], torch.int32), dtype=torch.uint8)
    if not ties[1].any():
        assert np.array_equal(crop[0].permute(1, 2, 0).cpu().numpy(), crops_oracle.warp_one(want[1], M[0], (32, 32)))
    assert np.array_equal(crop[0].permute(1, 2, 0).cpu().numpy(), crops_oracle.warp_one(got[1], M[0], (32, 32)))
    # and the scene's depth and instance maps annotate it: every instance's visible count is its share of the instance map
    rendered_depth = torch.stack([torch.where(scene.instance[int(s)] == b, scene.depth[int(s)], torch.zeros_like(scene.depth[0])) for b, s in enumerate(sc.scene_index)])
    rec = gtinfo.gt_info_from_depth(rendered_depth, scene.depth, _dev(cases.FRAME_K), delta=0.001, scene_index=_dev(sc.scene_index))
    assert rec.info[:, gtinfo.PX_VISIB].tolist() == [int((scene.instance == b).sum()) for b in range(4)]


def test_b_zero_launches_nothing():
    from lc_amd import shade

    ms, ap = _set("ico20")
    e = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    out = shade.shade(ms, ap, torch.zeros(0, 16, 16, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), e(0, 3, 3), e(0, 3), e(0, 3, 3),
                      light=shade.DEFAULT_LIGHT, phong=shade.DEFAULT_PHONG)
    assert tuple(out.shape) == (0, 16, 16, 3)
