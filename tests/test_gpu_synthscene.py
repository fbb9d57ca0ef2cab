"""`synthscene.synth_scenes` on the device: 2 scenes of 3 slots, one of them empty, on 48 x 64 frames with the 12-face box and the 20-face
icosphere of tests/render_cases.py.  The chain adds no pixel code, so it is judged against the hand-written composition of the same stages
on the same poses, byte for byte; then the slot that was not placed, a replayed graph after `seed.add_(1)`, and the textured route on the
meshes and textures of tests/texshade_cases.py's smallest batch case."""
import functools

import numpy as np
import pytest
import torch

from tests import render_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FRAME = (48, 64)
NEAR, FAR, DELTA = 0.01, 6.5, 0.015
SEED = 2 ** 40 + 17
SLOTS = np.array([[0, -1, 1], [1, 0, 0]], dtype=np.int32)
SCENE_IDS = np.array([3, 11], dtype=np.int32)


def _cfg():
    from lc_amd.posedraw import PoseDrawConfig

    return PoseDrawConfig(z_range=(0.6, 0.9), centre_box=(8.0, 8.0, 56.0, 40.0), gap=0.005, near=NEAR)


@functools.lru_cache(maxsize=None)
def _plain():
    from lc_amd import posedraw, render, shade

    meshes = [render_cases.box((0.08, 0.06, 0.05)), render_cases.icosphere(0, 0.1)]
    ms = render.MeshSet(meshes, DEV)
    rng = np.random.default_rng(4)
    ap = shade.Appearance(ms, [rng.integers(0, 256, (len(v), 3), dtype=np.uint8) for v, _ in meshes])
    return ms, ap, torch.from_numpy(posedraw.mesh_radii(meshes)).to(DEV)


@functools.lru_cache(maxsize=None)
def _textured():
    from lc_amd import posedraw, render, texture
    from tests import texshade_cases as tc

    c = tc.build("b3-1x1")  # the smallest of the batch cases: a 12-face box, an 80-face icosphere and an untextured quad
    b = c.base
    meshes = [(v, f) for v, f, _, _ in b.meshes]
    ms = render.MeshSet(meshes, DEV)
    store = texture.TextureStore.from_images(list(c.images), DEV)
    ap = texture.TexturedAppearance(ms, list(c.uvs), c.tex_index, store, [m[3] for m in b.meshes], [m[2] for m in b.meshes])
    return ms, ap, torch.from_numpy(posedraw.mesh_radii(meshes)).to(DEV)


@functools.lru_cache(maxsize=None)
def _uploaded():
    """Uploaded once, ahead of any capture."""
    return dict(scene_id=torch.from_numpy(SCENE_IDS).to(DEV), mesh_index=torch.from_numpy(SLOTS).to(DEV), cam_K=torch.from_numpy(render_cases.camera(FRAME)).to(DEV))


def _inputs(seed):
    return dict(_uploaded(), seed=seed)


@functools.lru_cache(maxsize=None)
def _lit():
    return torch.tensor([0.4, -0.4, -0.4], device=DEV), torch.tensor([0.4, 0.8, 0.3], device=DEV)


def _lights():
    return dict(light=_lit()[0], phong=_lit()[1])


def _chain(ms, ap, radius, seed, **kw):
    from lc_amd import synthscene

    return synthscene.synth_scenes(ms, ap, radius, _cfg(), **_inputs(seed), frame_hw=FRAME, near=NEAR, far=FAR, delta=DELTA, **_lights(), **kw)


def _by_hand(ms, ap, radius, seed, render_scene, background=None):
    """The same stages called one by one."""
    from lc_amd import gtinfo, posedraw, render

    ins = _inputs(seed)
    drawn = posedraw.draw_scene_poses(_cfg(), radius=radius, **ins)
    S, M = SLOTS.shape
    B = S * M
    R, t, mi = drawn.R.reshape(B, 3, 3), drawn.t.reshape(B, 3), drawn.mesh_index_out.reshape(B)
    scene_index = torch.tensor([s for s in range(S) for _ in range(M)], dtype=torch.int32, device=DEV)
    K = ins["cam_K"].expand(B, 3, 3).contiguous()
    frames, scene = render_scene(ms, ap, mi, scene_index, R, t, K, FRAME, S, near=NEAR, far=FAR, background=background, **_lights())
    inst = render.render_depth(ms, mi, R, t, K, FRAME, near=NEAR, far=FAR)
    composed = gtinfo.compose_scene_depth(inst.depth, scene_index, FRAME, S, want_instance=True)
    idx = torch.where(mi >= 0, scene_index, torch.full_like(scene_index, -1))
    gt = gtinfo.gt_info_from_depth(inst.depth, composed.depth, K, delta=DELTA, scene_index=idx, pixel_center=(0.5, 0.5))
    return drawn, frames, scene, composed, gt, inst


def _same_scenes(a, b, what):
    for name, x, y in (("frames", a.frames, b.frames), ("depth", a.scene.depth, b.scene.depth), ("instance", a.scene.instance, b.scene.instance),
                       ("records", a.gt.info, b.gt.info), ("masks", a.gt.mask_visib, b.gt.mask_visib), ("R", a.poses.R, b.poses.R), ("t", a.poses.t, b.poses.t),
                       ("mesh_index_out", a.poses.mesh_index_out, b.poses.mesh_index_out)):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name)


def test_the_chain_equals_the_hand_written_composition_byte_for_byte():
    from lc_amd import shade
    from lc_amd.posedraw import draw_scene_poses_host

    ms, ap, radius = _plain()
    rng = np.random.default_rng(8)
    for background in (None, torch.from_numpy(rng.integers(0, 256, (2, *FRAME, 3), dtype=np.uint8)).to(DEV)):
        out = _chain(ms, ap, radius, SEED, background=background)
        drawn, frames, scene, composed, gt, inst = _by_hand(ms, ap, radius, SEED, shade.render_scene, background)
        torch.cuda.synchronize()
        S, M = SLOTS.shape
        assert out.frames.shape == (S, *FRAME, 3) and out.frames.dtype == torch.uint8 and out.gt.info.shape == (S * M, 12) and out.gt.mask_visib.shape == (S * M, *FRAME)
        for name, got, want in (("frames", out.frames, frames), ("depth", out.scene.depth, scene.depth), ("instance", out.scene.instance, scene.instance),
                                ("depth of the separate composition", out.scene.depth, composed.depth), ("instance of the separate composition", out.scene.instance, composed.instance),
                                ("records", out.gt.info, gt.info), ("masks", out.gt.mask_visib, gt.mask_visib), ("R", out.poses.R, drawn.R.reshape(-1, 3, 3)),
                                ("t", out.poses.t, drawn.t.reshape(-1, 3)), ("mesh_index_out", out.poses.mesh_index_out, drawn.mesh_index_out.reshape(-1)),
                                ("tries", out.poses.tries, drawn.tries.reshape(-1)), ("info", out.poses.info, drawn.info.reshape(-1)), ("render_info", out.render_info, inst.info)):
            g, w = got.cpu().numpy(), want.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
        assert out.scene_index.tolist() == [0, 0, 0, 1, 1, 1]
    # the poses are the host contract's, and the scene shows them: every placed instance is seen, and the frame is drawn where the scene is hit
    host = draw_scene_poses_host(_cfg(), SEED, SCENE_IDS, SLOTS, radius.cpu().numpy(), render_cases.camera(FRAME))
    out = _chain(ms, ap, radius, SEED)
    assert np.array_equal(out.poses.R.cpu().numpy().view(np.int32), host.R.reshape(-1, 3, 3).view(np.int32))
    assert np.array_equal(out.poses.t.cpu().numpy().view(np.int32), host.t.reshape(-1, 3).view(np.int32))
    info, placed = out.gt.info.cpu().numpy(), host.info.reshape(-1) == 0
    assert placed.tolist() == [True, False, True, True, True, True] and (info[placed, 0] > 0).all() and (info[placed, 2] > 0).all()
    hit = out.scene.instance.cpu().numpy() >= 0
    assert hit.any() and np.array_equal(hit, out.scene.depth.cpu().numpy() > 0) and out.frames.cpu().numpy()[hit].any() and not out.frames.cpu().numpy()[~hit].any()
    vis = out.gt.visib_fract().cpu().numpy()
    assert ((vis > 0) & (vis <= 1))[placed].all() and vis[~placed].tolist() == [0.0]


def test_a_slot_that_was_not_placed_owns_no_pixel_and_has_the_refused_row_s_record():
    ms, ap, radius = _plain()
    slots = torch.tensor([[0, -1, 7], [-9, 0, 1]], dtype=torch.int32, device=DEV)  # an empty slot, and unknown meshes on both sides
    from lc_amd import synthscene

    ins = dict(_inputs(SEED), mesh_index=slots)
    out = synthscene.synth_scenes(ms, ap, radius, _cfg(), **ins, frame_hw=FRAME, near=NEAR, far=FAR, delta=DELTA, **_lights())
    torch.cuda.synchronize()
    assert out.poses.info.tolist() == [0, -3, -2, -2, 0, 0] and out.poses.mesh_index_out.tolist() == [0, -1, -1, -1, 0, 1]
    inst, info, mask = out.scene.instance.cpu().numpy(), out.gt.info.cpu().numpy(), out.gt.mask_visib.cpu().numpy()
    for row in (1, 2, 3):
        assert not (inst == row).any() and (info[row] == -1).all() and not mask[row].any() and out.render_info[row].item() == -1, row
    for row in (0, 4, 5):
        assert (inst == row).any() and info[row, 2] > 0 and mask[row].any() and np.array_equal(inst[row // 3] == row, mask[row] & (inst[row // 3] == row)), row


def test_a_replayed_graph_draws_renders_and_annotates_a_new_scene():
    ms, ap, radius = _plain()
    word = torch.full((1,), SEED, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(ms, ap, radius, word)  # warm-up: library loads, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        res = _chain(ms, ap, radius, word)
    g.replay()
    torch.cuda.synchronize()
    first = _chain(ms, ap, radius, SEED)
    _same_scenes(res, first, "replay at seed")
    word.add_(1)
    g.replay()
    torch.cuda.synchronize()
    _same_scenes(res, _chain(ms, ap, radius, SEED + 1), "replay at seed + 1")
    assert not torch.equal(res.frames, first.frames) and not torch.equal(res.poses.t, first.poses.t) and not torch.equal(res.gt.info, first.gt.info)


def test_the_textured_route():
    from lc_amd import texture

    ms, ap, radius = _textured()
    out = _chain(ms, ap, radius, SEED)
    drawn, frames, scene, composed, gt, inst = _by_hand(ms, ap, radius, SEED, texture.render_scene)
    torch.cuda.synchronize()
    for name, got, want in (("frames", out.frames, frames), ("depth", out.scene.depth, composed.depth), ("instance", out.scene.instance, composed.instance),
                            ("records", out.gt.info, gt.info), ("masks", out.gt.mask_visib, gt.mask_visib)):
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), name
    hit = out.scene.instance.cpu().numpy() >= 0
    assert hit.any() and out.frames.cpu().numpy()[hit].any()
    plain = _chain(*_plain(), SEED)  # other meshes and no textures: other frames, but the same rotations (they depend on seed, scene and slot alone)
    assert torch.equal(plain.poses.R, out.poses.R) and not torch.equal(plain.frames, out.frames)
