"""The scene poses drawn on the device against the host contract of lc_amd/posedraw.py, bit for bit, on every case of
tests/posedraw_cases.py (which tests/test_posedraw_host.py shows to reach every branch): the five outputs as bit patterns, the seed as a
device word and as a whole number, and a captured graph that follows its seed word."""
import numpy as np
import pytest
import torch

from tests import posedraw_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _word(seed):
    seed %= 2 ** 64
    return torch.full((1,), seed - 2 ** 64 if seed >= 2 ** 63 else seed, dtype=torch.int64, device=DEV)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, want, what):
    for name in got._fields:
        g, w = _bits(getattr(got, name)), _bits(getattr(want, name))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def differs(got, want):
    return not np.array_equal(_bits(got.R), _bits(want.R)) and not np.array_equal(_bits(got.t), _bits(want.t))


def uploaded(c):
    return dict(scene_id=torch.from_numpy(c.scene_ids).to(DEV), mesh_index=torch.from_numpy(c.mesh_index).to(DEV), radius=torch.from_numpy(c.radius).to(DEV),
                cam_K=torch.from_numpy(c.cam_K).to(DEV))


def draw(c, seed, ins=None):
    from lc_amd.posedraw import draw_scene_poses

    return draw_scene_poses(c.cfg, seed=seed, **(uploaded(c) if ins is None else ins))


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_device_equals_the_host_contract_bit_for_bit(name):
    c = cases.build(name)
    want, _ = cases.reference(name)
    got = draw(c, _word(c.seed))
    torch.cuda.synchronize()
    same(got, want, name)
    same(draw(c, c.seed), want, (name, "the seed as a whole number"))
    if c.seed < 2 ** 63:
        same(draw(c, torch.from_numpy(np.array([c.seed], dtype=np.uint64)).to(DEV)), want, (name, "a uint64 word"))


def test_a_radius_the_host_would_refuse_refuses_its_slots_on_the_device():
    c = cases.build("s3-m2")
    want, _ = cases.reference("s3-m2")
    for bad in (-0.001, np.inf, np.nan):
        radius = c.radius.copy()
        radius[1] = bad
        got = draw(c._replace(radius=radius), c.seed)
        hurt = c.mesh_index == 1
        info = got.info.cpu().numpy()
        assert (info[hurt] == -2).all() and not info[~hurt].any() and (got.mesh_index_out.cpu().numpy()[hurt] == -1).all(), bad
        assert not got.R.cpu().numpy()[hurt].any() and not got.t.cpu().numpy()[hurt].any()
        assert np.array_equal(_bits(got.R)[~hurt], _bits(want.R)[~hurt])  # the rotation does not depend on the other slots


@pytest.mark.parametrize("name", ["crowded", "s3-m64"])
def test_a_replayed_graph_follows_its_seed_word(name):
    c = cases.build(name)
    word, ins = _word(c.seed), uploaded(c)  # uploaded ahead of the capture

    def call():
        return draw(c, word, ins)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        res = call()
    g.replay()
    torch.cuda.synchronize()
    same(res, cases.reference(name)[0], (name, "replay at seed"))
    word.add_(1)
    g.replay()
    torch.cuda.synchronize()
    same(res, cases.reference(name, 1)[0], (name, "replay at seed + 1"))
    assert differs(res, cases.reference(name)[0])
