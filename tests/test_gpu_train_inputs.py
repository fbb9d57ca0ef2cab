"""The chained training input (`lc_amd.train_inputs.train_inputs`) against its stages called one by one with `zoom_geometry_host`'s arrays
uploaded: every returned tensor `torch.equal`, with the masks as bytes and as an RleStore, under a captured graph with a changing seed
word, and with meshes."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

B, H, W = 5, 48, 64
IN_HW, OUT_HW = (32, 32), (16, 16)
N_CHECK, VALID_TH = 16, 12
REFUSED, SMALL = 3, 1  # the row with a NaN in its box; the row whose mask leaves fewer than VALID_TH pixels in the crop
SEED = (1 << 40) + 78  # rows 0, 1 and 4 are rotated at this seed, row 2 is not
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NAMES = ("rgb_in", "msk_vis", "msk_noc", "sym_ck_pts2d", "valid_cnt", "out_K", "out_pix_scale", "in_affine", "info")


def case():
    """Host arrays: two 48 x 64 frames of noise, mask 0 a large rectangle and mask 1 a blob of 3 x 4 pixels, five rows over them."""
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    masks = np.zeros((2, H, W), dtype=np.uint8)
    masks[0, 10:40, 12:50] = 1
    masks[1, 22:25, 30:34] = 1
    frame_index = np.array([0, 1, 0, 0, 1], dtype=np.int32)
    box = np.array([[12, 10, 50, 40], [20, 14, 44, 34], [16, 12, 40, 36], [12, 10, 50, 40], [26, 18, 38, 28]], dtype=np.float32)
    box[REFUSED, 2] = np.nan
    K = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    sample_id = np.array([11, -4, 2 ** 31 - 1, 5, 11], dtype=np.int32)
    backgrounds = rng.integers(0, 256, size=(3, 3, IN_HW[0], IN_HW[1]), dtype=np.uint8)
    return dict(frames=frames, masks=masks, frame_index=frame_index, box=box, K=K, sample_id=sample_id, backgrounds=backgrounds)


def _cfg():
    from lc_amd import augment

    return augment.AugmentConfig(pixel_aug_prob=1.0, switch_bg_prob=0.7, rotate_prob=0.5)


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs():
    from lc_amd import rle

    c = case()
    d = {k: _dev(v) for k, v in c.items()}
    d["store"] = rle.RleStore.from_masks(d["masks"])
    return c, d


def chained(seed, masks="bytes", **kw):
    from lc_amd.train_inputs import train_inputs

    _, d = _inputs()
    src = dict(masks=d["masks"]) if masks == "bytes" else dict(rle_store=d["store"])
    return train_inputs(d["frames"], d["frame_index"], **src, mask_index=d["frame_index"], bbox_xyxy=d["box"], cam_K=d["K"], sample_id=d["sample_id"], cfg=_cfg(),
                        seed=seed, backgrounds=d["backgrounds"], in_hw=IN_HW, out_hw=OUT_HW, valid_th=VALID_TH, n_check=N_CHECK, normalize=(MEAN, STD), **kw)


@functools.lru_cache(maxsize=None)
def one_by_one(seed):
    """The same stages with the geometry formed on the host and uploaded: the route the chain replaces.  Computed once per seed."""
    from lc_amd import augment, crops, geometry, maskcrop

    c, d = _inputs()
    g = geometry.zoom_geometry_host(_cfg(), seed, c["sample_id"], c["box"], (H, W), c["K"], IN_HW[::-1], OUT_HW[::-1])
    in_affine, out_affine, step_id = _dev(g.in_affine), _dev(g.out_affine), _dev(g.step_id)
    mc = maskcrop.mask_crops(d["masks"], out_affine, OUT_HW, mask_index=d["frame_index"], valid_th=VALID_TH, n_check=N_CHECK, sample_id=step_id)
    mi = maskcrop.mask_crops(d["masks"], in_affine, IN_HW, mask_index=d["frame_index"], n_check=0, want=("msk_vis",))
    winfo = torch.empty(B, device=DEV, dtype=torch.int32)
    crop = crops.warp_affine(d["frames"], in_affine, IN_HW, frame_index=d["frame_index"], dtype=torch.uint8, info=winfo)
    rgb_in, ainfo = augment.augment_drawn(crop, _cfg(), seed=seed, sample_id=d["sample_id"], msk_in=mi.msk_vis, backgrounds=d["backgrounds"], normalize=(MEAN, STD))
    info = torch.stack((_dev(g.info), mc.info, mi.info, winfo, ainfo)).min(0).values
    torch.cuda.synchronize()
    out = dict(rgb_in=rgb_in, msk_vis=mc.msk_vis, msk_noc=mc.msk_noc, sym_ck_pts2d=mc.sym_ck_pts2d, valid_cnt=mc.valid_cnt, out_K=_dev(g.out_K),
               out_pix_scale=_dev(g.out_pix_scale), in_affine=in_affine, info=info)
    return {k: v.cpu() for k, v in out.items()}


def equal(a, b):
    """torch.equal, with a NaN equal to a NaN at the same place (a refused row's matrices)."""
    a, b = a.cpu(), b.cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        nan = torch.isnan(b)
        return torch.equal(torch.isnan(a), nan) and torch.equal(a[~nan], b[~nan])
    return torch.equal(a, b)


@pytest.mark.parametrize("masks", ["bytes", "rle"])
def test_the_chain_equals_its_stages_one_by_one(masks):
    got, want = chained(SEED, masks), one_by_one(SEED)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(NAMES)
    for name in NAMES:
        assert equal(got[name], want[name]), name
    info, cnt, ck = got["info"].cpu(), got["valid_cnt"].cpu(), got["sym_ck_pts2d"].cpu()
    assert info.tolist() == [-1 if b == REFUSED else 0 for b in range(B)]  # -1 exactly on the refused row
    assert torch.isnan(got["in_affine"][REFUSED]).all() and torch.isnan(got["out_K"][REFUSED]).all() and int(cnt[REFUSED]) == 0
    assert 0 < int(cnt[SMALL]) < VALID_TH and (ck[SMALL] == -1).all() and (ck[REFUSED] == -1).all()  # under the threshold: no check points
    for b in set(range(B)) - {REFUSED, SMALL}:
        assert int(cnt[b]) >= VALID_TH and (ck[b] >= 0).all(), b
        assert bool(got["msk_noc"][b].cpu()[ck[b, :, 1], ck[b, :, 0]].all()), b  # on set pixels
    assert got["rgb_in"].dtype == torch.float32 and tuple(got["rgb_in"].shape) == (B, 3) + IN_HW
    assert tuple(got["msk_vis"].shape) == (B,) + OUT_HW and got["sym_ck_pts2d"].dtype == torch.int64


def test_a_replayed_graph_redraws_with_its_seed_word():
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chained(word)  # warm-up: library loads, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        res = chained(word)
    word.fill_(SEED)
    seen = []
    for step in (0, 1):
        g.replay()
        torch.cuda.synchronize()
        seen.append({k: v.cpu().clone() for k, v in res.items()})
        eager = chained(SEED + step)  # by value: a word of its own
        torch.cuda.synchronize()
        for name in NAMES:
            assert equal(seen[-1][name], eager[name]), (step, name)
            assert equal(seen[-1][name], one_by_one(SEED + step)[name]), (step, name)
        word.add_(1)
    keep = [b for b in range(B) if b != REFUSED]
    assert not torch.equal(seen[0]["rgb_in"][keep], seen[1]["rgb_in"][keep]) and not torch.equal(seen[0]["in_affine"][keep], seen[1]["in_affine"][keep])
    assert not torch.equal(seen[0]["sym_ck_pts2d"], seen[1]["sym_ck_pts2d"])


def test_with_meshes_the_depth_follows_the_device_out_K():
    from lc_amd import render
    from tests import render_cases

    v, f = render_cases.MESHES["ico"]
    ms = render.MeshSet([(v, f)], DEV)
    R = torch.eye(3, device=DEV).expand(B, 3, 3).contiguous()
    t = torch.tensor([[0.0, 0.0, 6.0 * float(np.abs(v).max())]], device=DEV).expand(B, 3).contiguous()
    near, far = 0.1 * float(t[0, 2]), 10.0 * float(t[0, 2])
    idx = ms.index_of([0] * B)
    got = chained(SEED, meshes=ms, mesh_index=idx, R=R, t=t, near=near, far=far)
    want = one_by_one(SEED)
    _, d = _inputs()
    homo, _ = render.render_homo_z_out(ms, idx, R, t, d["K"].expand(B, 3, 3), want["out_K"].to(DEV), OUT_HW, near=near, far=far)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(NAMES + ("homo_z_out",)) and tuple(got["homo_z_out"].shape) == (B,) + OUT_HW + (3,)
    assert equal(got["homo_z_out"], homo)
    assert bool((got["homo_z_out"][0] != 0).any())  # the object is in view of the first crop
    for name in NAMES:
        assert equal(got[name], want[name]), name
