"""The resident background store and its switch (`lc_amd.backgrounds`) on the device, against the composition that defines them
(tests/bgstore_oracle.py: `augment.draw`, `augment.background_matrices`, `crops_oracle.warp_one`, `augment_oracle.blend`): the pick, the
region matrices and the switched bytes EQUAL on every case of tests/bgstore_cases.py; what stays untouched; the rows the switch refuses;
the library's restated tap combination and blend against crop's and augment's own kernels; `train_inputs(background_store=...)`; a
captured graph that redraws with its seed word; B = 0."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import bgstore_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = len(cases.IDS)


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _store(name):
    from lc_amd import backgrounds

    return backgrounds.BackgroundStore.from_images(cases.make_images(name), DEV)


def _cfg():
    from lc_amd import augment

    return augment.AugmentConfig()


def test_the_store_s_layout_on_the_device():
    from lc_amd import backgrounds

    images = cases.make_images("three")
    store = backgrounds.BackgroundStore.from_images([images[0], torch.from_numpy(images[1]), torch.from_numpy(images[2]).to(DEV)], DEV)
    offsets, total = backgrounds.layout(cases.STORES["three"])
    assert store.G == len(store) == 3 and store.sizes == cases.STORES["three"] and store.device == DEV
    assert store.pixels.dtype == torch.uint8 and tuple(store.pixels.shape) == (total,) and store.pixels.data_ptr() % 4 == 0
    assert store.offsets.dtype == torch.int64 and store.offsets.tolist() == offsets and all(o % 4 == 0 for o in offsets)
    assert store.hw.dtype == torch.int32 and store.hw.tolist() == [list(s) for s in cases.STORES["three"]]
    flat = store.pixels.cpu().numpy()
    for im, o in zip(images, offsets):
        assert np.array_equal(flat[o:o + im.size].reshape(im.shape), im)


@pytest.mark.parametrize("name", list(cases.STORES))
def test_the_pick_and_the_region_equal_the_host_s(name):
    from lc_amd import augment, backgrounds, geometry
    from tests import bgstore_oracle as oracle

    store, sid = _store(name), _dev(cases.IDS)
    for seed in (cases.SEED, torch.full((1,), cases.SEED, dtype=torch.int64, device=DEV)):  # by value, and as the word the kernel reads
        gate, which, bg_hw = backgrounds.pick_backgrounds(store, _cfg(), seed=seed, sample_id=sid)
        want = oracle.pick(_cfg(), cases.SEED, cases.IDS, cases.STORES[name])
        for got, ref in zip((gate, which, bg_hw), want):
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref)
    if name == "three":
        assert {int(b): int(which[b]) for b in torch.nonzero(gate).flatten()} == cases.SWITCHED
    P, _ = augment.draw(_cfg(), cases.SEED, cases.IDS, store.G)
    open_ = (P[:, 0] & 1) == 1
    assert np.array_equal(gate.cpu().numpy() == 1, open_) and np.array_equal(which.cpu().numpy()[open_], P[open_, 1])
    for hw in cases.SIZES:
        M = geometry.background_geometry(seed=cases.SEED, sample_id=sid, bg_hw=bg_hw, out_hw=hw)
        host = augment.background_matrices(cases.SEED, cases.IDS, bg_hw.cpu().numpy(), hw)
        assert np.array_equal(M.cpu().numpy().view(np.int32), host.view(np.int32)), hw
        assert np.array_equal(host.view(np.int32), cases.reference(name, hw)["M"].view(np.int32))
    # no gate opens at probability 0, every gate at 1; a seed apart, another pick
    from lc_amd.augment import AugmentConfig

    g0, w0, hw0 = backgrounds.pick_backgrounds(store, AugmentConfig(switch_bg_prob=0.0), seed=cases.SEED, sample_id=sid)
    g1, w1, _ = backgrounds.pick_backgrounds(store, AugmentConfig(switch_bg_prob=1.0), seed=cases.SEED, sample_id=sid)
    assert not g0.any() and (w0 == -1).all() and (hw0 == 1).all() and g1.all() and (w1 >= 0).all() and (w1 < store.G).all()
    assert np.array_equal(w1.cpu().numpy(), augment.draw(AugmentConfig(switch_bg_prob=1.0), cases.SEED, cases.IDS, store.G)[0][:, 1])


@pytest.mark.parametrize("name,hw", cases.CASES)
def test_the_switched_crops_equal_the_oracle_bit_for_bit(name, hw):
    from lc_amd import backgrounds

    ref = cases.reference(name, hw)
    crops, msk = _dev(ref["crops"]), _dev(ref["msk"])
    info, which = backgrounds.switch_backgrounds(crops, _store(name), _cfg(), seed=cases.SEED, sample_id=_dev(cases.IDS), msk_in=msk)
    got = crops.cpu().numpy()
    assert np.array_equal(info.cpu().numpy(), ref["info"]) and info.dtype == torch.int32 and set(info.tolist()) == {0, 1}
    assert np.array_equal(which.cpu().numpy(), ref["which"])
    wrong = np.argwhere(got != ref["out"])
    assert len(wrong) == 0, (len(wrong), wrong[:5].tolist())
    # what the switch must not touch keeps the sentinel's bytes: rows with a closed gate, and pixels with k = 1024
    closed = ref["info"] == 0
    assert closed.sum() == 5 and np.array_equal(got[closed], ref["crops"][closed])
    keep = np.broadcast_to((ref["msk"] >= 1.0)[:, None], got.shape)
    assert keep[~closed].any() and np.array_equal(got[keep], ref["crops"][keep])
    assert all(not np.array_equal(got[b], ref["crops"][b]) for b in np.flatnonzero(~closed))
    assert np.array_equal(msk.cpu().numpy().view(np.int32), ref["msk"].view(np.int32))  # (the mask is read, never written)


def test_a_row_with_a_non_finite_matrix_or_an_unlisted_image_is_refused_and_untouched():
    """Through the C entry with a hand-made `which` and `M`: rows 0 and 5 are in order, row 1 has a NaN and row 2 an infinity in M, row 3
    is closed, row 4 names image G, row 6 a NaN in M behind a closed gate (closed comes first)."""
    from lc_amd import _lib, augment, backgrounds

    name, hw = "three", (31, 40)
    ref, store = cases.reference(name, hw), _store(name)
    rows = 7
    crops, msk = _dev(ref["crops"][:rows]), _dev(ref["msk"][:rows])
    which = np.array([1, 2, 0, -1, 3, 2, -7], dtype=np.int32)
    sizes = [cases.STORES[name][g] if 0 <= g < 3 else (1, 1) for g in which]
    M = augment.background_matrices(cases.SEED, cases.IDS[:rows], np.array(sizes), hw)
    M[1, 0, 2], M[2, 1, 1], M[6, 0, 0] = np.nan, np.inf, np.nan
    info = torch.full((rows,), 99, dtype=torch.int32, device=DEV)
    wd, Md = _dev(which), _dev(M)
    rc = backgrounds.load().lc_bgstore_switch_u8(_lib.ptr(crops), _lib.ptr(msk), _lib.ptr(store.pixels), _lib.ptr(store.offsets), _lib.ptr(store.hw), store.G,
                                                 _lib.ptr(wd), _lib.ptr(Md), hw[0], hw[1], rows, _lib.ptr(info), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and info.tolist() == [1, -1, -1, 0, -1, 1, 0]
    got = crops.cpu().numpy()
    for b in (1, 2, 3, 4, 6):
        assert np.array_equal(got[b], ref["crops"][b]), b
    from tests import augment_oracle, crops_oracle

    images = ref["images"]
    for b in (0, 5):
        bg = crops_oracle.warp_one(images[which[b]], M[b], hw).transpose(2, 0, 1)
        assert np.array_equal(got[b], augment_oracle.blend(ref["crops"][b], bg, ref["msk"][b])), b


def test_images_of_one_size_give_what_warp_affine_and_augment_give():
    """The library restates crop's tap combination and augment's blend: on a store whose images share a size the switch EQUALS the device's
    existing route, `warp_affine(frame_index=which)` followed by `augment` with switch-only rows."""
    from lc_amd import augment, backgrounds, crops, geometry

    rng = np.random.default_rng(77)
    G, size, hw = 4, (23, 29), (33, 65)
    frames = rng.integers(0, 256, (G,) + size + (3,), dtype=np.uint8)
    store = backgrounds.BackgroundStore.from_images(list(frames), DEV)
    crop_h, msk_h = cases.make_inputs(*hw)
    sid = _dev(cases.IDS)
    switched, msk = _dev(crop_h), _dev(msk_h)
    info, which = backgrounds.switch_backgrounds(switched, store, _cfg(), seed=cases.SEED, sample_id=sid, msk_in=msk)
    M = geometry.background_geometry(seed=cases.SEED, sample_id=sid, bg_hw=size, out_hw=hw)
    cuts = crops.warp_affine(_dev(frames), M, hw, frame_index=which.clamp(min=0), dtype=torch.uint8)  # (B,3,h,w): row b's own background
    params = np.zeros((B, augment.WORDS), dtype=np.int32)
    params[:, 0], params[:, 1] = info.cpu().numpy() == 1, np.arange(B)
    lut = np.tile(np.arange(256, dtype=np.uint8), (B, 3, 1))
    want, ainfo = augment.augment(_dev(crop_h), params, lut, msk_in=msk, backgrounds=cuts, dtype=torch.uint8)
    assert 0 < int((info == 1).sum()) < B and not ainfo.any()
    assert torch.equal(switched, want)
    assert not torch.equal(switched, _dev(crop_h))


@functools.lru_cache(maxsize=None)
def _chain_inputs():
    from lc_amd import backgrounds
    from tests import test_gpu_train_inputs as base

    c = base.case()
    d = {k: _dev(v) for k, v in c.items()}
    rng = np.random.default_rng(9)
    d["store"] = backgrounds.BackgroundStore.from_images([rng.integers(0, 256, (hb, wb, 3), dtype=np.uint8) for hb, wb in ((40, 52), (37, 101), (20, 24))], DEV)
    return base, d


def _chained(seed, **kw):
    from lc_amd.train_inputs import train_inputs

    base, d = _chain_inputs()
    return train_inputs(d["frames"], d["frame_index"], masks=d["masks"], mask_index=d["frame_index"], bbox_xyxy=d["box"], cam_K=d["K"], sample_id=d["sample_id"],
                        cfg=base._cfg(), seed=seed, in_hw=base.IN_HW, out_hw=base.OUT_HW, valid_th=base.VALID_TH, n_check=base.N_CHECK,
                        normalize=(base.MEAN, base.STD), **kw)


def test_train_inputs_with_a_store_switches_before_the_colour_chain_and_changes_nothing_else():
    from lc_amd import augment, backgrounds, crops, maskcrop

    base, d = _chain_inputs()
    got, plain = _chained(base.SEED, background_store=d["store"]), _chained(base.SEED)
    assert sorted(got) == sorted(plain) == sorted(base.NAMES)
    for name in base.NAMES:
        if name != "rgb_in":
            assert base.equal(got[name], plain[name]), name
    crop = crops.warp_affine(d["frames"], got["in_affine"], base.IN_HW, frame_index=d["frame_index"], dtype=torch.uint8)
    mi = maskcrop.mask_crops(d["masks"], got["in_affine"], base.IN_HW, mask_index=d["frame_index"], n_check=0, want=("msk_vis",))
    before = crop.clone()
    sinfo, which = backgrounds.switch_backgrounds(crop, d["store"], base._cfg(), seed=base.SEED, sample_id=d["sample_id"], msk_in=mi.msk_vis)
    rgb, _ = augment.augment_drawn(crop, base._cfg(), seed=base.SEED, sample_id=d["sample_id"], msk_in=mi.msk_vis, backgrounds=None, normalize=(base.MEAN, base.STD))
    assert torch.equal(got["rgb_in"], rgb)
    P, _ = augment.draw(base._cfg(), base.SEED, base.case()["sample_id"], d["store"].G, base.IN_HW)
    assert np.array_equal(sinfo.cpu().numpy() == 1, (P[:, 0] & 1) == 1) and 0 < int((sinfo == 1).sum())
    changed = [b for b in range(base.B) if not torch.equal(crop[b], before[b])]
    assert changed and set(changed) <= set(torch.nonzero(sinfo == 1).flatten().tolist())
    assert not torch.equal(got["rgb_in"][changed], plain["rgb_in"][changed])


def test_a_replayed_graph_picks_and_cuts_anew_with_its_seed_word():
    from lc_amd import backgrounds, crops
    from lc_amd.augment import AugmentConfig

    name, hw = "three", (31, 40)
    ref, store = cases.reference(name, hw), _store(name)
    cfg = AugmentConfig(switch_bg_prob=0.9)
    frames, msk, sid = _dev(ref["crops"]).permute(0, 2, 3, 1).contiguous(), _dev(ref["msk"]), _dev(cases.IDS)
    eye = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], device=DEV).expand(B, 2, 3).contiguous()

    def step(seed):
        crop = crops.warp_affine(frames, eye, hw, dtype=torch.uint8)  # the identity: the sentinel crop, made anew at every replay
        info, which = backgrounds.switch_backgrounds(crop, store, cfg, seed=seed, sample_id=sid, msk_in=msk)
        return crop, info, which

    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(word)  # warm-up: library loads, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        res = step(word)
    word.fill_(cases.SEED)
    seen = []
    for k in (0, 1):
        g.replay()
        torch.cuda.synchronize()
        seen.append([t.cpu().clone() for t in res])
        eager = step(cases.SEED + k)
        torch.cuda.synchronize()
        for a, b in zip(seen[-1], eager):
            assert torch.equal(a, b.cpu()), k
        word.add_(1)
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][2], seen[1][2])


def test_an_empty_batch_launches_nothing():
    from lc_amd import backgrounds

    store = _store("one")
    crops = torch.empty(0, 3, 8, 12, dtype=torch.uint8, device=DEV)
    info, which = backgrounds.switch_backgrounds(crops, store, _cfg(), seed=5, sample_id=torch.empty(0, dtype=torch.int32, device=DEV),
                                                 msk_in=torch.empty(0, 8, 12, device=DEV))
    gate, w2, bg_hw = backgrounds.pick_backgrounds(store, _cfg(), seed=5, sample_id=torch.empty(0, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert tuple(info.shape) == tuple(which.shape) == tuple(gate.shape) == tuple(w2.shape) == (0,) and tuple(bg_hw.shape) == (0, 2)
    lib = backgrounds.load()
    assert lib.lc_bgstore_pick(ctypes.c_double(0.5), 1, None, None, None, 0, None, None, None, None) == 0
    assert lib.lc_bgstore_switch_u8(None, None, None, None, None, 1, None, None, 8, 12, 0, None, None) == 0
