"""The sampler's three kernels and the resident training set on the device, against the host restatements of lc_amd/sampler.py, bit for
bit: the drawn rows and their records, the selection at every wavefront and chunk edge, the gather on both of its paths, the three under
one captured graph, and `TrainSet.step_inputs` against `train_inputs` on the rows it took."""
import functools

import numpy as np
import pytest
import torch

from tests import sampler_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED0 = 2 ** 63 + 5  # (the signed word is negative, and step 2^40 - 1 does not wrap it)


def _word(seed):
    seed %= 2 ** 64
    return torch.full((1,), seed - 2 ** 64 if seed >= 2 ** 63 else seed, dtype=torch.int64, device=DEV)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_rows(got, want, what):
    for name in got._fields:
        g, w = _bits(getattr(got, name)), _bits(getattr(want, name))
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


@functools.lru_cache(maxsize=None)
def table(n):
    from lc_amd.sampler import AnnotationTable

    return AnnotationTable(**cases.table_columns(n, seed=n), device=DEV, n_frames=3, n_meshes=2)


@pytest.mark.parametrize("n", [1, 2, 5, 17, 257, 1000])
def test_draw_rows_equals_the_host_definition(n):
    from lc_amd.sampler import FIELDS, draw_rows, draw_rows_host

    tb = table(n)
    for B, S in ((1, 0), (7, 3), (32, 32), (64, 0)):
        for step in (0, 1, n // B, 2 ** 40 - 1):
            seed = (SEED0 + step) % 2 ** 64
            got, want = draw_rows(tb, seed=_word(seed), seed0=SEED0, batch=B, spare=S), draw_rows_host(tb, seed=seed, seed0=SEED0, batch=B, spare=S)
            same_rows(got, want, (n, B, S, step))
            index = got.index.cpu().numpy()
            assert not want.info.any() and (index >= 0).all() and (index < n).all()
            for name in FIELDS:  # the gathered records are the table's rows
                assert np.array_equal(_bits(getattr(got, name)), _bits(tb.host[name][index])), (n, B, S, step, name)
        by_value = draw_rows(tb, seed=(SEED0 + 1) % 2 ** 64, seed0=SEED0, batch=B, spare=S)
        same_rows(by_value, draw_rows_host(tb, seed=(SEED0 + 1) % 2 ** 64, seed0=SEED0, batch=B, spare=S), (n, B, S, "by value"))
    for seed in (SEED0 + 2 ** 40, SEED0 - 1):  # step = 2^40 and step = 2^64 - 1: refused
        got = draw_rows(tb, seed=_word(seed), seed0=SEED0, batch=7, spare=3)
        same_rows(got, draw_rows_host(tb, seed=seed % 2 ** 64, seed0=SEED0, batch=7, spare=3), (n, "refused"))
        assert (got.index == -1).all() and (got.info == -1).all() and (got.im_id == -1).all()
        assert all(bool(torch.isnan(getattr(got, name)).all()) for name in ("bbox_xyxy", "cam_K", "R", "t"))


def test_a_negative_index_in_the_resident_record_refuses_its_row_alone():
    from lc_amd.sampler import AnnotationTable, draw_rows, draw_rows_host

    tb = AnnotationTable(**cases.table_columns(17, seed=3), device=DEV)
    tb.columns["mask_index"][4] = -1  # in place: the kernel judges the resident data
    tb.host["mask_index"][4] = -1
    got, want = draw_rows(tb, seed=_word(SEED0), seed0=SEED0, batch=17, spare=15), draw_rows_host(tb, seed=SEED0, seed0=SEED0, batch=17, spare=15)
    same_rows(got, want, "hurt")
    assert int((want.info == -1).sum()) >= 1 and int((want.info == 0).sum()) >= 16


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 256, 1025])
def test_select_rows_equals_the_host_definition(rows):
    from lc_amd.sampler import select_rows, select_rows_host

    rng = np.random.default_rng(rows)
    for B in sorted({max(1, rows // 3), rows}):
        for name in cases.PATTERNS:
            cnt, info = cases.select_pattern(name, rows, B, rng)
            take, short = select_rows(torch.from_numpy(cnt).to(DEV), torch.from_numpy(info).to(DEV), batch=B, valid_th=cases.TH)
            want, want_short = select_rows_host(cnt, info, batch=B, valid_th=cases.TH)
            assert take.dtype == torch.int32 and np.array_equal(take.cpu().numpy(), want) and short.cpu().tolist() == [want_short], (rows, B, name)


@pytest.mark.parametrize("case", cases.SELECT_CASES, ids=[c[0] for c in cases.SELECT_CASES])
def test_select_rows_on_the_hand_written_cases(case):
    from lc_amd.sampler import select_rows

    _, cnt, info, batch, want, shortfall = case
    take, short = select_rows(torch.tensor(cnt, dtype=torch.int32, device=DEV), torch.tensor(info, dtype=torch.int32, device=DEV), batch=batch, valid_th=cases.TH)
    assert take.cpu().tolist() == want and short.cpu().tolist() == [shortfall]


ROW_BYTES = (1, 3, 4, 15, 16, 17, 4100)


def test_take_rows_on_both_paths_at_both_offsets():
    from lc_amd.sampler import take_rows

    R, B = 9, 7
    rng = np.random.default_rng(1)
    take = np.array([8, -1, 0, 3, 3, -1, 8], dtype=np.int32)  # -1 entries and repeats
    take_d = torch.from_numpy(take).to(DEV)
    src, dst, want = [], [], []
    for rb in ROW_BYTES:
        for s_off in (0, 1):
            for d_off in (0, 1):
                host = rng.integers(1, 256, size=R * rb + 1, dtype=np.uint8)
                buf = torch.from_numpy(host).to(DEV)
                src.append(buf[s_off:s_off + R * rb].view(R, rb))
                room = torch.full((B * rb + 2,), 0xAB, dtype=torch.uint8, device=DEV)
                dst.append(room[d_off:d_off + B * rb].view(B, rb))
                rows = host[s_off:s_off + R * rb].reshape(R, rb)
                want.append((np.where(take[:, None] >= 0, rows[np.maximum(take, 0)], 0).astype(np.uint8), room, d_off, B * rb))
                assert src[-1].data_ptr() % 16 == s_off and dst[-1].data_ptr() % 16 == d_off
    for group in (slice(16, 17), slice(0, 2), slice(4, 20), slice(0, len(src))):  # 1, 2 and 16 tensors in a call, and more than a launch holds
        for _, room, _, _ in want[group]:
            room.fill_(0xAB)
        got = take_rows(take_d, *src[group], out=tuple(dst[group]))
        torch.cuda.synchronize()
        for g, d, (w, room, d_off, nbytes) in zip(got, dst[group], want[group]):
            assert g is d and np.array_equal(g.cpu().numpy(), w), (group, w.shape, d_off)
            r = room.cpu().numpy()
            assert (r[:d_off] == 0xAB).all() and (r[d_off + nbytes:] == 0xAB).all(), (group, w.shape, d_off)  # nothing beside its rows is written
    # typed tensors without `out`, one of them not contiguous, and every entry outside [0, R) is a row of zeros
    f, k, b = torch.randn(R, 3, 3, device=DEV), torch.arange(R * 2, device=DEV).reshape(R, 2), torch.ones(R, 5, dtype=torch.bool, device=DEV)
    t = torch.randn(4, R, device=DEV).t()
    wild = torch.tensor([2, R, -7, 0], dtype=torch.int32, device=DEV)
    got = take_rows(wild, f, k, b, t, torch.arange(R, device=DEV, dtype=torch.int32))
    for g, s in zip(got, (f, k, b, t, torch.arange(R, device=DEV, dtype=torch.int32))):
        assert g.dtype == s.dtype and tuple(g.shape) == (4,) + tuple(s.shape[1:])
        assert torch.equal(g[0], s[2]) and torch.equal(g[3], s[0]) and not g[1].any() and not g[2].any()


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # warm-up: library loads, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        res = fn()
    return g, res


def test_the_three_launches_follow_the_seed_word_under_one_graph():
    from lc_amd.sampler import draw_rows, draw_rows_host, select_rows, select_rows_host, take_rows

    tb, B, S = table(257), 32, 32
    word = _word(SEED0)

    def chain():
        rows = draw_rows(tb, seed=word, seed0=SEED0, batch=B, spare=S)
        cnt = rows.obj_id % 7 * 20  # a count that follows the drawn instance: 0, 20, ..., 120 against a threshold of 100
        take, short = select_rows(cnt, rows.info, batch=B, valid_th=cases.TH)
        return rows, take, short, take_rows(take, rows.index, rows.R, rows.obj_id)

    g, (rows, take, short, (index, Rm, obj)) = _capture(chain)
    word.copy_(_word(SEED0 + 6))  # steps 6 .. 9: the first epoch of 257 ends in step 8
    for step in range(6, 10):
        g.replay()
        torch.cuda.synchronize()
        want = draw_rows_host(tb, seed=(SEED0 + step) % 2 ** 64, seed0=SEED0, batch=B, spare=S)
        same_rows(rows, want, step)
        want_take, want_short = select_rows_host(want.obj_id % 7 * 20, want.info, batch=B, valid_th=cases.TH)
        assert np.array_equal(take.cpu().numpy(), want_take) and short.cpu().tolist() == [want_short], step
        assert (want_take >= B).any() and (want_take < 0).any() and (want_take[want_take < B] >= 0).any()  # spares taken, rows left empty, primaries kept
        at = np.maximum(want_take, 0)
        gone = want_take < 0
        assert np.array_equal(index.cpu().numpy(), np.where(gone, 0, want.index[at])) and np.array_equal(obj.cpu().numpy(), np.where(gone, 0, want.obj_id[at])), step
        assert np.array_equal(_bits(Rm), _bits(np.where(gone[:, None, None], np.float32(0), want.R[at]))), step
        word.add_(1)


# ---- the resident training set ---------------------------------------------------------------------------------------------------------
H, W = 48, 64
IN_HW, OUT_HW = (32, 32), (16, 16)
N_CHECK, VALID_TH = 16, 12
BATCH, SPARE = 4, 4
EMPTY = (0, 5)  # the annotations whose mask leaves fewer than VALID_TH pixels in the output crop
SET_SEED0 = 1000
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NAMES = ("rgb_in", "msk_vis", "msk_noc", "sym_ck_pts2d", "valid_cnt", "out_K", "out_pix_scale", "in_affine", "info")


def _cfg():
    from lc_amd import augment

    return augment.AugmentConfig(pixel_aug_prob=1.0, switch_bg_prob=0.7, rotate_prob=0.5)


@functools.lru_cache(maxsize=None)
def scene():
    """Host arrays: two 48 x 64 frames of noise and six annotations, one mask each: four rectangles that fill their boxes, and two blobs
    of 2 x 2 pixels in boxes of 30 pixels, which the zoom shrinks to at most a few pixels of the 16 x 16 output."""
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    box = np.array([[12, 10, 50, 40], [20, 8, 50, 38], [16, 12, 40, 36], [4, 6, 34, 40], [10, 10, 40, 40], [26, 14, 58, 44]], dtype=np.float32)
    masks = np.zeros((6, H, W), dtype=np.uint8)
    for a, (x1, y1, x2, y2) in enumerate(box.astype(int)):
        if a in EMPTY:
            masks[a, (y1 + y2) // 2:(y1 + y2) // 2 + 2, (x1 + x2) // 2:(x1 + x2) // 2 + 2] = 1
        else:
            masks[a, y1:y2, x1:x2] = 1
    K = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    cols = dict(frame_index=np.array([0, 1, 0, 1, 0, 1]), mask_index=np.arange(6), mesh_index=np.zeros(6, int), obj_id=np.arange(6) + 1, scene_id=np.full(6, 48),
                im_id=np.arange(6) * 10, bbox_xyxy=box, cam_K=K, R=np.tile(np.eye(3, dtype=np.float32), (6, 1, 1)), t=np.tile(np.float32([0, 0, 1]), (6, 1)))
    backgrounds = rng.integers(0, 256, size=(3, 3) + IN_HW, dtype=np.uint8)
    return dict(frames=frames, masks=masks, cols=cols, backgrounds=backgrounds)


def host_step(step, spare):
    """The rows, their counts and the selection of one step, on the host: (Rows, valid_cnt, take, shortfall)."""
    from lc_amd import geometry, sampler
    from tests import maskcrop_oracle

    s = scene()
    cols = sampler.AnnotationTable.validate(**s["cols"])
    rows = sampler.draw_rows_host(cols, seed=SET_SEED0 + step, seed0=SET_SEED0, batch=BATCH, spare=spare)
    g = geometry.zoom_geometry_host(_cfg(), SET_SEED0 + step, rows.index, rows.bbox_xyxy, (H, W), rows.cam_K, IN_HW[::-1], OUT_HW[::-1])
    mc = maskcrop_oracle.mask_crops(s["masks"], g.out_affine, OUT_HW, mask_index=rows.mask_index, valid_th=VALID_TH, n_check=0)
    take, short = sampler.select_rows_host(mc["valid_cnt"], np.minimum(np.minimum(rows.info, g.info), mc["info"]), batch=BATCH, valid_th=VALID_TH)
    return rows, mc["valid_cnt"], take, short


@functools.lru_cache(maxsize=None)
def resident(masks, spare):
    from lc_amd import rle, sampler
    from lc_amd.trainset import TrainSet

    s = scene()
    frames, m = torch.from_numpy(s["frames"]).to(DEV), torch.from_numpy(s["masks"]).to(DEV)
    tb = sampler.AnnotationTable(**s["cols"], device=DEV, n_frames=2, n_masks=6)
    src = dict(masks=m) if masks == "bytes" else dict(rle_store=rle.RleStore.from_masks(m))
    ts = TrainSet(frames, tb, **src, cfg=_cfg(), seed0=SET_SEED0, batch=BATCH, spare=spare, in_hw=IN_HW, out_hw=OUT_HW, valid_th=VALID_TH, n_check=N_CHECK,
                  backgrounds=torch.from_numpy(s["backgrounds"]).to(DEV), normalize=(MEAN, STD))
    return ts, frames, m, src


def equal(a, b):
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_the_scene_is_what_the_test_needs():
    """On the CPU: the two blobs are too empty at every step used, the others are not, and with four spares nothing falls short."""
    for step in (0, 1, 2):
        rows, cnt, take, short = host_step(step, SPARE)
        empty = np.isin(rows.index, EMPTY)
        assert (cnt[empty] < VALID_TH).all() and (cnt[~empty] >= VALID_TH).all() and short == 0 and (take >= 0).all(), step
    assert sum(int(np.isin(host_step(step, SPARE)[0].index[:BATCH], EMPTY).sum()) for step in (0, 1)) >= 2  # the retry has work to do


@pytest.mark.parametrize("masks", ["bytes", "rle"])
def test_step_inputs_equals_train_inputs_on_the_taken_rows(masks):
    from lc_amd.train_inputs import train_inputs

    ts, frames, _, src = resident(masks, SPARE)
    for step in (0, 1):
        got = ts.step_inputs(_word(SET_SEED0 + step))
        rows, cnt, take, short = host_step(step, SPARE)
        assert np.array_equal(got["take"].cpu().numpy(), take) and got["shortfall"].cpu().tolist() == [0] == [short], step
        for name in ("index", "frame_index", "mask_index", "mesh_index", "obj_id", "scene_id", "im_id", "bbox_xyxy"):
            assert np.array_equal(_bits(got[name]), _bits(getattr(rows, name)[take])), (step, name)
        for name, field in (("K_no_aug", "cam_K"), ("R_no_aug", "R"), ("t_no_aug", "t")):
            assert np.array_equal(_bits(got[name]), _bits(getattr(rows, field)[take])), (step, name)
        want = train_inputs(frames, got["frame_index"], **src, mask_index=got["mask_index"], bbox_xyxy=got["bbox_xyxy"], cam_K=got["K_no_aug"], sample_id=got["index"],
                            cfg=_cfg(), seed=SET_SEED0 + step, backgrounds=ts.backgrounds, in_hw=IN_HW, out_hw=OUT_HW, valid_th=VALID_TH, n_check=N_CHECK,
                            normalize=(MEAN, STD), geometry=got["geometry"])
        torch.cuda.synchronize()
        assert set(NAMES) <= set(got) and sorted(want) == sorted(NAMES)
        for name in NAMES:
            assert equal(got[name], want[name]), (step, name)
        assert np.array_equal(got["valid_cnt"].cpu().numpy(), cnt[take]) and int(got["valid_cnt"].min()) >= VALID_TH and not got["info"].any(), step
        assert not np.isin(got["index"].cpu().numpy(), EMPTY).any() and (got["sym_ck_pts2d"] >= 0).all(), step


def test_without_spares_the_empty_rows_come_back_untaken():
    ts, _, _, _ = resident("bytes", 0)
    rows, cnt, take, short = host_step(0, 0)
    assert short == 2 and sorted(rows.index[take < 0]) == sorted(EMPTY)  # step 0 of an epoch of six in batches of four: both blobs are primaries here
    got = ts.step_inputs(_word(SET_SEED0))
    torch.cuda.synchronize()
    assert np.array_equal(got["take"].cpu().numpy(), take) and got["shortfall"].cpu().tolist() == [2]
    gone = torch.from_numpy(take < 0)
    assert got["info"].cpu()[gone].tolist() == [-1, -1] and not got["info"].cpu()[~gone].any()
    for name in ("msk_vis", "msk_noc", "valid_cnt", "out_K", "in_affine", "index", "K_no_aug"):
        assert not got[name].cpu()[gone].any(), name
    assert (got["sym_ck_pts2d"].cpu()[~gone] >= 0).all() and int(got["valid_cnt"].cpu()[~gone].min()) >= VALID_TH


def test_step_inputs_replayed_over_two_steps_equals_the_eager_result():
    ts, _, _, _ = resident("rle", SPARE)
    word = _word(SET_SEED0)
    g, res = _capture(lambda: ts.step_inputs(word))
    names = NAMES + ("index", "obj_id", "scene_id", "im_id", "K_no_aug", "R_no_aug", "t_no_aug", "take", "shortfall")
    seen = []
    for step in (0, 1):
        g.replay()
        torch.cuda.synchronize()
        seen.append({k: res[k].cpu().clone() for k in names})
        eager = ts.step_inputs(SET_SEED0 + step)  # by value: a word of its own
        torch.cuda.synchronize()
        for name in names:
            assert equal(seen[-1][name], eager[name]), (step, name)
        word.add_(1)
    assert not torch.equal(seen[0]["index"], seen[1]["index"]) and not torch.equal(seen[0]["rgb_in"], seen[1]["rgb_in"])
