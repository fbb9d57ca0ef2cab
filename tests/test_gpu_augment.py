"""The augmentation launch on the device: every output EQUAL to the numpy oracle's (tests/augment_oracle.py) at the shapes of
tests/augment_cases.py -- every stage alone, every pair of neighbours and the reflected-halo chain per size, both compiled forms, the four
output types, refused rows, sample ids, batch order and a replayed graph."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_cases as cases, augment_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# every compiled form (the template arguments in the mangled name: output type, filtered) and the test of this file that launches it;
# tests/test_augment_oracle.py checks the table against the library's symbols
KERNEL_FORMS = {
    r"lc_augment_kernelILi0ELb1E": "test_filtered_form_equals_the_oracle",
    r"lc_augment_kernelILi0ELb0E": "test_pointwise_form_equals_the_oracle",
    r"lc_augment_kernelILi1ELb1E": "test_float_outputs_are_the_bytes_through_the_stated_fp32_operations",
    r"lc_augment_kernelILi1ELb0E": "test_float_outputs_are_the_bytes_through_the_stated_fp32_operations",
    r"lc_augment_kernelILi2ELb1E": "test_float_outputs_are_the_bytes_through_the_stated_fp32_operations",
    r"lc_augment_kernelILi2ELb0E": "test_float_outputs_are_the_bytes_through_the_stated_fp32_operations",
    r"lc_augment_kernelILi3ELb1E": "test_float_outputs_are_the_bytes_through_the_stated_fp32_operations",
    r"lc_augment_kernelILi3ELb0E": "test_float_outputs_are_the_bytes_through_the_stated_fp32_operations",
}


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


def _run(crops, params, lut, msk=None, bg=None, sample_id=None, device_params=False, **kw):
    from lc_amd import augment

    out, info = augment.augment(_dev(crops), _dev(params) if device_params else params.copy(), _dev(lut) if device_params else lut.copy(),
                                msk_in=None if msk is None else _dev(msk), backgrounds=None if bg is None else _dev(bg),
                                sample_id=None if sample_id is None else _dev(sample_id, torch.int32), **kw)
    return out.cpu(), info.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(sets, h, w, seed, pointwise=False):
    """One batch and its oracle result, computed once and shared."""
    crops, bg, msk, params, lut = cases.make_batch(sets, h, w, seed)
    want, info = oracle.augment(crops, params, lut, msk, bg, seed=cases.SEED, pointwise=pointwise)
    for a in (crops, bg, msk, params, lut, want, info):
        a.setflags(write=False)
    return crops, bg, msk, params, lut, want, info


@pytest.mark.parametrize("hw", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filtered_form_equals_the_oracle(hw):
    for i, sets in enumerate(cases.BATCHES):
        crops, bg, msk, params, lut, want, info = _case(sets, *hw, 10 + i)
        assert not info.any()
        got, ginfo = _run(crops, params, lut, msk, bg, seed=cases.SEED, dtype=torch.uint8, pointwise=False)
        bad = np.argwhere(got.numpy() != want)
        assert not len(bad), (hw, sets, len(bad), bad[:4].tolist())
        assert not ginfo.any()
        if sets == (cases.FILTER_A | cases.DROPOUT | cases.FILTER_B, 63, 0):  # the stages did something in the last tile's corner
            assert (want[0, :, -2:, -2:] != crops[0, :, -2:, -2:]).any()


@pytest.mark.parametrize("hw", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pointwise_form_equals_the_oracle(hw):
    for i, sets in enumerate(cases.POINTWISE_BATCHES):
        crops, bg, msk, params, lut, want, info = _case(sets, *hw, 30 + i, True)
        assert not info.any()
        for pointwise in (None, False):  # host params without a filter take the point-wise form on their own; the filtered form agrees
            got, ginfo = _run(crops, params, lut, msk, bg, seed=cases.SEED, dtype=torch.uint8, pointwise=pointwise)
            assert np.array_equal(got.numpy(), want) and not ginfo.any(), (hw, sets, pointwise)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_float_outputs_are_the_bytes_through_the_stated_fp32_operations(dtype):
    for hw, sets, seed, pointwise in (((33, 65), cases.BATCHES[4], 14, False), ((32, 32), cases.BATCHES[3], 13, False),
                                      ((33, 65), cases.POINTWISE_BATCHES[2], 32, True), ((32, 32), cases.POINTWISE_BATCHES[1], 31, True)):
        crops, bg, msk, params, lut, want, _ = _case(sets, *hw, seed, pointwise)
        for normalize in (None, (cases.MEAN, cases.STD)):
            got, _ = _run(crops, params, lut, msk, bg, seed=cases.SEED, dtype=dtype, normalize=normalize, pointwise=pointwise)
            assert got.dtype == dtype and torch.equal(got, oracle.finish(want, dtype, normalize)), (hw, pointwise, normalize is not None)


def test_all_stages_off_returns_the_crop():
    crops, _, _, lut = cases.make_inputs(40, 31, 2, 3)
    params = np.zeros((2, 64), np.int32)
    for pointwise in (True, False):
        got, info = _run(crops, params, lut, dtype=torch.uint8, pointwise=pointwise)
        assert np.array_equal(got.numpy(), crops) and not info.any()


def test_blend_clamps_and_rounds_the_mask():
    """Mask values that are no k / 1024: NaN and negatives read 0, anything from 1 up reads 1024, halves of a step go to the even k."""
    h, w = 8, 12
    crops, bg, _, lut = cases.make_inputs(h, w, 1, 4)
    vals = np.array([np.nan, -1.0, -0.0, 2.0, np.inf, -np.inf, 0.5 / 1024, 1.5 / 1024, 2.5 / 1024, 1023.5 / 1024, 1e-30, 0.37], np.float32)
    msk = np.tile(vals, (1, h, 1))
    params = np.zeros((1, 64), np.int32)
    params[0, 0], params[0, 1] = cases.SWITCH, 1
    want, _ = oracle.augment(crops, params, lut, msk, bg)
    assert np.array_equal(want[0, :, :, 0], bg[1, :, :, 0]) and np.array_equal(want[0, :, :, 3], crops[0, :, :, 3])
    for pointwise in (True, False):
        got, info = _run(crops, params, lut, msk, bg, dtype=torch.uint8, pointwise=pointwise)
        assert np.array_equal(got.numpy(), want) and not info.any()


def test_refused_rows_are_the_unchanged_crop():
    h, w = 33, 40
    rng = np.random.default_rng(5)
    crops, bg, msk, lut = cases.make_inputs(h, w, 12, 6)
    good = cases.make_params(63, rng, h, w)
    rows = [good.copy() for _ in range(12)]
    rows[1][0] = 64 | 63            # a bit above bit 5
    rows[2][57] = 1                 # a reserved word
    rows[3][7] = -1                 # a negative weight (and the sum is off)
    rows[3][8] += 1
    rows[4][40] += 1                # filter B sums to 65537
    rows[5][4] = 0                  # the grid
    rows[6][5] = w + 1
    rows[7][1] = cases.G            # the background
    rows[8][1] = -1
    rows[9][0], rows[9][7] = 63 & ~4, -5   # filter A is off: its words are not judged
    rows[10][0] = -2 ** 31
    params = np.stack(rows)
    want, winfo = oracle.augment(crops, params, lut, msk, bg, seed=3)
    assert winfo.tolist() == [0, -1, -1, -1, -1, -1, -1, -1, -1, 0, -1, 0]
    got, info = _run(crops, params, lut, msk, bg, seed=3, dtype=torch.uint8, device_params=True)
    assert info.tolist() == winfo.tolist() and np.array_equal(got.numpy(), want)
    assert all(np.array_equal(got[b].numpy(), crops[b]) for b in range(12) if winfo[b]) and not np.array_equal(got[0].numpy(), crops[0])
    gotf, info = _run(crops, params, lut, msk, bg, seed=3, dtype=torch.float16, device_params=True, normalize=(cases.MEAN, cases.STD))
    assert torch.equal(gotf, oracle.finish(want, torch.float16, (cases.MEAN, cases.STD)))
    # the switch without a mask or without backgrounds; a filter bit in a point-wise launch: judged by the kernel for device params
    for kw, pointwise in ((dict(msk=None, bg=bg), False), (dict(msk=msk, bg=None), False), (dict(msk=msk, bg=bg), True)):
        want, winfo = oracle.augment(crops, params, lut, kw["msk"], kw["bg"], seed=3, pointwise=pointwise)
        assert winfo[0] == winfo[11] == -1 and (pointwise or winfo[9] == -1)
        got, info = _run(crops, params, lut, seed=3, dtype=torch.uint8, device_params=True, pointwise=pointwise, **kw)
        assert info.tolist() == winfo.tolist() and np.array_equal(got.numpy(), want)


def test_sample_ids_and_batch_order():
    h, w = 31, 40
    sets = (63, cases.SALT | cases.DROPOUT, cases.FILTER_A | cases.DROPOUT | cases.FILTER_B, cases.SALT, 63)
    crops, bg, msk, params, lut = cases.make_batch(sets, h, w, 50)
    kw = dict(seed=cases.SEED, dtype=torch.uint8)
    none, _ = _run(crops, params, lut, msk, bg, **kw)
    rowwise, _ = _run(crops, params, lut, msk, bg, sample_id=np.arange(5), **kw)
    assert torch.equal(none, rowwise)  # NULL means row b is sample b
    sid = np.array([7, -3, 2 ** 31 - 1, 0, 7], dtype=np.int32)
    want, _ = oracle.augment(crops, params, lut, msk, bg, seed=cases.SEED, sample_id=sid)
    got, _ = _run(crops, params, lut, msk, bg, sample_id=sid, **kw)
    assert np.array_equal(got.numpy(), want) and not torch.equal(got, none)
    perm = np.array([3, 0, 4, 2, 1])  # the same rows in another order: the same bits
    again, _ = _run(crops[perm], params[perm], lut[perm], msk[perm], bg, sample_id=sid[perm], **kw)
    assert torch.equal(again, got[perm])
    other, _ = _run(crops, params, lut, msk, bg, sample_id=sid, seed=cases.SEED ^ (1 << 40), dtype=torch.uint8)
    assert not torch.equal(other, got)  # the high half of the seed is read
    empty, info = _run(crops[:0], params[:0], lut[:0], msk[:0], bg, **kw)
    assert tuple(empty.shape) == (0, 3, h, w) and tuple(info.shape) == (0,)


def test_graph_replay_on_refilled_params():
    from lc_amd import augment

    h, w = 40, 40
    batches = [cases.make_batch(sets, h, w, 60 + i) for i, sets in enumerate(((63, cases.FILTER_A, cases.SWITCH), (cases.FILTER_B | cases.LUT, 0, 63), (cases.DROPOUT, 63, 63)))]
    sids = [np.array(s, dtype=np.int32) for s in ((0, 1, 2), (9, 9, 4), (5, 1, 100))]
    crops, bg, msk, params, lut = batches[0]
    s_crops, s_bg, s_msk, s_params, s_lut, s_sid = _dev(crops), _dev(bg), _dev(msk), _dev(params), _dev(lut), _dev(sids[0])

    def call():
        return augment.augment(s_crops, s_params, s_lut, msk_in=s_msk, backgrounds=s_bg, seed=77, sample_id=s_sid, dtype=torch.float32)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, info = call()
    for (_, _, _, params2, lut2), sid2 in zip(batches[1:], sids[1:]):
        for dst, src in ((s_params, params2), (s_lut, lut2), (s_sid, sid2)):
            dst.copy_(_dev(src))
        g.replay()
        torch.cuda.synchronize()
        want, winfo = oracle.augment(crops, params2, lut2, msk, bg, seed=77, sample_id=sid2)
        assert torch.equal(out.cpu(), oracle.finish(want, torch.float32)) and info.cpu().tolist() == winfo.tolist()


def test_chain_from_the_warps_to_the_network_input():
    """crops.warp_affine (uint8) and maskcrop.mask_crops (msk_in) feed the launch as they are; the backgrounds are cut by the same warp."""
    from lc_amd import augment, crops as lc_crops, maskcrop

    rng = np.random.default_rng(8)
    frame = rng.integers(0, 256, (1, 48, 64, 3), dtype=np.uint8)
    mask = np.zeros((1, 48, 64), np.uint8)
    mask[0, 10:40, 20:50] = 1
    M, _ = lc_crops.affine_from_box((35.0, 25.0), 40.0, 0.3, (32, 32))
    Md = _dev(np.stack([M, M]))
    idx = _dev(np.zeros(2, np.int32))
    crop = lc_crops.warp_affine(_dev(frame), Md, (32, 32), frame_index=idx, dtype=torch.uint8)
    msk_in = maskcrop.mask_crops(_dev(mask), Md, (32, 32), mask_index=idx, n_check=0, want=("msk_vis",)).msk_vis
    bgM = augment.background_matrices(4, [0, 1], (48, 64), (32, 32))
    bgs = lc_crops.warp_affine(_dev(frame[:, ::-1].copy()), _dev(bgM), (32, 32), frame_index=idx, dtype=torch.uint8)
    params, lut = augment.draw(augment.AugmentConfig(switch_bg_prob=1.0, pixel_aug_prob=1.0, use_peper_salt=True, use_motion_blur=True), 4, [0, 1], 2, hw=(32, 32))
    assert (params[:, 0] & 1).all()
    out, info = augment.augment(crop, params, lut, msk_in=msk_in, backgrounds=bgs, seed=4, dtype=torch.uint8)
    want, _ = oracle.augment(crop.cpu().numpy(), params, lut, msk_in.cpu().numpy(), bgs.cpu().numpy(), seed=4)
    assert np.array_equal(out.cpu().numpy(), want) and not info.cpu().any()
