"""The zoom-in crops (lc_amd.crops, lc_amd/csrc/crop/lc_crop.hip) on the GPU against the integer oracle of tests/crops_oracle.py on the
cases of tests/crops_cases.py.  The contract is integer arithmetic, so everything is compared bit for bit: the bytes, the fp32 output
stage, the 16-bit outputs against the oracle's fp32 rounded once, and `info`; a row's bytes do not depend on its place in the batch,
on how its frame is named, or on eager against graph replay; nothing outside the rows is written."""
import os

import numpy as np
import pytest
import torch

from tests import crops_cases as cc
from tests import crops_oracle as co

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xA5
BITS = {torch.uint8: torch.uint8, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(BITS[t.dtype]).cpu().numpy()


def _warp_guarded(frames, M, hw, dtype, **kw):
    """warp_affine into rows 1..B of a sentinel-filled (B + 2) buffer; asserts the guard rows, returns (rows, info)."""
    from lc_amd.crops import warp_affine

    B, C = M.shape[0], frames.shape[3]
    buf = torch.empty(B + 2, C, *hw, device=DEV, dtype=dtype)
    buf.view(torch.uint8).fill_(SENTINEL)
    info = torch.full((B + 2,), 77, device=DEV, dtype=torch.int32)
    out = warp_affine(frames, M, hw, dtype=dtype, out=buf[1:B + 1], info=info[1:B + 1], **kw)
    assert out.data_ptr() == buf[1].data_ptr()
    guards = buf[[0, B + 1]].view(torch.uint8)
    assert bool((guards == SENTINEL).all()), "a guard row was written"
    assert info[[0, B + 1]].tolist() == [77, 77]
    return out, info[1:B + 1]


def _norm(C):
    return tuple(a[:C] for a in cc.NORMALIZE)


@pytest.mark.parametrize("interp", [co.LINEAR, co.NEAREST])
@pytest.mark.parametrize("out_hw", cc.OUT_SIZES)
@pytest.mark.parametrize("C", [3, 1])
def test_every_case_equals_the_oracle_bit_for_bit(C, out_hw, interp):
    frames, idx = _dev(cc.FRAMES[C]), _dev(cc.FRAME_INDEX)
    for names, M, ref, ref_info in cc.reference(C, out_hw, interp):
        Md = _dev(M)
        got, info = _warp_guarded(frames, Md, out_hw, torch.uint8, frame_index=idx, interp=interp)
        bad = [(n, int((g != r).sum())) for n, g, r in zip(names, got.cpu().numpy(), ref) if (g != r).any()]
        assert not bad, f"bytes differ (case, count): {bad}"
        assert np.array_equal(info.cpu().numpy(), ref_info), names
        for normalize in (None, _norm(C)):
            want = co.finish(ref, normalize)
            got, info = _warp_guarded(frames, Md, out_hw, torch.float32, frame_index=idx, interp=interp, normalize=normalize)
            assert np.array_equal(_bits(got), want.view(np.int32)), (names, normalize)
            assert np.array_equal(info.cpu().numpy(), ref_info)
            for dtype in (torch.float16, torch.bfloat16):
                got, _ = _warp_guarded(frames, Md, out_hw, dtype, frame_index=idx, interp=interp, normalize=normalize)
                assert np.array_equal(_bits(got), _bits(torch.from_numpy(want).to(dtype))), (names, dtype, normalize)


@pytest.mark.parametrize("interp", [co.LINEAR, co.NEAREST])
def test_a_rows_bytes_do_not_depend_on_the_batch(interp):
    from lc_amd.crops import warp_affine

    C, hw = 3, (24, 40)
    frames, idx = _dev(cc.FRAMES[C]), _dev(cc.FRAME_INDEX)
    perm = np.array([3, 0, 4, 1, 2])
    for names, M, ref, _ in cc.reference(C, hw, interp):
        Md = _dev(M)
        for b in range(cc.B):  # the row run alone
            one = warp_affine(frames, Md[b:b + 1].contiguous(), hw, frame_index=idx[b:b + 1].contiguous(), interp=interp, dtype=torch.uint8)
            assert np.array_equal(one[0].cpu().numpy(), ref[b]), names[b]
        got = warp_affine(frames, _dev(M[perm]), hw, frame_index=_dev(cc.FRAME_INDEX[perm]), interp=interp, dtype=torch.uint8)
        assert np.array_equal(got.cpu().numpy(), ref[perm]), names
        # frame_index=None reads frame b: the same rows with their frames gathered in batch order
        gathered = _dev(cc.FRAMES[C][cc.FRAME_INDEX])
        got = warp_affine(gathered, Md, hw, interp=interp, dtype=torch.uint8)
        assert np.array_equal(got.cpu().numpy(), ref), names


def test_graph_replay_equals_eager():
    from lc_amd.crops import warp_affine

    C, hw = 3, (24, 40)
    frames, idx = _dev(cc.FRAMES[C]), _dev(cc.FRAME_INDEX)
    names, M, ref, ref_info = cc.reference(C, hw, co.LINEAR)[0]
    Md = _dev(M)
    out = torch.zeros(cc.B, C, *hw, device=DEV, dtype=torch.float32)
    info = torch.zeros(cc.B, device=DEV, dtype=torch.int32)
    eager = warp_affine(frames, Md, hw, frame_index=idx, normalize=_norm(C)).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        warp_affine(frames, Md, hw, frame_index=idx, normalize=_norm(C), out=out, info=info)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(eager)) and np.array_equal(_bits(out), co.finish(ref, _norm(C)).view(np.int32))
    Md.copy_(_dev(cc.reference(C, hw, co.LINEAR)[1][1]))  # a replay reads the matrices that are there now
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), co.finish(cc.reference(C, hw, co.LINEAR)[1][2], _norm(C)).view(np.int32))


def test_bad_frame_index_and_empty_batch():
    from lc_amd.crops import warp_affine

    frames = _dev(cc.FRAMES[3])
    M = _dev(np.stack([dict(cc.CASES)["identity"]] * 4))
    idx = torch.tensor([0, 2, -1, 1], dtype=torch.int32, device=DEV)
    got, info = _warp_guarded(frames, M, (16, 16), torch.uint8, frame_index=idx)
    ref, ref_info = co.warp(cc.FRAMES[3], M.cpu().numpy(), (16, 16), idx.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), ref) and info.tolist() == ref_info.tolist() == [0, -1, -1, 0]
    got, info = _warp_guarded(frames, M, (16, 16), torch.uint8)  # frame_index=None with more rows than frames
    assert info.tolist() == [0, 0, -1, -1] and not got[2:].any()
    empty = warp_affine(frames, M[:0].contiguous(), (16, 16))
    assert tuple(empty.shape) == (0, 3, 16, 16)


def test_working_shape_four_crops_of_256_from_480x640():
    from lc_amd.crops import affine_from_box, warp_affine

    frame = cc.make_frames(3, n=1, hw=(480, 640), seed=5)
    boxes = (((320.0, 240.0), 150.0, 0.0), ((40.5, 30.25), 90.0, 0.0), ((600.0, 470.0), 333.0, 0.0), ((200.0, 100.0), 64.0, 0.7))
    M = np.stack([affine_from_box(c, s, r, (256, 256))[0] for c, s, r in boxes])
    idx = np.zeros(4, dtype=np.int32)
    ref, ref_info = co.warp(frame, M, (256, 256), idx)
    got, info = _warp_guarded(_dev(frame), _dev(M), (256, 256), torch.uint8, frame_index=_dev(idx))
    assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(info.cpu().numpy(), ref_info) and ref.any()
    want = co.finish(ref, cc.NORMALIZE)
    got, _ = _warp_guarded(_dev(frame), _dev(M), (256, 256), torch.bfloat16, frame_index=_dev(idx), normalize=cc.NORMALIZE)
    assert np.array_equal(_bits(got), _bits(torch.from_numpy(want).to(torch.bfloat16)))


def _warp_offset(frames, M, hw, dtype, **kw):
    """warp_affine into a contiguous view that starts ONE element into a sentinel-filled buffer: the pointer is aligned to the element
    and to no four of them, so the launcher stores element by element at any w.  Asserts the elements around the view, returns the rows."""
    from lc_amd.crops import warp_affine

    n = M.shape[0] * frames.shape[3] * hw[0] * hw[1]
    flat = torch.empty(n + 9, device=DEV, dtype=dtype)
    flat.view(torch.uint8).fill_(SENTINEL)
    view = flat[1:1 + n].view(M.shape[0], frames.shape[3], *hw)
    assert view.is_contiguous() and view.data_ptr() % (4 * flat.element_size()) == flat.element_size()
    out = warp_affine(frames, M, hw, dtype=dtype, out=view, **kw)
    assert out.data_ptr() == view.data_ptr()
    guards = torch.cat((flat[:1], flat[1 + n:])).view(torch.uint8)
    assert bool((guards == SENTINEL).all()), "an element outside the view was written"
    return out


@pytest.mark.parametrize("interp", [co.LINEAR, co.NEAREST])
@pytest.mark.parametrize("out_hw", cc.WIDE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", [3, 1])
def test_wide_crops_equal_the_oracle_in_every_thread_layout(C, out_hw, interp):
    """64, 128 and 256 threads along x, a second trip of the quad loop and the workload's 256 x 256 (tests/crops_cases.WIDE_SIZES), each
    with four-pixel stores where w allows them and again element by element at an output pointer one element off: the same bytes."""
    frames, idx = _dev(cc.FRAMES[C]), _dev(cc.WIDE_FRAME_INDEX)
    M, ref, ref_info = cc.wide_reference(C, out_hw, interp)
    Md = _dev(M)
    got, info = _warp_guarded(frames, Md, out_hw, torch.uint8, frame_index=idx, interp=interp)
    assert got.data_ptr() % 4 == 0 or out_hw[1] % 4, "the guarded rows were meant to take the four-pixel stores"
    assert np.array_equal(got.cpu().numpy(), ref), int((got.cpu().numpy() != ref).sum())
    assert np.array_equal(info.cpu().numpy(), ref_info)
    off = _warp_offset(frames, Md, out_hw, torch.uint8, frame_index=idx, interp=interp)
    assert np.array_equal(off.cpu().numpy(), ref), int((off.cpu().numpy() != ref).sum())
    want = co.finish(ref, _norm(C))
    for dtype in (torch.float32, torch.float16):
        want_bits = _bits(torch.from_numpy(want).to(dtype))
        got, _ = _warp_guarded(frames, Md, out_hw, dtype, frame_index=idx, interp=interp, normalize=_norm(C))
        assert np.array_equal(_bits(got), want_bits), dtype
        off = _warp_offset(frames, Md, out_hw, dtype, frame_index=idx, interp=interp, normalize=_norm(C))
        assert np.array_equal(_bits(off), want_bits), dtype


def test_finish_blob_gives_the_reference_loaders_rgb_in():
    """The stored blobs of the unmodified reference loader (tests/golden/crops_item.npz, whose warp is the oracle's): collated, moved and
    finished on the device they hold the rgb_in the reference's `.to(float32).div(255)` of the oracle's bytes gives, and not the stand-ins."""
    from torch.utils.data.dataloader import default_collate

    from lc_amd.crops import finish_blob

    z = np.load(os.path.join(GOLDEN, "crops_item.npz"))
    n, (w, h) = int(z["n_items"]), z["net_input_wh"]
    items = [{"rgb_full": z["frame"], "in_affine": z[f"call{i}_in_M"], "obj_id": int(z[f"item{i}_obj_id"])} for i in range(n)]
    batch = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in default_collate(items).items()}
    out = finish_blob(batch, net_input_hw=(int(h), int(w)))
    assert set(out) == {"rgb_in", "obj_id"} and out["rgb_in"].dtype == torch.float32 and tuple(out["rgb_in"].shape) == (n, 3, int(h), int(w))
    for i in range(n):
        want = torch.from_numpy(co.warp_one(z["frame"], z[f"call{i}_in_M"], (int(h), int(w)))).permute(2, 0, 1).to(torch.float32).div(255)
        assert np.array_equal(_bits(out["rgb_in"][i]), want.contiguous().numpy().view(np.int32))
        assert np.array_equal(want.numpy(), z[f"item{i}_rgb_in"])  # and that is what the reference loader delivered
    assert finish_blob({"rgb_in": 1}) == {"rgb_in": 1}  # a batch of the reference's own loader passes through
