"""The augmentation with its rows drawn by the kernel (`lc_amd.augment.augment_drawn`): the rows against the host `draw` (everything but
the filter weights EQUAL; each Q16 weight within 1, non-negative, each set summing to 65536), the pixels against the numpy oracle and
against `augment` fed with the returned rows (bit for bit), a row as a function of (seed, sample id) alone, and a replayed graph that
draws anew when its seed word changes.  Shapes and inputs are those of tests/augment_cases.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import augment_cases as cases, augment_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B_ROWS = 67                       # more rows than a wavefront has lanes, and a multiple of nothing
SEED = 0x9E37_79B9_7F4A_7C15      # above 2^63: both halves in use, and the by-value upload has to wrap it into an int64
SEED2 = (1 << 32) + 12345
# sample ids with negatives, both ends of int32 and repeats (rows 5 / 40 and 0 / 66 are the same sample)
IDS = (np.arange(B_ROWS, dtype=np.int64) * 37 - 500)
IDS[1], IDS[2], IDS[3] = -1, -2 ** 31, 2 ** 31 - 1
IDS[40], IDS[66] = IDS[5], IDS[0]
IDS = IDS.astype(np.int32)
IDS.setflags(write=False)
G = cases.G

ALL_ON = dict(pixel_aug_prob=1.0, switch_bg_prob=1.0, use_peper_salt=True, use_motion_blur=True, use_invert=True)
CONFIGS = {"all_on": ALL_ON, "defaults": {}, "all_off": dict(pixel_aug_prob=0.0, switch_bg_prob=0.0),
           "defaults_with_switches": dict(use_peper_salt=True, use_motion_blur=True, use_invert=True)}


def _cfg(name):
    from lc_amd import augment

    return augment.AugmentConfig(**CONFIGS[name])


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(h, w, B, seed):
    crops, bg, msk, _ = cases.make_inputs(h, w, B, seed)
    for a in (crops, bg, msk):
        a.setflags(write=False)
    return crops, bg, msk


def _drawn(crops, cfg, seed, ids, msk=None, bg=None, **kw):
    from lc_amd import augment

    res = augment.augment_drawn(_dev(crops), cfg, seed=seed, sample_id=_dev(ids, torch.int32), msk_in=None if msk is None else _dev(msk),
                                backgrounds=None if bg is None else _dev(bg), return_rows=True, **kw)
    torch.cuda.synchronize()
    return res


def check_rows(params, lut, want_params, want_lut):
    """The contract of include/lc_amd_augment.h between drawn rows and `draw`'s.  -> the number of weights that differ (by one)."""
    params, want_params = params.astype(np.int64), want_params.astype(np.int64)
    exact = list(range(6)) + list(range(56, 64))
    bad = np.argwhere(params[:, exact] != want_params[:, exact])
    assert not len(bad), (len(bad), bad[:4].tolist(), params[bad[0][0], :6].tolist(), want_params[bad[0][0], :6].tolist())
    bad = np.argwhere(lut != want_lut)
    assert not len(bad), (len(bad), bad[:4].tolist())
    off = 0
    for bit, lo in ((4, 6), (16, 31)):
        on = (want_params[:, 0] & bit) != 0
        got, want = params[:, lo:lo + 25], want_params[:, lo:lo + 25]
        assert not got[~on].any() and not want[~on].any()
        d = np.abs(got[on] - want[on])
        print(f"filter bit {bit}: {int(on.sum())} rows, {int((d != 0).sum())} of {d.size} weights differ, the largest difference {int(d.max()) if d.size else 0}")
        assert (d <= 1).all(), (bit, int(d.max()), np.argwhere(d > 1)[:4].tolist())
        assert (got[on] >= 0).all() and (got[on].sum(axis=1) == 65536).all(), bit
        off += int((d != 0).sum())
    return off


@pytest.mark.parametrize("name", ["all_on", "defaults", "all_off", "defaults_with_switches"])
def test_rows_equal_the_host_draw(name):
    from lc_amd import augment

    h, w = 24, 40
    cfg = _cfg(name)
    crops, bg, msk = _inputs(h, w, B_ROWS, 70)
    for seed in (SEED, SEED2):
        want_params, want_lut = augment.draw(cfg, seed, IDS, G, hw=(h, w))
        _, info, params, lut = _drawn(crops, cfg, seed, IDS, msk, bg, dtype=torch.uint8)
        assert params.dtype == torch.int32 and tuple(params.shape) == (B_ROWS, 64) and lut.dtype == torch.uint8 and tuple(lut.shape) == (B_ROWS, 3, 256)
        check_rows(params.cpu().numpy(), lut.cpu().numpy(), want_params, want_lut)
        assert not info.cpu().any()
        bits = want_params[:, 0]
        if name == "all_on":  # the gates behind the two probabilities are all open; every stage occurs
            assert (bits & 1).all() and all((bits & b).any() for b in (2, 4, 8, 16, 32)) and len(set(want_params[:, 1])) == G
        if name == "all_off":  # identity rows
            assert not want_params.any() and (want_lut == np.arange(256, dtype=np.uint8)).all()
            assert not params.cpu().any() and (lut.cpu().numpy() == np.arange(256, dtype=np.uint8)).all()
    # without backgrounds no row switches, whatever the probability says
    want_params, want_lut = augment.draw(cfg, SEED, IDS, 0, hw=(h, w))
    _, info, params, lut = _drawn(crops, cfg, SEED, IDS, msk, None, dtype=torch.uint8)
    check_rows(params.cpu().numpy(), lut.cpu().numpy(), want_params, want_lut)
    assert not (params.cpu().numpy()[:, 0] & 1).any() and not info.cpu().any()


VARIANTS = (("u8", torch.uint8, False, True, True), ("f32", torch.float32, True, True, True), ("bf16", torch.bfloat16, True, True, True),
            ("u8_plain", torch.uint8, False, False, False), ("bf16_plain", torch.bfloat16, True, False, False),
            ("u8_backgrounds_without_mask", torch.uint8, False, False, True))


@pytest.mark.parametrize("hw", [(8, 8), (33, 65), (24, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["all_on", "defaults_with_switches", "switch_only"])
def test_pixels_are_exact_given_the_rows(hw, name):
    """`switch_only` rules the filters out (pixel_aug_prob = 0): the launch takes the point-wise form."""
    from lc_amd import augment

    h, w = hw
    B = 5
    cfg = augment.AugmentConfig(pixel_aug_prob=0.0, switch_bg_prob=1.0) if name == "switch_only" else _cfg(name)
    crops, bg, msk = _inputs(h, w, B, 71)
    ids = IDS[[0, 1, 2, 3, 5]]
    seen = 0
    for label, dtype, norm, with_msk, with_bg in VARIANTS:
        normalize = (cases.MEAN, cases.STD) if norm else None
        m, g = (msk if with_msk else None), (bg if with_bg else None)
        out, info, params, lut = _drawn(crops, cfg, SEED, ids, m, g, dtype=dtype, normalize=normalize)
        P, L = params.cpu().numpy(), lut.cpu().numpy()
        check_rows(P, L, *augment.draw(cfg, SEED, ids, G if with_bg else 0, hw=hw))
        want, winfo = oracle.augment(crops, P, L, m, g, seed=SEED, sample_id=ids, pointwise=name == "switch_only")
        assert info.cpu().tolist() == winfo.tolist(), (label, winfo.tolist())
        assert out.dtype == dtype and torch.equal(out.cpu(), oracle.finish(want, dtype, normalize)), (label, hw)
        if label == "u8_backgrounds_without_mask":  # a switch without a mask is drawn, written to the rows, and refused
            assert winfo.tolist() == (-(P[:, 0] & 1)).tolist() and np.array_equal(want[winfo == -1], crops[winfo == -1])
            assert (winfo == -1).all() or cfg.switch_bg_prob < 1.0
        else:
            assert not winfo.any()
        again, ainfo = augment.augment(_dev(crops), params, lut, msk_in=None if m is None else _dev(m), backgrounds=None if g is None else _dev(g), seed=SEED,
                                       sample_id=_dev(ids, torch.int32), dtype=dtype, normalize=normalize, pointwise=name == "switch_only")
        assert torch.equal(again, out) and torch.equal(ainfo, info), label
        seen |= int(np.bitwise_or.reduce(P[:, 0][winfo == 0])) if (winfo == 0).any() else 0
    if name == "all_on":
        assert seen == 63  # every stage ran in some row
    if name == "switch_only":
        assert seen == 1


def test_a_row_is_its_samples():
    """The same (seed, sample id) in batches of 1, 5 and 67, at different places: the same row and the same pixels."""
    from lc_amd import augment

    h, w = 33, 40
    cfg = _cfg("all_on")
    crops, bg, msk = _inputs(h, w, B_ROWS, 72)
    sid = np.int32(-77)
    got = []
    for B, at in ((1, 0), (5, 3), (B_ROWS, 50)):
        c, m, ids = crops[:B].copy(), msk[:B].copy(), IDS[:B].copy()
        c[at], m[at], ids[at] = crops[9], msk[9], sid
        out, info, params, lut = _drawn(c, cfg, SEED, ids, m, bg, dtype=torch.uint8)
        assert not info.cpu().any()
        got.append((out[at].cpu(), params[at].cpu(), lut[at].cpu()))
    for other in got[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[0], other))
    want_params, want_lut = augment.draw(cfg, SEED, [sid], G, hw=(h, w))
    check_rows(got[0][1].numpy()[None], got[0][2].numpy()[None], want_params, want_lut)
    assert not np.array_equal(got[0][0].numpy(), crops[9])


def test_seed_words_of_either_type_and_by_value_agree():
    h, w = 8, 8
    cfg = _cfg("all_on")
    crops, bg, msk = _inputs(h, w, 5, 73)
    ids = IDS[:5]
    by_value = _drawn(crops, cfg, SEED, ids, msk, bg, dtype=torch.uint8)
    for word in (torch.from_numpy(np.array([SEED], dtype=np.uint64)).to(DEV), torch.from_numpy(np.array([SEED], dtype=np.uint64).view(np.int64)).to(DEV)):
        got = _drawn(crops, cfg, word, ids, msk, bg, dtype=torch.uint8)
        assert all(torch.equal(a, b) for a, b in zip(got, by_value)), word.dtype
    other = _drawn(crops, cfg, SEED ^ (1 << 40), ids, msk, bg, dtype=torch.uint8)
    assert not torch.equal(other[2], by_value[2])  # the high half of the word is read


def test_the_graph_draws_anew_when_its_seed_word_changes():
    from lc_amd import augment

    h, w = 40, 40
    cfg = _cfg("all_on")
    crops, bg, msk = _inputs(h, w, 5, 74)
    ids = IDS[[0, 1, 2, 3, 5]]
    s_crops, s_bg, s_msk, s_ids = _dev(crops), _dev(bg), _dev(msk), _dev(ids, torch.int32)
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    norm = (cases.MEAN, cases.STD)

    def call(seed):
        return augment.augment_drawn(s_crops, cfg, seed=seed, sample_id=s_ids, msk_in=s_msk, backgrounds=s_bg, dtype=torch.float32, normalize=norm, return_rows=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(word)  # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = call(word)
    s1, s2 = SEED2, SEED2 + 1
    replays = []
    for s in (s1, s2, s1):
        word.fill_(s)
        g.replay()
        torch.cuda.synchronize()
        replays.append([t.cpu().clone() for t in res])
        eager = call(s)  # by value: a word of its own
        torch.cuda.synchronize()
        assert all(torch.equal(a, b.cpu()) for a, b in zip(replays[-1], eager)), s
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[0][2], replays[1][2])
    assert all(torch.equal(a, b) for a, b in zip(replays[0], replays[2]))
    # a whole-number seed is written by a fill: the call is capturable as it is
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        res2 = call(s2)
    g2.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), b) for a, b in zip(res2, replays[1]))


def test_eight_kernels_without_scratch_within_16_kb_of_lds():
    """The pin of tests/test_augment_oracle.py once more, beside the code path that added fp64 arithmetic to every kernel."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import augment, build

    augment.load()
    res = kernel_resources(build.AUGMENT.so_path)
    assert len(res) == 8 and all("lc_augment_" in n for n in res), sorted(res)
    for d in res.values():
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (d["name"], "scratch")
        assert d.get("group_segment_fixed_size", 0) <= 16 * 1024, d["name"]
