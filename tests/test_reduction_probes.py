"""The exact probes of tests/reduction_probes.py, proven without a GPU: every pattern's expected value is what the plain float64 torch
formula gives on the pattern's tensors, and the critical-position sets hold the ends and both sides of every edge -- against numbers
written out by hand from the launchers (lc_clip.hip grid_for_sqnorm, lc_dense_aux.hip launch_dense_aux_fwd / launch_xyz_bin_loss_fwd,
lc_dense_lse.h lse_share_loop)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import reduction_probes as rp


def _has(pos, **want):
    for label, i in want.items():
        assert pos.get(label.replace("_m", "-").replace("_p", "+")) == i, (label, i, dict(pos))


# ---- positions against hand-written numbers --------------------------------------------------------------------------------------------
def test_sqnorm_positions_by_hand():
    assert [rp.sqnorm_grid(n) for n in (1, 8192, 8193, 16384, 16385, 57344, 512 * 8192, 512 * 8192 + 8197)] == [1, 1, 2, 2, 3, 7, 512, 512]
    # 8193 elements: grid 2, stride 512 requests, 2048 requests = exactly one round of four slots, one tail element
    p = rp.sqnorm_positions(8193)
    _has(p, first=0, last=8192, group_m=3, group_p=4, tail_m=8191, tail_p=8192, tail0=8192, last_group=8188, slot1_m=2047, slot1_p=2048,
         slot2_m=4095, slot2_p=4096, slot3_m=6143, slot3_p=6144, slot4_m=8191, slot4_p=8192, wg_m=1023, wg_p=1024, wg_last=1024, wg_last_end=2047)
    assert "slot5+" not in p
    # the cap + 8197: grid 512, stride 131072 requests, 1050625 requests = two rounds and 2049 requests of a third, one tail element
    n = 512 * 8192 + 8197
    p = rp.sqnorm_positions(n)
    _has(p, last=4202500, tail_m=4202499, tail_p=4202500, last_group=4202496, slot1_m=524287, slot1_p=524288, slot4_m=2097151, slot4_p=2097152,
         slot8_m=4194303, slot8_p=4194304, wg255=261120, wg256=262144, wg_last=523264, wg_last_end=524287)
    assert "slot9+" not in p and len(p.pick(48)) <= 48 and {0, n - 1, 4194303, 4194304} <= set(p.pick(48))
    # the same 8193 elements from a view off the 16-byte boundary: no requests of four, element e belongs to thread e % 512
    p = rp.sqnorm_positions(8193, vec=False)
    _has(p, first=0, last=8192, slot1_m=511, slot1_p=512, slot16_m=8191, slot16_p=8192, wg_m=255, wg_p=256, wg_last=256, wg_last_end=511)
    assert "group+" not in p and "slot17+" not in p
    # every listed size: the ends, and every position inside the tensor
    for n in rp.sq_sizes():
        for vec in (True, False):
            q = rp.sqnorm_positions(n, vec).pick()
            assert {0, n - 1} <= set(q) and all(0 <= i < n for i in q) and len(set(q)) == len(q)
    s = rp.sq_sizes()
    assert {1, 3, 4, 5, 8191, 8192, 8193, 2047, 2049, 8189, 8195, 7167, 7169, 28672, 28675, 10240, 12288, 14336, 16384, 50176, 57344, 4194300, 4194304, 4202501} <= set(s)
    for g in (1, 2, 7, 512):
        assert {n % 4 for n in s if rp.sqnorm_grid(n) == g} == {0, 1, 2, 3}, g


def test_dense_aux_positions_by_hand():
    assert [rp.aux_geometry(B, H * W) for B, H, W in rp.AUX_SHAPES] == [(1, 2, 512, 1173), (4, 5, 1280, 1280), (4, 272, 69632, 69632),
                                                                       (4, 1024, 262144, 266240), (1, 266, 68096, 271803)]
    p = rp.aux_positions(3, 17 * 23)  # one pixel per request, two workgroups, three trips
    _has(p, first=0, last=1172, sample1_m=390, sample1_p=391, sample2_m=781, sample2_p=782, wg_m=255, wg_p=256, wrap1_m=511, wrap1_p=512,
         wrap2_m=1023, wrap2_p=1024, wg_last=256, wg_last_end=511)
    assert "wrap3+" not in p
    p = rp.aux_positions(65, 128 * 128)  # the capped grid: requests 262144 .. 266239 are second requests of the first 4096 threads
    _has(p, first=0, last=1064959, sample1_m=16383, sample1_p=16384, sample64_m=1048575, sample64_p=1048576, group_m=3, group_p=4,
         wrap1_m=1048575, wrap1_p=1048576, wg_m=1023, wg_p=1024, wg255=261120, wg256=262144, wg_last=1047552, wg_last_end=1048575, last_request=1064956)
    p = rp.aux_positions(17, 128 * 128)  # 272 workgroups: the last arriver's loop takes partials 0 .. 255, then 256 .. 271
    _has(p, wg255=261120, wg256=262144, wg_last=277504, wg_last_end=278527)
    for B, H, W in rp.AUX_SHAPES:
        q = rp.aux_positions(B, H * W).pick(64)
        assert {0, B * H * W - 1, H * W - 1, H * W} <= set(q) and all(0 <= i < B * H * W for i in q)


def test_code_loss_geometry_and_positions_by_hand():
    shapes = rp.BIN_SHAPES + [rp.BIN_TRAINING_SHAPE]
    assert [rp.bin_geometry(B, C, H * W) for B, C, H, W in shapes] == [(True, 2, 6, 6), (True, 1, 40, 32), (True, 1, 5, 5), (True, 1, 2, 2),
                                                                      (False, 0, 1, 1), (True, 4, 128, 24)]
    p = rp.bin_pixels(3, 2, 72 * 72)  # 1296 requests: a full slab and a partial one
    _has(p, first=0, last=5183, group_m=3, group_p=4, slab1_m=4095, slab1_p=4096, last_request=5180, wave_m=255, wave_p=256)
    assert rp.bin_samples(40, 2, 64 * 64) == [0, 1, 31, 32, 39] and rp.bin_samples(3, 2, 72 * 72) == [0, 1, 2] and rp.bin_channels(128) == [0, 1, 127]
    q = rp.bin_positions(3, 21, 37 * 29)  # the element-wise walk: 3219 pixels in trips of 1024, samples of 1073
    assert {(0, 0), (2, 1072), (0, 1072), (1, 0), (1, 1072), (2, 0), (0, 1023), (0, 1024), (1, 974), (1, 975), (2, 925), (2, 926)} <= set(q)
    q = rp.bin_positions(40, 2, 64 * 64)
    assert {(32, 0), (31, 4095), (39, 4095), (0, 4), (1, 3)} <= set(q)


def test_lse_positions_by_hand():
    p = rp.lse_positions(2 * 64 * 64)  # 2048 groups: exactly one round of block_lse
    _has(p, first=0, last=8191, channel_m=4095, channel_p=4096, slot1_m=2047, slot1_p=2048, slot2_m=4095, slot2_p=4096, slot3_m=6143, slot3_p=6144,
         slot4_m=8191, tail_m=8191, last_group=8188, part2_m=1023, part2_p=1024, part4_m=511, part4_p=512, part8_m=255, part8_p=256)
    assert "slot4+" not in p and "tail0" not in p
    p = rp.lse_positions(2 * 9 * 7)  # 31 groups and a two-element tail
    _has(p, first=0, last=125, channel_m=62, channel_p=63, tail_m=123, tail_p=124, tail0=124, tail1=125, last_group=120)
    assert "slot1+" not in p
    p = rp.lse_positions(2 * 45 * 47)  # 1057 groups: slot 2 holds 33 of them; two-element tail
    _has(p, last=4229, slot1_m=2047, slot1_p=2048, slot2_m=4095, slot2_p=4096, tail_m=4227, tail_p=4228, tail1=4229)
    assert "slot3+" not in p and (2 * 45 * 47) % 4 == 2  # the second sample starts off a 16-byte boundary
    p = rp.lse_positions(2 * 128 * 128)
    _has(p, slot4_m=8191, slot4_p=8192, slot8_m=16383, slot8_p=16384, slot16_m=32767)


# ---- expectations against the float64 torch formulas ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_sq_patterns_equal_the_float64_sum(dtype):
    for n in rp.sq_sizes():
        hots = ["all", ("random", n)] + rp.sqnorm_positions(n).pick(6) + rp.sqnorm_positions(n, vec=False).pick(4)
        for hot in hots if n < 100000 else hots[:4]:
            x, want = rp.sq_pattern(n, hot, dtype)
            assert float(x.double().square().sum()) == want and want < 2 ** 24


def test_sq_pattern_through_the_cpu_stand_in():
    from tests import cpu_backend

    parts, want = zip(*(rp.sq_pattern(n, hot) for n, hot in ((8193, ("random", 1)), (5, "all"), (8197, 8192))))
    sq, snap = cpu_backend._launch_sqnorm(list(parts), None, torch.tensor(-1.0))
    assert float(sq) == sum(want) and float(snap) == -1.0


def _aux_formulas(t, seg_type):
    from lc_amd.losses import Loss_seg_L1

    seg_fn = F.binary_cross_entropy_with_logits if seg_type == "bce" else Loss_seg_L1()
    vis = t["vis"][:, None].double()
    return torch.stack([F.l1_loss(t["xyz"].double() * t["msk_noc"][:, None], t["tgt"].double()), seg_fn(t["seg"].double(), vis, reduction="mean"),
                        seg_fn(t["wl"].double(), vis.expand_as(t["wl"]), reduction="mean")])


@pytest.mark.parametrize("seg_type", ["bce", "l1"])
@pytest.mark.parametrize("B,H,W", rp.AUX_SHAPES)
def test_aux_patterns_equal_the_float64_formulas(B, H, W, seg_type):
    n = B * H * W
    pos = rp.aux_positions(B, H * W).pick(3)

    def one(shape, i, c=None):
        m = torch.zeros(shape, dtype=torch.bool)
        b, px = divmod(i, H * W)
        if c is None:
            m.view(B, -1)[b, px] = True
        else:
            m.view(B, -1, H * W)[b, c, px] = True
        return m

    cases = [dict(vis_hot=torch.ones(B, H, W, dtype=torch.bool), x_hot=torch.ones(B, 3, H, W, dtype=torch.bool)),
             dict(vis_hot=torch.ones(B, H, W, dtype=torch.bool), mask_hot=torch.ones(B, H, W, dtype=torch.bool)),
             dict(vis_hot=rp.random_hot((B, H, W), 1), x_hot=rp.random_hot((B, 3, H, W), 2), w_hot=rp.random_hot((B, 2, H, W), 3)),
             dict(mask_hot=rp.random_hot((B, H, W), 4), w_hot=rp.random_hot((B, 2, H, W), 5)), dict()]
    for k, i in enumerate(pos):
        cases.append(dict(vis_hot=one((B, H, W), i), x_hot=one((B, 3, H, W), i, k % 3)))
        cases.append(dict(mask_hot=one((B, H, W), i), w_hot=one((B, 2, H, W), i, k % 2)))
    for dtype in (torch.float32, torch.float16, torch.bfloat16) if n < 100000 else (torch.float32,):
        for case in cases:
            t = rp.aux_inputs(B, H, W, dtype=dtype, **case)
            ks = rp.aux_counts(B, H, W, **case)
            got, want = _aux_formulas(t, seg_type), rp.aux_expected(*ks, n, seg_type)
            per = rp.BIG if seg_type == "bce" else 1.0
            exact = torch.tensor([ks[0] / (3.0 * n), per * ks[1] / n, per * ks[2] / (2.0 * n)], dtype=torch.float64)
            # (a cold BCE term is log1p(exp(-100)) = 3.7e-44 in float64 and nothing at all in float32)
            assert torch.allclose(got, exact, rtol=1e-12, atol=1e-40) and torch.equal(exact.float(), want), (case.keys(), got, want)
    assert rp.aux_counts(B, H, W, **cases[0]) == (3 * n, n, 2 * n) and rp.aux_counts(B, H, W, **cases[4]) == (0, 0, 0)


@pytest.mark.parametrize("B,C,H,W", rp.BIN_SHAPES + [rp.BIN_TRAINING_SHAPE])
def test_code_loss_patterns_equal_the_torch_count_lines(B, C, H, W):
    from lc_amd.losses import Loss_xyz_bin

    n = B * H * W
    b, px = rp.bin_positions(B, C, H * W)[-1]
    one_err = torch.zeros(B, C, H, W, dtype=torch.bool)
    one_err.view(B, C, -1)[b, C - 1, px] = True
    one_inv = torch.zeros(B, H, W, dtype=torch.bool)
    one_inv.view(B, -1)[b, px] = True
    full = torch.ones(B, C, H, W, dtype=torch.bool)
    cases = [dict(err_hot=full), dict(err_hot=rp.random_hot((B, C, H, W), 6)), dict(err_hot=rp.random_hot((B, C, H, W), 7), invis_hot=rp.random_hot((B, H, W), 8)),
             dict(err_hot=one_err), dict(err_hot=full, invis_hot=one_inv), dict(err_hot=one_err, invis_hot=one_inv)]
    for case in cases if n * C < 1 << 22 else cases[1:3]:
        logits, bits, vis = rp.bin_inputs(B, C, H, W, **case)
        want = rp.bin_counts(B, C, H, W, **case)
        # Loss_xyz_bin's count lines (losses.py:203-204)
        msk_hard = vis > 0
        hamm = (logits > 0).logical_xor(bits.to(torch.bool)).logical_and(msk_hard)
        assert want.dtype == torch.int64 and torch.equal(want, torch.cat((hamm.sum([0, 2, 3]), msk_hard.sum().reshape(1))))
        if "invis_hot" not in case:
            raw = F.binary_cross_entropy_with_logits(logits.double() * msk_hard, bits.double(), reduction="none").mean([0, 2, 3])
            assert torch.allclose(raw, rp.BIG * want[:-1].double() / n, rtol=1e-12, atol=1e-40)  # (cold terms: 3.7e-44 in float64)
            assert torch.equal((rp.BIG * want[:-1].double() / n).float(), rp.bin_bce_mean(want, n))
        if n * C < 1 << 22:  # one step of the module's torch formulas (float32 on the CPU) from a fresh histogram
            fn = Loss_xyz_bin(C)
            fn(logits, bits, vis)
            assert torch.equal(fn.histogram, rp.bin_histogram_step(want, fn.momentum))
    assert torch.equal(rp.bin_counts(B, C, H, W, err_hot=one_err, invis_hot=one_inv)[:-1], torch.zeros(C, dtype=torch.int64))  # an error nobody sees


@pytest.mark.parametrize("B,H,W,sample", rp.LSE_SHAPES)
def test_lse_patterns_equal_logsumexp(B, H, W, sample):
    from oracle import dense_oracle

    n = 2 * H * W
    pos = rp.lse_positions(n).pick()
    for k in range(0, len(pos), 5):
        spikes = [pos[(k + b) % len(pos)] for b in range(B)]
        wl = rp.lse_inputs(B, H, W, spikes, torch.float64)
        lse = torch.logsumexp(wl.view(B, -1), -1)
        assert torch.allclose(lse, torch.full((B,), math.log(n - 1 + math.exp(rp.SPIKE)), dtype=torch.float64), rtol=1e-14)
        _, w, _ = dense_oracle.dense_front_end(None, wl, torch.ones(B, dtype=torch.float64), None, 1, (0, 0))
        flat = w.mT.reshape(B, -1)  # (B, N, 2) rows back to the (2, H, W) order
        for b in range(B):
            assert abs(float(flat[b, spikes[b]]) * (n - 1 + math.exp(rp.SPIKE)) / math.exp(rp.SPIKE) - 1) < 1e-12
            assert abs(float(flat[b].sum()) - 1) < 1e-12
    _, w, _ = dense_oracle.dense_front_end(None, rp.lse_inputs(B, H, W, None, torch.float64), torch.ones(B, dtype=torch.float64), None, sample, (0, 0))
    assert torch.allclose(w, torch.full_like(w, 1.0 / n), rtol=1e-14)
    assert 1.0 / (2 * H * W) >= 3e-5 / 2 and 1.0 / n >= 3e-5  # one element more or less under uniform logits moves every weight by 1 / n


def test_a_lost_or_doubled_request_is_far_above_the_allowance():
    """One-hot probes: the output vanishes or doubles -- relative change 1 against 0 or 1 ulp (2^-23): more than 8e6 allowances everywhere.
    Random-hot probes of the exact integer outputs (sum of squares, code-loss counts): allowance 0.  Random-hot probes of the 1-ulp outputs: 4 / n
    of the output against 2^-23 -- thousands of allowances at the small shapes, 30 to 120 at the three large ones, which the one-hot sweeps cover."""
    for B, H, W in rp.AUX_SHAPES:
        one, rnd, allow = rp.bite(B * H * W, 1)
        assert one / allow > 8e6 and rnd / allow > 30
    assert [round(rp.bite(B * H * W, 1)[1] / 2.0 ** -23) for B, H, W in rp.AUX_SHAPES] == [28606, 6554, 120, 32, 123]
    for B, H, W, _ in rp.LSE_SHAPES:  # uniform logits: one element more or less in the normaliser against the 2e-6 of the check
        assert (1.0 / (2 * H * W)) / 2e-6 >= 15
